/* sf3d_sink_setup.inc - the host side of the sink block's tables (included by sf3d_sink_api.inc and by tests/sink_host.cpp): what
 * sf3d_sink_initialize and sf3d_sink_set_cracking derive from the soils and the layer grid before anything runs on the device - the
 * evaporation coefficients, which need the C library's exp (initializeEvaporationCoefficient), getHorizonIndex of every (soil, layer), the
 * horizons' water contents, and per soil the depth and the last layer of a crack.  No device code: the host program runs it under the
 * sanitizers. */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "sf3d_sink.h"

struct SinkTablesHost {
    int32_t lastEvapLayer = 0;
    std::vector<double> evapCoeff, layerEvapCoeff, horizonValues;
    std::vector<int32_t> horizon;
    std::vector<SinkUnitDev> units;
};

static const double kMaxEvaporationDepth = 0.25;      /* MAX_EVAPORATION_DEPTH, commonConstants.h:116 */

/* Project3D::getSoilLayerIndex, project3D.cpp:1764-1776 */
static inline int sinkLayerIndex(uint32_t nrLayers, const double* layerDepth, const double* layerThickness, double depth)
{
    if (nrLayers == 0 || depth < 0) return -9999;
    for (uint32_t layer = 0; layer < nrLayers; ++layer)
        if (depth <= layerDepth[layer] + layerThickness[layer] * 0.5) return (int)layer;
    return -9999;
}

/* SF3D_PARAMETER_ERROR where no layer reaches the evaporation depth */
static inline sf3d_error_t sinkBuildTables(uint32_t nrLayers, const double* layerDepth, const double* layerThickness, double computationSoilDepth, uint32_t nUnits,
                                           const sf3d_sink_unit_t* units, uint32_t nSoils, const sf3d_sink_soil_t* soils, SinkTablesHost& T)
{
    /* initializeEvaporationCoefficient, project3D.cpp:2331-2368 */
    int lastEvapLayer = sinkLayerIndex(nrLayers, layerDepth, layerThickness, kMaxEvaporationDepth);
    if (computationSoilDepth < kMaxEvaporationDepth) lastEvapLayer = sinkLayerIndex(nrLayers, layerDepth, layerThickness, computationSoilDepth);
    if (lastEvapLayer == -9999) return SF3D_PARAMETER_ERROR;
    std::vector<double>& evapCoeff = T.evapCoeff;
    std::vector<double>& layerEvapCoeff = T.layerEvapCoeff;
    evapCoeff.assign(nrLayers, 0.); layerEvapCoeff.assign(nrLayers, 0.);
    double coeffSum = 0;
    for (int layer = 1; layer <= lastEvapLayer; layer++) {
        const double depthCoeff = std::max((layerDepth[layer] - layerDepth[1]) / (kMaxEvaporationDepth - layerDepth[1]), 0.0);
        evapCoeff[layer] = exp(-2 * depthCoeff);
        layerEvapCoeff[layer] = evapCoeff[layer] * (layerThickness[layer] / 0.04);
        coeffSum += layerEvapCoeff[layer];
    }
    const double invCoeffSum = 1.0 / coeffSum;
    for (int layer = 1; layer <= lastEvapLayer; layer++) layerEvapCoeff[layer] *= invCoeffSum;
    T.lastEvapLayer = lastEvapLayer;

    T.units.resize(nUnits);
    for (uint32_t u = 0; u < nUnits; ++u) T.units[u] = SinkUnitDev{units[u].kcMax, units[u].fRAW, units[u].isWaterSurplusResistant ? 1 : 0, 0};
    T.horizon.assign((size_t)nSoils * nrLayers, -1);
    T.horizonValues.assign((size_t)nSoils * SF3D_ROOT_MAX_HORIZONS * SINK_HORIZON_VALUES, 0.);
    for (uint32_t s = 0; s < nSoils; ++s) {
        const sf3d_sink_soil_t& so = soils[s];
        for (int32_t h = 0; h < so.nrHorizons; ++h) {
            double* hz = T.horizonValues.data() + ((size_t)s * SF3D_ROOT_MAX_HORIZONS + h) * SINK_HORIZON_VALUES;
            hz[SINK_H_HH] = so.waterContentHH[h]; hz[SINK_H_FC] = so.waterContentFC[h]; hz[SINK_H_WP] = so.waterContentWP[h];
            hz[SINK_H_SAT] = so.waterContentSAT[h]; hz[SINK_H_FRACTION] = so.soilFraction[h];
        }
        for (uint32_t l = 0; l < nrLayers; ++l)                           /* Crit3DSoil::getHorizonIndex(layerDepth[l]), soil.cpp:192-201 */
            for (int32_t h = 0; h < so.nrHorizons; ++h)
                if (layerDepth[l] >= so.upperDepth[h] && layerDepth[l] <= (so.lowerDepth[h] + 0.00001)) { T.horizon[(size_t)s * nrLayers + l] = h; break; }
    }
    return SF3D_OK;
}

/* The part of Crit3DProject::computeSoilCracking (criteria3DProject.cpp:1003-1035, :1078) that depends on the soil and the layer grid only.
 * Every one of these exits returns the precipitation unchanged and has no side effect, so their place before or after the per-cell tests
 * (soil index, pond, crackDepth, avgVoidVolume) changes no result: a soil that fails one never cracks (-9999 in both tables).
 * upperDepth, lowerDepth: [soil][SF3D_ROOT_MAX_HORIZONS] of the soils sf3d_sink_initialize took */
static inline void sinkCrackTables(uint32_t nSoils, const sf3d_sink_crack_soil_t* soils, const double* upperDepth, const double* lowerDepth, double computationSoilDepth,
                                   uint32_t nrLayers, const double* layerDepth, const double* layerThickness, std::vector<double>& maxDepthOf,
                                   std::vector<int32_t>& lastLayerOf)
{
    const double MAX_CRACKING_DEPTH = 0.6, MIN_FINE_LAYER_DEPTH = 0.2, MIN_FINE_FRACTION = 0.5;
    maxDepthOf.assign(nSoils, -9999.);
    lastLayerOf.assign(nSoils, -9999);
    for (uint32_t s = 0; s < nSoils; ++s) {
        const sf3d_sink_crack_soil_t& so = soils[s];
        const double* upper = upperDepth + (size_t)s * SF3D_ROOT_MAX_HORIZONS;
        const double* lower = lowerDepth + (size_t)s * SF3D_ROOT_MAX_HORIZONS;
        const double soilDepth = std::min(computationSoilDepth, so.totalDepth);
        if (soilDepth <= MIN_FINE_LAYER_DEPTH) continue;
        int lastFineHorizon = -9999;
        double maxDepth = std::min(soilDepth, MAX_CRACKING_DEPTH);
        int32_t h = 0;
        while (h < so.nrHorizons && upper[h] < maxDepth) {
            const double fineFraction = (so.clay[h] + so.silt[h] * 0.5) / 100 * (1 - so.coarseFragments[h]) * (1 - so.organicMatter[h]);
            if (fineFraction < MIN_FINE_FRACTION) break;
            lastFineHorizon = h;
            ++h;
        }
        if (lastFineHorizon == -9999) continue;
        maxDepth = std::min(lower[lastFineHorizon], MAX_CRACKING_DEPTH);
        maxDepth = std::min(maxDepth, computationSoilDepth);
        if (maxDepth < MIN_FINE_LAYER_DEPTH) continue;
        const int lastLayer = sinkLayerIndex(nrLayers, layerDepth, layerThickness, maxDepth);
        if (lastLayer == -9999) continue;
        maxDepthOf[s] = maxDepth; lastLayerOf[s] = lastLayer;
    }
}
