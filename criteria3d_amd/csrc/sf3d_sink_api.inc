/* part of sf3d_api.cpp (included at its end, after the meteo entry points) - the C entry points of include/sf3d_sink.h.  The host keeps the
 * raster and the tables until the first hour uploads them (no device is needed before); what needs the C library's exp
 * (initializeEvaporationCoefficient), getHorizonIndex of every (soil, layer) and the crack tables come from sf3d_sink_setup.inc.  It hands
 * the column table of sf3d_maps.h to the device in the numbering of the model it works on, and moves the node sinks between that numbering
 * and the caller's. */
#include <cmath>

#include "sf3d_sink.h"
#include "sf3d_sink_setup.inc"

static_assert(sizeof(sf3d_sink_unit_t) == sizeof(SinkUnitDev) && sizeof(SinkUnitDev) == 24, "the sink unit table is copied as it is");
static_assert(sizeof(sf3d_sink_soil_t) == 8 + 7 * 8 * SF3D_ROOT_MAX_HORIZONS, "sf3d_sink_soil_t has no padding");
static_assert(sizeof(sf3d_sink_crack_soil_t) == 16 + 4 * 8 * SF3D_ROOT_MAX_HORIZONS, "sf3d_sink_crack_soil_t has no padding");
static_assert(SF3D_ROOT_MAX_HORIZONS == ROOT_MAX_HORIZONS, "sf3d_root.h and sf3d_device.h disagree");

namespace {

struct SinkHost {
    bool on = false, uploaded = false;
    uint32_t nRows = 0, nCols = 0, nrLayers = 0, nUnits = 0, nSoils = 0;
    int32_t lastEvapLayer = 0;
    float flag = -9999.f;
    double area = 0.;
    std::vector<float> dem;
    std::vector<int32_t> cropIndex, soilIndex, horizon;
    std::vector<SinkUnitDev> units;
    std::vector<double> horizonValues, layerDepth, thick, evapCoeff, layerEvapCoeff;
    std::vector<double> nodes;                 /* the last download, in the device model's numbering */
    /* soil cracking (sf3d_sink_set_cracking): the horizons' depths and the computation depth it needs, and its per-soil tables */
    double computationSoilDepth = 0.;
    std::vector<int32_t> nrHorizons;
    std::vector<double> upperDepth, lowerDepth;   /* [soil][SF3D_ROOT_MAX_HORIZONS] */
    bool crackOn = false;
    uint64_t crackVer = 0;
    std::vector<double> crackMaxDepth;         /* [soil], -9999: never cracks */
    std::vector<int32_t> crackLastLayer;       /* [soil], -9999: never cracks */
} SK;

uint64_t sinkCrackVersions = 0;                /* a new number for every table sf3d_sink_set_cracking leaves */

void sinkClear() { SK = SinkHost(); (void)dev().sink_free(); }

/* the node sinks of the last hour from the device into SK.nodes */
sf3d_error_t sinkFetch()
{
    if (!SK.on || !dev().sink_computed()) return SF3D_MEMORY_ERROR;
    const uint32_t count = LM.on ? (uint32_t)LM.l2g.size() : M.N;
    SK.nodes.resize(count);
    return rasterFail("sink nodes", dev().sink_download_nodes(SK.nodes.data(), count));
}

sf3d_error_t sinkComputeHour(uint32_t nrCells, const float* et0, const float* lai, const float* degreeDays, const float* liquidWater, bool rainFromMeteo);

}  // namespace

extern "C" {

sf3d_error_t sf3d_sink_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double cellSize, uint32_t nrLayers,
                                  const double* layerDepth, const double* layerThickness, double computationSoilDepth, const int32_t* cropIndex,
                                  const int32_t* soilIndex, uint32_t nUnits, const sf3d_sink_unit_t* units, uint32_t nSoils, const sf3d_sink_soil_t* soils)
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !cropIndex || !soilIndex) return SF3D_PARAMETER_ERROR;
    if (nrLayers == 0 || nrLayers > SF3D_ROOT_MAX_LAYERS || !layerDepth || !layerThickness || !(cellSize > 0)) return SF3D_PARAMETER_ERROR;
    if (nUnits > SF3D_CROP_MAX_UNITS || (nUnits > 0 && !units) || nSoils > SF3D_ROOT_MAX_SOILS || (nSoils > 0 && !soils)) return SF3D_PARAMETER_ERROR;
    for (uint32_t s = 0; s < nSoils; ++s)
        if (soils[s].nrHorizons < 0 || soils[s].nrHorizons > SF3D_ROOT_MAX_HORIZONS) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    for (uint32_t c = 0; c < n; ++c)
        if ((cropIndex[c] >= 0 && (uint32_t)cropIndex[c] >= nUnits) || (soilIndex[c] >= 0 && (uint32_t)soilIndex[c] >= nSoils)) return SF3D_PARAMETER_ERROR;
    SinkTablesHost T;
    const sf3d_error_t et = sinkBuildTables(nrLayers, layerDepth, layerThickness, computationSoilDepth, nUnits, units, nSoils, soils, T);
    if (et != SF3D_OK) return et;
    const int lastEvapLayer = T.lastEvapLayer;

    sinkClear();
    SK.nRows = nrRows; SK.nCols = nrCols; SK.nrLayers = nrLayers; SK.nUnits = nUnits; SK.nSoils = nSoils; SK.lastEvapLayer = lastEvapLayer;
    SK.flag = flag; SK.area = cellSize * cellSize; SK.computationSoilDepth = computationSoilDepth;
    SK.nrHorizons.resize(nSoils);
    SK.upperDepth.assign((size_t)nSoils * SF3D_ROOT_MAX_HORIZONS, 0.); SK.lowerDepth.assign((size_t)nSoils * SF3D_ROOT_MAX_HORIZONS, 0.);
    for (uint32_t s = 0; s < nSoils; ++s) {
        SK.nrHorizons[s] = soils[s].nrHorizons;
        std::copy(soils[s].upperDepth, soils[s].upperDepth + soils[s].nrHorizons, SK.upperDepth.begin() + (size_t)s * SF3D_ROOT_MAX_HORIZONS);
        std::copy(soils[s].lowerDepth, soils[s].lowerDepth + soils[s].nrHorizons, SK.lowerDepth.begin() + (size_t)s * SF3D_ROOT_MAX_HORIZONS);
    }
    SK.dem.assign(dem, dem + n);
    SK.cropIndex.resize(n); SK.soilIndex.resize(n);
    for (uint32_t c = 0; c < n; ++c) { SK.cropIndex[c] = cropIndex[c] < 0 ? -1 : cropIndex[c]; SK.soilIndex[c] = soilIndex[c] < 0 ? -1 : soilIndex[c]; }
    SK.units = T.units; SK.horizon = T.horizon; SK.horizonValues = T.horizonValues;
    SK.layerDepth.assign(layerDepth, layerDepth + nrLayers); SK.thick.assign(layerThickness, layerThickness + nrLayers);
    SK.evapCoeff = T.evapCoeff; SK.layerEvapCoeff = T.layerEvapCoeff;
    SK.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_sink_get_tables(double* evapCoeff, double* layerEvapCoeff, int32_t* lastEvapLayer, int32_t* horizonOfSoilLayer)
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    if (evapCoeff) std::copy(SK.evapCoeff.begin(), SK.evapCoeff.end(), evapCoeff);
    if (layerEvapCoeff) std::copy(SK.layerEvapCoeff.begin(), SK.layerEvapCoeff.end(), layerEvapCoeff);
    if (lastEvapLayer) *lastEvapLayer = SK.lastEvapLayer;
    if (horizonOfSoilLayer) for (size_t k = 0; k < SK.horizon.size(); ++k) horizonOfSoilLayer[k] = SK.horizon[k] < 0 ? -9999 : SK.horizon[k];
    return SF3D_OK;
}

/* the per-soil tables of soil cracking: sinkCrackTables of sf3d_sink_setup.inc */
sf3d_error_t sf3d_sink_set_cracking(uint32_t nSoils, const sf3d_sink_crack_soil_t* soils)
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    if (!soils || nSoils == 0) { SK.crackOn = false; SK.crackMaxDepth.clear(); SK.crackLastLayer.clear(); return SF3D_OK; }
    if (nSoils != SK.nSoils) return SF3D_PARAMETER_ERROR;
    for (uint32_t s = 0; s < nSoils; ++s)
        if (soils[s].nrHorizons < 0 || soils[s].nrHorizons > SF3D_ROOT_MAX_HORIZONS || soils[s].nrHorizons > SK.nrHorizons[s]) return SF3D_PARAMETER_ERROR;
    std::vector<double> maxDepthOf;
    std::vector<int32_t> lastLayerOf;
    sinkCrackTables(nSoils, soils, SK.upperDepth.data(), SK.lowerDepth.data(), SK.computationSoilDepth, SK.nrLayers, SK.layerDepth.data(), SK.thick.data(), maxDepthOf,
                    lastLayerOf);
    SK.crackMaxDepth = maxDepthOf; SK.crackLastLayer = lastLayerOf;
    SK.crackOn = true; SK.crackVer = ++sinkCrackVersions;
    return SF3D_OK;
}

sf3d_error_t sf3d_sink_get_crack_tables(double* maxDepth, int32_t* lastLayer)
{
    if (!SK.on || !SK.crackOn) return SF3D_MEMORY_ERROR;
    if (maxDepth) std::copy(SK.crackMaxDepth.begin(), SK.crackMaxDepth.end(), maxDepth);
    if (lastLayer) std::copy(SK.crackLastLayer.begin(), SK.crackLastLayer.end(), lastLayer);
    return SF3D_OK;
}

sf3d_error_t sf3d_sink_compute_hour(uint32_t nrCells, const float* et0, const float* lai, const float* degreeDays, const float* liquidWater)
{
    return sinkComputeHour(nrCells, et0, lai, degreeDays, liquidWater, false);
}

} /* extern "C" */

namespace {

/* sf3d_sink_compute_hour; rainFromMeteo (sf3d_hour_sinks of include/sf3d_hour.h): where no snow hour was done on this raster a null
 * liquidWater is the precipitation map of the meteo block (assignPrecipitation:943 with isSnow false) */
sf3d_error_t sinkComputeHour(uint32_t nrCells, const float* et0, const float* lai, const float* degreeDays, const float* liquidWater, bool rainFromMeteo)
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    if (nrCells != SK.nRows * SK.nCols) return SF3D_PARAMETER_ERROR;
    NEED_INIT_E;
    if (!MP.set || MP.nCells != nrCells || MP.nLayers != SK.nrLayers) return SF3D_TOPOGRAPHY_ERROR;
    if (MP.maxNode >= 0 && (uint32_t)MP.maxNode >= M.N) return SF3D_TOPOGRAPHY_ERROR;
    if ((!et0 || !lai || !degreeDays) && !(rasterFeeds(CR, SK.nRows, SK.nCols) && dev().crop_allocated(nrCells))) return SF3D_PARAMETER_ERROR;
    const bool fromSnow = rasterFeeds(SN, SK.nRows, SK.nCols) && dev().snow_hour_done(nrCells);
    const bool fromMeteo = !liquidWater && !fromSnow && rainFromMeteo && rasterFeeds(MT, SK.nRows, SK.nCols)
                           && dev().meteo_produced(METEO_PRECIPITATION, SK.nRows, SK.nCols);
    if (!liquidWater && !fromSnow && !fromMeteo) return SF3D_PARAMETER_ERROR;
    if (!(rasterFeeds(RT, SK.nRows, SK.nCols) && dev().root_computed(nrCells, SK.nrLayers))) return SF3D_PARAMETER_ERROR;
    if (!SK.uploaded || !dev().sink_allocated()) {
        SinkSetup S{};
        S.nCells = nrCells; S.nrLayers = SK.nrLayers; S.nUnits = SK.nUnits; S.nSoils = SK.nSoils; S.lastEvapLayer = SK.lastEvapLayer;
        S.dem = SK.dem.data(); S.cropIndex = SK.cropIndex.data(); S.soilIndex = SK.soilIndex.data(); S.units = SK.units.data();
        S.horizon = SK.horizon.data(); S.horizonValues = SK.horizonValues.data(); S.layerDepth = SK.layerDepth.data(); S.thick = SK.thick.data();
        S.evapCoeff = SK.evapCoeff.data(); S.layerEvapCoeff = SK.layerEvapCoeff.data(); S.area = SK.area; S.flag = SK.flag;
        const sf3d_error_t e = dev().sink_alloc(S);
        if (e != SF3D_OK) return rasterFail("sink upload", e);
        SK.uploaded = true;
    }
    HostModel& D = deviceModel();
    MapsInput in;
    mapsDeviceInput(in);
    SinkCall call{et0, lai, degreeDays, liquidWater, mapsOwnedCells(nrCells), nullptr, nullptr, 0, fromMeteo};
    if (SK.crackOn) { call.crackMaxDepth = SK.crackMaxDepth.data(); call.crackLastLayer = SK.crackLastLayer.data(); call.crackVer = SK.crackVer; }
    return rasterFail("sink compute hour", dev().sink_hour(D, P, in, call));
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_sink_get_node_sinks(uint32_t nrNodes, double* sinks)
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    NEED_INIT_E;
    if (!sinks || nrNodes != M.N) return SF3D_PARAMETER_ERROR;
    const sf3d_error_t e = sinkFetch();
    if (e != SF3D_OK) return e;
    if (!LM.on) { std::copy(SK.nodes.begin(), SK.nodes.end(), sinks); return SF3D_OK; }
    std::fill(sinks, sinks + nrNodes, 0.);
    for (size_t k = 0; k < LM.l2g.size(); ++k) sinks[LM.l2g[k]] = SK.nodes[k];
    return SF3D_OK;
}

sf3d_error_t sf3d_sink_get_actual(uint32_t nrCells, double* evaporation, double* transpiration)
{
    if (!SK.on || !dev().sink_allocated()) return SF3D_MEMORY_ERROR;
    if (nrCells != SK.nRows * SK.nCols) return SF3D_PARAMETER_ERROR;
    sf3d_error_t e = SF3D_OK;
    if (evaporation) e = dev().sink_download_cells(SINK_MAP_EVAPORATION, evaporation);
    if (e == SF3D_OK && transpiration) e = dev().sink_download_cells(SINK_MAP_TRANSPIRATION, transpiration);
    return rasterFail("sink get actual", e);
}

sf3d_error_t sf3d_sink_get_crack(uint32_t nrCells, float* precSurfaceWater, double* crackWater)
{
    if (!SK.on || !SK.crackOn || !dev().sink_crack_computed()) return SF3D_MEMORY_ERROR;
    if (nrCells != SK.nRows * SK.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("sink get crack", dev().sink_download_crack(precSurfaceWater, crackWater));
}

sf3d_error_t sf3d_sink_apply(void)
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    NEED_INIT_E;
    const sf3d_error_t e = sinkFetch();
    if (e != SF3D_OK) return e;
    if (M.sink.size() < M.N) return SF3D_MEMORY_ERROR;
    if (!LM.on) std::copy(SK.nodes.begin(), SK.nodes.end(), M.sink.begin());
    else {
        /* a rank's staging copy is read at its own nodes only (and may hold no pages elsewhere): the other ranks' nodes, 0 in this rank's array, are left alone */
        if (!LM.trimmed) std::fill(M.sink.begin(), M.sink.begin() + M.N, 0.);
        for (size_t k = 0; k < LM.l2g.size(); ++k) M.sink[LM.l2g[k]] = SK.nodes[k];
    }
    if (!M.sinkDirty) { M.sinkLo = 0; M.sinkHi = M.N; M.sinkDirty = true; }      /* what N single setters leave */
    else { M.sinkLo = 0; if (M.N > M.sinkHi) M.sinkHi = M.N; }
    return SF3D_OK;
}

double sf3d_sink_kernel_ms(void) { return dev().sink_kernel_ms(); }

sf3d_error_t sf3d_sink_clean(void)
{
    sinkClear();
    return SF3D_OK;
}

} /* extern "C" */
