/* sf3d_root_setup.inc - the host side of the root block's tables (included by sf3d_root_api.inc and by tests/root_host.cpp): what
 * sf3d_root_initialize derives from the raster, the soils and the layer grid before anything runs on the device - the (unit, soil) pairs
 * of the raster, the rows of the density table, getHorizonIndex of every (soil, layer), and lunette[] of cardioidDistribution, which
 * needs the C library's atan2.  No device code: the host program runs it under the sanitizers. */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "sf3d_root.h"

struct RootTablesHost {
    std::vector<int32_t> ci, si;                /* the index maps with every negative value as -1 */
    std::vector<double> soilDepth, layerFrac, lunette;
    std::vector<int32_t> soilMaxN, pairRow, rowUnit, rowSoil, rowN;
    uint32_t lunetteMax = 0;
};

/* lunette[0 .. m-1] of cardioidDistribution (root.cpp:277-284) for m = 1 .. maxM, m's values at m (m - 1) / 2: they depend on the two
 * integers only; atan2 and sqrt are the C library's, PI is commonConstants.h:249 */
static inline std::vector<double> rootLunette(uint32_t maxM)
{
    const double PI_ = 3.1415926535898;
    std::vector<double> t((size_t)maxM * (maxM + 1) / 2);
    for (uint32_t m = 1; m <= maxM; ++m) {
        double* lunette = t.data() + (size_t)(m - 1) * m / 2;
        const double halfPI = PI_ / 2.0;
        for (uint32_t i = 0; i < m; ++i) {
            const double sinAlfa = 1.0 - double(i + 1.0) / double(m);
            const double v = std::max(0.0, 1.0 - sinAlfa * sinAlfa);
            const double cosAlfa = std::max(std::sqrt(v), 0.0001);
            const double alfa = atan2(sinAlfa, cosAlfa);
            lunette[i] = (halfPI - alfa - sinAlfa * cosAlfa) / PI_;
        }
    }
    return t;
}

/* the tables of a raster of n cells; SF3D_PARAMETER_ERROR where an index, a soil of the raster or the table's size is outside the caps */
static inline sf3d_error_t rootBuildTables(uint32_t n, const float* dem, float flag, uint32_t nrLayers, const double* layerDepth, const int32_t* cropIndex,
                                           const int32_t* soilIndex, uint32_t nUnits, uint32_t nSoils, const sf3d_root_soil_t* soils, RootTablesHost& T)
{
    for (uint32_t s = 0; s < nSoils; ++s)
        if (soils[s].nrHorizons < 0 || soils[s].nrHorizons > SF3D_ROOT_MAX_HORIZONS) return SF3D_PARAMETER_ERROR;
    std::vector<int32_t>& ci = T.ci;
    std::vector<int32_t>& si = T.si;
    ci.assign(n, -1); si.assign(n, -1);
    std::vector<uint8_t> pairOn((size_t)nUnits * nSoils, 0), soilOn(nSoils, 0);
    for (uint32_t c = 0; c < n; ++c) {
        if ((cropIndex[c] >= 0 && (uint32_t)cropIndex[c] >= nUnits) || (soilIndex[c] >= 0 && (uint32_t)soilIndex[c] >= nSoils)) return SF3D_PARAMETER_ERROR;
        ci[c] = cropIndex[c] < 0 ? -1 : cropIndex[c];
        si[c] = soilIndex[c] < 0 ? -1 : soilIndex[c];
        const bool isFlag = std::fabs(static_cast<double>(dem[c]) - static_cast<double>(flag)) < 0.00001;      /* isEqual(float, float) */
        if (ci[c] >= 0 && si[c] >= 0 && !isFlag) { pairOn[(size_t)ci[c] * nSoils + si[c]] = 1; soilOn[si[c]] = 1; }
    }
    /* per soil: the largest number of rooted atoms a cell can ask for, and the atoms; the caps hold for the soils of the raster */
    std::vector<double>& soilDepth = T.soilDepth;
    std::vector<double>& layerFrac = T.layerFrac;
    std::vector<int32_t>& soilMaxN = T.soilMaxN;
    soilDepth.assign(nSoils, 0.); layerFrac.assign((size_t)nSoils * nrLayers, -1.0); soilMaxN.assign(nSoils, 0);
    uint32_t lunetteMax = 0;
    for (uint32_t s = 0; s < nSoils; ++s) {
        const sf3d_root_soil_t& so = soils[s];
        soilDepth[s] = so.totalDepth;
        for (uint32_t l = 0; l < nrLayers; ++l)                           /* Crit3DSoil::getHorizonIndex(layerDepth[l]), soil.cpp:192-201 */
            for (int32_t h = 0; h < so.nrHorizons; ++h)
                if (layerDepth[l] >= so.upperDepth[h] && layerDepth[l] <= (so.lowerDepth[h] + 0.00001)) {
                    if (soilOn[s] && !(so.soilFraction[h] >= 0)) return SF3D_PARAMETER_ERROR;
                    layerFrac[(size_t)s * nrLayers + l] = so.soilFraction[h];
                    break;
                }
        if (!soilOn[s]) continue;
        if (!(so.totalDepth > 0) || !(so.totalDepth * 100 < (double)SF3D_ROOT_MAX_ATOMS - 1)) return SF3D_PARAMETER_ERROR;
        const int32_t nrAtoms = (int32_t)(so.totalDepth * 100) + 1;
        soilMaxN[s] = (int32_t)std::round(so.totalDepth / 0.01);
        if (nrAtoms > SF3D_ROOT_MAX_ATOMS || soilMaxN[s] > SF3D_ROOT_MAX_ATOMS) return SF3D_PARAMETER_ERROR;
        lunetteMax = std::max(lunetteMax, (uint32_t)std::max(nrAtoms, soilMaxN[s]));
    }
    /* the rows of the density table: for every pair of the raster, 0 .. soilMaxN rooted atoms */
    std::vector<int32_t>& pairRow = T.pairRow;
    std::vector<int32_t>& rowUnit = T.rowUnit;
    std::vector<int32_t>& rowSoil = T.rowSoil;
    std::vector<int32_t>& rowN = T.rowN;
    pairRow.assign((size_t)nUnits * nSoils, -1); rowUnit.clear(); rowSoil.clear(); rowN.clear();
    uint64_t rows = 0;
    for (uint32_t u = 0; u < nUnits; ++u)
        for (uint32_t s = 0; s < nSoils; ++s)
            if (pairOn[(size_t)u * nSoils + s]) rows += (uint64_t)soilMaxN[s] + 1;
    if (rows * nrLayers > SF3D_ROOT_MAX_TABLE_VALUES) return SF3D_PARAMETER_ERROR;
    rowUnit.reserve(rows); rowSoil.reserve(rows); rowN.reserve(rows);
    for (uint32_t u = 0; u < nUnits; ++u)
        for (uint32_t s = 0; s < nSoils; ++s) {
            if (!pairOn[(size_t)u * nSoils + s]) continue;
            pairRow[(size_t)u * nSoils + s] = (int32_t)rowUnit.size();
            for (int32_t k = 0; k <= soilMaxN[s]; ++k) { rowUnit.push_back((int32_t)u); rowSoil.push_back((int32_t)s); rowN.push_back(k); }
        }
    T.lunetteMax = lunetteMax;
    T.lunette = rootLunette(lunetteMax);
    return SF3D_OK;
}
