/* part of sf3d_api.cpp (included at its end, after the crop entry points) - the C entry points of include/sf3d_root.h.  The host keeps the
 * raster's size and flag, checks the tables against the caps, lists the (unit, soil) pairs of the raster and the rows of the density
 * table, and evaluates what needs the C library's atan2 (lunette[] of cardioidDistribution); everything else lives on the device
 * (sf3d_root.inc). */
#include <cmath>

#include "sf3d_root.h"

static_assert(sizeof(sf3d_root_unit_t) == sizeof(RootUnitDev) && sizeof(RootUnitDev) == 48, "the root unit table is copied as it is");
static_assert(sizeof(sf3d_root_soil_t) == 16 + 3 * 8 * SF3D_ROOT_MAX_HORIZONS, "sf3d_root_soil_t has no padding");
static_assert(SF3D_ROOT_MAX_SOILS == ROOT_MAX_SOILS && SF3D_ROOT_MAX_LAYERS == ROOT_MAX_LAYERS && SF3D_ROOT_MAX_ATOMS == ROOT_MAX_ATOMS,
              "sf3d_root.h and sf3d_device.h disagree");

namespace {

struct RootHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0, nrLayers = 0;
    float flag = -9999.f;
} RT;

void rootClear() { RT = RootHost(); (void)dev().root_free(); }

/* lunette[0 .. m-1] of cardioidDistribution (root.cpp:277-284) for m = 1 .. maxM, m's values at m (m - 1) / 2: they depend on the two
 * integers only; atan2 and sqrt are the C library's, PI is commonConstants.h:249 */
std::vector<double> rootLunette(uint32_t maxM)
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

}  // namespace

extern "C" {

sf3d_error_t sf3d_root_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, uint32_t nrLayers, const double* layerDepth,
                                  const double* layerThickness, const int32_t* cropIndex, const int32_t* soilIndex, uint32_t nUnits,
                                  const sf3d_root_unit_t* units, uint32_t nSoils, const sf3d_root_soil_t* soils)
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !cropIndex || !soilIndex) return SF3D_PARAMETER_ERROR;
    if (nrLayers == 0 || nrLayers > SF3D_ROOT_MAX_LAYERS || !layerDepth || !layerThickness) return SF3D_PARAMETER_ERROR;
    if (nUnits > SF3D_CROP_MAX_UNITS || (nUnits > 0 && !units) || nSoils > SF3D_ROOT_MAX_SOILS || (nSoils > 0 && !soils)) return SF3D_PARAMETER_ERROR;
    for (uint32_t s = 0; s < nSoils; ++s)
        if (soils[s].nrHorizons < 0 || soils[s].nrHorizons > SF3D_ROOT_MAX_HORIZONS) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    std::vector<int32_t> ci(n), si(n);
    std::vector<uint8_t> pairOn((size_t)nUnits * nSoils, 0), soilOn(nSoils, 0);
    for (uint32_t c = 0; c < n; ++c) {
        if ((cropIndex[c] >= 0 && (uint32_t)cropIndex[c] >= nUnits) || (soilIndex[c] >= 0 && (uint32_t)soilIndex[c] >= nSoils)) return SF3D_PARAMETER_ERROR;
        ci[c] = cropIndex[c] < 0 ? -1 : cropIndex[c];
        si[c] = soilIndex[c] < 0 ? -1 : soilIndex[c];
        if (ci[c] >= 0 && si[c] >= 0 && !rasterIsFlag(dem[c], flag)) { pairOn[(size_t)ci[c] * nSoils + si[c]] = 1; soilOn[si[c]] = 1; }
    }
    /* per soil: the largest number of rooted atoms a cell can ask for, and the atoms; the caps hold for the soils of the raster */
    std::vector<double> soilDepth(nSoils), layerFrac((size_t)nSoils * nrLayers, -1.0);
    std::vector<int32_t> soilMaxN(nSoils, 0);
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
    std::vector<int32_t> pairRow((size_t)nUnits * nSoils, -1), rowUnit, rowSoil, rowN;
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
    const std::vector<double> lunette = rootLunette(lunetteMax);
    rootClear();
    RootSetup S{};
    S.nCells = n; S.nUnits = nUnits; S.nSoils = nSoils; S.nrLayers = nrLayers; S.nRows = (uint32_t)rowUnit.size(); S.lunetteMax = lunetteMax;
    S.dem = dem; S.cropIndex = ci.data(); S.soilIndex = si.data();
    S.units = reinterpret_cast<const RootUnitDev*>(units); S.soilDepth = soilDepth.data(); S.soilMaxN = soilMaxN.data(); S.pairRow = pairRow.data();
    S.layerDepth = layerDepth; S.layerThickness = layerThickness; S.layerFrac = layerFrac.data(); S.lunette = lunette.data();
    S.rowUnit = rowUnit.data(); S.rowSoil = rowSoil.data(); S.rowN = rowN.data(); S.flag = flag;
    const sf3d_error_t e = dev().root_alloc(S);
    if (e != SF3D_OK) { rasterFail("root initialize", e); rootClear(); return e; }
    RT.nRows = nrRows; RT.nCols = nrCols; RT.nrLayers = nrLayers; RT.flag = flag;
    RT.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_root_compute(uint32_t nrCells, const float* degreeDays)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    if (!degreeDays && !(rasterFeeds(CR, RT.nRows, RT.nCols) && dev().crop_allocated(nrCells))) return SF3D_PARAMETER_ERROR;
    return rasterFail("root compute", dev().root_compute(degreeDays, RT.flag, mapsOwnedCells(nrCells)));
}

sf3d_error_t sf3d_root_get_length(uint32_t nrCells, double* map)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("root get length", dev().root_download(ROOT_MAP_LENGTH, map));
}

sf3d_error_t sf3d_root_get_depth(uint32_t nrCells, double* map)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("root get depth", dev().root_download(ROOT_MAP_DEPTH, map));
}

sf3d_error_t sf3d_root_get_layers(uint32_t nrCells, int32_t* first, int32_t* last)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (!first || !last || nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    sf3d_error_t e = dev().root_download(ROOT_MAP_FIRST, first);
    if (e == SF3D_OK) e = dev().root_download(ROOT_MAP_LAST, last);
    return rasterFail("root get layers", e);
}

sf3d_error_t sf3d_root_get_density(int layer, uint32_t nrCells, double* map)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    if (layer < -1 || layer >= (int)RT.nrLayers) return SF3D_INDEX_ERROR;
    return rasterFail("root get density", dev().root_density(layer, map, RT.flag));
}

sf3d_error_t sf3d_root_get_keys(uint32_t nrCells, int32_t* map)
{
    if (!RT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != RT.nRows * RT.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("root get keys", dev().root_download(ROOT_MAP_KEY, map));
}

uint32_t sf3d_root_table_rows(void) { return RT.on ? dev().root_table_rows() : 0; }

double sf3d_root_kernel_ms(int which) { return dev().root_kernel_ms(which); }

sf3d_error_t sf3d_root_clean(void)
{
    rootClear();
    return SF3D_OK;
}

} /* extern "C" */
