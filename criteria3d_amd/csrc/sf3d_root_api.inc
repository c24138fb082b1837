/* part of sf3d_api.cpp (included at its end, after the crop entry points) - the C entry points of include/sf3d_root.h.  The host keeps the
 * raster's size and flag and checks the tables against the caps; the (unit, soil) pairs of the raster, the rows of the density table and
 * what needs the C library's atan2 (lunette[] of cardioidDistribution) come from sf3d_root_setup.inc; everything else lives on the device
 * (sf3d_root.inc). */
#include <cmath>

#include "sf3d_root.h"
#include "sf3d_root_setup.inc"

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

}  // namespace

extern "C" {

sf3d_error_t sf3d_root_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, uint32_t nrLayers, const double* layerDepth,
                                  const double* layerThickness, const int32_t* cropIndex, const int32_t* soilIndex, uint32_t nUnits,
                                  const sf3d_root_unit_t* units, uint32_t nSoils, const sf3d_root_soil_t* soils)
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !cropIndex || !soilIndex) return SF3D_PARAMETER_ERROR;
    if (nrLayers == 0 || nrLayers > SF3D_ROOT_MAX_LAYERS || !layerDepth || !layerThickness) return SF3D_PARAMETER_ERROR;
    if (nUnits > SF3D_CROP_MAX_UNITS || (nUnits > 0 && !units) || nSoils > SF3D_ROOT_MAX_SOILS || (nSoils > 0 && !soils)) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    RootTablesHost T;
    const sf3d_error_t et = rootBuildTables(n, dem, flag, nrLayers, layerDepth, cropIndex, soilIndex, nUnits, nSoils, soils, T);
    if (et != SF3D_OK) return et;
    rootClear();
    RootSetup S{};
    S.nCells = n; S.nUnits = nUnits; S.nSoils = nSoils; S.nrLayers = nrLayers; S.nRows = (uint32_t)T.rowUnit.size(); S.lunetteMax = T.lunetteMax;
    S.dem = dem; S.cropIndex = T.ci.data(); S.soilIndex = T.si.data();
    S.units = reinterpret_cast<const RootUnitDev*>(units); S.soilDepth = T.soilDepth.data(); S.soilMaxN = T.soilMaxN.data(); S.pairRow = T.pairRow.data();
    S.layerDepth = layerDepth; S.layerThickness = layerThickness; S.layerFrac = T.layerFrac.data(); S.lunette = T.lunette.data();
    S.rowUnit = T.rowUnit.data(); S.rowSoil = T.rowSoil.data(); S.rowN = T.rowN.data(); S.flag = flag;
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
