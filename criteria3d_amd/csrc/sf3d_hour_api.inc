/* part of sf3d_api.cpp (included at its end, after the other raster blocks) - the C entry points of include/sf3d_hour.h.  Every call checks
 * on the host that the block it works for is initialised, that the blocks it reads are on the same raster and have produced their maps,
 * and only then reaches the device (sf3d_hour.inc).  The host keeps what sf3d_hour_set_ponds was given - the tangent of the slope is the C
 * library's - until the first sf3d_hour_update_ponds uploads it, and moves the day's ponds from the cells to the surface nodes. */
#include <cmath>

#include "sf3d_hour.h"

namespace {

struct PondHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0, nUnits = 0;
    bool computeCrop = false;
    uint64_t ver = 0;
    std::vector<double> tanSlope;
    std::vector<int32_t> unit;                 /* -1: no land unit, or no slope */
    std::vector<HourPondUnitDev> units;
    std::vector<float> cells;                  /* the last download */
} PD;

uint64_t pondVersions = 0;                     /* a new number for every sf3d_hour_set_ponds */

void hourClear() { PD = PondHost(); (void)dev().hour_free(); }

/* the meteo block is on the raster of nrRows x nrCols cells and has produced every one of `vars` */
bool hourMeteoFeeds(uint32_t nrRows, uint32_t nrCols, std::initializer_list<int> vars)
{
    if (!rasterFeeds(MT, nrRows, nrCols)) return false;
    for (int v : vars) if (!dev().meteo_produced(v, nrRows, nrCols)) return false;
    return true;
}

/* the radiation block is on that raster, an hour has run and the transmissivity map it read is still there */
bool hourRadFeeds(uint32_t nrRows, uint32_t nrCols) { return rasterFeeds(RD, nrRows, nrCols) && dev().rad_hour_done(nrRows, nrCols); }

}  // namespace

extern "C" {

sf3d_error_t sf3d_hour_relative_humidity(uint32_t nrCells, float* out)      /* computeRelativeHumidityMap, meteoMaps.cpp:301-321 */
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != MT.nRows * MT.nCols) return SF3D_PARAMETER_ERROR;
    if (!hourMeteoFeeds(MT.nRows, MT.nCols, {METEO_AIR_TEMPERATURE, METEO_AIR_DEW_TEMPERATURE})) return SF3D_PARAMETER_ERROR;
    return rasterFail("hour relative humidity", dev().hour_relhum(mapsOwnedCells(nrCells), out));
}

sf3d_error_t sf3d_hour_snow(uint32_t nrCells, const float* surfaceWater, double clearSkyTransmissivity)      /* computeSnowModel, criteria3DProject.cpp:1815-1878 */
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    if (nrCells != SN.nRows * SN.nCols) return SF3D_PARAMETER_ERROR;
    if (!hourMeteoFeeds(SN.nRows, SN.nCols, {METEO_AIR_TEMPERATURE, METEO_PRECIPITATION, METEO_AIR_REL_HUMIDITY, METEO_WIND_SCALAR_INTENSITY})) return SF3D_PARAMETER_ERROR;
    if (!hourRadFeeds(SN.nRows, SN.nCols)) return SF3D_PARAMETER_ERROR;
    const SnowParamsDev p = {SN.par.skinThickness, SN.par.soilAlbedo, SN.par.snowVegetationHeight, SN.par.snowWaterHoldingCapacity,
                             SN.par.tempMaxWithSnow, SN.par.tempMinWithRain, SN.par.snowSurfaceDampingDepth, clearSkyTransmissivity};
    return rasterFail("hour snow", dev().hour_snow(surfaceWater, p, SN.flag, mapsOwnedCells(nrCells)));
}

sf3d_error_t sf3d_hour_et0(uint32_t nrCells, float clearSkyTransmissivity)      /* computeET0PMMap, meteoMaps.cpp:238-271; updateDailyTemperatures, criteria3DProject.cpp:1994-2018 */
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (nrCells != CR.nRows * CR.nCols) return SF3D_PARAMETER_ERROR;
    if (!hourMeteoFeeds(CR.nRows, CR.nCols, {METEO_AIR_TEMPERATURE, METEO_AIR_REL_HUMIDITY, METEO_WIND_SCALAR_INTENSITY})) return SF3D_PARAMETER_ERROR;
    if (!hourRadFeeds(CR.nRows, CR.nCols)) return SF3D_PARAMETER_ERROR;
    return rasterFail("hour et0", dev().hour_et0(clearSkyTransmissivity, CR.flag, mapsOwnedCells(nrCells)));
}

sf3d_error_t sf3d_hour_sinks(uint32_t nrCells)      /* assignETreal, assignPrecipitation, criteria3DProject.cpp:796-964 */
{
    return sinkComputeHour(nrCells, nullptr, nullptr, nullptr, nullptr, true);
}

sf3d_error_t sf3d_hour_totals(uint32_t nrCells, double* totals)      /* criteria3DProject.cpp:827-829, :867-870, :939-957 */
{
    if (!SK.on) return SF3D_MEMORY_ERROR;
    if (!totals || nrCells != SK.nRows * SK.nCols) return SF3D_PARAMETER_ERROR;
    NEED_INIT_E;
    if (!MP.set || MP.nCells != nrCells || MP.nLayers != SK.nrLayers) return SF3D_TOPOGRAPHY_ERROR;
    if (MP.maxNode >= 0 && (uint32_t)MP.maxNode >= M.N) return SF3D_TOPOGRAPHY_ERROR;
    if (!dev().hour_totals_ready(nrCells)) return SF3D_PARAMETER_ERROR;
    HostModel& D = deviceModel();
    MapsInput in;
    mapsDeviceInput(in);
    return rasterFail("hour totals", dev().hour_totals(D, P, in, mapsOwnedCells(nrCells), totals));
}

sf3d_error_t sf3d_hour_set_ponds(uint32_t nrRows, uint32_t nrCols, const float* slopeDegree, float slopeFlag, const int32_t* landUnitIndex, uint32_t nUnits,
                                 const double* maximumPond, const double* laiMax, const int32_t* isCrop, int computeCrop)      /* computeCurrentPond, project3D.cpp:1779-1816 */
{
    if (!rasterShapeOk(nrRows, nrCols, slopeDegree) || !landUnitIndex) return SF3D_PARAMETER_ERROR;
    if (nUnits > SF3D_CROP_MAX_UNITS || (nUnits > 0 && (!maximumPond || !laiMax || !isCrop))) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    for (uint32_t c = 0; c < n; ++c)
        if (landUnitIndex[c] >= 0 && (uint32_t)landUnitIndex[c] >= nUnits) return SF3D_PARAMETER_ERROR;
    if (computeCrop && !rasterFeeds(CR, nrRows, nrCols)) return SF3D_PARAMETER_ERROR;
    PD = PondHost();
    PD.nRows = nrRows; PD.nCols = nrCols; PD.nUnits = nUnits; PD.computeCrop = computeCrop != 0;
    PD.tanSlope.assign(n, 0.); PD.unit.assign(n, -1);
    for (uint32_t c = 0; c < n; ++c) {
        if (rasterIsFlag(slopeDegree[c], slopeFlag) || landUnitIndex[c] < 0) continue;
        PD.tanSlope[c] = std::tan(slopeDegree[c] * kMapDegToRad);                /* project3D.cpp:1789 */
        PD.unit[c] = landUnitIndex[c];
    }
    PD.units.resize(nUnits);
    for (uint32_t u = 0; u < nUnits; ++u) PD.units[u] = HourPondUnitDev{maximumPond[u], laiMax[u], isCrop[u] ? 1 : 0, 0};
    PD.ver = ++pondVersions;
    PD.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_hour_update_ponds(uint32_t nrCells, float* pondMap)      /* dailyUpdatePond, project3D.cpp:1819-1843 */
{
    if (!PD.on) return SF3D_MEMORY_ERROR;
    if (nrCells != PD.nRows * PD.nCols) return SF3D_PARAMETER_ERROR;
    NEED_INIT_E;
    if (!MP.set || MP.nCells != nrCells) return SF3D_TOPOGRAPHY_ERROR;
    if (MP.maxNode >= 0 && (uint32_t)MP.maxNode >= M.N) return SF3D_TOPOGRAPHY_ERROR;
    if (PD.computeCrop && !(rasterFeeds(CR, PD.nRows, PD.nCols) && dev().crop_allocated(nrCells))) return SF3D_PARAMETER_ERROR;
    HostModel& D = deviceModel();
    MapsInput in;
    mapsDeviceInput(in);
    const HourPondSetup setup{PD.tanSlope.data(), PD.unit.data(), PD.units.data(), nrCells, PD.nUnits, PD.ver};
    PD.cells.resize(nrCells);
    const uint8_t* mine = mapsOwnedCells(nrCells);
    const sf3d_error_t e = dev().hour_pond(D, P, in, setup, PD.computeCrop, PD.computeCrop ? CR.flag : -9999.f, mine, PD.cells.data());
    if (e != SF3D_OK) return rasterFail("hour update ponds", e);
    /* the surface nodes in the caller's (global) numbering, as sf3d_set_nodes_pond takes them; a rank sets the nodes of its own cells */
    for (uint32_t c = 0; c < nrCells; ++c) {
        const int32_t node = MP.col[c];
        const float pond = PD.cells[c];
        if (node < 0 || (mine && !mine[c]) || rasterIsFlag(pond, -9999.f)) continue;      /* isEqual(pond, NODATA): continue */
        if (skippedByTrim((uint32_t)node)) continue;
        const sf3d_error_t es = sf3d_set_node_pond((uint32_t)node, pond);
        if (es != SF3D_OK) return es;
    }
    if (pondMap) std::copy(PD.cells.begin(), PD.cells.end(), pondMap);
    return SF3D_OK;
}

double sf3d_hour_kernel_ms(int which) { return dev().hour_kernel_ms(which); }

sf3d_error_t sf3d_hour_clean(void)
{
    hourClear();
    return SF3D_OK;
}

} /* extern "C" */
