/* part of sf3d_api.cpp (included at its end, after the snow entry points) - the C entry points of include/sf3d_crop.h.  The host keeps the
 * raster's size, its flag and the latitude; the maps and the crop table live on the device (sf3d_crop.inc). */
#include "sf3d_crop.h"

static_assert(sizeof(sf3d_crop_unit_t) == sizeof(CropUnitDev) && sizeof(CropUnitDev) == 96, "the crop table is copied as it is");
static_assert(SF3D_CROP_MAX_UNITS == CROP_MAX_UNITS, "sf3d_crop.h and sf3d_device.h disagree");

namespace {

struct CropHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0;
    float flag = -9999.f;
    double latitude = 0.;
} CR;

void cropClear() { CR = CropHost(); (void)dev().crop_free(); }

}  // namespace

extern "C" {

sf3d_error_t sf3d_crop_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, const int32_t* cropIndex, uint32_t nUnits,
                                  const sf3d_crop_unit_t* units, double latitude)       /* initializeCropMaps, criteria3DProject.cpp:415-433 */
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !cropIndex) return SF3D_PARAMETER_ERROR;
    if (nUnits > SF3D_CROP_MAX_UNITS || (nUnits > 0 && !units)) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    std::vector<int32_t> index(n);
    for (uint32_t c = 0; c < n; ++c) {
        if (cropIndex[c] >= 0 && (uint32_t)cropIndex[c] >= nUnits) return SF3D_PARAMETER_ERROR;
        index[c] = cropIndex[c] < 0 ? -1 : cropIndex[c];
    }
    cropClear();
    sf3d_error_t e = dev().crop_alloc(n, reinterpret_cast<const CropUnitDev*>(units), nUnits);
    if (e != SF3D_OK) return rasterFail("crop initialize", e);
    CR.nRows = nrRows; CR.nCols = nrCols; CR.flag = flag; CR.latitude = latitude;
    const std::vector<float> empty(n, flag);
    e = dev().crop_upload(CROP_MAP_DEM, dem);
    if (e == SF3D_OK) e = dev().crop_upload(CROP_MAP_INDEX, index.data());
    for (int k = 0; k < 5 && e == SF3D_OK; ++k) e = dev().crop_upload(CROP_MAP_STATE + k, empty.data());      /* the four state maps and ET0 */
    for (int k = 0; k < 5 && e == SF3D_OK; ++k) e = dev().crop_upload(CROP_MAP_IN + k, empty.data());
    if (e != SF3D_OK) { rasterFail("crop initialize", e); cropClear(); return e; }
    CR.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_crop_set_state(int which, uint32_t nrCells, const float* map)
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != CR.nRows * CR.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_CROP_STATE_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("crop set state", dev().crop_upload(CROP_MAP_STATE + which, map));
}

sf3d_error_t sf3d_crop_get_state(int which, uint32_t nrCells, float* map)
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != CR.nRows * CR.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_CROP_STATE_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("crop get state", dev().crop_download(CROP_MAP_STATE + which, map));
}

sf3d_error_t sf3d_crop_get_et0(uint32_t nrCells, float* map)
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != CR.nRows * CR.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("crop get et0", dev().crop_download(CROP_MAP_ET0, map));
}

sf3d_error_t sf3d_crop_set_degree_days(uint32_t nrCells, const float* map, int currentDoy)      /* initializeCropFromDegreeDays, criteria3DProject.cpp:524-573 */
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != CR.nRows * CR.nCols || currentDoy < 1 || currentDoy > 366) return SF3D_PARAMETER_ERROR;
    sf3d_error_t e = dev().crop_upload(CROP_MAP_STATE + SF3D_CROP_DEGREE_DAYS, map);
    if (e == SF3D_OK) e = dev().crop_day(-1, currentDoy, CR.latitude, CR.flag, nullptr);
    return rasterFail("crop set degree days", e);
}

sf3d_error_t sf3d_crop_compute_hour(uint32_t nrCells, const float* airTemperature, const float* relativeHumidity, const float* windIntensity,
                                    const float* globalRadiation, const float* transmissivity, float clearSkyTransmissivity)
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (nrCells != CR.nRows * CR.nCols) return SF3D_PARAMETER_ERROR;
    const float* in[5] = {airTemperature, relativeHumidity, windIntensity, globalRadiation, transmissivity};
    int given = 0;
    for (int k = 0; k < 5; ++k) given += in[k] ? 1 : 0;
    if (given != 0 && given != 5) return SF3D_PARAMETER_ERROR;
    /* (after sf3d_hour_snow the snow hour's inputs are maps of the meteo and radiation blocks: they are gone once one of those is freed) */
    if (given == 0 && !(rasterFeeds(SN, CR.nRows, CR.nCols) && dev().snow_inputs_held(nrCells))) return SF3D_PARAMETER_ERROR;
    return rasterFail("crop compute hour", dev().crop_hour(given ? in : nullptr, clearSkyTransmissivity, CR.flag, mapsOwnedCells(nrCells)));
}

sf3d_error_t sf3d_crop_daily_update(int dateDoy, int currentDoy)
{
    if (!CR.on) return SF3D_MEMORY_ERROR;
    if (dateDoy < 1 || dateDoy > 366 || currentDoy < 1 || currentDoy > 366) return SF3D_PARAMETER_ERROR;
    return rasterFail("crop daily update", dev().crop_day(dateDoy, currentDoy, CR.latitude, CR.flag, mapsOwnedCells((size_t)CR.nRows * CR.nCols)));
}

double sf3d_crop_kernel_ms(int which) { return dev().crop_kernel_ms(which); }

sf3d_error_t sf3d_crop_clean(void)
{
    cropClear();
    return SF3D_OK;
}

} /* extern "C" */
