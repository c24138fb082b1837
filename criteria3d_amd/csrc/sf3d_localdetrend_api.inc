/* part of sf3d_api.cpp (included after sf3d_topodist_api.inc; it uses the raster and the call checks of sf3d_meteo_api.inc) - the C entry
 * points of include/sf3d_localdetrend.h.  The host checks the call against the scope of the block before any device work and sets it up
 * with sf3d_localdetrend_setup.inc (the table the kernel reads, the numbers every cell shares); the selection, the fits and the
 * interpolation live on the device (sf3d_localdetrend.inc). */
#include "sf3d_localdetrend.h"
#include "sf3d_localdetrend_setup.inc"

static_assert(SF3D_LOCALDETREND_MAX_PARAMETERS == LOCALDETREND_MAX_PARAMETERS && SF3D_LOCALDETREND_MAX_FIRST_GUESS == LOCALDETREND_MAX_FIRST_GUESS,
              "sf3d_localdetrend.h and sf3d_device.h disagree");
static_assert(sizeof(sf3d_localdetrend_fit_t) == 24 + (3 + SF3D_LOCALDETREND_MAX_FIRST_GUESS) * SF3D_LOCALDETREND_MAX_PARAMETERS * sizeof(double),
              "sf3d_localdetrend_fit_t has no padding");

extern "C" {

sf3d_error_t sf3d_localdetrend_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* height, const float* value,
                                           float boundingBoxArea, const sf3d_meteo_settings_t* settings, const sf3d_localdetrend_fit_t* fit, float* out)
{
    if (!localCallOk(variable, nStations, x, y, height, settings, fit)) return SF3D_PARAMETER_ERROR;
    /* the rest of the call is sf3d_meteo_interpolate's, which knows neither option */
    sf3d_meteo_settings_t plain = *settings;
    plain.useMultipleDetrending = 0; plain.useLocalDetrending = 0;
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, &plain, false, call);
    if (e != SF3D_OK) return e;
    double table[LOCALDETREND_TABLE_DOUBLES] = {0.};
    LocalDetrendCall local{};
    local.table = table; local.height = height;
    localSetup(fit, nStations, boundingBoxArea, table, local.setup);
    return rasterFail("localdetrend interpolate", dev().localdetrend_interpolate(call, local, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
}

sf3d_error_t sf3d_localdetrend_get_fit(uint32_t nrCells, uint8_t* significant, float* r2, double* parameters)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != MT.nRows * MT.nCols || !dev().localdetrend_done()) return SF3D_PARAMETER_ERROR;
    return rasterFail("localdetrend get fit", dev().localdetrend_fit(significant, r2, parameters));
}

sf3d_error_t sf3d_localdetrend_get_selection(uint32_t nrCells, uint32_t* count, float* radius)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != MT.nRows * MT.nCols || !dev().localdetrend_done()) return SF3D_PARAMETER_ERROR;
    return rasterFail("localdetrend get selection", dev().localdetrend_selection(count, radius));
}

double sf3d_localdetrend_kernel_ms(void) { return dev().localdetrend_kernel_ms(); }

uint64_t sf3d_localdetrend_bytes(void) { return MT.on ? dev().localdetrend_bytes() : 0; }

sf3d_error_t sf3d_localdetrend_clean(void)
{
    (void)dev().localdetrend_free();
    return SF3D_OK;
}

} /* extern "C" */
