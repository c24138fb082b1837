/* part of sf3d_api.cpp (included after sf3d_localdetrend_api.inc, whose call checks and set-up it uses) - the C entry points of
 * include/sf3d_localproxies.h.  The host checks the call against the scope of the block before any device work and lays the active
 * proxies out as the kernel reads them (proxiesCallOk of sf3d_localdetrend_setup.inc); everything else lives on the device
 * (sf3d_localproxies.inc). */
#include "sf3d_localproxies.h"

static_assert(SF3D_LOCALPROXIES_MAX_OTHERS == LOCALPROXIES_MAX_OTHERS && SF3D_LOCALPROXIES_MAX_OTHERS == SF3D_METEO_MAX_PROXIES - 1,
              "sf3d_localproxies.h and sf3d_device.h disagree");
static_assert(sizeof(sf3d_localproxies_proxy_t) == 40 && sizeof(sf3d_localproxies_others_t) == 40 * SF3D_METEO_MAX_PROXIES, "sf3d_localproxies_others_t has no padding");

extern "C" {

sf3d_error_t sf3d_localproxies_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, uint32_t nProxies,
                                           const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings, const sf3d_localdetrend_fit_t* fit,
                                           const sf3d_localproxies_others_t* others, float* out)
{
    static const float noHeight[SF3D_METEO_MAX_STATIONS] = {0.f};       /* the height is not active: its row is read by the selection, never used */
    if (!localCallOk(variable, nStations, x, y, noHeight, settings, fit, false)) return SF3D_PARAMETER_ERROR;
    LocalProxiesCall local{};
    if (!proxiesCallOk(nStations, nProxies, proxyValues, settings, others, local.proxies, local.rows, &local.height)) return SF3D_PARAMETER_ERROR;
    if (!local.height) local.height = noHeight;
    /* the rest of the call is sf3d_meteo_interpolate's, which knows neither option */
    sf3d_meteo_settings_t plain = *settings;
    plain.useMultipleDetrending = 0; plain.useLocalDetrending = 0;
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, &plain, false, call);
    if (e != SF3D_OK) return e;
    /* getProxyValuesXY reads a raster per active proxy; the height's may be the DEM itself */
    for (int r = 0; r < local.proxies.nOthers; ++r)
        if (!dev().meteo_has_map((uint32_t)local.proxies.slot[r])) return SF3D_PARAMETER_ERROR;
    double table[LOCALDETREND_TABLE_DOUBLES] = {0.};
    local.table = table;
    localSetup(fit, nStations, boundingBoxArea, table, local.setup);
    return rasterFail("localproxies interpolate", dev().localproxies_interpolate(call, local, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
}

sf3d_error_t sf3d_localproxies_get_interpolated(uint32_t nrCells, uint32_t* count)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != MT.nRows * MT.nCols || !dev().localproxies_done()) return SF3D_PARAMETER_ERROR;
    return rasterFail("localproxies get interpolated", dev().localproxies_interpolated(count));
}

sf3d_error_t sf3d_localproxies_get_proxy_fit(uint32_t nrCells, uint8_t* significant, double* slope, double* intercept)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (nrCells != MT.nRows * MT.nCols || !dev().localproxies_done()) return SF3D_PARAMETER_ERROR;
    /* the device holds (slope, intercept) pairs */
    std::vector<double> lines((slope || intercept) ? (size_t)nrCells * SF3D_METEO_MAX_PROXIES * 2 : 0);
    const sf3d_error_t e = dev().localproxies_fit(significant, lines.empty() ? nullptr : lines.data());
    if (e != SF3D_OK) return rasterFail("localproxies get proxy fit", e);
    for (size_t k = 0; k < lines.size() / 2; ++k) {
        if (slope) slope[k] = lines[2 * k];
        if (intercept) intercept[k] = lines[2 * k + 1];
    }
    return SF3D_OK;
}

double sf3d_localproxies_kernel_ms(void) { return dev().localproxies_kernel_ms(); }

uint64_t sf3d_localproxies_bytes(void) { return MT.on ? dev().localproxies_bytes() : 0; }

sf3d_error_t sf3d_localproxies_clean(void)
{
    (void)dev().localproxies_free();
    return SF3D_OK;
}

} /* extern "C" */
