/* part of sf3d_api.cpp (included at its end, after the root entry points) - the C entry points of include/sf3d_meteo.h.  The host keeps the
 * raster's size, checks the call against the caps and the options that stay with the caller, and evaluates what needs the C library's sqrt
 * (computeShepardInitialRadius, once per call); everything else lives on the device (sf3d_meteo.inc). */
#include <cmath>

#include "sf3d_meteo.h"

static_assert(sizeof(sf3d_meteo_proxy_t) == sizeof(MeteoProxyDev) && sizeof(MeteoProxyDev) == 32, "the proxy table is copied as it is");
static_assert(sizeof(sf3d_meteo_settings_t) == 48 + 32 * SF3D_METEO_MAX_PROXIES, "sf3d_meteo_settings_t has no padding");
static_assert(SF3D_METEO_MAX_STATIONS == METEO_MAX_STATIONS && SF3D_METEO_MAX_PROXIES == METEO_MAX_PROXIES && SF3D_METEO_VARIABLES == METEO_VARIABLES,
              "sf3d_meteo.h and sf3d_device.h disagree");

namespace {

struct MeteoHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0, nProxies = 0;
    double xll = 0., yll = 0., cellSize = 0.;      /* the header: what sf3d_topodist_api.inc bounds a walk with */
} MT;

void topoHostClear();                          /* sf3d_topodist_api.inc: the topographic distance maps go with their raster */
void glocalHostClear();                        /* sf3d_glocal_api.inc: so do the macro areas */
void multidetrendHostClear();                  /* sf3d_multidetrend_api.inc: and the one fit of the last call */

void meteoClear() { MT = MeteoHost(); topoHostClear(); glocalHostClear(); multidetrendHostClear(); (void)dev().meteo_free(); }

/* computeShepardInitialRadius(area, nrPoints, SHEPARD_AVG_NRPOINTS), interpolation.cpp:800-803: float products, PI of commonConstants.h:249 */
float meteoInitialRadius(float area, uint32_t allPointsNr)
{
    const unsigned minPointsNr = 8;
    return float(std::sqrt((minPointsNr * area) / (float(3.1415926535898) * allPointsNr)));
}

/* the checks of a call and what the device needs of it: sf3d_meteo_interpolate, and sf3d_topodist_interpolate (sf3d_topodist_api.inc),
 * the one caller that may set useTopographicDistance */
sf3d_error_t meteoPrepare(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, float boundingBoxArea,
                          const sf3d_meteo_settings_t* settings, bool topographicDistance, MeteoCall& call)
{
    /* the checks that need no raster come first: a caller learns of an unsupported option before it has one */
    if (variable < 0 || variable >= SF3D_METEO_VARIABLES || method < SF3D_METEO_IDW || method > SF3D_METEO_SHEPARD_MODIFIED || !settings) return SF3D_PARAMETER_ERROR;
    if (nStations > SF3D_METEO_MAX_STATIONS || (nStations > 0 && (!x || !y || !value))) return SF3D_PARAMETER_ERROR;
    if (settings->nProxies < 0 || settings->nProxies > SF3D_METEO_MAX_PROXIES) return SF3D_PARAMETER_ERROR;
    if (settings->useMultipleDetrending || settings->useLocalDetrending || (settings->useTopographicDistance && !topographicDistance) || settings->useKriging ||
        settings->useSupplementalStations || settings->useCrossValidationIndex || settings->updateMinMax) return SF3D_PARAMETER_ERROR;
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if ((uint32_t)settings->nProxies > MT.nProxies) return SF3D_PARAMETER_ERROR;
    call = MeteoCall{};
    call.x = x; call.y = y; call.value = value;
    call.nStations = nStations; call.nProxies = (uint32_t)settings->nProxies;
    call.var = variable; call.method = method; call.allZero = settings->allZero != 0; call.useDetrending = settings->useDetrending != 0;
    call.detrendingVar = variable == SF3D_METEO_AIR_TEMPERATURE || variable == SF3D_METEO_AIR_DEW_TEMPERATURE;      /* getUseDetrendingVar */
    call.radius0 = meteoInitialRadius(boundingBoxArea, nStations);
    call.rainfallThreshold = settings->rainfallThreshold;
    for (int p = 0; p < settings->nProxies; ++p) std::memcpy(&call.proxy[p], &settings->proxy[p], sizeof(MeteoProxyDev));
    return SF3D_OK;
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_meteo_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double xllCorner, double yllCorner, double cellSize,
                                   uint32_t nProxies, const float* const* proxyMaps)
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !(cellSize > 0)) return SF3D_PARAMETER_ERROR;
    if (nProxies > SF3D_METEO_MAX_PROXIES || (nProxies > 0 && !proxyMaps)) return SF3D_PARAMETER_ERROR;
    meteoClear();
    const sf3d_error_t e = dev().meteo_alloc(nrRows, nrCols, dem, flag, xllCorner, yllCorner, cellSize, nProxies, proxyMaps);
    if (e != SF3D_OK) { rasterFail("meteo initialize", e); meteoClear(); return e; }
    MT.nRows = nrRows; MT.nCols = nrCols; MT.nProxies = nProxies;
    MT.xll = xllCorner; MT.yll = yllCorner; MT.cellSize = cellSize;
    MT.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_meteo_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, float boundingBoxArea,
                                    const sf3d_meteo_settings_t* settings, float* out)
{
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, settings, false, call);
    if (e != SF3D_OK) return e;
    return rasterFail("meteo interpolate", dev().meteo_interpolate(call, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
}

sf3d_error_t sf3d_meteo_get_map(int variable, uint32_t nrCells, float* map)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (variable < 0 || variable >= SF3D_METEO_VARIABLES || !map || nrCells != MT.nRows * MT.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("meteo get map", dev().meteo_download(variable, map));
}

sf3d_error_t sf3d_meteo_set_map(int variable, uint32_t nrCells, const float* map)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (variable < 0 || variable >= SF3D_METEO_VARIABLES || !map || nrCells != MT.nRows * MT.nCols) return SF3D_PARAMETER_ERROR;
    return rasterFail("meteo set map", dev().meteo_upload(variable, map));
}

double sf3d_meteo_kernel_ms(void) { return dev().meteo_kernel_ms(); }

sf3d_error_t sf3d_meteo_clean(void)
{
    meteoClear();
    return SF3D_OK;
}

} /* extern "C" */
