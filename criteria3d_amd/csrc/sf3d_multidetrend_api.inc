/* part of sf3d_api.cpp (included after sf3d_glocal_api.inc; it uses the call checks and the set-up of sf3d_localdetrend_setup.inc) - the
 * C entry points of include/sf3d_multidetrend.h.  The host checks every call before any device work (sf3d_multidetrend_setup.inc) and
 * lays the active proxies out as the kernels read them; everything else lives on the device (sf3d_multidetrend.inc). */
#include "sf3d_multidetrend.h"
#include "sf3d_multidetrend_setup.inc"

static_assert(sizeof(MultiDetrendRecord) == 200, "MultiDetrendRecord has no padding");

namespace {

MultiDetrendHost MD;

void multidetrendHostClear() { MD = MultiDetrendHost(); }

}  // namespace

extern "C" {

sf3d_error_t sf3d_multidetrend_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, uint32_t nProxies,
                                           const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings,
                                           const sf3d_localdetrend_fit_t* fit, const sf3d_localproxies_others_t* others, float* out)
{
    static const float noHeight[SF3D_METEO_MAX_STATIONS] = {0.f};       /* the height is not active: its row is never used */
    MultiDetrendCall g{};
    if (!multidetrendCallOk(variable, method, nStations, x, y, value, nProxies, proxyValues, settings, fit, others, noHeight, g.proxies, g.rows, &g.height))
        return SF3D_PARAMETER_ERROR;
    if (!g.height) g.height = noHeight;
    /* the rest of the call is sf3d_meteo_interpolate's, which knows neither option */
    sf3d_meteo_settings_t plain = *settings;
    plain.useMultipleDetrending = 0; plain.useLocalDetrending = 0;
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, &plain, false, call);
    if (e != SF3D_OK) return e;
    /* getProxyValuesXY reads a raster per active proxy; the height's may be the DEM itself */
    for (int r = 0; r < g.proxies.nOthers; ++r)
        if (!dev().meteo_has_map((uint32_t)g.proxies.slot[r])) return SF3D_PARAMETER_ERROR;
    double table[LOCALDETREND_TABLE_DOUBLES] = {0.};
    g.table = table;
    multidetrendSetup(fit, nStations, boundingBoxArea, table, g.setup);
    multidetrendHostClear();
    const sf3d_error_t done = rasterFail("multidetrend interpolate", dev().multidetrend_interpolate(call, g, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
    if (done == SF3D_OK) { MD.done = true; MD.nStations = nStations; MD.nProxies = nProxies; }
    return done;
}

sf3d_error_t sf3d_multidetrend_points(uint32_t nPoints, const float* x, const float* y, const float* z, const float* proxyValues, float* out)
{
    (void)z;                                                             /* computeDistances reads it with topographic distance only */
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!multidetrendPointsOk(MD, nPoints, x, y, proxyValues, out) || !dev().multidetrend_done()) return SF3D_PARAMETER_ERROR;
    return rasterFail("multidetrend points", dev().multidetrend_points(nPoints, MD.nProxies, x, y, proxyValues, out));
}

sf3d_error_t sf3d_multidetrend_get_fit(uint32_t nStations, float* detrended, uint8_t* stationKept, uint8_t* significant, float* r2, double* parameters,
                                       uint8_t* proxySignificant, double* slope, double* intercept, uint32_t* fitted, uint32_t* kept)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!multidetrendGetOk(MD, nStations) || !dev().multidetrend_done()) return SF3D_PARAMETER_ERROR;
    MultiDetrendRecord o{};
    LocalProxiesSetup ps{};
    const sf3d_error_t e = dev().multidetrend_records(&o, detrended, stationKept, &ps);
    if (e != SF3D_OK) return rasterFail("multidetrend get fit", e);
    const int S = SF3D_METEO_MAX_PROXIES, P = SF3D_LOCALDETREND_MAX_PARAMETERS;
    if (significant) *significant = (uint8_t)(o.significant != 0);
    if (r2) *r2 = o.r2;
    if (fitted) *fitted = o.fitted;
    if (kept) *kept = o.kept;
    for (int j = 0; parameters && j < P; ++j) parameters[j] = o.parameters[j];
    for (int p = 0; p < S; ++p) {
        if (proxySignificant) proxySignificant[p] = 0;
        if (slope) slope[p] = -9999.;
        if (intercept) intercept[p] = -9999.;
    }
    /* the device packs the lines of the significant other proxies in slot order */
    int j = 0;
    for (int r = 0; r < ps.nOthers; ++r) {
        if (!((o.mask >> r) & 1u)) continue;
        const int at = ps.slot[r];
        if (proxySignificant) proxySignificant[at] = 1;
        if (slope) slope[at] = o.line[j][0];
        if (intercept) intercept[at] = o.line[j][1];
        ++j;
    }
    return SF3D_OK;
}

double sf3d_multidetrend_kernel_ms(int which) { return dev().multidetrend_kernel_ms(which); }

uint64_t sf3d_multidetrend_bytes(void) { return MT.on ? dev().multidetrend_bytes() : 0; }

sf3d_error_t sf3d_multidetrend_clean(void)
{
    multidetrendHostClear();
    (void)dev().multidetrend_free();
    return SF3D_OK;
}

} /* extern "C" */
