/* sf3d_multidetrend_setup.inc - the host side of multiple detrending without areas (included by sf3d_multidetrend_api.inc and by
 * tests/multidetrend_host.cpp, after sf3d_localdetrend_setup.inc, whose call checks and set-up it uses): what
 * sf3d_multidetrend_interpolate, sf3d_multidetrend_points and sf3d_multidetrend_get_fit check before any device work, and the set-up the
 * three kernels share.  No device code: the host program runs it under the sanitizers. */
#include <cmath>
#include <cstdint>

#include "sf3d_multidetrend.h"

/* what the entry points remember of the last sf3d_multidetrend_interpolate */
struct MultiDetrendHost {
    bool done = false;
    uint32_t nStations = 0, nProxies = 0;
};

/* the checks of sf3d_multidetrend_interpolate that need no raster: the method, localCallOk without the height-only rule and without local
 * detrending, proxiesCallOk; fills the proxies of the call as proxiesCallOk does.  noHeight: METEO_MAX_STATIONS zeros */
static inline bool multidetrendCallOk(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, uint32_t nProxies,
                                      const float* proxyValues, const sf3d_meteo_settings_t* settings, const sf3d_localdetrend_fit_t* fit,
                                      const sf3d_localproxies_others_t* others, const float* noHeight, LocalProxiesSetup& ps, const float** rows, const float** height)
{
    if (method < SF3D_METEO_IDW || method > SF3D_METEO_SHEPARD_MODIFIED) return false;
    if (nStations > 0 && !value) return false;
    if (!localCallOk(variable, nStations, x, y, noHeight, settings, fit, false, false)) return false;
    return proxiesCallOk(nStations, nProxies, proxyValues, settings, others, ps, rows, height);
}

/* the checks of sf3d_multidetrend_points: a call before the first interpolate, more points than a float index holds exactly, a NULL
 * array that is read, an x or y that is not finite, a proxy value that is a NaN */
static inline bool multidetrendPointsOk(const MultiDetrendHost& M, uint32_t nPoints, const float* x, const float* y, const float* proxyValues, const float* out)
{
    if (!M.done || nPoints > SF3D_MULTIDETREND_MAX_POINTS) return false;
    if (nPoints == 0) return true;
    if (!x || !y || !out || (M.nProxies > 0 && !proxyValues)) return false;
    for (uint32_t i = 0; i < nPoints; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i])) return false;
    for (size_t k = 0; k < (size_t)M.nProxies * nPoints; ++k)
        if (std::isnan(proxyValues[k])) return false;
    return true;
}

/* the check of sf3d_multidetrend_get_fit */
static inline bool multidetrendGetOk(const MultiDetrendHost& M, uint32_t nStations) { return M.done && nStations == M.nStations; }

/* the set-up the fit, every cell and every point of a call share: localSetup's table, neither minimum-points rule (the
 * getUseLocalDetrending() rules of interpolation.cpp:1885 and :2140 are off) */
static inline void multidetrendSetup(const sf3d_localdetrend_fit_t* fit, uint32_t nStations, float boundingBoxArea, double* table, LocalDetrendSetup& s)
{
    sf3d_localdetrend_fit_t own = *fit;
    own.minPointsLocalDetrending = 1;                                           /* not read of the caller's; the selection's numbers are not used */
    localSetup(&own, nStations ? nStations : 1u, boundingBoxArea, table, s);
    s.minPointsLocal = 0; s.minPoints = 0; s.minPointsStep = 0; s.radiusAll = 0.f;
}
