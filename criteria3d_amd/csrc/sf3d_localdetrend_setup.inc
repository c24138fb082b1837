/* sf3d_localdetrend_setup.inc - the host side of a local-detrending call (included by sf3d_localdetrend_api.inc, which
 * sf3d_localproxies_api.inc follows, and by tests/localdetrend_host.cpp and tests/localproxies_host.cpp): what
 * sf3d_localdetrend_interpolate and sf3d_localproxies_interpolate fix before any device work - the numbers every cell shares, among them
 * the one that needs the C library's sqrt (the radius of localSelection where every station is selected), the fit's ranges and first
 * guesses as the table the kernels read, and the active proxies as k_localdetrend_proxies reads them: the height's slot, the other proxies
 * in slot order with their station rows, ranges and thresholds.  No device code: the host programs run it under the sanitizers. */
#include <cmath>
#include <cstdint>

#include "sf3d_device.h"
#include "sf3d_localproxies.h"

/* the number of parameters of a function, 0: unknown */
static inline int localParameters(int function)
{
    return function == SF3D_LOCALDETREND_PIECEWISE_TWO ? 4 : function == SF3D_LOCALDETREND_PIECEWISE_THREE_FREE ? 6 : function == SF3D_LOCALDETREND_PIECEWISE_THREE ? 5 : 0;
}

/* what the call fixes for every cell beside the table; the host programs, whose input holds the table laid out, call this alone */
static inline void localNumbers(int function, int nFirstGuess, int minPointsLocalDetrending, float stdDevThreshold, uint32_t nStations, float boundingBoxArea,
                                LocalDetrendSetup& s)
{
    s.function = function; s.nFirstGuess = nFirstGuess; s.minPointsLocal = minPointsLocalDetrending;
    s.minPoints = unsigned(minPointsLocalDetrending * 1.2f);                /* interpolation.cpp:1092-1093 */
    s.minPointsStep = unsigned(s.minPoints * 0.8);                          /* :1150 */
    s.stdDevThreshold = stdDevThreshold; s.area = boundingBoxArea;
    /* computeShepardInitialRadius(area, N, minPoints), :1098 with :800-803 */
    s.radiusAll = float(std::sqrt((s.minPoints * boundingBoxArea) / (float(3.1415926535898) * nStations)));
}

/* the table the kernel reads (LOCALDETREND_TABLE_DOUBLES doubles, zeroed by the caller) and what the call fixes for every cell */
static inline void localSetup(const sf3d_localdetrend_fit_t* fit, uint32_t nStations, float boundingBoxArea, double* table, LocalDetrendSetup& s)
{
    const int P = SF3D_LOCALDETREND_MAX_PARAMETERS;
    for (int j = 0; j < fit->nParameters; ++j) {
        table[j] = fit->parametersMin[j]; table[P + j] = fit->parametersMax[j]; table[2 * P + j] = fit->parametersDelta[j];
        for (int k = 0; k < fit->nFirstGuess; ++k) table[(3 + k) * P + j] = fit->firstGuess[k][j];
    }
    localNumbers(fit->function, fit->nFirstGuess, fit->minPointsLocalDetrending, fit->stdDevThreshold, nStations, boundingBoxArea, s);
}

/* the checks of a call that need no raster; heightOnly: the proxy rule of sf3d_localdetrend.h (proxiesCallOk below has its own); local: local
 * detrending - without it (sf3d_glocal.h) useLocalDetrending must be 0 and minPointsLocalDetrending is not read */
static inline bool localCallOk(int variable, uint32_t nStations, const double* x, const double* y, const float* height, const sf3d_meteo_settings_t* settings,
                 const sf3d_localdetrend_fit_t* fit, bool heightOnly = true, bool local = true)
{
    if (!settings || !fit) return false;
    if (variable != SF3D_METEO_AIR_TEMPERATURE && variable != SF3D_METEO_AIR_DEW_TEMPERATURE) return false;     /* getUseDetrendingVar, project.cpp:3160 */
    if (!settings->useMultipleDetrending || (settings->useLocalDetrending != 0) != local) return false;
    if (settings->useTopographicDistance || settings->useKriging || settings->useSupplementalStations || settings->useCrossValidationIndex || settings->updateMinMax)
        return false;
    if (settings->nProxies < 0 || settings->nProxies > SF3D_METEO_MAX_PROXIES) return false;
    int active = 0;
    for (int p = 0; heightOnly && p < settings->nProxies; ++p) {
        if (!settings->proxy[p].active) continue;
        if (!settings->proxy[p].isHeight) return false;
        ++active;
    }
    if (heightOnly && active != 1) return false;
    const int np = localParameters(fit->function);
    if (np == 0 || fit->nParameters != np) return false;
    if (fit->nFirstGuess < 1 || fit->nFirstGuess > SF3D_LOCALDETREND_MAX_FIRST_GUESS || (local && fit->minPointsLocalDetrending < 1)) return false;
    if (std::isnan(fit->stdDevThreshold)) return false;
    for (int j = 0; j < np; ++j) {
        if (!std::isfinite(fit->parametersMin[j]) || !std::isfinite(fit->parametersMax[j]) || !std::isfinite(fit->parametersDelta[j])) return false;
        for (int k = 0; k < fit->nFirstGuess; ++k)
            if (!std::isfinite(fit->firstGuess[k][j])) return false;
    }
    if (nStations > SF3D_METEO_MAX_STATIONS || (nStations > 0 && (!x || !y || !height))) return false;
    for (uint32_t k = 0; k < nStations; ++k)
        if (!std::isfinite(x[k]) || !std::isfinite(y[k]) || !std::isfinite(height[k])) return false;
    return true;
}

/* the checks of sf3d_localproxies_interpolate that need no raster, beyond localCallOk's; fills the proxies of the call: rows[r] is the
 * station row of ps.slot[r], *height the active height's row (nullptr: the height is not active) */
static inline bool proxiesCallOk(uint32_t nStations, uint32_t nProxies, const float* proxyValues, const sf3d_meteo_settings_t* settings,
                                 const sf3d_localproxies_others_t* others, LocalProxiesSetup& ps, const float** rows, const float** height)
{
    if (!others || nProxies != (uint32_t)settings->nProxies || (nStations > 0 && nProxies > 0 && !proxyValues)) return false;
    int heights = 0;
    ps.heightSlot = -1; ps.nOthers = 0;
    *height = nullptr;
    for (int p = 0; p < settings->nProxies; ++p) {
        const float* row = proxyValues ? proxyValues + (size_t)p * nStations : nullptr;
        if (settings->proxy[p].isHeight) {
            if (++heights > 1) return false;
            if (settings->proxy[p].active) { ps.heightSlot = p; *height = row; }
        }
        if (!settings->proxy[p].active) continue;
        for (uint32_t k = 0; k < nStations; ++k)
            if (!std::isfinite(row[k])) return false;
        if (settings->proxy[p].isHeight) continue;
        if (ps.nOthers == SF3D_LOCALPROXIES_MAX_OTHERS) return false;
        const sf3d_localproxies_proxy_t& o = others->proxy[p];
        if (std::isnan(o.stdDevThreshold)) return false;
        for (int t = 0; t < 2; ++t) {
            if (!std::isfinite(o.min[t]) || !std::isfinite(o.max[t]) || o.min[t] > o.max[t]) return false;
            ps.range[ps.nOthers][t] = o.min[t]; ps.range[ps.nOthers][2 + t] = o.max[t];
        }
        ps.stdDevThreshold[ps.nOthers] = o.stdDevThreshold;
        ps.slot[ps.nOthers] = p;
        rows[ps.nOthers] = row;
        ++ps.nOthers;
    }
    return true;
}
