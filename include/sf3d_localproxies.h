/*
 * sf3d_localproxies.h - air and dew-point temperature with local detrending and EVERY active proxy on the MI355X, on the raster of the
 * meteo block (sf3d_meteo.h): what a project with useLocalDetrending and useMultipleDetrending set and more than the height in its proxy
 * list (sea distance, orographic index, urban fraction, water index ...) needs of the hour's interpolation.  sf3d_localdetrend.h is the
 * same block for the height alone.  For every DEM cell, as the cell loop of Project::interpolationDemLocalDetrending does
 * (agrolib/project/project.cpp:3226-3254):
 *
 *  - getProxyValuesXY (agrolib/interpolation/interpolation.cpp:2620-2647): the cell's value of every active proxy from the rasters of
 *    sf3d_meteo_initialize (the DEM for a height proxy without a raster), NODATA where it equals the flag;
 *  - localSelection and, with the height active, multipleDetrendingElevationFitting and detrendingElevation: as sf3d_localdetrend.h;
 *  - multipleDetrendingOtherProxiesFitting (:1975-2171): proxyValidity per other active proxy, the two prunings (a station leaves the
 *    interpolated list for a NODATA significant value or when all its significant values are 0, the fit list only for the NODATA), the
 *    second validity pass over the pruned fit list, the minimum of fit points, setFittingParameters_otherProxies (:1680-1728) and the
 *    weighted bestFittingMarquardt_nDimension(&functionSum, ..., 100, 0.005, ...) of functionLinear_intercept per significant proxy
 *    (agrolib/mathFunctions/furtherMathFunctions.cpp:1535-1580 over :1740-1947);
 *  - detrendingOtherProxies (:2173-2236), interpolate() over what is left of the list, retrend through getMultipleDetrendingValues
 *    (:1298-1313, :2563-2617): 0 where the cell's value of any significant proxy is NODATA.
 * The values are the reference's to the bit (tests/golden/localproxies.npz: a pin of the compiled reference).
 *
 * With the caller: what sf3d_localdetrend.h leaves there except the other proxies - the point list, the height's range, delta and first
 * guesses, lapse-rate codes (every station is primary), output points.  multipleDetrending without localDetrending is
 * sf3d_multidetrend.h.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The block
 * belongs to the meteo block's raster: sf3d_meteo_initialize comes first, and sf3d_localproxies_clean, sf3d_meteo_clean, a second
 * sf3d_meteo_initialize and sf3d_clean free what it holds.
 *
 * Errors: SF3D_MEMORY_ERROR no raster (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR what sf3d_localdetrend.h refuses except its proxy
 * rule, and: more than SF3D_LOCALPROXIES_MAX_OTHERS active proxies that are not the height, two height proxies, an active proxy that is
 * not the height in a slot for which the meteo block holds no raster, nProxies that is not settings->nProxies, a range with min > max or
 * a non-finite value, a NaN threshold, a non-finite proxy value (-9999 is a value), a getter before the first call; SF3D_SOLVER_ERROR a
 * HIP failure (no device).  Every refusal comes before any device work.
 */
#ifndef SF3D_LOCALPROXIES_H
#define SF3D_LOCALPROXIES_H

#include <stdint.h>

#include "sf3d_localdetrend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF3D_LOCALPROXIES_MAX_OTHERS 7          /* every slot of sf3d_meteo_settings_t beside the height's */

/* what multipleDetrendingOtherProxiesFitting reads of a proxy, per slot of settings->proxy[]: min, max: the two halves of
 * getFittingParametersRange() (slope, intercept); stdDevThreshold: getStdDevThreshold() (-9999: none).  The slots of the height and of
 * proxies that are not active are not read. */
typedef struct {
    double min[2];
    double max[2];
    float stdDevThreshold;
    int32_t reserved;
} sf3d_localproxies_proxy_t;

typedef struct {
    sf3d_localproxies_proxy_t proxy[SF3D_METEO_MAX_PROXIES];
} sf3d_localproxies_others_t;

/* As sf3d_localdetrend_interpolate, with proxyValues in the place of height: [nProxies][nStations] floats, getProxyValue(pos) in the slot
 * order of settings->proxy[] and of sf3d_meteo_initialize (nProxies == settings->nProxies), -9999 where a station has none; the row of
 * a proxy that is not active is not read.  settings: useMultipleDetrending and useLocalDetrending 1, the five other options 0, at most
 * one proxy with isHeight, any subset active.  fit: sf3d_localdetrend.h's, checked as there; when the height is not active only its
 * minPointsLocalDetrending is used (localSelection and the minimum of fit points read it).  The result lands in the meteo block's slot of
 * the variable and counts as produced.  After the call sf3d_localdetrend_get_fit and sf3d_localdetrend_get_selection return the
 * elevation's outcome and the selection of this call (count: the selected count). */
sf3d_error_t sf3d_localproxies_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, uint32_t nProxies,
                                           const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings, const sf3d_localdetrend_fit_t* fit,
                                           const sf3d_localproxies_others_t* others, float* out);

/* per cell the number of stations interpolated after the prunings (the selected count where nothing was pruned).  A cell outside the
 * DEM or of another rank: 0. */
sf3d_error_t sf3d_localproxies_get_interpolated(uint32_t nrCells, uint32_t* count);

/* per cell and proxy slot (nrCells x SF3D_METEO_MAX_PROXIES each; a NULL array is skipped): isProxySignificant of a proxy that is not the
 * height, and its fitted slope and intercept, -9999 where it is not significant (the height's slot included: its fit is
 * sf3d_localdetrend_get_fit's), outside the DEM and on another rank's cells. */
sf3d_error_t sf3d_localproxies_get_proxy_fit(uint32_t nrCells, uint8_t* significant, double* slope, double* intercept);

/* event-timed duration [ms] of the last k_localdetrend_proxies launch when sf3d_kernel_timing is on, else 0 */
double sf3d_localproxies_kernel_ms(void);

/* device memory the block holds beside the meteo block's and sf3d_localdetrend_bytes() [bytes] */
uint64_t sf3d_localproxies_bytes(void);

sf3d_error_t sf3d_localproxies_clean(void);

#ifdef __cplusplus
}
#endif

#endif
