/*
 * sf3d_multidetrend.h - air and dew-point temperature with MULTIPLE DETRENDING and no sub-option on the MI355X, on the raster of the
 * meteo block (sf3d_meteo.h): what a project with useMultipleDetrending set, and neither local nor glocal detrending, needs of the
 * hour's interpolation - the third arm of Project::interpolationDemMain (agrolib/project/project.cpp:3531-3561), plain interpolationDem:
 *
 *  1. ONE fit over all the call's stations, in call order (preInterpolation -> multipleDetrendingMain,
 *     agrolib/interpolation/interpolation.cpp:2444-2499, 1832-1859): multipleDetrendingElevationFitting(.., isWeighted = true)
 *     (:1862-1953) with every regressionWeight NODATA, which is weight 1, and no minimum of points (the getUseLocalDetrending() rules of
 *     :1885 and :2140 are off); detrendingElevation (:1956-1972) over EVERY point - a point whose height is -9999 was left out of the fit
 *     only, the function of -9999 is subtracted from its value; multipleDetrendingOtherProxiesFitting (:1975-2171), which erases
 *     stations from the list itself (:2038-2069: a first-pass proxy close to -9999, or every first-pass proxy 0); detrendingOtherProxies
 *     (:2173-2236), which erases more.  The prunings CARRY OVER to the interpolation: sf3d_localproxies.h's behaviour on a selection,
 *     not sf3d_glocal.h's, which rebuilds its subsets.
 *  2. the cell loop, interpolationRaster (agrolib/project/interpolationCmd.cpp:354-395).  The cell's float (x, y) is that of
 *     gis::getUtmXYFromRowColSinglePrecision(header, ..) (agrolib/gis/gis.cpp:799-804), which as its parentheses stand is the cell's west
 *     edge + 0.5 m and its north edge - 0.5 m - NOT the centre the loops of sf3d_localproxies.h and sf3d_glocal.h take; the maps are the
 *     reference's at that point.  getProxyValuesXY (:2620-2647: every active proxy, read by Crit3DRasterGrid::getValueFromXY at that
 *     point, gis.cpp:533-546), interpolate(.., excludeSupplemental = true) (:2502-2560) over what 1 left; the Shepard methods get the radius -9999 (no
 *     local radius): sf3d_meteo.h's neighbour search with computeShepardInitialRadius of the kept list's size and boundingBoxArea;
 *     retrend (:1298-1313) over getMultipleDetrendingValues (:2563-2617): a cell that lacks a value of a significant proxy KEEPS its
 *     interpolated value and gets retrend 0 (sf3d_glocal.h sets such a cell to -9999; this path does not); a cell whose interpolate()
 *     gives -9999 stores -9999 and the call still succeeds, as sf3d_meteo_interpolate treats it: no SF3D_MISSING_DATA_ERROR from this
 *     path.  The reference's OpenMP loop is over independent cells: there is no ordering question.
 *  3. points: computeResiduals (agrolib/interpolation/spatialControl.cpp:102-160, behind Project::interpolationCv) and
 *     interpolationOutputPoints (project.cpp:2892-2937) call interpolate(.., excludeSupplemental = false) at a float x, y, z with the
 *     point's own proxy values, over the same kept list with the same fit.  A station evaluated at its own coordinates is in the list at
 *     distance 0: inverseDistanceWeighted skips a distance that is not above EPSILON, the Shepard methods leave it out of their lists.
 *     Stations the prunings erased from the list are still evaluated.
 * The values are the compiled reference's to the bit.
 *
 * Bounds: lists of at most SF3D_METEO_MAX_STATIONS (1 024) stations - the entry point refuses longer lists, the kernels clamp; the
 * height's fit ends after 1 001 iterations per first guess, the proxies' fit after 101; the neighbour search is sf3d_meteo.h's (ten
 * slots); at most SF3D_MULTIDETREND_MAX_POINTS points a call.
 *
 * With the caller: the height's range (setMultipleDetrendingHeightTemperatureRange, preInterpolation :2468-2469), delta and first
 * guesses as in sf3d_localdetrend.h; lapse-rate codes (every station is primary); topographic distance; optimalDetrending; the
 * meteo-grid variant; the station list and its quality control; computeResidualsLocalDetrending / ...GlocalDetrending and the statistics
 * of computeStatisticsCrossValidation (host arithmetic on the residuals).
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The block
 * belongs to the meteo block's raster: sf3d_meteo_initialize comes first, and sf3d_multidetrend_clean, sf3d_meteo_clean, a second
 * sf3d_meteo_initialize and sf3d_clean free what it holds.
 *
 * Errors: SF3D_MEMORY_ERROR no raster (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR see each entry point; SF3D_SOLVER_ERROR a HIP failure
 * (no device).  Every refusal comes before any device work.
 */
#ifndef SF3D_MULTIDETREND_H
#define SF3D_MULTIDETREND_H

#include <stdint.h>

#include "sf3d_localproxies.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF3D_MULTIDETREND_MAX_POINTS (1u << 24)

/* One temperature map.  The stations as in sf3d_localproxies_interpolate: x, y doubles [m]; value floats, not detrended;
 * proxyValues[nProxies][nStations] floats in slot order, -9999 where a station has none.  settings: useMultipleDetrending 1,
 * useLocalDetrending 0, the five other options 0.  fit: sf3d_localdetrend.h's (localdetrend.make_fit); its minPointsLocalDetrending is not
 * read.  boundingBoxArea: getPointsBoundingBoxArea(), which shepardSearchNeighbour reads.  The result lands in the meteo block's slot of
 * the variable and counts as produced there; out may be NULL.
 * SF3D_PARAMETER_ERROR: what sf3d_localproxies_interpolate refuses (with useLocalDetrending set in the place of clear): a variable that
 * is not a temperature, an unknown method or function, more than SF3D_METEO_MAX_STATIONS stations, a NULL array that is read, an x, y or
 * active proxy value that is not finite, a fit table that is not finite, more active proxies than the raster has maps for. */
sf3d_error_t sf3d_multidetrend_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, uint32_t nProxies,
                                           const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings,
                                           const sf3d_localdetrend_fit_t* fit, const sf3d_localproxies_others_t* others, float* out);

/* interpolate() at nPoints float points with the fit and the kept list of the last sf3d_multidetrend_interpolate, whatever other
 * variables were interpolated since: x, y, z as computeResiduals casts them (z is read with topographic distance only: not here, it may
 * be NULL); proxyValues[nProxies][nPoints], nProxies that call's, every slot's value at the point (-9999: none): the station's own for
 * computeResiduals, getProxyValuesXY's for interpolationOutputPoints.  out[nPoints]: -9999 where interpolate() gives it.
 * SF3D_PARAMETER_ERROR: a call before the first sf3d_multidetrend_interpolate (or after what freed the block), more than
 * SF3D_MULTIDETREND_MAX_POINTS points, a NULL array that is read, an x or y that is not finite, a proxy value that is a NaN. */
sf3d_error_t sf3d_multidetrend_points(uint32_t nPoints, const float* x, const float* y, const float* z, const float* proxyValues, float* out);

/* What k_multidetrend_fit recorded of the last call (a NULL array is skipped).  Per station, nStations that call's: detrended (the value
 * the cells interpolate, -9999 where the station is not kept) and stationKept.  Of the call: significant (the height's flag), r2
 * (float(R2), -9999 where no fit ran), parameters[SF3D_LOCALDETREND_MAX_PARAMETERS] (-9999 where the height is not significant);
 * proxySignificant, slope and intercept [SF3D_METEO_MAX_PROXIES] per slot (-9999 where the slot is not a significant other proxy);
 * fitted: the call's stations; kept: what the prunings and detrendingOtherProxies left of them.
 * SF3D_PARAMETER_ERROR: nStations that is not the last call's, a call before the first sf3d_multidetrend_interpolate. */
sf3d_error_t sf3d_multidetrend_get_fit(uint32_t nStations, float* detrended, uint8_t* stationKept, uint8_t* significant, float* r2, double* parameters,
                                       uint8_t* proxySignificant, double* slope, double* intercept, uint32_t* fitted, uint32_t* kept);

/* event-timed duration [ms] of the last launch when sf3d_kernel_timing is on, else 0; which: 0 k_multidetrend_fit, 1 k_multidetrend_cells,
 * 2 k_multidetrend_points */
double sf3d_multidetrend_kernel_ms(int which);

/* device memory the block holds beside the meteo block's [bytes] */
uint64_t sf3d_multidetrend_bytes(void);

sf3d_error_t sf3d_multidetrend_clean(void);

#ifdef __cplusplus
}
#endif

#endif
