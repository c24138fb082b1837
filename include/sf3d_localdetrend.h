/*
 * sf3d_localdetrend.h - air and dew-point temperature with local detrending on the MI355X, on the raster of the meteo block
 * (sf3d_meteo.h): what a project with useLocalDetrending and useMultipleDetrending set needs of the hour's interpolation.  For every DEM
 * cell, as the cell loop of Project::interpolationDemLocalDetrending does (agrolib/project/project.cpp:3226-3254):
 *
 *  - localSelection (agrolib/interpolation/interpolation.cpp:1087-1170): the stations around the cell, in rings of 7 500 m and then
 *    1 000 m, with their regression weights and the local radius; every station where there are no more than
 *    unsigned(minPointsLocalDetrending * 1.2f) of them;
 *  - multipleDetrendingMain (:1832-1859) with the height proxy as the only active proxy: proxyValidity (:1418-1457) and the minimum of
 *    elevation points (:1885), the weighted bestFittingMarquardt_nDimension over the caller's first-guess combinations
 *    (agrolib/mathFunctions/furtherMathFunctions.cpp:1360-1427 over :1954-2118, maxIterationsNr 1000, myEpsilon 0.002, deltaR2 0.005)
 *    of lapseRatePiecewise_two, _three or _three_free (:115-179), the significance rule (:1939) and detrendingElevation (:1956-1972);
 *  - interpolate() (:2502-2560) over the selected stations: inverseDistanceWeighted, shepardIdw, or modifiedShepardIdw with the local
 *    radius handed in (:961-965), then retrend with the cell's own parameters (:1298-1313).
 * The values are the reference's to the bit (tests/golden/localdetrend.npz: a pin of the compiled reference).
 *
 * With the caller: the point list (quality control, checkAndPassDataToInterpolation); the parameter range after
 * setMultipleDetrendingHeightTemperatureRange (:1506-1553), parametersDelta = (max - min) / 800 (:1671) and the list of
 * calculateFirstGuessCombinations (:1556-1622) - criteria3d_amd/localdetrend.py restates the three; other proxies (sf3d_localproxies.h
 * is this block with every active proxy; sf3d_glocal.h is glocal detrending, sf3d_multidetrend.h multiple detrending with neither), lapse-rate codes (every station is primary), output points; and everything
 * sf3d_meteo.h leaves with the caller.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The block
 * belongs to the meteo block's raster: sf3d_meteo_initialize comes first, and sf3d_localdetrend_clean, sf3d_meteo_clean, a second
 * sf3d_meteo_initialize and sf3d_clean free what it holds.
 *
 * Errors: SF3D_MEMORY_ERROR no raster (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR null pointer, a variable other than the two
 * temperatures, an unknown method, useMultipleDetrending or useLocalDetrending not set, any of the five other options of
 * sf3d_meteo_settings_t set, more than one active proxy or an active proxy that is not the height, an unknown function or a parameter count
 * that is not the function's, no or too many first-guess combinations, minPointsLocalDetrending < 1, too many stations, a non-finite
 * coordinate, height or fit value, a map size (nrCells) that is not the raster's, a getter before the first call; SF3D_SOLVER_ERROR a HIP
 * failure (no device).  Every refusal comes before any device work.
 */
#ifndef SF3D_LOCALDETREND_H
#define SF3D_LOCALDETREND_H

#include <stdint.h>

#include "sf3d_meteo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF3D_LOCALDETREND_MAX_PARAMETERS 6      /* lapseRatePiecewise_three_free */
#define SF3D_LOCALDETREND_MAX_FIRST_GUESS 31    /* the most calculateFirstGuessCombinations produces */

/* TFittingFunction (interpolationConstants.h:41) with the number of parameters of each: 4, 6, 5 */
enum { SF3D_LOCALDETREND_PIECEWISE_TWO = 0, SF3D_LOCALDETREND_PIECEWISE_THREE_FREE = 1, SF3D_LOCALDETREND_PIECEWISE_THREE = 2 };

/* what multipleDetrendingElevationFitting reads of the height proxy and the settings.  parametersMin / Max: getFittingParametersRange()
 * after setMultipleDetrendingHeightTemperatureRange; parametersDelta: (max - min) / 800; firstGuess: getFirstGuessCombinations(), in
 * their order; minPointsLocalDetrending: getMinPointsLocalDetrending(); stdDevThreshold: getStdDevThreshold() (-9999: none).  Slots
 * beyond nParameters and nFirstGuess are not read. */
typedef struct {
    int32_t function;
    int32_t nParameters;
    int32_t nFirstGuess;
    int32_t minPointsLocalDetrending;
    float stdDevThreshold;
    int32_t reserved;
    double parametersMin[SF3D_LOCALDETREND_MAX_PARAMETERS];
    double parametersMax[SF3D_LOCALDETREND_MAX_PARAMETERS];
    double parametersDelta[SF3D_LOCALDETREND_MAX_PARAMETERS];
    double firstGuess[SF3D_LOCALDETREND_MAX_FIRST_GUESS][SF3D_LOCALDETREND_MAX_PARAMETERS];
} sf3d_localdetrend_fit_t;

/* One variable (SF3D_METEO_AIR_TEMPERATURE or SF3D_METEO_AIR_DEW_TEMPERATURE), one launch.  x, y [m]: utm of the stations; height [m]:
 * getProxyValue(elevationPos), -9999 where a station has none; value: the station values, NOT detrended; boundingBoxArea:
 * getPointsBoundingBoxArea(); settings: useMultipleDetrending and useLocalDetrending must be 1, the five other options 0, exactly one
 * proxy active and that one the height (its slope and lapse-rate fields are not read); useDetrending: ! getUseDoNotRetrend().  out:
 * nrRows x nrCols floats or NULL.  The result lands in the meteo block's slot of the variable and counts as produced, as that of
 * sf3d_meteo_interpolate does: a cell outside the DEM holds the flag, a cell where the method returns NODATA holds NODATA.  nStations == 0
 * is allowed.  Multi-GPU: as sf3d_meteo_interpolate, a rank computes the cells whose column it owns and leaves the others at the flag. */
sf3d_error_t sf3d_localdetrend_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* height, const float* value,
                                           float boundingBoxArea, const sf3d_meteo_settings_t* settings, const sf3d_localdetrend_fit_t* fit, float* out);

/* the per-cell outcome of the last call (a NULL array is skipped).  significant: isProxySignificant(elevationPos) when the cell was
 * interpolated; r2: getRegressionR2(), float(R2), -9999 where no fit ran; parameters: nrCells x SF3D_LOCALDETREND_MAX_PARAMETERS doubles,
 * getFittingParameters().front(), -9999 where the height was not significant and in the slots beyond nParameters.  A cell outside the DEM
 * or of another rank: 0, -9999, -9999. */
sf3d_error_t sf3d_localdetrend_get_fit(uint32_t nrCells, uint8_t* significant, float* r2, double* parameters);

/* count: the number of selected stations; radius: getLocalRadius().  A cell outside the DEM or of another rank: 0, -9999. */
sf3d_error_t sf3d_localdetrend_get_selection(uint32_t nrCells, uint32_t* count, float* radius);

/* event-timed duration [ms] of the last k_localdetrend launch when sf3d_kernel_timing is on, else 0 */
double sf3d_localdetrend_kernel_ms(void);

/* device memory the block holds beside the meteo block's [bytes] */
uint64_t sf3d_localdetrend_bytes(void);

sf3d_error_t sf3d_localdetrend_clean(void);

#ifdef __cplusplus
}
#endif

#endif
