/*
 * sf3d_glocal.h - air and dew-point temperature with GLOCAL detrending on the MI355X, on the raster of the meteo block (sf3d_meteo.h):
 * what a project with useMultipleDetrending and glocal detrending set needs of the hour's interpolation, as
 * Project::interpolationDemGlocalDetrending does (agrolib/project/project.cpp:3267-3384).  The domain is split into macro areas, each with
 * its own station list and a weight map over the DEM:
 *
 *  1. per area over its stations that have a point this hour (glocalDetrendingFitting, agrolib/interpolation/interpolation.cpp:2239-2294):
 *     the unweighted fit of the height (multipleDetrendingElevationFitting(.., isWeighted = false), :1862-1953, over
 *     bestFittingMarquardt_nDimension without weights, agrolib/mathFunctions/furtherMathFunctions.cpp:1433-1529), detrendingElevation,
 *     and multipleDetrendingOtherProxiesFitting (:1975-2171) with regression weights 1 and no minimum of fit points;
 *  2. per area macroAreaDetrending (:1759-1829): the subset rebuilt from all the area's points, detrended with the area's parameters;
 *  3. per (area, cell, weight) the cell loop (project.cpp:3343-3379): getSignificantProxyValuesXY (a cell without a significant proxy
 *     value is SET to -9999 by that area), interpolate() over the area's stations with the neighbour search of sf3d_meteo.h, the retrend
 *     with the area's parameters, and value * weight assigned where the cell holds -9999, added otherwise.  The weights are not normalised.
 * The reference's area loop is an OpenMP loop whose order is not defined; here the areas are visited in index order, which is the loop on
 * one thread.  The values are that loop's to the bit (tests/golden/glocal.npz: a pin of the compiled reference).
 *
 * With the caller: the point list and its indices, the height's range (setMultipleDetrendingHeightTemperatureRange), delta and first
 * guesses as in sf3d_localdetrend.h, the weight maps (loadGlocalWeightMaps), lapse-rate codes (every station is primary), topographic
 * distance inside an area, the meteo-grid variant (areaCellsGrid), cross validation and output points.  multipleDetrending without areas, with its points, is sf3d_multidetrend.h.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The block
 * belongs to the meteo block's raster: sf3d_meteo_initialize comes first, and sf3d_glocal_clean, sf3d_meteo_clean, a second
 * sf3d_meteo_initialize and sf3d_clean free what it holds.
 *
 * Errors: SF3D_MEMORY_ERROR no raster (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR see each entry point; SF3D_MISSING_DATA_ERROR an
 * interpolate() of the cell loop gave -9999 (the reference's isOk = false: the variable's map then does not count as produced);
 * SF3D_SOLVER_ERROR a HIP failure (no device).  Every refusal comes before any device work.
 */
#ifndef SF3D_GLOCAL_H
#define SF3D_GLOCAL_H

#include <stdint.h>

#include "sf3d_localproxies.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The project's static part, as loadGlocalStationsAndCells and loadGlocalWeightMaps leave it (project.cpp:2555-2716).  Area a has the
 * cells cell[cellOffset[a] .. cellOffset[a + 1]) - the FLOAT cell number row * nrCols + col the reference stores (:2691), from which row
 * and column are taken as int(cell / nrCols) and int(cell) % nrCols - with their weights, and the stations
 * stationIndex[stationOffset[a] .. stationOffset[a + 1]): Crit3DInterpolationDataPoint::index values, in the area's order.  An area
 * may have no cells or no stations.
 * SF3D_PARAMETER_ERROR: nAreas 0, offsets that do not start at 0 or decrease, a NULL array that is read, a raster of more than 2^24
 * cells (the float cell number is no longer exact), a cell number that is negative, not finite or >= rows x cols or whose row leaves
 * the raster, a weight that is 0, -9999 or not finite (the loader never stores one), one cell twice in one area, a station list of more
 * than SF3D_METEO_MAX_STATIONS entries. */
sf3d_error_t sf3d_glocal_set_areas(uint32_t nAreas, const uint32_t* cellOffset, const float* cell, const float* weight, const uint32_t* stationOffset,
                                   const int32_t* stationIndex);

/* One temperature map with glocal detrending.  The points as in sf3d_localproxies_interpolate, and pointIndex[nStations]: the index of
 * every point, which the areas' station lists name.  settings: useMultipleDetrending 1, useLocalDetrending 0, the five other options 0;
 * the entry point is the glocal switch.  fit: sf3d_localdetrend.h's; its minPointsLocalDetrending is not read.  boundingBoxArea:
 * getPointsBoundingBoxArea(), which shepardSearchNeighbour reads.  The result lands in the meteo block's slot of the variable and counts
 * as produced there; out may be NULL.
 * SF3D_PARAMETER_ERROR: what sf3d_localproxies_interpolate refuses (with useLocalDetrending set in the place of clear), a call before
 * sf3d_glocal_set_areas, a NULL or repeated pointIndex, an area that has cells but no point this hour (the reference fails on it). */
sf3d_error_t sf3d_glocal_interpolate(int variable, int method, uint32_t nStations, const int32_t* pointIndex, const double* x, const double* y, const float* value,
                                     uint32_t nProxies, const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings,
                                     const sf3d_localdetrend_fit_t* fit, const sf3d_localproxies_others_t* others, float* out);

/* What k_glocal_areas recorded of the last call, per area (a NULL array is skipped): significant, r2 (float(R2), -9999 where no fit ran)
 * and parameters[nAreas][SF3D_LOCALDETREND_MAX_PARAMETERS] of the height; proxySignificant, slope and intercept
 * [nAreas][SF3D_METEO_MAX_PROXIES] (-9999 where the slot is not a significant other proxy); fitted: the area's stations with a point this
 * hour; kept: what detrendingOtherProxies left of them; and per entry of the areas' station lists (nList = stationOffset[nAreas] of
 * sf3d_glocal_set_areas) the detrended value of the rebuilt subset (-9999 where the station is not kept) and whether it is kept.
 * SF3D_PARAMETER_ERROR: nAreas or nList that are not the areas', a call before the first sf3d_glocal_interpolate. */
sf3d_error_t sf3d_glocal_get_area_fit(uint32_t nAreas, uint32_t nList, uint8_t* significant, float* r2, double* parameters, uint8_t* proxySignificant, double* slope,
                                      double* intercept, uint32_t* fitted, uint32_t* kept, float* detrended, uint8_t* stationKept);

/* event-timed duration [ms] of the last launch when sf3d_kernel_timing is on, else 0; which: 0 k_glocal_areas, 1 k_glocal_cells */
double sf3d_glocal_kernel_ms(int which);

/* device memory the block holds beside the meteo block's [bytes] */
uint64_t sf3d_glocal_bytes(void);

sf3d_error_t sf3d_glocal_clean(void);

#ifdef __cplusplus
}
#endif

#endif
