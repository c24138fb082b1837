/*
 * sf3d_meteo.h - the hourly meteo maps of the application from station data on the MI355X: what the library function interpolate()
 * (agrolib/interpolation/interpolation.cpp:2502-2560) does for every DEM cell in the application's default non-local set-up, for the four
 * or five calls of interpolateAndSaveHourlyMeteo an hour of Crit3DProject::runModelHour begins with (bin/CRITERIA3D/
 * criteria3DProject.cpp:2084-2108): air temperature, precipitation, relative humidity, wind intensity and, optionally, global irradiance.
 * The values are the reference's to the bit (tests/golden/meteo_idw.npz: a pin of the compiled reference).
 *
 * In scope, per cell: the float distances of computeDistances without topographic distance (gis::computeDistance, gis.cpp:685-691);
 * inverseDistanceWeighted (:1031-1051), shepardIdw (:871-945) or modifiedShepardIdw (:948-1028, radius == NODATA) over
 * shepardSearchNeighbour (:806-868); retrend (:1288-1351) with single detrending; the tail of interpolate() (all-zero precipitation, the
 * rain threshold, the clamps).  Cell centres are those of gis::getUtmXYFromRowCol (gis.cpp:806-810), converted to float where
 * interpolate() takes them.
 *
 * With the caller: everything that produces the point list - quality control, checkPrecipitationZero, preInterpolation with its
 * regressions and detrendPoints (once per variable and hour, on N points): the calls take detrended values and the fitted slopes.  Also
 * multiple and local detrending, topographic distance, kriging, supplemental stations (every station is primary), the cross-validation
 * index and updateMinMaxRasterGrid: a settings struct that asks for one of them is refused (SF3D_PARAMETER_ERROR).  Topographic distance
 * has entry points of its own on this block's raster: sf3d_topodist.h; so have multiple detrending with local detrending (sf3d_localdetrend.h,
 * sf3d_localproxies.h), with glocal detrending (sf3d_glocal.h) and with neither (sf3d_multidetrend.h).
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The meteo
 * state belongs to the raster as the snow, crop and root maps do: it does not need sf3d_initialize and survives it, uses the device
 * sf3d_set_device chose and the solver's stream, and touches nothing of the solver.  sf3d_meteo_clean and sf3d_clean free it.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR null pointer, empty raster, a map size
 * (nrCells) that is not nrRows x nrCols of sf3d_meteo_initialize, an unknown variable or method, anything beyond a cap below, more
 * proxies in the settings than sf3d_meteo_initialize got rasters, an unsupported option; SF3D_SOLVER_ERROR a HIP failure (no device).
 */
#ifndef SF3D_METEO_H
#define SF3D_METEO_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* caps: the station table (x, y, value) of a call lives in the LDS of every block; SHEPARD_MIN_NRPOINTS 5, SHEPARD_AVG_NRPOINTS 8 and
 * SHEPARD_MAX_NRPOINTS 10 (interpolationConstants.h:6-8) are fixed */
#define SF3D_METEO_MAX_STATIONS 1024
#define SF3D_METEO_MAX_PROXIES 8

/* the variables (the first five in the order sf3d_snow_compute_hour takes its maps); getUseDetrendingVar is true for the two
 * temperatures; the tail: rain threshold (precipitation), [0, 100] (humidity), >= 0 (wind, irradiance, transmissivity) */
enum { SF3D_METEO_AIR_TEMPERATURE = 0, SF3D_METEO_PRECIPITATION = 1, SF3D_METEO_AIR_REL_HUMIDITY = 2, SF3D_METEO_WIND_SCALAR_INTENSITY = 3,
       SF3D_METEO_GLOBAL_IRRADIANCE = 4, SF3D_METEO_ATM_TRANSMISSIVITY = 5, SF3D_METEO_AIR_DEW_TEMPERATURE = 6, SF3D_METEO_VARIABLES = 7 };
/* TInterpolationMethod (interpolationConstants.h:18) */
enum { SF3D_METEO_IDW = 0, SF3D_METEO_SHEPARD = 1, SF3D_METEO_SHEPARD_MODIFIED = 2 };

/* one proxy of the current combination.  active: isProxyActive && isProxySignificant; isHeight: getProxyPragaName(name) == proxyHeight;
 * inversion: getUseThermalInversion() && getInversionIsSignificative(); slope: getRegressionSlope(); the lapse-rate fields as the
 * getters of Crit3DProxy return them (floats).  32 bytes. */
typedef struct {
    int32_t active;
    int32_t isHeight;
    int32_t inversion;
    float slope, lapseRateH0, lapseRateH1, inversionLapseRate;
    int32_t reserved;
} sf3d_meteo_proxy_t;

/* what interpolate() reads of Crit3DInterpolationSettings and Crit3DMeteoSettings.  allZero: getPrecipitationAllZero(); useDetrending:
 * ! getUseDoNotRetrend(); the seven options that stay with the caller must be 0. */
typedef struct {
    int32_t allZero;
    float rainfallThreshold;
    int32_t useDetrending;
    int32_t useMultipleDetrending;
    int32_t useLocalDetrending;
    int32_t useTopographicDistance;
    int32_t useKriging;
    int32_t useSupplementalStations;
    int32_t useCrossValidationIndex;
    int32_t updateMinMax;
    int32_t nProxies;
    int32_t reserved;
    sf3d_meteo_proxy_t proxy[SF3D_METEO_MAX_PROXIES];
} sf3d_meteo_settings_t;

/* The raster (a DEM cell: !isEqual(dem, flag)) with the lower-left corner and the cell size of its header, and one float raster of
 * nrRows x nrCols per proxy, in the order of the settings' proxy[]; a NULL entry: the proxy's values are the DEM's (the height proxy).
 * A proxy value equal to the flag is NODATA to retrend.  Afterwards every map holds the flag.  A second call replaces the raster. */
sf3d_error_t sf3d_meteo_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double xllCorner, double yllCorner, double cellSize,
                                   uint32_t nProxies, const float* const* proxyMaps);

/* One variable, one launch.  x, y [m]: utm of the stations; value: the (detrended) station values; boundingBoxArea:
 * getPointsBoundingBoxArea(); out: nrRows x nrCols floats or NULL (the map stays on the device: sf3d_meteo_get_map).  A cell outside the
 * DEM holds the flag; a cell where the method returns NODATA holds NODATA.  nStations == 0 is allowed (NODATA on every DEM cell).
 * Multi-GPU (sf3d_dist_* prepared and the column table of sf3d_maps.h set for this raster): a rank computes the cells whose column it
 * owns and leaves the others at the flag; merge by sf3d_dist_owner. */
sf3d_error_t sf3d_meteo_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const float* value, float boundingBoxArea,
                                    const sf3d_meteo_settings_t* settings, float* out);

/* the map the last sf3d_meteo_interpolate of the variable left on the device (the flag everywhere before the first) */
sf3d_error_t sf3d_meteo_get_map(int variable, uint32_t nrCells, float* map);

/* a map the caller holds (read from a file, computed elsewhere) in the place of an interpolation of the variable: it goes to the device
 * as it is, every cell of every rank, and counts as produced for the blocks that read this one in place (sf3d_rad.h, sf3d_hour.h) */
sf3d_error_t sf3d_meteo_set_map(int variable, uint32_t nrCells, const float* map);

/* event-timed duration [ms] of the last k_meteo_idw launch when sf3d_kernel_timing is on, else 0 */
double sf3d_meteo_kernel_ms(void);

sf3d_error_t sf3d_meteo_clean(void);

#ifdef __cplusplus
}
#endif

#endif
