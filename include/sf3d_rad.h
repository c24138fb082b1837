/*
 * sf3d_rad.h - the hourly r.sun radiation maps with DEM shadows on the MI355X: what Project::interpolateDemRadiation
 * (agrolib/project/project.cpp:3387-3465) runs at the half hour right after it interpolates the transmissivity map -
 * radiation::computeRadiationDEM (agrolib/solarRadiation/solarRadiation.cpp:1045-1069): per DEM cell the NREL sun position (solPos.cpp,
 * through computeSunPosition :1092-1131), the shadow ray across the DEM (computeShadow :547-617) and the r.sun clear-sky / real-sky model
 * on the inclined cell (computeRadiationRsun :700-832).  One kernel launch per hour (k_rad_hour, one thread per raster cell); the five
 * maps stay on the device and are state across hours, as the reference's are (a cell the model does not write keeps its value).  The
 * bar is the compiled reference's bits (tests/golden/rad_rsun.npz); DESIGN 19 states where equality is by construction and where it is
 * expected (the double sin / cos / tan of the device are faithful routines, not the C library's).  The global and beam irradiance and
 * the transmissivity are what sf3d_snow_compute_hour and sf3d_crop_compute_hour take; a caller downloads and passes them.
 *
 * computeTransmissivity and its window estimate are include/sf3d_transmissivity.h (per station, on the device, on this block's raster
 * and settings).  With the caller: the station series behind them, the Brooks point model and the
 * meteo-point / output-point variants, updateMinMaxRasterGrid, and the sun-position error return beyond leaving the cell untouched.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.
 *
 * The maps belong to the raster, not to the node graph: they do not need sf3d_initialize and survive it; they use the device
 * sf3d_set_device chose (or the default choice of sf3d.h) and the solver's stream.  No call touches the solver's state, flags, graphs
 * or launch plans.  sf3d_rad_clean and sf3d_clean free the maps.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_rad_initialize); SF3D_PARAMETER_ERROR null pointer, empty raster, a cell size that is
 * not positive, a map size (nrCells) that is not nrRows x nrCols of sf3d_rad_initialize, a mode out of range, map mode without its map,
 * DEM tilt without slope / aspect maps, a time zone beyond +-12, a date or time that is none or that S_solpos refuses (years outside
 * 1950-2100, solPos.cpp:301), NULL transmissivity without an interpolated transmissivity map of the meteo block on the same raster;
 * SF3D_INDEX_ERROR a map number out of range; SF3D_SOLVER_ERROR a HIP failure (no device).  Every map is nrCells = nrRows x nrCols
 * floats, row-major.
 */
#ifndef SF3D_RAD_H
#define SF3D_RAD_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TradiationRealSkyAlgorithm, TparameterMode, TtiltMode (agrolib/solarRadiation/radiationDefinitions.h:37-40), with their values */
enum { SF3D_RAD_REALSKY_TOTALTRANSMISSIVITY = 0, SF3D_RAD_REALSKY_LINKE = 1 };
enum { SF3D_RAD_MODE_FIXED = 0, SF3D_RAD_MODE_MAP = 1, SF3D_RAD_MODE_MONTHLY = 2 };
enum { SF3D_RAD_TILT_FIXED = 1, SF3D_RAD_TILT_DEM = 2 };
/* the maps of Crit3DRadiationMaps this block computes */
enum { SF3D_RAD_SUN_ELEVATION = 0, SF3D_RAD_GLOBAL = 1, SF3D_RAD_BEAM = 2, SF3D_RAD_DIFFUSE = 3, SF3D_RAD_REFLECTED = 4, SF3D_RAD_MAP_COUNT = 5 };

/* what Crit3DRadiationSettings (radiationSettings.h) and Crit3DGisSettings (gis.h) contribute to computeRadiationDEM */
typedef struct {
    int32_t realSky;                   /* transmissivity scales the clear-sky model */
    int32_t realSkyAlgorithm;          /* SF3D_RAD_REALSKY_* */
    int32_t shadowing;
    int32_t linkeMode;                 /* SF3D_RAD_MODE_FIXED: linke; _MONTHLY: linkeMonthly[month - 1]; _MAP: see sf3d_rad_initialize */
    int32_t albedoMode;                /* SF3D_RAD_MODE_FIXED: albedo; _MAP: see sf3d_rad_initialize */
    int32_t tiltMode;                  /* SF3D_RAD_TILT_DEM: the slope / aspect maps; _FIXED: tilt / aspect on every cell */
    int32_t timeZone;                  /* Crit3DGisSettings::timeZone [h] */
    int32_t isUTC;                     /* the times of sf3d_rad_compute_hour are UTC: shifted by timeZone before use */
    float linke;                       /* linkeDefault */
    float linkeMonthly[12];
    float albedo;
    float tilt, aspect;                /* [deg] */
    float clearSky;                    /* clear-sky transmissivity */
} sf3d_rad_settings_t;

/* Crit3DRadiationSettings::initialize (radiationSettings.cpp:41-72) and Crit3DGisSettings (gis.cpp:47-54): real sky by Linke 4, shadowing,
 * albedo 0.2, DEM tilt, clear sky 0.75, monthly values NODATA, time zone 1, UTC */
sf3d_error_t sf3d_rad_default_parameters(sf3d_rad_settings_t* settings);

/* Crit3DRadiationMaps(dem, gisSettings) (solarRadiation.cpp:57-86) for a DEM of nrRows x nrCols cells whose lower left corner is
 * (xllCorner, yllCorner) [m]: allocates the five output maps at `flag` (initializeGrid(dem)), evaluates on the host what depends on the
 * cell only - float(cos / sin(raddeg * latitude)), the float pressure of pressureFromAltitude(height) * 0.01, cos / sin of aspect and tilt
 * as tilt() uses them, the slope-only terms of Muneer's model and of getReflectedIrradiance, the range checks of S_solpos on the cell -
 * and dem.maximum, and uploads them with the DEM.  latMap / lonMap: gis::computeLatLonMaps (criteria3d_amd.radiation.latlon_maps);
 * slopeMap / aspectMap: gis::computeSlopeAspectMaps [deg], NULL allowed under SF3D_RAD_TILT_FIXED.  linkeMap / albedoMap: required in
 * map mode - and not read: the reference's getLinke(row, col) / getAlbedo(row, col) (radiationSettings.cpp:124-136, 173-184) fetch the map
 * only where the cell is OUT of the grid, so every cell of the DEM gets NODATA (-9999) for its Linke factor or albedo, and so it does
 * here.  settings = NULL: the defaults.  A second call replaces the raster. */
sf3d_error_t sf3d_rad_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double xllCorner, double yllCorner, double cellSize,
                                 const float* latMap, const float* lonMap, const float* slopeMap, const float* aspectMap,
                                 const float* linkeMap, const float* albedoMap, const sf3d_rad_settings_t* settings);

/* computeRadiationDEM(settings, dem, maps, Crit3DTime(date, hour:minute:second)) (solarRadiation.cpp:1045-1069).  On the host, once per
 * call: the local-time shift of :714-726 with its date roll-over, the range checks of S_solpos on date and time (SF3D_PARAMETER_ERROR
 * before any device work) and everything of S_solpos that depends on date and time only.  transmissivity: the hour's map, or NULL for
 * the map the last sf3d_meteo_interpolate(SF3D_METEO_ATM_TRANSMISSIVITY, ...) left on the device.  Cells where the DEM holds its flag
 * keep the flag.  By day a cell whose transmissivity is NODATA (-9999) under realSky, or whose S_solpos range check fails, keeps the
 * previous hour's value in all five maps; by night it gets four zeros and its sun elevation.  With settings.shadowing off the
 * reference reads TsunPosition::shadow without ever setting it (solarRadiation.cpp:744-750, 801); its compiled build finds a non-zero
 * byte there, so every cell counts as shaded (no beam, global = diffuse) - and so it does here.
 * Multi-GPU (sf3d_dist_* prepared and the column table of sf3d_maps.h set for this raster): a rank writes the cells whose column it
 * owns - its rays read the whole DEM - and leaves the others as they were (the flag); merge by sf3d_dist_owner. */
sf3d_error_t sf3d_rad_compute_hour(int year, int month, int day, int hour, int minute, int second, uint32_t nrCells, const float* transmissivity);

/* one of the five maps (SF3D_RAD_*) from the device - the rasters computeRadiationDemPoint writes (solarRadiation.cpp:974-978); the sun
 * elevation map holds the refracted elevation [deg], the others W m-2 */
sf3d_error_t sf3d_rad_get_map(int which, uint32_t nrCells, float* map);

/* test hook: the device build of the routines of criteria3d_amd/csrc/sf3d_trig.inc on `count` arguments.  which: 0 sin, 1 cos, 2 tan, 3 acos
 * (the faithful double routines that stand in for the C library's in solPos.cpp:740-741, 779, 805, 912-918 and solarRadiation.cpp:353,
 * 560-564); 4 acosf, 5 powf(x, y) (the library's float routines of solPos.cpp:603 and :825; floats carried in doubles; y only for 5) */
sf3d_error_t sf3d_rad_device_trig(int which, uint32_t count, const double* x, const double* y, double* out);

/* event-timed duration [ms] of the last k_rad_hour launch (the loop of solarRadiation.cpp:1053-1064) when sf3d_kernel_timing is on, else 0 */
double sf3d_rad_kernel_ms(void);

/* Crit3DRadiationMaps::clear (solarRadiation.cpp:94-119): frees the maps on the device */
sf3d_error_t sf3d_rad_clean(void);

#ifdef __cplusplus
}
#endif

#endif
