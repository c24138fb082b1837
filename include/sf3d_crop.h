/*
 * sf3d_crop.h - the hourly reference evapotranspiration and the daily crop maps of the application on the MI355X: what
 * Crit3DProject::runModelHour (bin/CRITERIA3D/criteria3DProject.cpp:2130-2153) does between the snow model and the solver -
 * Crit3DHourlyMeteoMaps::computeET0PMMap (agrolib/project/meteoMaps.cpp:238-271) over ET0_Penman_hourly (agrolib/meteo/meteo.cpp:550-609),
 * updateDailyTemperatures (criteria3DProject.cpp:1994-2018) - and, once a day, dailyUpdateCropMaps (:576-640): degree days
 * (Crit3DCrop::getDailyDegreeIncrease, agrolib/crop/crop.cpp:161-174) and LAI (computeSimpleLAI, crop.cpp:177-224; the curves of
 * agrolib/crop/development.cpp:117-154).  One kernel launch per hour (k_et0_hour) and one per day (k_crop_day), one thread per raster
 * cell; the maps stay on the device, and the values are the reference's to the bit (tests/golden/crop_et0.npz: a pin of the compiled
 * reference).  ET0, LAI and degree days are what assignEvaporation / assignTranspiration start from; those stay with the caller.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.
 *
 * The crop state belongs to the raster, not to the node graph: it does not need sf3d_initialize and survives it; it uses the device
 * sf3d_set_device chose (or the default choice of sf3d.h) and the solver's stream.  No call touches the solver's state, flags, graphs
 * or launch plans.  sf3d_crop_clean and sf3d_clean free the maps.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_crop_initialize), SF3D_PARAMETER_ERROR null pointer, empty raster, a map size
 * (nrCells) that is not nrRows x nrCols of sf3d_crop_initialize, more than SF3D_CROP_MAX_UNITS land units, a crop index >= nUnits, a
 * mix of NULL and non-NULL input maps, NULL input maps without a snow hour on the same raster; SF3D_INDEX_ERROR a map number out of
 * range; SF3D_SOLVER_ERROR a HIP failure (no device).  Every map is nrCells = nrRows x nrCols floats, row-major.
 */
#ifndef SF3D_CROP_H
#define SF3D_CROP_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the crop table has one entry per land unit (landUnitList and cropList have the same index); k_crop_day keeps it in LDS, 96 B each */
#define SF3D_CROP_MAX_UNITS 64

/* speciesType (agrolib/crop/crop.h:14) */
enum {
    SF3D_CROP_HERBACEOUS_ANNUAL = 0, SF3D_CROP_HERBACEOUS_PERENNIAL = 1, SF3D_CROP_HORTICULTURAL = 2, SF3D_CROP_GRASS = 3, SF3D_CROP_TREE = 4,
    SF3D_CROP_FALLOW = 5, SF3D_CROP_FALLOW_ANNUAL = 6, SF3D_CROP_BARESOIL = 7
};

/* one land unit: the fields of Crit3DCrop (agrolib/crop/crop.h:26-41) that getDailyDegreeIncrease and computeSimpleLAI read, and
 * Project3D::isCrop of the unit (src/project3D/project3D.cpp:1526-1537: 0 when its id_crop is empty or BARE) */
typedef struct {
    int32_t type;                      /* speciesType */
    int32_t isCrop;
    int32_t sowingDoy;
    int32_t plantCycle;
    double LAImin, LAImax, LAIgrass;
    double LAIcurve_a, LAIcurve_b;
    double thermalThreshold, upperThermalThreshold;
    double degreeDaysIncrease, degreeDaysDecrease, degreeDaysEmergence;
} sf3d_crop_unit_t;

/* the state maps: degreeDaysMap, laiMap, dailyTminMap, dailyTmaxMap of Crit3DProject */
enum { SF3D_CROP_DEGREE_DAYS = 0, SF3D_CROP_LAI = 1, SF3D_CROP_DAILY_TMIN = 2, SF3D_CROP_DAILY_TMAX = 3, SF3D_CROP_STATE_COUNT = 4 };
/* sf3d_crop_kernel_ms */
enum { SF3D_CROP_KERNEL_ET0_HOUR = 0, SF3D_CROP_KERNEL_CROP_DAY = 1 };

/* initializeCropMaps (criteria3DProject.cpp:415-433): allocates the maps on the device; the four state maps and ET0 hold `flag`
 * everywhere.  cropIndex: per cell, what getLandUnitIndexRowCol (project3D.cpp:1476-1492) returns - the index of the cell's land unit
 * in `units`, -1 (any negative value) where there is none.  latitude: gisSettings.startLocation.latitude [deg]; south of the equator
 * the crop year starts at doy 182 and the leaf fall at doy 120.  A second call replaces the raster. */
sf3d_error_t sf3d_crop_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, const int32_t* cropIndex, uint32_t nUnits,
                                  const sf3d_crop_unit_t* units, double latitude);

/* one state map to / from the device (a resumed run) and the ET0 map [mm] of the last hour from the device */
sf3d_error_t sf3d_crop_set_state(int which, uint32_t nrCells, const float* map);
sf3d_error_t sf3d_crop_get_state(int which, uint32_t nrCells, float* map);
sf3d_error_t sf3d_crop_get_et0(uint32_t nrCells, float* map);

/* initializeCropFromDegreeDays (criteria3DProject.cpp:524-573) on a map of the DEM's header: the four state maps are set to the flag,
 * then on every DEM cell (isEqual) with a crop whose map value is not the flag: degree days = the value, LAI =
 * computeSimpleLAI(value, latitude, currentDoy).  Every cell, also under sf3d_dist_*. */
sf3d_error_t sf3d_crop_set_degree_days(uint32_t nrCells, const float* map, int currentDoy);

/* One hour: computeET0PMMap (meteoMaps.cpp:238-271) and updateDailyTemperatures (criteria3DProject.cpp:1994-2018) in one launch of
 * k_et0_hour.  Inputs: air temperature [degC], relative humidity [%], scalar wind intensity at 10 m [m s-1], global irradiance [W m-2],
 * transmissivity [-]; clearSkyTransmissivity: CLEAR_SKY_TRANSMISSIVITY_DEFAULT (0.75) in the application.  ET0 is computed where
 * int(dem) != int(flag) and none of the five inputs is the flag (isEqual), the flag elsewhere; the daily extremes take the air
 * temperature wherever it is not the flag, DEM or not.
 * All five maps NULL: the call uploads nothing and reads the maps the last sf3d_snow_compute_hour left on the device (sf3d_snow.h; the
 * snow raster must have the same nrRows x nrCols and must have computed an hour).
 * Multi-GPU (sf3d_dist_* prepared and the column table of sf3d_maps.h set for this raster): a rank computes the cells whose column it
 * owns, leaves the state of the others untouched and their ET0 at the flag; merge by sf3d_dist_owner. */
sf3d_error_t sf3d_crop_compute_hour(uint32_t nrCells, const float* airTemperature, const float* relativeHumidity, const float* windIntensity,
                                    const float* globalRadiation, const float* transmissivity, float clearSkyTransmissivity);

/* One day: dailyUpdateCropMaps (criteria3DProject.cpp:576-640) in one launch of k_crop_day.  dateDoy: day of year of the date that
 * closes (the reset of LAI and degree days happens when it is the first doy of the crop year: 1, or 182 south of the equator);
 * currentDoy: getCurrentDate().dayOfYear().  Both 1..366.  Afterwards both daily extremes hold the flag.  Multi-GPU: as the hourly
 * call, the cells of other ranks are left untouched. */
sf3d_error_t sf3d_crop_daily_update(int dateDoy, int currentDoy);

/* event-timed duration [ms] of the last k_et0_hour (0) / k_crop_day (1) launch when sf3d_kernel_timing is on, else 0 */
double sf3d_crop_kernel_ms(int which);

sf3d_error_t sf3d_crop_clean(void);

#ifdef __cplusplus
}
#endif

#endif
