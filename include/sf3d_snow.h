/*
 * sf3d_snow.h - the hourly snow model of the application on the MI355X: what Crit3DProject::computeSnowModel
 * (bin/CRITERIA3D/criteria3DProject.cpp:1815-1878) runs before the hour's water is handed to the solver -
 * Crit3DSnow::computeSnowBrooksModel (src/snow/snow.cpp:142-525, the Brooks energy balance) on the seven float state maps of
 * Crit3DSnowMaps - and the liquid water assignPrecipitation (:914-968) then feeds the solver (prec - snowFall + snowMelt; sf3d_sink.h
 * reads it on the device and adds the rain term to the node sinks).
 * One kernel launch per hour (k_snow_hour, one thread per raster cell); the maps stay on the device, and the values are the
 * reference's to the bit (tests/golden/snow_brooks.npz: a pin of the compiled reference).
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.
 *
 * The snow state belongs to the raster, not to the node graph: it does not need sf3d_initialize and survives it; it uses the device
 * sf3d_set_device chose (or the default choice of sf3d.h) and the solver's stream.  No call touches the solver's state, flags, graphs
 * or launch plans.  sf3d_snow_clean and sf3d_clean free the maps.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_snow_initialize), SF3D_PARAMETER_ERROR null pointer or empty raster,
 * or a map size (nrCells) that is not nrRows x nrCols of sf3d_snow_initialize, SF3D_INDEX_ERROR a map number out of range,
 * SF3D_SOLVER_ERROR a HIP failure (no device).  Every map is nrCells = nrRows x nrCols floats, row-major.
 */
#ifndef SF3D_SNOW_H
#define SF3D_SNOW_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Crit3DSnowParameters (src/snow/snow.h:29-43) */
typedef struct {
    double skinThickness;              /* [m] */
    double soilAlbedo;                 /* [-] */
    double snowVegetationHeight;       /* [m] */
    double snowWaterHoldingCapacity;   /* [-] */
    double tempMaxWithSnow;            /* [degC] */
    double tempMinWithRain;            /* [degC] */
    double snowSurfaceDampingDepth;    /* [m] */
} sf3d_snow_parameters_t;

/* the state maps of Crit3DSnowMaps */
enum {
    SF3D_SNOW_SWE = 0, SF3D_SNOW_ICE_CONTENT = 1, SF3D_SNOW_LW_CONTENT = 2, SF3D_SNOW_INTERNAL_ENERGY = 3, SF3D_SNOW_SURFACE_ENERGY = 4,
    SF3D_SNOW_SURFACE_TEMP = 5, SF3D_SNOW_AGE_OF_SNOW = 6, SF3D_SNOW_STATE_COUNT = 7
};
/* the hourly outputs: the five maps the application keeps and the liquid water that reaches the soil surface [mm] */
enum {
    SF3D_SNOW_OUT_SNOW_FALL = 0, SF3D_SNOW_OUT_SNOW_MELT = 1, SF3D_SNOW_OUT_DELTA_SWE = 2, SF3D_SNOW_OUT_SENSIBLE_HEAT = 3,
    SF3D_SNOW_OUT_LATENT_HEAT = 4, SF3D_SNOW_OUT_LIQUID_WATER = 5, SF3D_SNOW_OUTPUT_COUNT = 6
};

/* initializeSnowParameters (snow.cpp:39-50) */
sf3d_error_t sf3d_snow_default_parameters(sf3d_snow_parameters_t* parameters);

/* initializeSnowMaps + resetSnowModel (snowMaps.cpp:82-108, 177-218): allocates the maps on the device; on every cell whose dem value
 * is not `flag` (isEqual): SWE 0, ice 0, liquid 0, age NODATA, surface temperature 5.0, surface energy of soil at 5.0, internal energy
 * at the pack temperature 3.4, outputs 0; `flag` on the others.  parameters = NULL: the defaults.  A second call replaces the raster. */
sf3d_error_t sf3d_snow_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, const sf3d_snow_parameters_t* parameters);
sf3d_error_t sf3d_snow_set_parameters(const sf3d_snow_parameters_t* parameters);

/* resetSnowModel on the SWE map the device holds (after sf3d_snow_set_state(SF3D_SNOW_SWE, ...) with an observed map): ice = SWE,
 * liquid 0, age NODATA, temperatures and energies as at initialisation (surface energy of snow where SWE > 0), outputs 0 */
sf3d_error_t sf3d_snow_reset(void);

/* one state map to / from the device (a resumed run; a hand-edited SWE map) and one output map of the last hour from the device */
sf3d_error_t sf3d_snow_set_state(int which, uint32_t nrCells, const float* map);
sf3d_error_t sf3d_snow_get_state(int which, uint32_t nrCells, float* map);
sf3d_error_t sf3d_snow_get_output(int which, uint32_t nrCells, float* map);

/* One hour: uploads the input maps (computeSnowPoint, criteria3DProject.cpp:1792-1811: air temperature [degC], precipitation [mm],
 * relative humidity [%], scalar wind intensity [m s-1], global and beam radiation [W m-2], transmissivity [-]; surfaceWater [mm] may be
 * NULL: 0 everywhere, what the application passes), launches k_snow_hour and copies nothing back.  Cells where the DEM holds its flag
 * get the flag in all thirteen maps (flagMapRowCol); a cell with more than 100 mm of surface water or without air temperature,
 * precipitation, radiation, SWE or surface temperature gets NODATA (-9999) in its state and outputs as in the reference - except its
 * internal energy, which keeps its value, and its snowmelt, which is 0 (getSnowMelt).  The liquid-water map holds prec, or
 * prec - snowFall + snowMelt where neither is the flag, and the flag where prec is.
 * Multi-GPU (sf3d_dist_* prepared and the column table of sf3d_maps.h set for this raster): a rank computes the cells whose column it
 * owns, leaves the state of the others untouched and their outputs at the flag; merge by sf3d_dist_owner. */
sf3d_error_t sf3d_snow_compute_hour(uint32_t nrCells, const float* airTemperature, const float* precipitation, const float* relativeHumidity,
                                    const float* windIntensity, const float* globalRadiation, const float* beamRadiation,
                                    const float* transmissivity, const float* surfaceWater, double clearSkyTransmissivity);

/* event-timed duration [ms] of the last k_snow_hour launch when sf3d_kernel_timing is on, else 0 */
double sf3d_snow_kernel_ms(void);

sf3d_error_t sf3d_snow_clean(void);

#ifdef __cplusplus
}
#endif

#endif
