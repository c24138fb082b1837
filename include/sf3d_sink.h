/*
 * sf3d_sink.h - the hourly water sinks of the application on the MI355X: the cell loop of Crit3DProject::assignETreal
 * (bin/CRITERIA3D/criteria3DProject.cpp:796-911) around Project3D::assignEvaporation (src/project3D/project3D.cpp:2377-2451, over
 * getPotentialEvaporation / getCoveredSurfaceFraction :2295-2314 and the coefficients of initializeEvaporationCoefficient :2331-2368) and
 * Project3D::assignTranspiration (:2461-2610, over getPotentialTranspiration :2323-2328), and the rain term of
 * Crit3DProject::assignPrecipitation (criteria3DProject.cpp:939-964) that runModelHour adds afterwards.  One kernel launch per hour
 * (k_sink_hour, one thread per raster cell walking its column of nodes).  Every input is read on the device: ET0, LAI and degree days from
 * the crop block (sf3d_crop.h), the liquid water from the snow block (sf3d_snow.h), root length, first / last root layer and the keyed
 * density table from the root block (sf3d_root.h), the water content of every node from the solver's accepted state - what
 * getCriteria3DVar(volumetricWaterContent) returns.  Evaporation and transpiration are the reference's to the bit
 * (tests/golden/water_sinks.npz: a pin of the compiled reference); the rain term is precSurfaceWater = liquidWater unless soil cracking
 * (Crit3DProject::computeSoilCracking, criteria3DProject.cpp:978-1123) is asked for with sf3d_sink_set_cracking: then part of the rain goes
 * straight into the soil nodes of the crack (k_sink_hour_crack, still one launch; tests/golden/soil_cracking.npz).
 *
 * The node of (layer, cell) comes from the column table of sf3d_set_output_columns (sf3d_maps.h), which must be set for this raster and
 * this layer grid.  The call leaves on the device a node array of sinks [m3 s-1] and two cell maps, actual evaporation and actual
 * transpiration [mm]; sf3d_sink_apply hands the node array to the solver exactly as one sf3d_set_node_water_sink_source per node would.
 * The sums totalEvaporation / totalTranspiration / totalPrecipitation and the Hydrall and RothC hooks of assignETreal are the caller's.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The tables and
 * cell maps belong to the raster as the snow, crop and root maps do (sf3d_sink_initialize needs neither sf3d_initialize nor a device: the
 * first sf3d_sink_compute_hour uploads them); the node array belongs to the model.  sf3d_sink_compute_hour reads the solver's state and
 * changes nothing of it: no state, flag, graph or launch plan.  sf3d_sink_clean and sf3d_clean free the block.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_sink_initialize; sf3d_initialize for the hour), or a getter / sf3d_sink_apply before the
 * first hour, or a cracking getter while cracking is off; SF3D_PARAMETER_ERROR null pointer, empty raster, a map size (nrCells / nrNodes) that is not the raster's / the model's, anything
 * beyond a cap below, a crop index >= nUnits, a soil index >= nSoils, a layer grid on which initializeEvaporationCoefficient fails, a NULL map
 * without the crop / snow block on the same raster, no root block (sf3d_root_initialize and sf3d_root_compute) on the same raster and layer
 * grid; SF3D_TOPOGRAPHY_ERROR no column table, or one of another raster, layer grid or model; SF3D_SOLVER_ERROR a HIP failure (no device).
 */
#ifndef SF3D_SINK_H
#define SF3D_SINK_H

#include <stdint.h>

#include "sf3d.h"
#include "sf3d_maps.h"
#include "sf3d_root.h"

#ifdef __cplusplus
extern "C" {
#endif

/* caps: those of the root block - SF3D_CROP_MAX_UNITS land units, SF3D_ROOT_MAX_SOILS soils of SF3D_ROOT_MAX_HORIZONS horizons,
 * SF3D_ROOT_MAX_LAYERS layers */

/* one land unit: kcMax, fRAW and isWaterSurplusResistant() of Crit3DCrop (agrolib/crop/crop.cpp:353-356).  24 bytes. */
typedef struct {
    double kcMax;
    double fRAW;
    int32_t isWaterSurplusResistant;
    int32_t reserved;
} sf3d_sink_unit_t;

/* one soil: per horizon upperDepth, lowerDepth [m], waterContentHH / FC / WP / SAT [m3 m-3] and getSoilFraction() = 1 - coarseFragments */
typedef struct {
    int32_t nrHorizons;
    int32_t reserved;
    double upperDepth[SF3D_ROOT_MAX_HORIZONS], lowerDepth[SF3D_ROOT_MAX_HORIZONS];
    double waterContentHH[SF3D_ROOT_MAX_HORIZONS], waterContentFC[SF3D_ROOT_MAX_HORIZONS], waterContentWP[SF3D_ROOT_MAX_HORIZONS],
           waterContentSAT[SF3D_ROOT_MAX_HORIZONS], soilFraction[SF3D_ROOT_MAX_HORIZONS];
} sf3d_sink_soil_t;

/* The raster (a DEM cell: !isEqual(dem, flag)), cellSize [m], the layer grid (layer 0: the surface; layerDepth the centres) and
 * computationSoilDepth [m], cropIndex / soilIndex per cell (any negative value: none), the unit and soil tables.  The host evaluates
 * initializeEvaporationCoefficient (its one exp per layer with the C library) and getHorizonIndex(layerDepth[layer]) of every soil and
 * layer.  A second call replaces the raster. */
sf3d_error_t sf3d_sink_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double cellSize, uint32_t nrLayers,
                                  const double* layerDepth, const double* layerThickness, double computationSoilDepth, const int32_t* cropIndex,
                                  const int32_t* soilIndex, uint32_t nUnits, const sf3d_sink_unit_t* units, uint32_t nSoils, const sf3d_sink_soil_t* soils);

/* what the host evaluated: evapCoeff and layerEvapCoeff (nrLayers doubles each, 0 beyond the last evaporation layer, whose index goes to
 * *lastEvapLayer) and the horizon table [soil][layer] (nSoils x nrLayers, -9999: none); any pointer may be NULL */
sf3d_error_t sf3d_sink_get_tables(double* evapCoeff, double* layerEvapCoeff, int32_t* lastEvapLayer, int32_t* horizonOfSoilLayer);

/* one soil for soil cracking: totalDepth [m] of Crit3DSoil; per horizon texture.clay, texture.silt [%], coarseFragments and organicMatter [-].
 * Upper and lower depths are those of the sf3d_sink_soil_t of the same index. */
typedef struct {
    int32_t nrHorizons;
    int32_t reserved;
    double totalDepth;
    double clay[SF3D_ROOT_MAX_HORIZONS], silt[SF3D_ROOT_MAX_HORIZONS], coarseFragments[SF3D_ROOT_MAX_HORIZONS], organicMatter[SF3D_ROOT_MAX_HORIZONS];
} sf3d_sink_crack_soil_t;

/* Soil cracking (Crit3DProject::computeSoilCracking, criteria3DProject.cpp:978-1123, called from assignPrecipitation :959) as an option of
 * the hour: off unless set.  After sf3d_sink_initialize, no device needed; nSoils must be the block's (else SF3D_PARAMETER_ERROR, as for more
 * horizons than the cap or than the soil of sf3d_sink_initialize has); NULL / 0 turns it off again, and so does a new sf3d_sink_initialize.
 * The host evaluates once per soil what depends on the soil and the layer grid only (:1003-1035, :1078): soilDepth, the fine-fraction loop
 * over the horizons, maxDepth and lastLayer = getSoilLayerIndex(maxDepth) (project3D.cpp:1764-1776); a soil that fails one of the tests never
 * cracks.  With cracking on, sf3d_sink_compute_hour runs k_sink_hour_crack and the node array holds the cracked sinks. */
sf3d_error_t sf3d_sink_set_cracking(uint32_t nSoils, const sf3d_sink_crack_soil_t* soils);

/* what the host evaluated for cracking: maxDepth [m] and lastLayer per soil, -9999 where the soil never cracks; any pointer may be NULL */
sf3d_error_t sf3d_sink_get_crack_tables(double* maxDepth, int32_t* lastLayer);

/* One hour, one launch.  et0 [mm], lai, degreeDays: NULL reads the crop block's map on the device (sf3d_crop_initialize on the same
 * nrRows x nrCols); liquidWater [mm]: NULL reads the liquid-water output of the snow block (sf3d_snow_compute_hour on the same raster).
 * sf3d_root_compute of this hour is a precondition.  A cell is computed when it is a DEM cell with a surface node in the column table;
 * every other cell holds the flag in both actual maps and leaves the sinks of its column at 0.  LAI at the flag counts as 0; transpiration
 * needs a crop index, LAI > 0 and a soil index, evaporation below the surface a soil index.
 * Multi-GPU (sf3d_dist_* prepared): a rank computes the cells whose column it owns; merge by sf3d_dist_owner. */
sf3d_error_t sf3d_sink_compute_hour(uint32_t nrCells, const float* et0, const float* lai, const float* degreeDays, const float* liquidWater);

/* the node sinks [m3 s-1] of the last hour in the caller's (global) numbering, nrNodes = the nodes of sf3d_initialize; 0 on the nodes of
 * cells that were not computed here */
sf3d_error_t sf3d_sink_get_node_sinks(uint32_t nrNodes, double* sinks);
/* actual evaporation and transpiration [mm] of the last hour, the flag (widened) where not computed; either pointer may be NULL */
sf3d_error_t sf3d_sink_get_actual(uint32_t nrCells, double* evaporation, double* transpiration);

/* the cracking maps of the last hour: what computeSoilCracking returned for the cell [mm] (liquidWater where cracking did not apply) and the
 * water that went into the crack's nodes [mm] (the sum of layerWater over the layers filled); the flag where the cell was not computed.
 * Either pointer may be NULL.  SF3D_MEMORY_ERROR before the first hour with cracking, or when cracking is off. */
sf3d_error_t sf3d_sink_get_crack(uint32_t nrCells, float* precSurfaceWater, double* crackWater);

/* Hands the node sinks of the last hour to the solver: the state N calls of sf3d_set_node_water_sink_source(i, sink[i]) leave.  The array
 * is copied into the staging model and its whole range marked changed; the next computeStep uploads it. */
sf3d_error_t sf3d_sink_apply(void);

/* event-timed duration [ms] of the last k_sink_hour launch when sf3d_kernel_timing is on, else 0 */
double sf3d_sink_kernel_ms(void);

sf3d_error_t sf3d_sink_clean(void);

#ifdef __cplusplus
}
#endif

#endif
