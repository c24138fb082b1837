/*
 * sf3d_root.h - root length, root depth, first / last root layer and root density maps of the application on the MI355X: the two calls
 * Project3D::assignTranspiration (src/project3D/project3D.cpp:2487-2498) and Crit3DProject::assignETreal (hydrall,
 * bin/CRITERIA3D/criteria3DProject.cpp:875-886) make for every crop cell, every hour - Crit3DCrop::computeRootLength3D
 * (agrolib/crop/crop.cpp:651-691, over root::getRootLengthDD, agrolib/crop/root.cpp:139-170) and root::computeRootDensity3D
 * (root.cpp:505-633, over cardioidDistribution / cylindricalDistribution, root.cpp:255-364) - each on a fresh copy of cropList[unit].
 * The values are the reference's to the bit (tests/golden/root_density.npz: a pin of the compiled reference).  The transpiration sink
 * itself (the stress logic of assignTranspiration, the sink arrays), evaporation and the rain term read these maps on the device: sf3d_sink.h.
 *
 * The density vector of a cell depends on its land unit, its soil and numberOfRootedLayers = round(min(currentRootLength, totalDepth) /
 * 0.01) only.  sf3d_root_initialize builds the vectors of every (unit, soil) pair of the raster for every number of rooted atoms once
 * (k_root_table); sf3d_root_compute is one launch of k_root_cell (root length, depth and the key of every cell); the density getter
 * gathers (k_root_gather).
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The root
 * state belongs to the raster as the snow and crop maps do: it does not need sf3d_initialize and survives it, uses the device
 * sf3d_set_device chose and the solver's stream, and touches nothing of the solver.  sf3d_root_clean and sf3d_clean free it.
 *
 * Errors: SF3D_MEMORY_ERROR not initialised (sf3d_root_initialize); SF3D_PARAMETER_ERROR null pointer, empty raster, a map size
 * (nrCells) that is not nrRows x nrCols of sf3d_root_initialize, anything beyond a cap below, a crop index >= nUnits, a soil index >=
 * nSoils, a soil of the raster without positive depth, degreeDays == NULL without a crop block on the same raster; SF3D_INDEX_ERROR a
 * layer out of range; SF3D_SOLVER_ERROR a HIP failure (no device).
 */
#ifndef SF3D_ROOT_H
#define SF3D_ROOT_H

#include <stdint.h>

#include "sf3d.h"
#include "sf3d_crop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* caps: land units as the crop table (SF3D_CROP_MAX_UNITS); the Ravone project has 461 soils of at most 9 horizons and 3.2 m (321 atoms)
 * and 14 layers */
#define SF3D_ROOT_MAX_SOILS 1024
#define SF3D_ROOT_MAX_HORIZONS 16
#define SF3D_ROOT_MAX_LAYERS 64
#define SF3D_ROOT_MAX_ATOMS 1024                /* int(totalDepth * 100) + 1 of a soil that occurs on the raster: totalDepth < 10.23 m */
#define SF3D_ROOT_MAX_TABLE_VALUES (1u << 24)   /* rows of the density table x nrLayers (128 MiB of doubles) */

/* rootDistributionType and rootGrowthType (agrolib/crop/root.h:11-14) */
enum { SF3D_ROOT_CYLINDRICAL_DISTRIBUTION = 0, SF3D_ROOT_CARDIOID_DISTRIBUTION = 1, SF3D_ROOT_GAMMA_DISTRIBUTION = 2 };
enum { SF3D_ROOT_LINEAR = 0, SF3D_ROOT_EXPONENTIAL = 1, SF3D_ROOT_LOGISTIC = 2 };

/* one land unit: what the two functions read of Crit3DCrop / Crit3DRoot.  isRootStatic: Crit3DCrop::isRootStatic() of the unit
 * (crop.cpp:359-365).  degreeDaysRootGrowth is an int in the reference too.  48 bytes. */
typedef struct {
    int32_t rootShape;                 /* rootDistributionType; a gamma unit is computed as a cardioid (root.cpp:530-533) */
    int32_t growth;                    /* rootGrowthType; EXPONENTIAL yields NODATA as in getRootLengthDD */
    int32_t isRootStatic;
    int32_t degreeDaysRootGrowth;
    double shapeDeformation, rootDepthMin, rootDepthMax, degreeDaysEmergence;
} sf3d_root_unit_t;

/* one soil: totalDepth [m] and per horizon upperDepth, lowerDepth [m] and getSoilFraction() = 1 - coarseFragments.  400 bytes. */
typedef struct {
    double totalDepth;
    int32_t nrHorizons;
    int32_t reserved;
    double upperDepth[SF3D_ROOT_MAX_HORIZONS], lowerDepth[SF3D_ROOT_MAX_HORIZONS], soilFraction[SF3D_ROOT_MAX_HORIZONS];
} sf3d_root_soil_t;

/* sf3d_root_kernel_ms */
enum { SF3D_ROOT_KERNEL_CELL = 0, SF3D_ROOT_KERNEL_TABLE = 1, SF3D_ROOT_KERNEL_GATHER = 2 };

/* The raster (a DEM cell: !isEqual(dem, flag), as sf3d_crop_initialize), the layer grid (layer 0: the surface; layerDepth the centres),
 * cropIndex / soilIndex per cell (what getLandUnitIndexRowCol and soilIndexMap return; any negative value: none), the unit and soil
 * tables.  Builds the density table of every (unit, soil) pair of the DEM cells; afterwards every output holds the flag.  A second call
 * replaces the raster. */
sf3d_error_t sf3d_root_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, uint32_t nrLayers, const double* layerDepth,
                                  const double* layerThickness, const int32_t* cropIndex, const int32_t* soilIndex, uint32_t nUnits,
                                  const sf3d_root_unit_t* units, uint32_t nSoils, const sf3d_root_soil_t* soils);

/* One hour.  A cell is computed when it is a DEM cell, has a crop and a soil index and its degree days are neither the flag nor NODATA
 * (isEqual, assignTranspiration:2464); every other cell holds the flag in every output.  degreeDays == NULL: the call uploads nothing and
 * reads the degree-day map of the crop block on the device (sf3d_crop.h; sf3d_crop_initialize on the same nrRows x nrCols).
 * Multi-GPU (sf3d_dist_* prepared and the column table of sf3d_maps.h set for this raster): a rank computes the cells whose column it
 * owns and leaves the others at the flag; merge by sf3d_dist_owner. */
sf3d_error_t sf3d_root_compute(uint32_t nrCells, const float* degreeDays);

/* currentRootLength and rootDepth [m]: double maps, as the fields of Crit3DRoot are doubles (the number of rooted atoms is rounded from
 * them, and a caller that continues on the host gets the value the reference would hold); the flag, widened, where not computed */
sf3d_error_t sf3d_root_get_length(uint32_t nrCells, double* map);
sf3d_error_t sf3d_root_get_depth(uint32_t nrCells, double* map);
/* firstRootLayer, lastRootLayer: NODATA (-9999) where computeRootDensity3D returned early, int(flag) where not computed */
sf3d_error_t sf3d_root_get_layers(uint32_t nrCells, int32_t* first, int32_t* last);
/* rootDensity of one layer (nrCells doubles) or, layer = -1, of every layer as [layer][cell] (nrLayers x nrCells doubles) */
sf3d_error_t sf3d_root_get_density(int layer, uint32_t nrCells, double* map);
/* the row of the density table every cell reads, -1 where not computed: equal keys share (unit, soil, number of rooted atoms) */
sf3d_error_t sf3d_root_get_keys(uint32_t nrCells, int32_t* map);
uint32_t sf3d_root_table_rows(void);

/* event-timed duration [ms] of the last k_root_cell (0) / k_root_table (1) / k_root_gather (2) launch when sf3d_kernel_timing is on, else 0 */
double sf3d_root_kernel_ms(int which);

sf3d_error_t sf3d_root_clean(void);

#ifdef __cplusplus
}
#endif

#endif
