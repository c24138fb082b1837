/*
 * sf3d_maps.h - output maps of the MI355X-native soilFluxes3D library: what the application computes from the state after each
 * hour (Project3D::computeCriteria3DMap, project3D.cpp:1896-1948; computeMinimumFoS :2128-2157; computeAvgDegreeOfSaturation
 * :2076-2125; computeFactorOfSafety :2614-2721), computed on the device from the state it already holds.  Only the float maps cross
 * the bus.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.
 *
 * Call order: the model as for sf3d.h (sf3d_initialize, nodes, links, soils, sf3d_set_node_soil ...); then sf3d_set_output_columns once
 * per model, sf3d_set_horizon_geotechnics per (soil, horizon) and sf3d_set_cell_slopes once (both needed by the factor of safety only);
 * then sf3d_compute_output_map after any computeStep.  sf3d_clean / sf3d_initialize forget all three (they belong to one model).
 */
#ifndef SF3D_MAPS_H
#define SF3D_MAPS_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* criteria3DVariable, agrolib/meteo/meteo.h:110-114: the values `variable` takes.  soilTemperature, soilSurfaceMoisture and
 * bottomDrainage are not served (getCriteria3DVar does not serve them either): SF3D_PARAMETER_ERROR. */
enum {
    SF3D_MAP_VOLUMETRIC_WATER_CONTENT = 0, SF3D_MAP_WATER_TOTAL_POTENTIAL = 1, SF3D_MAP_WATER_MATRIC_POTENTIAL = 2,
    SF3D_MAP_AVAILABLE_WATER_CONTENT = 3, SF3D_MAP_DEGREE_OF_SATURATION = 4, SF3D_MAP_AVG_DEGREE_OF_SATURATION = 5,
    SF3D_MAP_WATER_DEFICIT = 9, SF3D_MAP_WATER_INFLOW = 10, SF3D_MAP_WATER_OUTFLOW = 11, SF3D_MAP_FACTOR_OF_SAFETY = 12,
    SF3D_MAP_MINIMUM_FACTOR_OF_SAFETY = 13, SF3D_MAP_SURFACE_POND = 14, SF3D_MAP_MIN_VOLUMETRIC_WATER_CONTENT = 15,
    SF3D_MAP_MAX_VOLUMETRIC_WATER_CONTENT = 16
};

/* The raster behind the maps: nodeOfLayerCell[layer * nrCells + cell] is the node of the cell in that layer (Project3D::indexMap, GLOBAL
 * node numbering as in sf3d.h), -1 where there is none; layerThickness[layer] in m (layer 0 = surface).  The arrays are copied.
 * SF3D_MEMORY_ERROR before sf3d_initialize, SF3D_PARAMETER_ERROR for an empty table, SF3D_INDEX_ERROR for a node index out of range. */
sf3d_error_t sf3d_set_output_columns(uint32_t nrCells, uint32_t nrLayers, const int32_t* nodeOfLayerCell, const double* layerThickness);

/* Geotechnical data of horizon `horizonIndex` of soil `soilIndex` (the indices of sf3d_set_node_soil): effective cohesion [kPa], friction
 * angle [degrees], bulk density [g cm-3].  tan(frictionAngle * DEG_TO_RAD) is evaluated here, on the host, with the C library. */
sf3d_error_t sf3d_set_horizon_geotechnics(uint16_t soilIndex, uint16_t horizonIndex, double effectiveCohesion, double frictionAngle,
                                          double bulkDensity);

/* Slope [degrees] of every cell of the column table (radiationMaps->slopeMap); increaseSlope != 0: x 1.5, at most 89 degrees
 * (computeFactorOfSafety's option).  Per cell the host evaluates tanAngle = max(EPSILON, tan(max(slope * DEG_TO_RAD, EPSILON))) and
 * sin(2 slopeAngle) with the C library; a later call replaces them. */
sf3d_error_t sf3d_set_cell_slopes(uint32_t nrCells, const float* slopeDegree, int increaseSlope);

/* One map of the accepted state into out (caller-owned floats): layer >= 0 writes nrCells values, layer = -1 writes every layer
 * (out[layer * nrCells + cell]); minimumFactorOfSafety and avgDegreeOfSaturation are whole-column maps of nrCells values whatever `layer`
 * says.  Cells without a node, and values getCriteria3DVar reports as NODATA, hold `flag`.  The values are those of the application's
 * loops over the getters of sf3d.h, bit for bit (the surface layer's water content in mm, inflow / outflow / pond x 1000, water deficit at
 * fieldCapacity 3.0, the factor of safety rounded to float), except layer 0 of factorOfSafety: the flag (the application never reads it).
 * The solver's state and its host-side copies are not touched.
 * Multi-GPU (sf3d_dist_* connected): a rank fills the cells whose column it owns and writes `flag` elsewhere; merge by sf3d_dist_owner.
 * Errors: SF3D_MEMORY_ERROR not initialised; SF3D_TOPOGRAPHY_ERROR no column table (or one that names nodes the model no longer has);
 * SF3D_PARAMETER_ERROR bad variable or null out; SF3D_INDEX_ERROR layer out of range; SF3D_MISSING_DATA_ERROR a factor of safety needed
 * the cell slopes (no map is computed) or the geotechnics of a node's (soil, horizon) (the map is written all the same) and they were not set;
 * SF3D_SOLVER_ERROR no device. */
sf3d_error_t sf3d_compute_output_map(int variable, int layer, float flag, float* out);

#ifdef __cplusplus
}
#endif

#endif
