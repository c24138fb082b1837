/*
 * sf3d_topodist.h - topographic distance on the MI355X, on the raster of the meteo block (sf3d_meteo.h): what a project with
 * getUseTD() set needs of the hour's interpolation.
 *
 *  - the maps: gis::topographicDistanceMap (agrolib/gis/gis.cpp:1650-1675) for every station in one launch - for each DEM cell the
 *    largest rise of the DEM above the lower end of the line between the cell centre and the station, sampled every cell size
 *    (gis::topographicDistance, :1595-1647).  The application writes them once as TD_<dem>_<id>.flt and loads them before the first hour
 *    (bin/CRITERIA3D/criteria3DProject.cpp:1198-1203); here they are computed, or handed in, and stay on the device;
 *  - the interpolation: sf3d_meteo_interpolate with the distances of computeDistances under getUseTD()
 *    (agrolib/interpolation/interpolation.cpp:208-256): for temperature, humidity, dew point and wind (getUseTdVar, :1220-1234) and
 *    kh != 0, distance += kh * topoDistance, where topoDistance is the value of the station's map at the cell (looked up by the cell's
 *    float coordinates, as the reference does) or, without a map, outside it or on a NODATA value, the walk itself.  The methods, retrend
 *    and the tail are those of sf3d_meteo.h, the same device text;
 *  - the station matrix: the topoDistance of every station at every station's position, which the caller's Kh search
 *    (topographicDistanceOptimize, :2297-2368) evaluates interpolate() with.
 * The values are the reference's to the bit (tests/golden/topodist.npz: a pin of the compiled reference).
 *
 * With the caller: the Kh search itself and the rest of preInterpolation; the six other options of sf3d_meteo_settings_t are refused as
 * sf3d_meteo_interpolate refuses them; maps on a header other than the DEM's.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  The block
 * belongs to the meteo block's raster: sf3d_meteo_initialize comes first, and sf3d_topodist_clean, sf3d_meteo_clean, a second
 * sf3d_meteo_initialize and sf3d_clean free it.
 *
 * Errors: SF3D_MEMORY_ERROR no raster (sf3d_meteo_initialize); SF3D_PARAMETER_ERROR null pointer, a map size (nrCells) that is not the
 * raster's, anything beyond a cap below, a non-finite coordinate, a point too far from the raster, kh < 0, a map index that is not held
 * or names a dropped map, an unsupported option, and what sf3d_meteo_interpolate refuses; SF3D_SOLVER_ERROR a HIP failure (no device).
 * Every refusal comes before any device work.
 */
#ifndef SF3D_TOPODIST_H
#define SF3D_TOPODIST_H

#include <stdint.h>

#include "sf3d_meteo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest walk a call may ask for, in steps of one cell size: a point is refused where the distance from it to the farthest corner
 * of the raster, over the cell size, exceeds it.  At most SF3D_METEO_MAX_STATIONS points a call. */
#define SF3D_TOPODIST_MAX_STEPS 65536

/* gis::topographicDistanceMap for nPoints stations.  x, y [m]: point.utm; z [m]: point.z (the kernel takes float(...) where the
 * reference does).  The maps replace those of an earlier call and stay on the device: nPoints x nrCells floats, map k for point k; a cell
 * outside the DEM holds the flag.  nPoints == 0 is allowed (no maps).  Multi-GPU: as sf3d_meteo_interpolate, a rank computes the cells
 * whose column it owns and leaves the others at the flag. */
sf3d_error_t sf3d_topodist_compute(uint32_t nPoints, const double* x, const double* y, const double* z);

/* device memory the maps hold [bytes] */
uint64_t sf3d_topodist_bytes(void);

/* one map back / a map the caller read from the application's TD_<dem>_<id>.flt in the place of map `index` (every cell of every rank) */
sf3d_error_t sf3d_topodist_get_map(uint32_t index, uint32_t nrCells, float* map);
sf3d_error_t sf3d_topodist_set_map(uint32_t index, uint32_t nrCells, const float* map);

/* the station of map `index` has no map from now on (the reference's topographicDistance == nullptr) until a set_map or a compute */
sf3d_error_t sf3d_topodist_drop_map(uint32_t index);

/* sf3d_meteo_interpolate under getUseTD().  z: point->z of the stations; mapIndex: per station the map it carries, -1 for none (NULL:
 * none carries one); settings: useTopographicDistance may be 0 or 1, the six other options must be 0; kh: getTopoDist_Kh().  The result
 * lands in the meteo block's slot of the variable and counts as produced, as that of sf3d_meteo_interpolate does. */
sf3d_error_t sf3d_topodist_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const double* z, const float* value,
                                       const int32_t* mapIndex, float boundingBoxArea, const sf3d_meteo_settings_t* settings, int kh, float* out);

/* matrix[j * nPoints + i]: the topoDistance computeDistances uses for station i at station j's (float x, float y, float z) - the map
 * of station i (mapIndex as above) looked up there, else the walk */
sf3d_error_t sf3d_topodist_station_matrix(uint32_t nPoints, const double* x, const double* y, const double* z, const int32_t* mapIndex, float* matrix);

/* event-timed duration [ms] of the last launch when sf3d_kernel_timing is on, else 0.  which: 0 k_topodist_maps, 1 k_meteo_idw_td,
 * 2 k_topodist_matrix */
double sf3d_topodist_kernel_ms(int which);

sf3d_error_t sf3d_topodist_clean(void);

#ifdef __cplusplus
}
#endif

#endif
