/*
 * sf3d_hour.h - the application's hour, device to device on the MI355X: Crit3DProject::runModelHour
 * (bin/CRITERIA3D/criteria3DProject.cpp:2074-2189) with no raster crossing the bus between its stages.  The blocks of sf3d_meteo.h,
 * sf3d_rad.h, sf3d_snow.h, sf3d_crop.h, sf3d_root.h and sf3d_sink.h each hold their maps on the device; the calls of this header hand the
 * kernels of one block the maps of another where they lie, and add what the hour and the day still lacked:
 *   - the snow hour and the ET0 hour on the maps of the meteo and radiation blocks (k_snow_hour, k_et0_hour: the kernels are unchanged);
 *   - the sink hour whose rain, without the snow model, is the meteo block's precipitation map;
 *   - the relative humidity map from the dew point map (k_hour_relhum), the application's default humidity path;
 *   - totalPrecipitation, totalEvaporation and totalTranspiration of the hour's balance (k_hour_totals);
 *   - the day's pond of every surface node, Project3D::dailyUpdatePond (k_hour_pond).
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.
 *
 * Nothing here touches the solver's state, flags, graphs or launch plans, except sf3d_hour_update_ponds, which sets the ponds of surface
 * nodes the way sf3d_set_nodes_pond does.  The calls run on the solver's stream and return when their work is done.
 *
 * Reads in place are guarded: a call is refused, before any device work, unless every block it reads is initialised on the caller's
 * raster (the same nrRows x nrCols) and has produced the map.  A block that is cleaned or initialised again takes the maps it fed with it:
 * what another block had recorded of them is forgotten, and the next reader is refused (SF3D_PARAMETER_ERROR) until the maps are
 * produced again.
 *
 * Errors: SF3D_MEMORY_ERROR the consuming block (snow, crop, sink, meteo; the ponds: sf3d_hour_set_ponds, sf3d_initialize) is not
 * initialised; SF3D_PARAMETER_ERROR null pointer, a map size (nrCells) that is not the consuming block's raster, a feeding block that is not
 * on that raster or has not produced the map, more than SF3D_CROP_MAX_UNITS land units, a land unit index >= nUnits, computeCrop without
 * the crop block on the raster; SF3D_TOPOGRAPHY_ERROR no column table (sf3d_set_output_columns) for the raster; SF3D_SOLVER_ERROR a HIP
 * failure (no device).  Every map is nrCells = nrRows x nrCols values, row-major.
 *
 * Multi-GPU (sf3d_dist_* prepared and the column table set for this raster): the ownership rule of the other raster blocks - a rank
 * computes the cells whose column it owns.
 */
#ifndef SF3D_HOUR_H
#define SF3D_HOUR_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sf3d_hour_kernel_ms */
enum { SF3D_HOUR_KERNEL_RELHUM = 0, SF3D_HOUR_KERNEL_TOTALS = 1, SF3D_HOUR_KERNEL_POND = 2 };

/* Crit3DHourlyMeteoMaps::computeRelativeHumidityMap (agrolib/project/meteoMaps.cpp:301-321) over relHumFromTdew(float, float)
 * (agrolib/meteo/meteo.cpp:301-315), what interpolateHourlyMeteoVar (src/project3D/project3D.cpp:1848-1878) calls after the dew point
 * when useDewPoint is set (the default, interpolationSettings.cpp:354).  Reads the SF3D_METEO_AIR_TEMPERATURE and
 * SF3D_METEO_AIR_DEW_TEMPERATURE maps of the meteo block - both must have been interpolated - and writes its SF3D_METEO_AIR_REL_HUMIDITY
 * map: sf3d_meteo_get_map and the calls below see it.  The flag of the meteo block where either input holds it, -9999 where either input
 * is NODATA, else the reference's value to the bit.  out: nrCells floats or NULL (the map stays on the device).  Multi-GPU: the flag in
 * the cells of other ranks.  updateMinMaxRasterGrid stays with the caller. */
sf3d_error_t sf3d_hour_relative_humidity(uint32_t nrCells, float* out);

/* sf3d_snow_compute_hour (computeSnowModel, criteria3DProject.cpp:1792-1878) with the seven maps taken where they are: air temperature,
 * precipitation, relative humidity and wind of the meteo block, global and beam irradiance of the radiation block and the transmissivity
 * map the last sf3d_rad_compute_hour read (its own copy, or the meteo block's map when it was called with NULL).  Nothing is copied but
 * surfaceWater [mm] (NULL: 0 everywhere).  Afterwards sf3d_crop_compute_hour with five NULL maps and sf3d_sink_compute_hour with a NULL
 * liquidWater read what this hour read and wrote, as after a host-fed hour. */
sf3d_error_t sf3d_hour_snow(uint32_t nrCells, const float* surfaceWater, double clearSkyTransmissivity);

/* sf3d_crop_compute_hour (computeET0PMMap, agrolib/project/meteoMaps.cpp:238-271, and updateDailyTemperatures,
 * criteria3DProject.cpp:1994-2018) for a run without the snow model: air temperature, relative humidity and wind of the meteo block, the
 * global irradiance of the radiation block and the transmissivity map it read. */
sf3d_error_t sf3d_hour_et0(uint32_t nrCells, float clearSkyTransmissivity);

/* sf3d_sink_compute_hour(nrCells, NULL, NULL, NULL, NULL) (assignETreal and assignPrecipitation, criteria3DProject.cpp:796-964): ET0, LAI
 * and degree days of the crop block, the liquid water of the snow block - and, where no snow hour was done on this raster, the meteo
 * block's precipitation map (assignPrecipitation:943 with isSnow false). */
sf3d_error_t sf3d_hour_sinks(uint32_t nrCells);

/* totals[0..2] = totalPrecipitation, totalEvaporation, totalTranspiration [m3 h-1] of the last sink hour, the terms of the mass balance of
 * runWaterFluxes3DModel (src/project3D/project3D.cpp:1307-1386).  Precipitation: over the cells with a surface node in the column table,
 * area * (liquidWater / 1000.) where the liquid water map that hour read is not the flag and > 0 (criteria3DProject.cpp:939-957);
 * evaporation and transpiration: area * (actual / 1000.) of the cells that hour computed (:827-829, :867-870).  Each term in doubles as
 * written; the sum in a fixed order (a tree per block of 256 cells, then the block partials by index), without atomics: the same bits on
 * every run.  The reference's own order is an OpenMP reduction.  Multi-GPU: a rank sums its cells, the caller adds the ranks. */
sf3d_error_t sf3d_hour_totals(uint32_t nrCells, double* totals);

/* What Project3D::computeCurrentPond (src/project3D/project3D.cpp:1779-1816) reads that does not change during a run; call once (a second
 * call replaces the raster).  slopeDegree: radiationMaps->slopeMap [deg] with its flag; landUnitIndex: per cell getLandUnitIndexRowCol,
 * -1 (any negative value) for NODATA; per land unit landUnitList[u].pond [m], cropList[u].LAImax and isCrop(u); computeCrop:
 * processes.computeCrop.  tan(slopeDegree * DEG_TO_RAD) is evaluated here, on the host, with the C library.  No device is needed yet. */
sf3d_error_t sf3d_hour_set_ponds(uint32_t nrRows, uint32_t nrCols, const float* slopeDegree, float slopeFlag, const int32_t* landUnitIndex, uint32_t nUnits,
                                 const double* maximumPond, const double* laiMax, const int32_t* isCrop, int computeCrop);

/* Project3D::dailyUpdatePond (project3D.cpp:1819-1843): the day's pond of every cell with a surface node (the column table of
 * sf3d_maps.h), a slope and a land unit - with computeCrop from the LAI map the crop block holds - set on the cell's surface node as
 * sf3d_set_nodes_pond sets it; the nodes of the other cells keep their pond.  pondMap: nrCells floats or NULL; -9999 in the cells that
 * were skipped.  Multi-GPU: a rank sets the surface nodes of the cells it owns. */
sf3d_error_t sf3d_hour_update_ponds(uint32_t nrCells, float* pondMap);

/* event-timed duration [ms] of the last k_hour_relhum (0), k_hour_totals (1, both passes) or k_hour_pond (2) launch when sf3d_kernel_timing is
 * on, else 0 */
double sf3d_hour_kernel_ms(int which);

/* forgets sf3d_hour_set_ponds and frees what the calls of this header allocated; sf3d_clean does the same */
sf3d_error_t sf3d_hour_clean(void);

#ifdef __cplusplus
}
#endif

#endif
