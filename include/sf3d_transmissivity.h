/*
 * sf3d_transmissivity.h - the clear-sky ratio of every radiation station over a time window, and the width of that window, on the
 * MI355X: the two values at the head of Project::interpolateDemRadiation (agrolib/project/project.cpp:3401-3406) that go into the
 * interpolation of the transmissivity map - computeTransmissivity (agrolib/solarRadiation/transmissivity.cpp:105-169) through
 * radiation::computePointTransmissivity (agrolib/solarRadiation/solarRadiation.cpp:1265-1367), and
 * radiation::estimateTransmissivityWindow (:835-922).  One kernel launch per call (k_transmissivity_points: one wave64 per station, a
 * lane per evaluation of computeRadiationRsun, one lane adds up in the reference's order).  With sf3d_meteo_interpolate
 * (SF3D_METEO_ATM_TRANSMISSIVITY) and sf3d_rad_compute_hour(..., NULL) after it the radiation chain of an hour runs on the device.
 *
 * The block works on the raster and the settings of sf3d_rad_initialize (include/sf3d_rad.h): the DEM the shadow rays cross, the
 * clear-sky value, the Linke factor, the shadowing switch, the time zone.  The stations are horizontal (slope 0, aspect 180), both
 * transmissivities of an evaluation are the clear-sky value and the temperature is TEMPERATURE_DEFAULT, as in the reference.  The
 * bar is the compiled reference's float and int results (tests/golden/transmissivity.npz); DESIGN 20 states what is kept and where
 * equality is expected rather than guaranteed.
 *
 * With the caller: the station series and their quality control, computeTransmissivityFromTRange's walk over the day's records
 * (criteria3d_amd.transmissivity.samani is its point formula), the output-point variant (computeRadiationOutputPoints), the Brooks
 * point model, and feeding the snow and ET0 kernels from device maps.
 *
 * This header extends the product library only (libsf3d_hip.so); it is not part of the soilFluxes3D drop-in ABI of sf3d.h.  Its scratch
 * belongs to the radiation block: it survives sf3d_initialize and goes with sf3d_rad_clean / sf3d_clean.  No call touches the solver's
 * state or the radiation maps.  With several ranks every rank computes every point (points are not cells; a rank's DEM is the whole DEM).
 *
 * Errors: SF3D_PARAMETER_ERROR, before any device work - a null pointer; a window width that is even, not positive or above
 * SF3D_TRANSMISSIVITY_MAX_WIDTH; more than SF3D_TRANSMISSIVITY_MAX_POINTS points; timeStepSecond <= 0 or above 86 400; a centre date or
 * time that is none; sf3d_transmissivity_get_evaluations with sizes other than the last call's; and, once the radiation block is there,
 * Linke or albedo in map mode with a point whose row or column is outside the raster (the reference indexes its map out of bounds
 * there, radiationSettings.cpp:138-154, 186-202; inside the raster it yields NODATA, as sf3d_rad.h says) and, for the window, a point
 * or a noon S_solpos refuses (the reference would read an unset sunPosition).  SF3D_MEMORY_ERROR: no sf3d_rad_initialize.
 * SF3D_SOLVER_ERROR: a HIP failure.
 */
#ifndef SF3D_TRANSMISSIVITY_H
#define SF3D_TRANSMISSIVITY_H

#include <stdint.h>

#include "sf3d.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SF3D_TRANSMISSIVITY_MAX_WIDTH = 63, SF3D_TRANSMISSIVITY_MAX_POINTS = 65536, SF3D_TRANSMISSIVITY_WINDOW_SLOTS = 24 };

/* gis::Crit3DPoint of a station with its latitude and longitude [deg] (gis::getLatLonFromUtm, gis.cpp:847-850:
 * criteria3d_amd.radiation.utm_to_latlon).  z is a height [m]: a caller resolves a NODATA height through gis::getValueFromXY
 * (gis.cpp:533-546; criteria3d_amd.transmissivity.station_points) before the call, as solarRadiation.cpp:1280-1282 does */
typedef struct {
    double x, y, z;
    double lat, lon;
} sf3d_transmissivity_point_t;

/* radiation::estimateTransmissivityWindow(settings, point, Crit3DTime(date, hour:minute:second), dem, timeStepSecond)
 * (solarRadiation.cpp:835-922) for one point: the number of steps (1, 3, .. 23) whose clear-sky radiation adds up to a quarter of the
 * noon value (at least 50 W m-2), counting only steps with the sun above 3 degrees.  Noon, the centre and the 22 candidate steps are
 * evaluated in one launch (sf3d_transmissivity_get_evaluations: windowWidth = SF3D_TRANSMISSIVITY_WINDOW_SLOTS, in the order noon,
 * centre, -1, +1, -2, +2, ..) */
sf3d_error_t sf3d_transmissivity_window(int year, int month, int day, int hour, int minute, int second, int timeStepSecond,
                                        const sf3d_transmissivity_point_t* point, int32_t* windowSteps);

/* computeTransmissivity(settings, meteoPoints, windowWidth, Crit3DTime(date, hour:minute:second), dem) (transmissivity.cpp:105-169) with
 * dt = timeStepSecond: measured[p * windowWidth + i] is station p's global irradiance at time + (i - (windowWidth - 1) / 2) *
 * timeStepSecond, NODATA (-9999) where it has none.  transmissivity[p] = float(Kt * clearSky) of computePointTransmissivity
 * (solarRadiation.cpp:1265-1367), NODATA where the centre measurement is NODATA or fewer than 0.66 * windowWidth are there; *nValid: the
 * number of stations with a result (the reference returns nValid > 0).  nPoints == 0 is allowed */
sf3d_error_t sf3d_transmissivity_points(int year, int month, int day, int hour, int minute, int second, int windowWidth, int timeStepSecond,
                                        uint32_t nPoints, const sf3d_transmissivity_point_t* points, const float* measured,
                                        float* transmissivity, uint32_t* nValid);

/* what the last call evaluated per (point, slot), [nPoints][windowWidth]: written - computeRadiationRsun (solarRadiation.cpp:700-832)
 * wrote radPoint.global (0: skipped, or it returned false); elevationRefr - sunPosition.elevationRefr, NODATA where the sun position
 * was not computed; global - radPoint.global as the double it is, NODATA where not written.  For diagnostics and tests */
sf3d_error_t sf3d_transmissivity_get_evaluations(uint32_t nPoints, int windowWidth, uint8_t* written, float* elevationRefr, double* global);

/* milliseconds of the last launch of k_transmissivity_points, which stands for the evaluations and sums of solarRadiation.cpp:1300-1366 or
 * :880-919 (0 unless sf3d_kernel_timing is on) */
double sf3d_transmissivity_kernel_ms(void);

#ifdef __cplusplus
}
#endif

#endif
