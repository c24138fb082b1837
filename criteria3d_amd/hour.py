"""The application's hour, device to device (include/sf3d_hour.h, criteria3d_amd/csrc/sf3d_hour.inc): `Crit3DProject::runModelHour`
(bin/CRITERIA3D/criteria3DProject.cpp:2074-2189) with no raster crossing the bus between its stages, and the day around it
(`runModels`, :1223-1304).

Three parts:
  * the binding (`bind` and thin wrappers of the seven calls): the snow, ET0 and sink hours on the maps the feeding blocks hold, the relative
    humidity map from the dew point map, the hour's three totals, the day's ponds; a missing kernel or library is an error;
  * `run_hour` / `run_day`: the hour and the day driven through the blocks, station values in, balance out;
  * `restate_relative_humidity`, `restate_pond`, `restate_totals`: the point functions on whole maps in numpy with the reference's operation
    order and the C library's exp / pow / tan (python's `math`) - the checkers of the CPU tests against the compiled-reference pins
    (tests/golden/relhum_dew.npz, pond_day.npz).  Checkers, never a fallback."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi, crop, meteo, radiation, raster, root, sinks, snow, transmissivity
from .capi import pf32, pi32

NODATA = -9999.0
EPSILON = 0.00001                               # commonConstants.h:252
DEG_TO_RAD = 0.01745329252                      # commonConstants.h:255
CLEAR_SKY_TRANSMISSIVITY_DEFAULT = 0.75         # solarRadiation/radiationDefinitions.h:33
MAX_UNITS = 64                                  # SF3D_CROP_MAX_UNITS
TOTALS = ("precipitation", "evaporation", "transpiration")
KERNEL_RELHUM, KERNEL_TOTALS, KERNEL_POND = 0, 1, 2
BND_RUNOFF, BND_FREE_DRAINAGE, BND_FREE_LATERAL_DRAINAGE = 1, 2, 3          # sf3d_boundary_t

pf64 = C.POINTER(C.c_double)
# name -> (restype, argtypes): every symbol include/sf3d_hour.h declares
SIGNATURES = {
    "sf3d_hour_relative_humidity": (capi.u8, [capi.u32, pf32]),
    "sf3d_hour_snow": (capi.u8, [capi.u32, pf32, capi.f64]),
    "sf3d_hour_et0": (capi.u8, [capi.u32, capi.f32]),
    "sf3d_hour_sinks": (capi.u8, [capi.u32]),
    "sf3d_hour_totals": (capi.u8, [capi.u32, pf64]),
    "sf3d_hour_set_ponds": (capi.u8, [capi.u32, capi.u32, pf32, capi.f32, pi32, capi.u32, pf64, pf64, pi32, capi.i32]),
    "sf3d_hour_update_ponds": (capi.u8, [capi.u32, pf32]),
    "sf3d_hour_kernel_ms": (capi.f64, [capi.i32]),
    "sf3d_hour_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_hour.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def _cells(shape) -> int:
    return int(shape[0]) * int(shape[1])


def relative_humidity(sf: capi.SF3D, download: bool = True):
    """computeRelativeHumidityMap: the meteo block's humidity map from its air and dew temperature maps; download=False: the map stays
    on the device (meteo.get_map(sf, "relHum"))"""
    bind(sf)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_hour_relative_humidity(_cells(sf._meteo_shape), out.ctypes.data_as(pf32) if download else pf32()), "hour_relative_humidity")
    return out


def snow_hour(sf: capi.SF3D, surface_water=None, clear_sky: float = CLEAR_SKY_TRANSMISSIVITY_DEFAULT) -> None:
    """snow.compute_hour on the maps the meteo and radiation blocks hold; surface_water [mm]: a map, or None (0, as the application passes)"""
    bind(sf)
    w = None if surface_water is None else raster.f32(surface_water, sf._snow_shape, "snow")
    sf.check(sf.lib.sf3d_hour_snow(_cells(sf._snow_shape), w.ctypes.data_as(pf32) if w is not None else pf32(), float(clear_sky)), "hour_snow")


def et0_hour(sf: capi.SF3D, clear_sky: float = CLEAR_SKY_TRANSMISSIVITY_DEFAULT) -> None:
    """crop.compute_hour on the maps the meteo and radiation blocks hold (a run without the snow model)"""
    bind(sf)
    sf.check(sf.lib.sf3d_hour_et0(_cells(sf._crop_shape), float(clear_sky)), "hour_et0")


def sink_hour(sf: capi.SF3D) -> None:
    """sinks.compute_hour with every map read in place; without a snow hour on the raster the rain is the meteo block's precipitation map"""
    bind(sf)
    sf.check(sf.lib.sf3d_hour_sinks(_cells(sf._sink_shape)), "hour_sinks")


def totals(sf: capi.SF3D) -> np.ndarray:
    """(totalPrecipitation, totalEvaporation, totalTranspiration) [m3 h-1] of the last sink hour"""
    bind(sf)
    out = np.zeros(3, np.float64)
    sf.check(sf.lib.sf3d_hour_totals(_cells(sf._sink_shape), out.ctypes.data_as(pf64)), "hour_totals")
    return out


def set_ponds(sf: capi.SF3D, slope_degree, land_unit_index, maximum_pond, lai_max, is_crop, compute_crop: bool, slope_flag: float = NODATA) -> None:
    """what computeCurrentPond reads that does not change: the slope map [deg] with its flag, the land unit per cell (negative: none) and, per
    land unit, landUnitList[u].pond [m], cropList[u].LAImax and isCrop(u); needs no device"""
    bind(sf)
    slope = np.ascontiguousarray(slope_degree, np.float32)
    idx = raster.i32(land_unit_index, slope.shape, "pond")
    mp, lm = np.ascontiguousarray(maximum_pond, np.float64), np.ascontiguousarray(lai_max, np.float64)
    ic = np.ascontiguousarray(is_crop, np.int32)
    if not (mp.shape == lm.shape == ic.shape and mp.ndim == 1):
        raise ValueError("maximum_pond, lai_max and is_crop differ in length")
    sf._pond_shape = slope.shape
    sf.check(sf.lib.sf3d_hour_set_ponds(slope.shape[0], slope.shape[1], slope.ctypes.data_as(pf32), float(slope_flag), idx.ctypes.data_as(pi32), len(mp),
                                        mp.ctypes.data_as(pf64), lm.ctypes.data_as(pf64), ic.ctypes.data_as(pi32), int(bool(compute_crop))), "hour_set_ponds")


def update_ponds(sf: capi.SF3D, download: bool = True):
    """dailyUpdatePond: the day's pond on the surface node of every cell that has one, a slope and a land unit; the pond map, -9999 where
    the cell was skipped"""
    bind(sf)
    out = np.empty(sf._pond_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_hour_update_ponds(_cells(sf._pond_shape), out.ctypes.data_as(pf32) if download else pf32()), "hour_update_ponds")
    return out


def kernel_ms(sf: capi.SF3D, which: int) -> float:
    bind(sf)
    return float(sf.lib.sf3d_hour_kernel_ms(int(which)))


def clean(sf: capi.SF3D) -> None:
    bind(sf)
    sf.check(sf.lib.sf3d_hour_clean(), "hour_clean")


# ------------------------------------------------------------------------------------------------ the hour and the day

DEFAULT_PROCESSES = dict(computeSnow=True, computeCrop=True, useDewPoint=True, method="idw", settings=None,
                         clearSkyTransmissivity=CLEAR_SKY_TRANSMISSIVITY_DEFAULT, surfaceWater=None, surfaceArea=None)


def _interpolate(sf, name, stations, processes):
    x, y, v, area, *own = stations[name]
    meteo.interpolate(sf, name, processes["method"], x, y, v, area, own[0] if own else processes["settings"], download=False)


def run_hour(sf: capi.SF3D, when, stations: dict, processes: dict | None = None) -> dict:
    """runModelHour at `when` = (year, month, day, hour, minute, second) on blocks that are initialised on one raster, for a prepared
    station list per variable (preInterpolation stays with the caller): stations[name] = (x, y, value, bounding_box_area[, settings]) as
    meteo.interpolate takes them, for "airT", "prec", "windInt" and "dewT" (processes["useDewPoint"], the application's default) or
    "relHum"; stations["transmissivity"] = dict(width, time_step_second, points [n, 5] (x, y, z, lat, lon), measured [n, width], area
    [, settings]) as transmissivity.points takes them.  Nothing but station values goes up and nothing but the balance comes down.
    processes: DEFAULT_PROCESSES and what differs from them; "surfaceArea" [m2]: cellSize^2 * nrSurfaceNodes, what the balance's error in mm
    divides by (project3D.cpp:1380; None: no figure in mm).  Returns the balance runWaterFluxes3DModel logs (project3D.cpp:1307-1386)."""
    p = dict(DEFAULT_PROCESSES)
    p.update(processes or {})
    bind(sf)
    clear_sky = float(p["clearSkyTransmissivity"])
    # the four meteo maps (:2084-2100); the humidity from the dew point where the settings say so (project3D.cpp:1848-1878)
    _interpolate(sf, "airT", stations, p)
    _interpolate(sf, "prec", stations, p)
    if p["useDewPoint"]:
        _interpolate(sf, "dewT", stations, p)
        relative_humidity(sf, download=False)
    else:
        _interpolate(sf, "relHum", stations, p)
    _interpolate(sf, "windInt", stations, p)
    # globalIrradiance (:2102-2108): station transmissivity, its map, the radiation maps
    tr = stations["transmissivity"]
    points = transmissivity.point_array(tr["points"])
    values, _ = transmissivity.points(sf, when, tr["width"], tr["time_step_second"], points, tr["measured"])
    has = np.abs(values.astype(np.float64) - NODATA) >= EPSILON
    meteo.interpolate(sf, "transmissivity", p["method"], points[has, 0], points[has, 1], values[has], tr["area"], tr.get("settings", p["settings"]), download=False)
    radiation.compute_hour(sf, when, None)
    # the snow model (:2110-2119), ET0 and the daily extremes (:2130-2146)
    if p["computeSnow"]:
        snow_hour(sf, p["surfaceWater"], clear_sky)
        crop.compute_hour(sf, None, clear_sky)
    else:
        et0_hour(sf, clear_sky)
    # assignETreal, assignPrecipitation, setSinkSource (:2148-2161)
    root.compute(sf, None)
    sink_hour(sf)
    sinks.apply(sf)
    tot = totals(sf)
    return run_water_fluxes(sf, tot, p["surfaceArea"])


def run_water_fluxes(sf: capi.SF3D, tot, surface_area: float | None = None, total_time_step: float = 3600.0) -> dict:
    """runWaterFluxes3DModel (project3D.cpp:1307-1386) for the three totals of the hour: initializeBalance, the computeStep loop, the balance"""
    lib = sf.lib
    sf.check(lib.sf3d_initialize_balance(), "initialize_balance")
    previous = float(lib.sf3d_get_total_water_content())
    t, steps = 0.0, 0
    while t < total_time_step:
        dt = lib.sf3d_compute_step(total_time_step - t)
        if not (dt > 0.0):
            raise capi.SF3DError(f"{sf.backend}: compute_step returned {dt}")
        t += dt
        steps += 1
    runoff = float(lib.sf3d_get_total_boundary_water_flow(BND_RUNOFF))
    free_drainage = float(lib.sf3d_get_total_boundary_water_flow(BND_FREE_DRAINAGE))
    lateral_drainage = float(lib.sf3d_get_total_boundary_water_flow(BND_FREE_LATERAL_DRAINAGE))
    forecast = previous + runoff + free_drainage + lateral_drainage + float(tot[0]) - float(tot[1]) - float(tot[2])
    current = float(lib.sf3d_get_total_water_content())
    error = current - forecast
    return dict(previousTotalWaterContent=previous, currentWaterContent=current, runoff=runoff, freeDrainage=free_drainage, lateralDrainage=lateral_drainage,
                totalPrecipitation=float(tot[0]), totalEvaporation=float(tot[1]), totalTranspiration=float(tot[2]), massBalanceError=error,
                massBalanceError_mm=None if not surface_area else error / surface_area * 1000, steps=steps)


def run_day(sf: capi.SF3D, date, hours, stations_of, processes: dict | None = None, previous_hour: int = 23, date_doy: int | None = None) -> list:
    """one date of runModels (criteria3DProject.cpp:1223-1304): the crop maps' daily update when the hour before was the day's last (and
    computeCrop), the day's ponds, then run_hour for every hour of `hours`.  date = (year, month, day); stations_of(hour) -> the stations of
    run_hour; date_doy: the date's day of the year (computed when None).  Returns the hours' balances."""
    import datetime
    p = dict(DEFAULT_PROCESSES)
    p.update(processes or {})
    doy = date_doy if date_doy is not None else datetime.date(*map(int, date)).timetuple().tm_yday
    if p["computeCrop"] and previous_hour == 23:
        crop.daily_update(sf, doy)
    update_ponds(sf, download=False)
    return [run_hour(sf, tuple(date) + (int(h), 0, 0), stations_of(h), p) for h in hours]


# ------------------------------------------------------------------------------------------------ restatement (checkers)

_exp = np.frompyfunc(math.exp, 1, 1)
_pow = np.frompyfunc(math.pow, 2, 1)
_tan = np.frompyfunc(math.tan, 1, 1)


def _lib(fn, *a):
    """the C library's function, element by element (numpy's own exp / pow / tan are other algorithms)"""
    return fn(*a).astype(np.float64)


def _eq(a, b):
    """isEqual (basicMath.h:25-29) on arrays: both operands widened to double"""
    return np.abs(np.asarray(a).astype(np.float64) - np.float64(b)) < EPSILON


def rel_hum_from_tdew(td, t) -> np.ndarray:
    """relHumFromTdew(float Td, float T) (meteo.cpp:301-315) on float32 arrays -> float32"""
    td, t = np.asarray(td, np.float32), np.asarray(t, np.float32)
    out = np.full(td.shape, np.float32(NODATA), np.float32)
    ok = ~(_eq(td, NODATA) | _eq(t, NODATA))
    if ok.any():
        d, c = 237.3, 17.2693882
        tdd, tt = td[ok].astype(np.float64), t[ok].astype(np.float64)
        esp = 1 / (tt + d)
        rh = _lib(_pow, _lib(_exp, (c * tdd) - ((c * tt / (tt + d))) * (tdd + d)), esp)
        rh = rh * 100
        f = rh.astype(np.float32)
        out[ok] = np.where(rh > 100, np.float32(100), np.where(np.float32(1) < f, f, np.float32(1)))
    return out


def restate_relative_humidity(air_t, dew_t, flag: float = NODATA, mine=None) -> np.ndarray:
    """computeRelativeHumidityMap (meteoMaps.cpp:301-321): the flag where either input holds it (the emptied grid), relHumFromTdew elsewhere;
    mine: the cells this rank computes (the flag in the others)"""
    air_t, dew_t = np.asarray(air_t, np.float32), np.asarray(dew_t, np.float32)
    fl = float(np.float32(flag))
    out = np.full(air_t.shape, np.float32(flag), np.float32)
    ok = ~_eq(air_t, fl) & ~_eq(dew_t, fl)
    if mine is not None:
        ok &= np.asarray(mine, bool)
    out[ok] = rel_hum_from_tdew(dew_t[ok], air_t[ok])
    return out


def restate_pond(slope_degree, land_unit_index, maximum_pond, lai_max, is_crop, compute_crop: bool, lai=None, slope_flag: float = NODATA, lai_flag: float = NODATA,
                 surface_index=None, mine=None) -> np.ndarray:
    """computeCurrentPond (project3D.cpp:1779-1816) per cell -> float32, -9999 where it returns NODATA; surface_index (the index map of
    layer 0, negative: no node) and mine: the cells dailyUpdatePond (:1819-1843) skips hold -9999 too"""
    slope = np.asarray(slope_degree, np.float32)
    idx = np.asarray(land_unit_index)
    out = np.full(slope.shape, np.float32(NODATA), np.float32)
    ok = ~_eq(slope, float(np.float32(slope_flag))) & (idx >= 0)
    if surface_index is not None:
        ok &= np.asarray(surface_index) >= 0
    if mine is not None:
        ok &= np.asarray(mine, bool)
    if not ok.any():
        return out
    u = idx[ok]
    tan_slope = _lib(_tan, slope[ok].astype(np.float64) * DEG_TO_RAD)
    maximum = np.asarray(maximum_pond, np.float64)[u]
    soil = maximum / (tan_slope + 1.)
    interception = np.zeros(soil.shape)
    if compute_crop:
        crop_cell = np.asarray(is_crop)[u] != 0
        soil = np.where(crop_cell, soil * 0.5, soil)
        current = np.asarray(lai, np.float32)[ok]
        has = crop_cell & ~_eq(current, float(np.float32(lai_flag)))
        with np.errstate(divide="ignore", invalid="ignore"):
            share = current.astype(np.float64) / np.asarray(lai_max, np.float64)[u]
        interception = np.where(has, maximum * 0.5 * share, 0.0)
    out[ok] = (soil + interception).astype(np.float32)
    return out


def total_terms(surface_index, dem, flag: float, area: float, liquid_water, evaporation, transpiration, mine=None) -> np.ndarray:
    """[3, cells] float64, row-major: the terms of totalPrecipitation (criteria3DProject.cpp:939-957: a surface node, liquid water that is not
    the flag and > 0), totalEvaporation (:827-829) and totalTranspiration (:867-870: the cells the sink hour computed - a surface node and a
    DEM value), 0 elsewhere"""
    fl = float(np.float32(flag))
    rain = np.asarray(surface_index).ravel() >= 0
    if mine is not None:
        rain &= np.asarray(mine, bool).ravel()
    sunk = rain & ~_eq(np.asarray(dem, np.float32).ravel(), fl)
    liquid = np.asarray(liquid_water, np.float32).ravel()
    wet = rain & ~_eq(liquid, fl) & (liquid > 0)
    terms = np.zeros((3, rain.size), np.float64)
    terms[0][wet] = area * (liquid[wet].astype(np.float64) / 1000.)
    terms[1][sunk] = area * (np.asarray(evaporation, np.float64).ravel()[sunk] / 1000.)
    terms[2][sunk] = area * (np.asarray(transpiration, np.float64).ravel()[sunk] / 1000.)
    return terms


def restate_totals(surface_index, dem, flag: float, area: float, liquid_water, evaporation, transpiration, mine=None) -> np.ndarray:
    """the three totals as a sequential row-major sum of total_terms"""
    out = np.zeros(3, np.float64)
    for q, row in enumerate(total_terms(surface_index, dem, flag, area, liquid_water, evaporation, transpiration, mine)):
        s = 0.0
        for v in row.tolist():
            s += v
        out[q] = s
    return out
