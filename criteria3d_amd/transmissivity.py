"""Station transmissivity and its window on the device (include/sf3d_transmissivity.h, criteria3d_amd/csrc/sf3d_transmissivity.inc): the
two values at the head of `Project::interpolateDemRadiation` (agrolib/project/project.cpp:3401-3406) - `computeTransmissivity`
(agrolib/solarRadiation/transmissivity.cpp:105-169) over `radiation::computePointTransmissivity`
(agrolib/solarRadiation/solarRadiation.cpp:1265-1367), and `radiation::estimateTransmissivityWindow` (:835-922).

Three parts:
  * the binding (`bind`, `window`, `points`, `evaluations`, `kernel_ms`) on the raster and settings of `radiation.initialize`; a missing
    kernel or library is an error;
  * `station_points`: latitude and longitude from `radiation.utm_to_latlon`, a NODATA height from the DEM (gis::getValueFromXY);
  * the restatement of the three reference functions on `radiation.rad_eval`'s pieces (`restate_points`, `restate_point`,
    `restate_window`), which reports the arms a call took (ARMS) - the checker of the CPU tests against the compiled-reference pin
    (tests/golden/transmissivity.npz) and of the GPU tests off the pin.  A checker, never a fallback.
`samani` is computePointTransmissivitySamani (transmissivity.cpp:36-45), the point formula of the temperature-range estimate."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi, radiation as rad
from .radiation import NODATA, f32

MAX_WIDTH, MAX_POINTS, WINDOW_SLOTS = 63, 65536, 24
MAX_STEPS, MIN_ELEV = 23, 3.0                   # solarRadiation.cpp:838-839
EPSILON = rad.EPSILON


class Point(C.Structure):
    """sf3d_transmissivity_point_t"""
    _fields_ = [(n, C.c_double) for n in ("x", "y", "z", "lat", "lon")]


ppoint = C.POINTER(Point)
pu8, pu32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
_when = [capi.i32] * 6
# name -> (restype, argtypes): every symbol include/sf3d_transmissivity.h declares
SIGNATURES = {
    "sf3d_transmissivity_window": (capi.u8, _when + [capi.i32, ppoint, capi.pi32]),
    "sf3d_transmissivity_points": (capi.u8, _when + [capi.i32, capi.i32, capi.u32, ppoint, capi.pf32, capi.pf32, pu32]),
    "sf3d_transmissivity_get_evaluations": (capi.u8, [capi.u32, capi.i32, pu8, capi.pf32, capi.pd]),
    "sf3d_transmissivity_kernel_ms": (capi.f64, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_transmissivity.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def point_array(stations) -> np.ndarray:
    """[n, 5] float64 (x, y, z, lat, lon), the memory layout of sf3d_transmissivity_point_t[n]"""
    a = np.ascontiguousarray(stations, np.float64)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("transmissivity: stations are rows of (x, y, z, lat, lon)")
    return a


def station_points(x, y, z, gis_settings: dict | None, dem, header: dict, flag: float = NODATA) -> np.ndarray:
    """the stations of a call: latitude and longitude by gis::getLatLonFromUtm, a NODATA height resolved through gis::getValueFromXY
    (gis.cpp:533-546: the DEM's value at the point's cell, the DEM's flag outside), as solarRadiation.cpp:1280-1282 does"""
    g = dict(rad.DEFAULT_GIS)
    g.update(gis_settings or {})
    dem = np.asarray(dem, np.float32)
    nrows, ncols = dem.shape
    xll, yll, cs = float(header["xllcorner"]), float(header["yllcorner"]), float(header["cellsize"])
    inv = 1.0 / cs
    out = np.empty((len(x), 5), np.float64)
    for k, (px, py, pz) in enumerate(zip(x, y, z)):
        px, py, pz = float(px), float(py), float(pz)
        if abs(pz - NODATA) < EPSILON:
            row = (nrows - 1) - int((py - yll) * inv)
            col = int((px - xll) * inv)
            pz = float(dem[row, col]) if (0 <= row < nrows and 0 <= col < ncols) else float(np.float32(flag))
        lat, lon = rad.utm_to_latlon(g["utmZone"], g["startLatitude"], px, py)
        out[k] = (px, py, pz, lat, lon)
    return out


def window(sf: capi.SF3D, when, time_step_second: int, station) -> int:
    """estimateTransmissivityWindow for one station (x, y, z, lat, lon) at `when` = (year, month, day, hour, minute, second)"""
    bind(sf)
    p = point_array(station)
    steps = C.c_int32(0)
    sf.check(sf.lib.sf3d_transmissivity_window(*map(int, when), int(time_step_second), p.ctypes.data_as(ppoint), C.byref(steps)), "transmissivity_window")
    return int(steps.value)


def points(sf: capi.SF3D, when, width: int, time_step_second: int, stations, measured):
    """computeTransmissivity -> (transmissivity [n] float32, nValid); measured: [n, width] float32, NODATA where a station has no value"""
    bind(sf)
    p = point_array(stations) if len(stations) else np.zeros((0, 5), np.float64)
    m = np.ascontiguousarray(measured, np.float32).reshape(len(p), int(width))
    out = np.empty(len(p), np.float32)
    n_valid = C.c_uint32(0)
    sf.check(sf.lib.sf3d_transmissivity_points(*map(int, when), int(width), int(time_step_second), len(p), p.ctypes.data_as(ppoint),
                                               m.ctypes.data_as(capi.pf32), out.ctypes.data_as(capi.pf32), C.byref(n_valid)), "transmissivity_points")
    return out, int(n_valid.value)


def evaluations(sf: capi.SF3D, n_points: int, width: int):
    """what the last call evaluated -> (written [n, width] uint8, elevationRefr [n, width] float32, global [n, width] float64)"""
    bind(sf)
    w = np.empty((n_points, width), np.uint8)
    e = np.empty((n_points, width), np.float32)
    g = np.empty((n_points, width), np.float64)
    sf.check(sf.lib.sf3d_transmissivity_get_evaluations(int(n_points), int(width), w.ctypes.data_as(pu8), e.ctypes.data_as(capi.pf32),
                                                        g.ctypes.data_as(capi.pd)), "transmissivity_get_evaluations")
    return w, e, g


def kernel_ms(sf: capi.SF3D) -> float:
    bind(sf)
    return float(sf.lib.sf3d_transmissivity_kernel_ms())


def samani(tmin: float, tmax: float, coeff: float) -> float:
    """computePointTransmissivitySamani, transmissivity.cpp:36-45: NODATA without its inputs, `return false` = 0 for tmin > tmax"""
    if coeff != NODATA and tmin != NODATA and tmax != NODATA:
        if tmin <= tmax:
            return f32(f32(coeff) * f32(math.sqrt(f32(f32(tmax) - f32(tmin)))))
        return 0.0
    return NODATA


# ------------------------------------------------------------------------------------------------ restatement (checker)

ARMS = ("result NODATA: the centre measurement is NODATA", "result NODATA: validSamples < 0.66 width", "result computed",
        "backward slot skipped (NODATA)", "forward slot skipped (NODATA)", "slot added",
        "failed evaluation adds the previous value", "failed evaluation adds NODATA (none has written yet)",
        "sumClearSky <= 1e-6: Kt = 0", "Kt clamped to 1.2", "Kt below 1.2", "all measurements zero",
        "station outside the DEM: no ray", "station inside the DEM", "station above dem.maximum: the ray ends at once",
        "window: ends at 1", "window: ends in between", "window: ends at 23", "window: a step left out by the 3 degree filter",
        "window: a failed evaluation leaves the stale value")
_A = {n: 1 << k for k, n in enumerate(ARMS)}


def _eq(a: float, b: float) -> bool:
    return abs(a - b) < EPSILON             # isEqual


def grid_of(dem, flag, xll, yll, cell_size) -> dict:
    """the DEM as radiation.shadow reads it, with Crit3DRasterGrid::maximum (gis::updateMinMaxRasterGrid)"""
    dem = np.ascontiguousarray(dem, np.float32)
    d = dem.astype(np.float64)
    real = (np.abs(d - float(flag)) >= EPSILON) & (np.abs(d - NODATA) >= EPSILON)
    return dict(dem=dem, flag=np.float32(flag), xll=float(xll), yll=float(yll), cellsize=float(cell_size),
                demMax=float(dem[real].max()) if real.any() else NODATA)


def _hour(s: dict, when, offset: int, month: int):
    """the date-and-time terms of the slot `offset` seconds from `when`, or None when S_solpos refuses its date; month: of the time handed in"""
    y, mo, d, hh, mi, ss = map(int, when)
    h = rad.hour_setup((y, mo, d, hh, mi, ss + int(offset)), int(s["timeZone"]), bool(s["isUTC"]))
    if h is None:
        return None
    if s["linkeMode"] == rad.MODE_MONTHLY:
        h["linke"] = f32(s["linkeMonthly"][month - 1])
    else:
        h["linke"] = f32(s["linke"]) if s["linkeMode"] == rad.MODE_FIXED else NODATA
    h["albedo"] = f32(s["albedo"]) if s["albedoMode"] == rad.MODE_FIXED else NODATA
    h["clearSky"] = f32(s["clearSky"])
    h["realSky"], h["realSkyAlgorithm"], h["shadowing"] = bool(s["realSky"]), int(s["realSkyAlgorithm"]), bool(s["shadowing"])
    return h


class _Station:
    """radPoint and sunPosition of one reference call: what an evaluation leaves behind is what the next one finds"""

    def __init__(self, grid: dict, station):
        self.grid = grid
        self.x, self.y, self.z, lat, lon = map(float, station)
        self.cell = rad.cell_setup(self.z, f32(lat), f32(lon), 0.0, 180.0)
        nrows, ncols = grid["dem"].shape
        cs = grid["cellsize"]
        out = self.x < grid["xll"] or self.y < grid["yll"] or self.x >= grid["xll"] + ncols * cs or self.y >= grid["yll"] + nrows * cs
        self.march = not out                    # gis::isOutOfGridXY
        self.glob, self.elev = NODATA, None     # radPoint.global; sunPosition.elevationRefr (unset)
        self.arms = (_A["station inside the DEM"] if self.march else _A["station outside the DEM: no ray"])
        if self.march and self.z >= grid["demMax"]:
            self.arms |= _A["station above dem.maximum: the ray ends at once"]
        self.model_arms = 0
        self.record = []                        # (written, elevationRefr or NODATA, global or NODATA) per evaluation

    def evaluate(self, h) -> bool:
        """computeRadiationRsun (its return value is what the callers ignore)"""
        v, sun = None, []
        if h is not None:
            v, a = rad.rad_eval(self.grid, h, self.cell, self.x, self.y, self.z, self.march, float(h["clearSky"]), sun_out=sun)
            self.model_arms |= a
        if sun:
            self.elev = sun[0]["elevationRefr"]
        if v is not None:
            self.glob = v[1]
        else:
            self.arms |= _A["failed evaluation adds the previous value"] if self.record and any(r[0] for r in self.record) else \
                _A["failed evaluation adds NODATA (none has written yet)"]
        self.record.append((1 if v is not None else 0, sun[0]["elevationRefr"] if sun else NODATA, v[1] if v is not None else NODATA))
        return v is not None


def restate_point(grid: dict, settings: dict | None, when, station, measured, width: int, time_step_second: int):
    """radiation::computePointTransmissivity -> (float32 result, ARMS bits, model arm bits (radiation.ARMS), evaluations {slot: record})"""
    s = rad.settings_dict(settings)
    measured = [float(np.float32(m)) for m in measured]
    if width % 2 != 1:
        return NODATA, 0, 0, {}
    centre = (width - 1) // 2
    if measured[centre] == NODATA:
        return NODATA, _A["result NODATA: the centre measurement is NODATA"], 0, {}
    p = _Station(grid, station)
    month = int(when[1])
    slots = {}

    def run(i):
        p.evaluate(_hour(s, when, (i - centre) * time_step_second, month))
        slots[i] = p.record[-1]
    sum_ghi = measured[centre]
    run(centre)
    sum_clear = p.glob
    arms = _A["result computed"]
    for i in range(centre - 1, -1, -1):
        for j, skipped in ((i, "backward slot skipped (NODATA)"), (width - i - 1, "forward slot skipped (NODATA)")):
            if not _eq(measured[j], NODATA):
                sum_ghi += measured[j]
                run(j)
                sum_clear += p.glob
                arms |= _A["slot added"]
            else:
                arms |= _A[skipped]
    if sum_clear > 1e-6:
        kt = rad._div(sum_ghi, sum_clear)
    else:
        kt = 0.0
        arms |= _A["sumClearSky <= 1e-6: Kt = 0"]
    if 1.2 < kt:
        arms |= _A["Kt clamped to 1.2"]
    elif sum_clear > 1e-6:
        arms |= _A["Kt below 1.2"]
    if all(m == 0.0 for m in measured):
        arms |= _A["all measurements zero"]
    kt = rad._clamp(kt, 0.0, 1.2)
    return f32(kt * f32(s["clearSky"])), arms | p.arms, p.model_arms, slots


def restate_points(grid: dict, settings: dict | None, when, width: int, time_step_second: int, stations, measured):
    """computeTransmissivity -> (transmissivity [n] float32, nValid, ARMS bits [n], model arm bits [n], evaluations [n] of {slot: record})"""
    stations = point_array(stations) if len(stations) else np.zeros((0, 5))
    measured = np.ascontiguousarray(measured, np.float32).reshape(len(stations), width)
    if width % 2 != 1:
        raise ValueError("computeTransmissivity fails on an even width")
    out = np.full(len(stations), NODATA, np.float32)
    arms, model, evals = np.zeros(len(stations), np.int64), np.zeros(len(stations), np.int64), []
    for k, st in enumerate(stations):
        row = measured[k]
        evals.append({})
        if _eq(float(row[(width - 1) // 2]), NODATA):
            arms[k] = _A["result NODATA: the centre measurement is NODATA"]
            continue
        valid = sum(0 if _eq(float(m), NODATA) else 1 for m in row)
        if valid < width * 0.66:
            arms[k] = _A["result NODATA: validSamples < 0.66 width"]
            continue
        out[k], arms[k], model[k], evals[k] = restate_point(grid, settings, when, st, row, width, time_step_second)
    n_valid = int(sum(0 if _eq(float(v), NODATA) else 1 for v in out))
    return out, n_valid, arms, model, evals


def restate_window(grid: dict, settings: dict | None, when, station, time_step_second: int):
    """radiation::estimateTransmissivityWindow -> (windowSteps, ARMS bits, model arm bits), or (None, 0, 0) where the reference would read an
    unset sunPosition (S_solpos refuses the point or the noon)"""
    s = rad.settings_dict(settings)
    p = _Station(grid, station)
    month = int(when[1])
    y, mo, d = map(int, when[:3])
    noon = _hour(s, (y, mo, d, 12, 0, 0), -int(s["timeZone"]) * 3600 if s["isUTC"] else 0, month)
    if not p.cell["ok"] or noon is None:
        return None, 0, 0
    arms = 0
    p.evaluate(noon)
    quarter = f32(p.glob * 0.25)
    threshold = quarter if 50.0 < quarter else 50.0
    if not p.evaluate(_hour(s, when, 0, month)):
        arms |= _A["window: a failed evaluation leaves the stale value"]
    total = p.glob
    steps = 1
    k = 0
    while total < threshold and steps < MAX_STEPS:
        steps += 2
        k += 1
        for off in (-k * time_step_second, k * time_step_second):
            if not p.evaluate(_hour(s, when, off, month)):
                arms |= _A["window: a failed evaluation leaves the stale value"]
            if p.elev > MIN_ELEV:
                total += p.glob
            else:
                arms |= _A["window: a step left out by the 3 degree filter"]
    if steps == 1:
        arms |= _A["window: ends at 1"]
    else:
        arms |= _A["window: ends in between"] if steps < MAX_STEPS else _A["window: ends at 23"]
    return steps, arms | p.arms, p.model_arms
