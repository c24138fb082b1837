"""The hourly meteo maps from station data on the device (include/sf3d_meteo.h, criteria3d_amd/csrc/sf3d_meteo.inc): what the library
function `interpolate()` (agrolib/interpolation/interpolation.cpp:2502-2560) does for every DEM cell in the application's default non-local
set-up - `inverseDistanceWeighted`, `shepardIdw` or `modifiedShepardIdw` over `shepardSearchNeighbour`, `retrend` with single detrending and
the variable's tail - for the four or five calls of `interpolateAndSaveHourlyMeteo` an hour begins with (criteria3DProject.cpp:2084-2108).

Two parts:
  * the binding (`bind`, `initialize`, `interpolate`, `get_map`, `interpolate_hour` ...): one launch of k_meteo_idw per variable; a missing
    kernel or library is an error;
  * `restate_interpolate` (and `shepard_initial_radius`, `cell_centres`): the same arithmetic in numpy float32 / float64 with the
    reference's types and operation order - the checker of the CPU tests against the compiled-reference pin (tests/golden/meteo_idw.npz).
    A checker, never a fallback.

The point list (quality control, checkPrecipitationZero, preInterpolation with its regressions and detrendPoints) stays with the caller:
the calls take detrended station values and the fitted slopes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, raster
from .capi import pf32, pf64

NODATA = -9999.0
EPSILON = 0.00001                               # commonConstants.h:252
PI = 3.1415926535898                            # commonConstants.h:249
MAX_STATIONS = 1024                             # SF3D_METEO_MAX_STATIONS
MAX_PROXIES = 8                                 # SF3D_METEO_MAX_PROXIES
SHEPARD_MIN, SHEPARD_AVG, SHEPARD_MAX = 5, 8, 10                # interpolationConstants.h:6-8
VARIABLES = ("airT", "prec", "relHum", "windInt", "globalRad", "transmissivity", "dewT")       # the first five: the order snow.compute_hour takes them
AIR_TEMPERATURE, PRECIPITATION, AIR_REL_HUMIDITY, WIND_SCALAR_INTENSITY, GLOBAL_IRRADIANCE, ATM_TRANSMISSIVITY, AIR_DEW_TEMPERATURE = range(7)
IDW, SHEPARD, SHEPARD_MODIFIED = 0, 1, 2        # TInterpolationMethod (interpolationConstants.h:18)
METHODS = ("idw", "shepard", "shepard_modified")
DETRENDING_VARIABLES = (AIR_TEMPERATURE, AIR_DEW_TEMPERATURE)   # getUseDetrendingVar (interpolation.cpp:1205-1218) among VARIABLES

PROXY_INT_FIELDS = ("active", "isHeight", "inversion")
PROXY_FLOAT_FIELDS = ("slope", "lapseRateH0", "lapseRateH1", "inversionLapseRate")
UNSUPPORTED = ("useMultipleDetrending", "useLocalDetrending", "useTopographicDistance", "useKriging", "useSupplementalStations", "useCrossValidationIndex",
               "updateMinMax")


class Proxy(C.Structure):
    """sf3d_meteo_proxy_t"""
    _fields_ = [(n, C.c_int32) for n in PROXY_INT_FIELDS] + [(n, C.c_float) for n in PROXY_FLOAT_FIELDS] + [("reserved", C.c_int32)]


class Settings(C.Structure):
    """sf3d_meteo_settings_t"""
    _fields_ = [("allZero", C.c_int32), ("rainfallThreshold", C.c_float), ("useDetrending", C.c_int32)] + [(n, C.c_int32) for n in UNSUPPORTED] + \
               [("nProxies", C.c_int32), ("reserved", C.c_int32), ("proxy", Proxy * MAX_PROXIES)]


ppf32 = C.POINTER(pf32)
psettings = C.POINTER(Settings)
# name -> (restype, argtypes): every symbol include/sf3d_meteo.h declares
SIGNATURES = {
    "sf3d_meteo_initialize": (capi.u8, [capi.u32, capi.u32, pf32, capi.f32, capi.f64, capi.f64, capi.f64, capi.u32, ppf32]),
    "sf3d_meteo_interpolate": (capi.u8, [capi.i32, capi.i32, capi.u32, pf64, pf64, pf32, capi.f32, psettings, pf32]),
    "sf3d_meteo_get_map": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_meteo_set_map": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_meteo_kernel_ms": (capi.f64, []),
    "sf3d_meteo_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_meteo.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def settings_struct(settings: dict | None) -> Settings:
    """dict (allZero, rainfallThreshold, useDetrending, proxies: list of dicts with PROXY_*_FIELDS, any of UNSUPPORTED) -> sf3d_meteo_settings_t;
    more than MAX_PROXIES proxies keep their count (the library refuses it)"""
    s = settings or {}
    out = Settings()
    out.allZero = int(bool(s.get("allZero", 0)))
    out.rainfallThreshold = float(s.get("rainfallThreshold", 0.0))
    out.useDetrending = int(bool(s.get("useDetrending", 1)))
    for n in UNSUPPORTED:
        setattr(out, n, int(bool(s.get(n, 0))))
    proxies = s.get("proxies", [])
    out.nProxies = len(proxies)
    for k, p in enumerate(proxies[:MAX_PROXIES]):
        for n in PROXY_INT_FIELDS:
            setattr(out.proxy[k], n, int(bool(p.get(n, 0))))
        for n in PROXY_FLOAT_FIELDS:
            setattr(out.proxy[k], n, float(p.get(n, NODATA)))
    return out


def initialize(sf: capi.SF3D, dem, xll: float, yll: float, cell_size: float, proxy_maps=(), flag: float = NODATA) -> None:
    """the raster `dem` [rows, cols] with its lower-left corner and cell size, and one float raster per proxy of the settings, in their
    order; None in the place of the height proxy (its values are the DEM's)"""
    bind(sf)
    dem = np.ascontiguousarray(dem, np.float32)
    maps = [None if m is None else raster.f32(m, dem.shape, "meteo") for m in proxy_maps]
    ptrs = (pf32 * max(len(maps), 1))(*[pf32() if m is None else m.ctypes.data_as(pf32) for m in maps])
    sf._meteo_shape = dem.shape
    sf.check(sf.lib.sf3d_meteo_initialize(dem.shape[0], dem.shape[1], dem.ctypes.data_as(pf32), float(flag), float(xll), float(yll), float(cell_size),
                                          len(maps), ptrs), "meteo_initialize")


def interpolate(sf: capi.SF3D, var, method, x, y, value, bounding_box_area: float, settings: dict | None = None, download: bool = True):
    """one variable's map from the station list (x, y: doubles [m], value: floats, detrended where the variable is detrended);
    download=False: the map stays on the device (get_map)"""
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    v = np.ascontiguousarray(value, np.float32)
    if not (x.shape == y.shape == v.shape and x.ndim == 1):
        raise ValueError("x, y and value differ in length")
    st = settings_struct(settings)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_meteo_interpolate(raster.index(var, VARIABLES), raster.index(method, METHODS), len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64),
                                           v.ctypes.data_as(pf32), float(np.float32(bounding_box_area)), C.byref(st),
                                           out.ctypes.data_as(pf32) if download else pf32()), "meteo_interpolate")
    return out


def get_map(sf: capi.SF3D, var) -> np.ndarray:
    out = np.empty(sf._meteo_shape, np.float32)
    sf.check(sf.lib.sf3d_meteo_get_map(raster.index(var, VARIABLES), out.size, out.ctypes.data_as(pf32)), "meteo_get_map")
    return out


def set_map(sf: capi.SF3D, var, values) -> None:
    """a map the caller holds in the place of an interpolation of the variable"""
    v = raster.f32(values, sf._meteo_shape, "meteo")
    sf.check(sf.lib.sf3d_meteo_set_map(raster.index(var, VARIABLES), v.size, v.ctypes.data_as(pf32)), "meteo_set_map")


def interpolate_hour(sf: capi.SF3D, stations: dict, method, settings: dict | None = None) -> dict:
    """the hour's maps: stations[name] = (x, y, value, bounding_box_area[, settings]) for "airT", "prec", "relHum", "windInt" and,
    optionally, "globalRad"; returns the maps by the same names, in the order snow.compute_hour takes them"""
    names = [n for n in VARIABLES[:5] if n in stations]
    if names[:4] != list(VARIABLES[:4]):
        raise ValueError(f"stations of {VARIABLES[:4]} are needed, got {sorted(stations)}")
    out = {}
    for n in names:
        x, y, v, area, *own = stations[n]
        out[n] = interpolate(sf, n, method, x, y, v, area, own[0] if own else settings)
    return out


def kernel_ms(sf: capi.SF3D) -> float:
    return float(sf.lib.sf3d_meteo_kernel_ms())


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_meteo_clean(), "meteo_clean")


# ------------------------------------------------------------------------------------------------ restatement (checker)

f32 = np.float32
F_EPS = f32(EPSILON)


def shepard_initial_radius(bounding_box_area, n: int) -> np.float32:
    """computeShepardInitialRadius(area, n, SHEPARD_AVG_NRPOINTS) (interpolation.cpp:800-803): float products, the C library's sqrt"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (f32(SHEPARD_AVG) * f32(bounding_box_area)) / (f32(PI) * f32(n))            # unsigned -> float: exact
        return f32(np.sqrt(np.float64(q)))


def cell_centres(shape, xll: float, yll: float, cell_size: float):
    """gis::getUtmXYFromRowCol (gis.cpp:806-810) for every cell: doubles [rows, cols]"""
    rows, cols = shape
    r, c = np.mgrid[0:rows, 0:cols]
    return xll + cell_size * (c + 0.5), yll + cell_size * (rows - r - 0.5)


def _retrend(var: int, settings: dict, proxy_values) -> np.float32:
    """retrend (interpolation.cpp:1288-1351), single detrending: a double sum, returned as float"""
    if var not in DETRENDING_VARIABLES:
        return f32(0.)
    total = 0.0
    for p, pv in zip(settings.get("proxies", []), proxy_values):
        if not p.get("active", 0):
            continue
        pv = float(pv)
        if pv == NODATA:
            continue
        slope = float(f32(p["slope"]))
        if p.get("isHeight", 0):
            if p.get("inversion", 0):
                h0, h1, below = f32(p["lapseRateH0"]), f32(p["lapseRateH1"]), f32(p["inversionLapseRate"])
                if pv <= float(h1):
                    a = pv - float(h0)
                    total += (a if a > 0 else 0.0) * float(below)
                else:
                    total += float((h1 - h0) * below) + (pv - float(h1)) * slope
            else:
                total += (pv if pv > 0 else 0.0) * slope
        else:
            total += pv * slope
    return f32(total)


def _neighbours(d, radius0):
    """shepardSearchNeighbour (interpolation.cpp:806-868) for one cell: (indices in list order, radius); radius NODATA: no list"""
    first = [i for i in range(len(d)) if d[i] <= radius0 and d[i] > 0]
    not_zero = lambda i: abs(float(d[i])) >= EPSILON and abs(float(d[i]) - NODATA) >= EPSILON          # sortPointsByDistance: ! isEqual
    if len(first) < SHEPARD_MIN:
        idx = sorted((i for i in range(len(d)) if not_zero(i)), key=lambda i: d[i])[:SHEPARD_MIN]
        return idx, (d[idx[-1]] + F_EPS if idx else f32(NODATA))
    if len(first) > SHEPARD_MAX:
        idx = sorted((i for i in first if not_zero(i)), key=lambda i: d[i])[:SHEPARD_MAX]
        return idx, d[idx[-1]] + F_EPS
    return first, radius0


def _shepard(idx, radius, d, sx, sy, sv, x, y):
    """shepardIdw (interpolation.cpp:871-945) on the list `idx`; x, y: the cell's float coordinates"""
    n = len(idx)
    S = [0.0] * n
    wsum = 0.0
    radius_3 = float(radius) / 3.
    radius_27_4 = 6.75 / float(radius)
    for i, k in enumerate(idx):
        if float(d[k]) > EPSILON:
            if float(d[k]) <= radius_3:
                S[i] = float(f32(1) / d[k])
            elif d[k] <= radius:
                tmp = float((d[k] / radius) - f32(1))
                S[i] = radius_27_4 * tmp * tmp
            wsum += S[i]
    if wsum == 0:
        return f32(NODATA)
    xd, yd = float(x), float(y)
    t = [0.0] * n
    for i, ki in enumerate(idx):
        for j, kj in enumerate(idx):
            if i != j:
                cosine = ((xd - sx[ki]) * (xd - sx[kj]) + (yd - sy[ki]) * (yd - sy[kj])) / float(d[ki] * d[kj])
                t[i] += S[j] * (1 - cosine)
        t[i] /= wsum
    w = [S[i] * S[i] * (1 + t[i]) for i in range(n)]
    wsum = 0.0
    for v in w:
        wsum += v
    res = 0.0
    for i, k in enumerate(idx):
        res += (w[i] / wsum) * float(sv[k])
    return f32(res)


def _shepard_modified(idx, radius, d, sx, sy, sv, x, y):
    """modifiedShepardIdw (interpolation.cpp:948-1028) with radius == NODATA on entry.  interpolate() hands (radius, x, y) to a signature
    declared (radius, y, x) (:2527 against :949): the direction terms pair the cell's y with the stations' x"""
    n = len(idx)
    if n == 0:
        return f32(NODATA)
    s = [0.0] * n
    wsum = 0.0
    for i, k in enumerate(idx):
        if float(d[k]) > EPSILON and d[k] <= radius:
            s[i] = float((radius - d[k]) / (radius * d[k]))
            wsum += s[i]
    if wsum == 0.0:
        return f32(NODATA)
    inv = 1.0 / wsum
    xd, yd = float(y), float(x)                     # the swap
    t = [0.0] * n
    for i, ki in enumerate(idx):
        if s[i] == 0.0 or d[ki] <= 0:
            continue
        for j, kj in enumerate(idx):
            if i == j or s[j] == 0.0 or d[kj] <= 0:
                continue
            cosine = ((xd - sx[ki]) * (xd - sx[kj]) + (yd - sy[ki]) * (yd - sy[kj])) / float(d[ki] * d[kj])
            t[i] += s[j] * (1.0 - cosine)
        t[i] *= inv
    w = [s[i] * s[i] * (1.0 + t[i]) for i in range(n)]
    wsum = 0.0
    for v in w:
        wsum += v
    inv = 1.0 / wsum
    res = 0.0
    for i, k in enumerate(idx):
        res += (w[i] * inv) * float(sv[k])
    return f32(res)


def _tail(var: int, result: np.float32, threshold: np.float32) -> np.float32:
    """the switch at the end of interpolate() (interpolation.cpp:2540-2558) with the comparisons of std::min / std::max"""
    zero, hundred = f32(0), f32(100)
    if var == PRECIPITATION:
        return zero if result < threshold else result
    if var == AIR_REL_HUMIDITY:
        m = hundred if hundred < result else result
        return m if zero < m else zero
    if var in (WIND_SCALAR_INTENSITY, GLOBAL_IRRADIANCE, ATM_TRANSMISSIVITY):
        return zero if result < zero else result
    return result


def restate_interpolate(dem, xll, yll, cell_size, proxy_maps, var, method, x, y, value, bounding_box_area, settings: dict | None = None,
                        flag: float = NODATA, mine=None) -> np.ndarray:
    """interpolate() (interpolation.cpp:2502-2560) on every DEM cell (isEqual(dem, flag): the flag), `mine` (bool map): the cells computed"""
    settings = settings or {}
    var, method = raster.index(var, VARIABLES), raster.index(method, METHODS)
    dem = np.asarray(dem, np.float32)
    fl = f32(flag)
    out = np.full(dem.shape, fl, np.float32)
    sx, sy = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sv = np.asarray(value, np.float32)
    n = len(sx)
    cx, cy = cell_centres(dem.shape, float(xll), float(yll), float(cell_size))
    cxf, cyf = cx.astype(np.float32), cy.astype(np.float32)
    sxf, syf = sx.astype(np.float32), sy.astype(np.float32)
    radius0 = shepard_initial_radius(bounding_box_area, n)
    threshold = f32(settings.get("rainfallThreshold", 0.0))
    detrend = bool(settings.get("useDetrending", 1))
    valid = np.abs(dem.astype(np.float64) - float(fl)) >= EPSILON
    if mine is not None:
        valid &= np.asarray(mine, bool)
    cells = np.argwhere(valid)
    with np.errstate(all="ignore"):
        if var == PRECIPITATION and settings.get("allZero", 0):
            out[valid] = 0.
            return out
        xf, yf = cxf[valid], cyf[valid]
        dx, dy = sxf[None, :] - xf[:, None], syf[None, :] - yf[:, None]
        dist = np.sqrt(dx * dx + dy * dy)                                   # float32 throughout: gis::computeDistance
        if method == IDW:                                                   # the station loop, every cell at once: the sums keep the stations' order
            s, sw = np.zeros(len(cells)), np.zeros(len(cells))
            for i in range(n):
                km = dist[:, i].astype(np.float64) / 10000.
                use = dist[:, i].astype(np.float64) > EPSILON
                w = np.where(use, 1.0 / (km * km * km), 0.0)
                sw = np.where(use, sw + w, sw)
                s = np.where(use, s + float(sv[i]) * w, s)
            idw = np.where(sw > 0.0, (s / sw).astype(np.float32), f32(NODATA))
        for k, (r, c) in enumerate(cells):
            if method == IDW:
                res = idw[k]
            else:
                idx, radius = _neighbours(dist[k], radius0)
                res = (_shepard if method == SHEPARD else _shepard_modified)(idx, radius, dist[k], sx, sy, sv, xf[k], yf[k])
            if abs(float(res) - NODATA) < EPSILON:
                out[r, c] = NODATA
                continue
            if detrend:
                pv = []
                for q, p in enumerate(settings.get("proxies", [])):
                    m = dem if (q >= len(proxy_maps) or proxy_maps[q] is None) else np.asarray(proxy_maps[q], np.float32)
                    pv.append(float(m[r, c]) if (p.get("active", 0) and m[r, c] != fl) else NODATA)
                res = f32(res + _retrend(var, settings, pv))
            out[r, c] = _tail(var, res, threshold)
    return out
