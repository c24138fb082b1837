"""Air and dew-point temperature with multiple detrending and no sub-option on the device (include/sf3d_multidetrend.h,
criteria3d_amd/csrc/sf3d_multidetrend.inc), on the raster of the meteo block (`meteo.initialize` with one raster per proxy comes first):
the plain `interpolationDem` arm of `Project::interpolationDemMain` (agrolib/project/project.cpp:3531-3561) - one fit over all the call's
stations (`preInterpolation` -> `multipleDetrendingMain`), then `interpolationRaster` over every DEM cell - and the same fit evaluated at
a list of points, as `computeResiduals` and `interpolationOutputPoints` do.  `localproxies` and `glocal` are the two sub-options of this
path; this module stands on them and on `localdetrend`.

Four parts:
  * the binding (`bind`, `interpolate`, `points`, `get_fit`, `interpolate_hour` ...): one launch of k_multidetrend_fit and one of
    k_multidetrend_cells per variable, one of k_multidetrend_points per list of points; a missing kernel or library is an error;
  * `residuals`: computeResiduals' arithmetic (agrolib/interpolation/spatialControl.cpp:102-160, the precipitation arm left out) over
    `points`;
  * `proxy_values_xy`: getProxyValuesXY (agrolib/interpolation/interpolation.cpp:2620-2647) for points, the proxy table of
    interpolationOutputPoints;
  * the restatements `restate_fit`, `restate_at`, `restate_interpolate` and `restate_points`, built from `localproxies.elevation_fit`,
    `localproxies.other_proxies` and `glocal.interpolate_over`, in Python floats and numpy float32 scalars with the reference's types and
    operation order, with an `arms` counter - the checkers of the CPU tests.  Checkers, never a fallback.

With the caller stay lapse-rate codes, topographic distance, optimalDetrending, the meteo-grid variant, and the station list and its
quality control."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, glocal as gl, localdetrend as ld, localproxies as lp, meteo, raster
from .capi import pf32, pf64
from .localproxies import _eqf
from .meteo import EPSILON, NODATA, VARIABLES, METHODS, f32

MAX_PROXIES = meteo.MAX_PROXIES
MAX_POINTS = 1 << 24                            # SF3D_MULTIDETREND_MAX_POINTS
KERNELS = ("k_multidetrend_fit", "k_multidetrend_cells", "k_multidetrend_points")

pu8, pu32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
# name -> (restype, argtypes): every symbol include/sf3d_multidetrend.h declares
SIGNATURES = {
    "sf3d_multidetrend_interpolate": (capi.u8, [capi.i32, capi.i32, capi.u32, pf64, pf64, pf32, capi.u32, pf32, capi.f32, meteo.psettings, ld.pfit, lp.pothers, pf32]),
    "sf3d_multidetrend_points": (capi.u8, [capi.u32, pf32, pf32, pf32, pf32, pf32]),
    "sf3d_multidetrend_get_fit": (capi.u8, [capi.u32, pf32, pu8, pu8, pf32, pf64, pu8, pf64, pf64, pu32, pu32]),
    "sf3d_multidetrend_kernel_ms": (capi.f64, [capi.i32]),
    "sf3d_multidetrend_bytes": (capi.u64, []),
    "sf3d_multidetrend_clean": (capi.u8, []),
}
# the rule of tests/raster_helpers.py same for every quantity of a fit
FIT_QUANTITIES = dict(significant="value", r2="nan", parameters="nan", proxy_significant="value", slope="nan", intercept="nan", fitted="value", kept="value",
                      detrended="bits", station_kept="value")


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_multidetrend.h (and of the headers it stands on) to a loaded product library"""
    lp.bind(sf)
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def multi_settings(proxies, settings: dict | None = None) -> dict:
    """the settings of a call: `proxies` (dicts with active, isHeight), useMultipleDetrending set, useLocalDetrending clear"""
    return gl.glocal_settings(proxies, settings)


def interpolate(sf: capi.SF3D, var, method, x, y, value, proxy_values, bounding_box_area: float, fit: dict, proxies, others, settings: dict | None = None,
                download: bool = True):
    """one temperature map from the station list (x, y: doubles [m]; value: floats, not detrended; proxy_values: [len(proxies), stations]
    floats in slot order, NODATA where a station has none).  The map lands in the meteo block's slot of the variable; download=False: it
    stays there"""
    bind(sf)
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    v = np.ascontiguousarray(value, np.float32)
    pv = np.ascontiguousarray(proxy_values, np.float32).reshape(len(proxies), -1) if len(proxies) else np.zeros((0, len(x)), np.float32)
    if not (x.shape == y.shape == v.shape and x.ndim == 1 and pv.shape[1] == len(x)):
        raise ValueError("x, y, value and the rows of proxy_values differ in length")
    st = meteo.settings_struct(multi_settings(proxies, settings))
    ft, ot = ld.fit_struct(dict(fit, minPointsLocalDetrending=fit.get("minPointsLocalDetrending", 0))), lp.others_struct(others)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_multidetrend_interpolate(raster.index(var, VARIABLES), raster.index(method, METHODS), len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64),
                                                  v.ctypes.data_as(pf32), len(proxies), pv.ctypes.data_as(pf32), float(np.float32(bounding_box_area)), C.byref(st),
                                                  C.byref(ft), C.byref(ot), out.ctypes.data_as(pf32) if download else pf32()), "multidetrend_interpolate")
    sf._multidetrend_stations, sf._multidetrend_proxies = len(x), len(proxies)
    return out


def points(sf: capi.SF3D, x, y, z, proxy_values) -> np.ndarray:
    """interpolate() at float points with the fit and the kept list of the last `interpolate`: x, y, z cast to float as computeResiduals
    casts them; proxy_values: [the last call's proxies, points], NODATA where a point has none"""
    bind(sf)
    x, y, z = (np.ascontiguousarray(a, np.float32).ravel() for a in (x, y, z))
    slots = getattr(sf, "_multidetrend_proxies", 0)
    pv = np.ascontiguousarray(proxy_values, np.float32).reshape(slots, -1) if slots else np.zeros((0, len(x)), np.float32)
    if not (x.shape == y.shape == z.shape and pv.shape[1] == len(x)):
        raise ValueError("x, y, z and the rows of proxy_values differ in length")
    out = np.empty(len(x), np.float32)
    sf.check(sf.lib.sf3d_multidetrend_points(len(x), x.ctypes.data_as(pf32), y.ctypes.data_as(pf32), z.ctypes.data_as(pf32), pv.ctypes.data_as(pf32),
                                             out.ctypes.data_as(pf32)), "multidetrend_points")
    return out


def get_fit(sf: capi.SF3D) -> dict:
    """of the last call: per station detrended and station_kept; significant, r2, parameters (the height); proxy_significant, slope,
    intercept per slot; fitted, kept"""
    bind(sf)
    n = getattr(sf, "_multidetrend_stations", 0)                                    # before the first call: the library refuses
    det, bit = np.empty(n, np.float32), np.empty(n, np.uint8)
    sig, r2, par = np.empty(1, np.uint8), np.empty(1, np.float32), np.empty(ld.MAX_PARAMETERS, np.float64)
    psig, slope, icpt = np.empty(MAX_PROXIES, np.uint8), np.empty(MAX_PROXIES, np.float64), np.empty(MAX_PROXIES, np.float64)
    fitted, kept = np.empty(1, np.uint32), np.empty(1, np.uint32)
    sf.check(sf.lib.sf3d_multidetrend_get_fit(n, det.ctypes.data_as(pf32), bit.ctypes.data_as(pu8), sig.ctypes.data_as(pu8), r2.ctypes.data_as(pf32),
                                              par.ctypes.data_as(pf64), psig.ctypes.data_as(pu8), slope.ctypes.data_as(pf64), icpt.ctypes.data_as(pf64),
                                              fitted.ctypes.data_as(pu32), kept.ctypes.data_as(pu32)), "multidetrend_get_fit")
    return dict(significant=bool(sig[0]), r2=r2[0], parameters=par, proxy_significant=psig.astype(bool), slope=slope, intercept=icpt, fitted=int(fitted[0]),
                kept=int(kept[0]), detrended=det, station_kept=bit.astype(bool))


def interpolate_hour(sf: capi.SF3D, stations: dict, method, fit: dict, proxies, others, settings: dict | None = None) -> dict:
    """the hour's two temperature maps, in the order snow.compute_hour takes them: stations[name] = (x, y, value, proxy_values,
    bounding_box_area[, fit]) for "airT" and / or "dewT"; they stay in the meteo block's slots, where the radiation, snow, ET0 and hour
    blocks read them"""
    names = [n for n in ("airT", "dewT") if n in stations]
    if not names or set(stations) - set(names):
        raise ValueError(f"stations of airT and / or dewT are needed, got {sorted(stations)}")
    out = {}
    for n in names:
        x, y, v, pv, area, *own = stations[n]
        out[n] = interpolate(sf, n, method, x, y, v, pv, area, own[0] if own else fit, proxies, others, settings)
    return out


def residual_of(value, interpolated) -> np.ndarray:
    """computeResiduals' arithmetic (spatialControl.cpp:126-154) without the precipitation arm: currentValue - interpolated as floats,
    NODATA where either is"""
    v, g = np.asarray(value, np.float32), np.asarray(interpolated, np.float32)
    with np.errstate(all="ignore"):
        return np.where((g != f32(NODATA)) & (v != f32(NODATA)), v - g, f32(NODATA)).astype(np.float32)


def residuals(sf: capi.SF3D, x, y, z, value, proxy_values) -> np.ndarray:
    """computeResiduals over the last call's fit: every station evaluated at its own float coordinates with its own proxy values - the
    stations the prunings erased from the list too"""
    return residual_of(value, points(sf, x, y, z, proxy_values))


def kernel_ms(sf: capi.SF3D) -> tuple:
    """(k_multidetrend_fit, k_multidetrend_cells, k_multidetrend_points) of their last launches"""
    return tuple(float(sf.lib.sf3d_multidetrend_kernel_ms(k)) for k in range(3))


def bytes_held(sf: capi.SF3D) -> int:
    return int(sf.lib.sf3d_multidetrend_bytes())


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_multidetrend_clean(), "multidetrend_clean")
    sf._multidetrend_stations = sf._multidetrend_proxies = 0


# ------------------------------------------------------------------------------------------------ getProxyValuesXY for points

def cell_xy(shape, xll: float, yll: float, cell_size: float):
    """gis::getUtmXYFromRowColSinglePrecision(header, ..) (agrolib/gis/gis.cpp:799-804) for every cell, as interpolationRaster calls it:
    floats [rows, cols] - the cell's west edge + 0.5 m and its north edge - 0.5 m as the function's parentheses stand, not the centre"""
    rows, cols = shape
    r, c = np.mgrid[0:rows, 0:cols]
    return ((float(xll) + float(cell_size) * c) + 0.5).astype(np.float32), ((float(yll) + float(cell_size) * (rows - r)) - 0.5).astype(np.float32)


def cell_at(shape, xll: float, yll: float, cell_size: float, x, y):
    """the (row, col) Crit3DRasterGrid::getValueFromXY (gis.cpp:533-546) reads at (x, y): int() of the offsets times invCellSize; None
    outside the raster"""
    rows, cols = shape
    inv = 1.0 / float(cell_size)
    row = (rows - 1) - int((float(y) - float(yll)) * inv)
    col = int((float(x) - float(xll)) * inv)
    return (row, col) if 0 <= row < rows and 0 <= col < cols else None


def proxy_values_xy(dem, xll: float, yll: float, cell_size: float, proxy_maps, proxies, x, y, flag: float = NODATA) -> np.ndarray:
    """getProxyValuesXY (interpolation.cpp:2620-2647) at the float points (x, y): [len(proxies), points] floats - NODATA for a proxy that
    is not active, and where the proxy's raster holds its flag or the point lies outside it (Crit3DRasterGrid::getValueFromXY).
    proxy_maps as meteo.initialize takes them: None in the place of the height's raster (the DEM)"""
    dem = np.asarray(dem, np.float32)
    x, y = np.asarray(x, np.float32).ravel(), np.asarray(y, np.float32).ravel()
    out = np.full((len(proxies), len(x)), NODATA, np.float32)
    for p, q in enumerate(proxies):
        if not q.get("active"):
            continue
        grid = dem if proxy_maps[p] is None else np.asarray(proxy_maps[p], np.float32)
        for i in range(len(x)):
            at = cell_at(dem.shape, xll, yll, cell_size, x[i], y[i])
            if at is not None and grid[at] != f32(flag):
                out[p, i] = grid[at]
    return out


# ------------------------------------------------------------------------------------------------ restatement (checker)

def _note(arms, key, n=1):
    if arms is not None:
        arms[key] = arms.get(key, 0) + n


def restate_fit(value, proxy_values, fit: dict, proxies, others, arms: dict | None = None) -> dict:
    """multipleDetrendingMain over all the call's stations in call order, unit weights, no minimum of points.  get_fit's quantities, and
    `left`: the places of the kept stations in the call, `val`: their detrended values, `lines`: {slot: (slope, intercept)}, `par`: the
    height's parameters or None"""
    height, slots = gl._slots(proxies)
    function = raster.index(fit["function"], ld.FUNCTIONS)
    pv = np.asarray(proxy_values, np.float32).reshape(len(proxies), -1)
    n = pv.shape[1] if len(proxies) else len(value)
    rows = {p: pv[p] for p in range(len(proxies))}
    val = np.asarray(value, np.float32).copy()
    own = dict(fit, minPointsLocalDetrending=0)                                     # interpolation.cpp:1885 is off
    r2, par = NODATA, None
    if height is None:
        _note(arms, "the height not active")
    else:
        nr = int((rows[height] != f32(NODATA)).sum())
        ok, why = lp.proxy_validity(rows[height], fit.get("stdDevThreshold", NODATA))
        r2, par = lp.elevation_fit(rows[height], val, None, function, own, arms)
        if par is not None:
            _note(arms, "the height significant")
            if nr < n:
                _note(arms, "a station with a NODATA height while the height is significant")
        elif not ok:
            _note(arms, "the height not significant: fewer than five heights" if why == "count" else "the height not significant: the standard deviation")
        else:
            _note(arms, "the height withdrawn by isVectorNodataOrZero")
    seen = {}
    left, lines = lp.other_proxies(rows, val, None, slots, others, 0, seen)
    for k, c in seen.items():
        _note(arms, k, c)
    if not slots:
        _note(arms, "no other proxy active")
    if par is not None:
        _note(arms, "the height significant alone" if not lines else f"the height significant with {len(lines)} other proxies")
    out = dict(significant=par is not None, r2=f32(r2), parameters=np.full(ld.MAX_PARAMETERS, NODATA, np.float64), proxy_significant=np.zeros(MAX_PROXIES, bool),
               slope=np.full(MAX_PROXIES, NODATA, np.float64), intercept=np.full(MAX_PROXIES, NODATA, np.float64), fitted=n, kept=len(left),
               detrended=np.full(n, NODATA, np.float32), station_kept=np.zeros(n, bool), left=list(left), val=val[left], lines=lines, par=par, function=function,
               height=height)
    if par is not None:
        out["parameters"][:len(par)] = par
    for p, (s, i) in lines.items():
        out["proxy_significant"][p], out["slope"][p], out["intercept"][p] = True, s, i
    out["detrended"][left], out["station_kept"][left] = val[left], True
    return out


def retrend_of(f: dict, values, arms: dict | None = None) -> np.float32:
    """retrend (interpolation.cpp:1298-1313) over getMultipleDetrendingValues (:2563-2617) with the fit `f` (restate_fit) and every
    slot's value at the place (doubles, NODATA: none): 0 where a significant proxy has none"""
    used = ([f["height"]] if f["par"] is not None else []) + sorted(f["lines"])
    if not used:
        return f32(0)
    if any(float(values[p]) == NODATA for p in used):
        _note(arms, "a place lacking a significant proxy: value kept, retrend 0")
        return f32(0)
    total = 0.0
    if f["par"] is not None:
        total += ld.lapse_rate(f["function"], float(values[f["height"]]), list(f["par"]))
    for p in sorted(f["lines"]):
        total += f["lines"][p][0] * float(values[p]) + f["lines"][p][1]
    return f32(float(f32(total)))


def restate_at(f: dict, method: int, x, y, values, kx, ky, bounding_box_area, use_detrending: bool = True, arms: dict | None = None) -> np.float32:
    """interpolate() at the float (x, y) with every slot's value `values` there, over the kept stations (kx, ky: doubles) of the fit `f`"""
    res = gl.interpolate_over(method, f32(x), f32(y), kx, ky, f["val"], bounding_box_area)
    if abs(float(res) - NODATA) < EPSILON:
        _note(arms, "an interpolate() that gives NODATA")
        return f32(NODATA)
    if use_detrending:
        with np.errstate(all="ignore"):
            res = f32(res + retrend_of(f, values, arms))
    return f32(res)


def restate_interpolate(dem, xll, yll, cell_size, proxy_maps, var, method, x, y, value, proxy_values, bounding_box_area, fit: dict, proxies, others,
                        settings: dict | None = None, flag: float = NODATA, mine=None, arms: dict | None = None) -> dict:
    """the one fit, then interpolationRaster.  dict(value: the map, and get_fit's quantities, and `fit`: restate_fit's dict)"""
    if raster.index(var, VARIABLES) not in ld.LOCAL_VARIABLES:
        raise ValueError("multiple detrending is for the two temperatures")
    method = raster.index(method, METHODS)
    dem = np.asarray(dem, np.float32)
    fl = f32(flag)
    shape = dem.shape
    sx, sy = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        f = restate_fit(value, proxy_values, fit, proxies, others, arms)
    out = dict(value=np.full(shape, fl, np.float32), fit=f, **{q: f[q] for q in FIT_QUANTITIES})
    kx, ky = sx[f["left"]], sy[f["left"]]
    cx, cy = cell_xy(shape, xll, yll, cell_size)
    cells = lp.cell_proxy_values(dem, proxy_maps, flag)
    outside = np.full(len(proxy_maps), NODATA, np.float64)
    _, slots = gl._slots(proxies)
    valid = np.abs(dem.astype(np.float64) - float(fl)) >= EPSILON
    if mine is not None:
        valid &= np.asarray(mine, bool)
    use = bool((settings or {}).get("useDetrending", 1))
    if not use:
        _note(arms, "useDetrending 0")
    with np.errstate(all="ignore"):
        for r, c in np.argwhere(valid):
            at = cell_at(shape, xll, yll, cell_size, cx[r, c], cy[r, c])       # getProxyValuesXY at the loop's (x, y)
            if at != (r, c):
                _note(arms, "a cell whose (x, y) is read in another cell")
            values = outside if at is None else cells[at]
            if arms is not None and any(float(values[p]) == NODATA for p in slots if p not in f["lines"]) and \
                    not any(float(values[p]) == NODATA for p in ([f["height"]] if f["par"] is not None else []) + sorted(f["lines"])):
                _note(arms, "a cell lacking only a non-significant active proxy")
            out["value"][r, c] = restate_at(f, method, cx[r, c], cy[r, c], values, kx, ky, bounding_box_area, use, arms)
    return out


def restate_points(f: dict, method, sx, sy, px, py, point_values, bounding_box_area, settings: dict | None = None, arms: dict | None = None) -> np.ndarray:
    """interpolate() at float points with the fit `f` (restate_fit) of the stations (sx, sy); point_values: [proxies, points]"""
    method = raster.index(method, METHODS)
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    kx, ky = sx[f["left"]], sy[f["left"]]
    px, py = np.asarray(px, np.float32).ravel(), np.asarray(py, np.float32).ravel()
    pv = np.asarray(point_values, np.float32).reshape(-1, len(px)).astype(np.float64)
    use = bool((settings or {}).get("useDetrending", 1))
    out = np.empty(len(px), np.float32)
    with np.errstate(all="ignore"):
        for i in range(len(px)):
            out[i] = restate_at(f, method, px[i], py[i], pv[:, i], kx, ky, bounding_box_area, use, arms)
    return out
