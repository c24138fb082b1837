"""Air and dew-point temperature with local detrending and every active proxy on the device (include/sf3d_localproxies.h,
criteria3d_amd/csrc/sf3d_localproxies.inc), on the raster of the meteo block (`meteo.initialize` with one raster per proxy comes first):
for every DEM cell what the cell loop of `Project::interpolationDemLocalDetrending` (agrolib/project/project.cpp:3226-3254) does with the
height and up to MAX_OTHERS other active proxies.  `localdetrend` is the same block for the height alone; this module stands on it.

Three parts:
  * the binding (`bind`, `others_struct`, `interpolate`, `get_interpolated`, `get_proxy_fit`, `interpolate_hour` ...): one launch of
    k_localdetrend_proxies per variable; a missing kernel or library is an error;
  * `make_others`: the per-slot table of a call from the proxies' configured ranges (getFittingParametersRange(): the minima, then the
    maxima, of slope and intercept) and thresholds;
  * the restatements `proxy_validity`, `marquardt_others`, `other_proxies`, `interpolate_cell` and `restate_interpolate`: steps 3 to 10 of
    the reference (multipleDetrendingOtherProxiesFitting, detrendingOtherProxies, interpolate(), retrend through
    getMultipleDetrendingValues) on top of `localdetrend`'s selection and elevation fit, in Python floats and numpy float32 scalars with
    the reference's types and operation order - `marquardt_others` keeps the reference's P[k][j], which the kernel does not - the
    checkers of the CPU tests against the compiled-reference pin (tests/golden/localproxies.npz).  Checkers, never a fallback.

With the caller stay lapse-rate codes and output points.  multipleDetrending without localDetrending is `multidetrend`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, localdetrend as ld, meteo, raster
from .capi import pf32, pf64
from .localdetrend import _div, _eq, _sqrt
from .meteo import EPSILON, NODATA, VARIABLES, METHODS, f32

MAX_OTHERS = 7                                  # SF3D_LOCALPROXIES_MAX_OTHERS
MAX_PROXIES = meteo.MAX_PROXIES
MAX_ITERATIONS, FIT_EPSILON, RATIO_DELTA = 100, 0.005, 1000        # interpolation.cpp:2165, :1686
MIN_NR = ld.MIN_NR
KERNEL = "k_localdetrend_proxies"


class OtherProxy(C.Structure):
    """sf3d_localproxies_proxy_t"""
    _fields_ = [("min", C.c_double * 2), ("max", C.c_double * 2), ("stdDevThreshold", C.c_float), ("reserved", C.c_int32)]


class Others(C.Structure):
    """sf3d_localproxies_others_t"""
    _fields_ = [("proxy", OtherProxy * MAX_PROXIES)]


pothers = C.POINTER(Others)
pu8, pu32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
# name -> (restype, argtypes): every symbol include/sf3d_localproxies.h declares
SIGNATURES = {
    "sf3d_localproxies_interpolate": (capi.u8, [capi.i32, capi.i32, capi.u32, pf64, pf64, pf32, capi.u32, pf32, capi.f32, meteo.psettings, ld.pfit, pothers, pf32]),
    "sf3d_localproxies_get_interpolated": (capi.u8, [capi.u32, pu32]),
    "sf3d_localproxies_get_proxy_fit": (capi.u8, [capi.u32, pu8, pf64, pf64]),
    "sf3d_localproxies_kernel_ms": (capi.f64, []),
    "sf3d_localproxies_bytes": (capi.u64, []),
    "sf3d_localproxies_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_localproxies.h (and of sf3d_localdetrend.h, sf3d_meteo.h) to a loaded product library"""
    ld.bind(sf)
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def make_others(proxies) -> list:
    """per proxy slot None (the height, or a proxy that is never active) or dict(range=[min slope, min intercept, max slope, max intercept]
    - getFittingParametersRange() -, stdDevThreshold=...) -> the `others` of a call: dict(min, max, stdDevThreshold) per slot"""
    out = []
    for p in proxies:
        if p is None:
            out.append(dict(min=[0.0, 0.0], max=[0.0, 0.0], stdDevThreshold=NODATA))
            continue
        rng = [float(v) for v in p["range"]]
        if len(rng) != 4:
            raise ValueError(f"functionLinear_intercept takes 2 parameters, the range holds {len(rng)} values")
        out.append(dict(min=rng[:2], max=rng[2:], stdDevThreshold=float(p.get("stdDevThreshold", NODATA))))
    return out


def others_struct(others) -> Others:
    out = Others()
    for k, o in enumerate(list(others)[:MAX_PROXIES]):
        for t in range(2):
            out.proxy[k].min[t], out.proxy[k].max[t] = float(o["min"][t]), float(o["max"][t])
        out.proxy[k].stdDevThreshold = float(o.get("stdDevThreshold", NODATA))
    return out


def local_settings(proxies, settings: dict | None = None) -> dict:
    """the settings of a call: `proxies` (dicts with active, isHeight) and the two options of the block set"""
    s = dict(settings or {})
    s["proxies"] = [dict(p) for p in proxies]
    s["useMultipleDetrending"] = s.get("useMultipleDetrending", 1)
    s["useLocalDetrending"] = s.get("useLocalDetrending", 1)
    return s


def interpolate(sf: capi.SF3D, var, method, x, y, value, proxy_values, bounding_box_area: float, fit: dict, proxies, others, settings: dict | None = None,
                download: bool = True):
    """one temperature map with local detrending from the station list (x, y: doubles [m]; value: floats, not detrended; proxy_values:
    [len(proxies), stations] floats in slot order, NODATA where a station has none).  proxies: dict(active, isHeight) per slot; others:
    make_others().  The map lands in the meteo block's slot of the variable; download=False: it stays there"""
    bind(sf)
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    v = np.ascontiguousarray(value, np.float32)
    pv = np.ascontiguousarray(proxy_values, np.float32).reshape(len(proxies), -1) if len(proxies) else np.zeros((0, len(x)), np.float32)
    if not (x.shape == y.shape == v.shape and x.ndim == 1 and pv.shape[1] == len(x)):
        raise ValueError("x, y, value and the rows of proxy_values differ in length")
    st = meteo.settings_struct(local_settings(proxies, settings))
    ft, ot = ld.fit_struct(fit), others_struct(others)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_localproxies_interpolate(raster.index(var, VARIABLES), raster.index(method, METHODS), len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64),
                                                  v.ctypes.data_as(pf32), len(proxies), pv.ctypes.data_as(pf32), float(np.float32(bounding_box_area)), C.byref(st),
                                                  C.byref(ft), C.byref(ot), out.ctypes.data_as(pf32) if download else pf32()), "localproxies_interpolate")
    return out


def get_interpolated(sf: capi.SF3D) -> np.ndarray:
    """per cell the number of stations interpolated after the prunings of the last call"""
    count = np.empty(sf._meteo_shape, np.uint32)
    sf.check(sf.lib.sf3d_localproxies_get_interpolated(count.size, count.ctypes.data_as(pu32)), "localproxies_get_interpolated")
    return count


def get_proxy_fit(sf: capi.SF3D) -> dict:
    """per cell and proxy slot of the last call: proxy_significant (bool), slope, intercept (float64, NODATA where not significant)"""
    shape = sf._meteo_shape + (MAX_PROXIES,)
    sig, slope, intercept = np.empty(shape, np.uint8), np.empty(shape, np.float64), np.empty(shape, np.float64)
    sf.check(sf.lib.sf3d_localproxies_get_proxy_fit(sig.size // MAX_PROXIES, sig.ctypes.data_as(pu8), slope.ctypes.data_as(pf64), intercept.ctypes.data_as(pf64)),
             "localproxies_get_proxy_fit")
    return dict(proxy_significant=sig.astype(bool), slope=slope, intercept=intercept)


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


def kernel_ms(sf: capi.SF3D) -> float:
    return float(sf.lib.sf3d_localproxies_kernel_ms())


def bytes_held(sf: capi.SF3D) -> int:
    return int(sf.lib.sf3d_localproxies_bytes())


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_localproxies_clean(), "localproxies_clean")


# ------------------------------------------------------------------------------------------------ restatement (checker)

def _eqf(a, b) -> bool:
    """isEqual(float, float), basicMath.h:25"""
    return abs(float(f32(a)) - float(f32(b))) < EPSILON


def proxy_validity(values, threshold) -> tuple:
    """proxyValidity (interpolation.cpp:1418-1457) over the float values of a proxy at the points of a list: (valid, why it is not)"""
    kept = [float(v) for v in values if f32(v) != f32(NODATA)]
    total = 0.0
    for v in kept:
        total += v
    if len(kept) < MIN_NR:
        return False, "count"
    avg = total / len(kept)
    total = 0.0
    for v in kept:
        total += (v - avg) * (v - avg)
    std_dev = _sqrt(_div(total, len(kept) - 1))
    if f32(threshold) != f32(NODATA):
        return (std_dev > float(f32(threshold))), "deviation"
    return True, ""


def function_sum(x, par) -> float:
    """functionSum of functionLinear_intercept (furtherMathFunctions.cpp:181-201); par: flat, slope and intercept per proxy"""
    result = 0.0
    for k in range(len(x)):
        result += par[2 * k] * x[k] + par[2 * k + 1]
    return result


def marquardt_others(par: list, pmin, pmax, pdelta, xs, ys, ws, arms: dict | None = None) -> None:
    """fittingMarquardt_nDimension with weights (furtherMathFunctions.cpp:1740-1947) of functionSum, as it stands there: the raw pivots, the
    walk of the parameter vector across all proxies.  `par` (flat) is fitted in place"""
    n, nd = len(par), len(ys)
    change, fresh, lam = [0.0] * n, [0.0] * n, [0.01] * n
    with np.errstate(all="ignore"):
        sse = 0.0
        for i in range(nd):
            error = ys[i] - function_sum(xs[i], par)
            sse += error * error * ws[i] * ws[i]
        iteration = 0
        clamped_min = clamped_max = False
        while True:
            g = [0.0] * n
            a = [[0.0] * n for _ in range(n)]
            first = [function_sum(xs[i], par) for i in range(nd)]
            P = [[0.0] * nd for _ in range(n)]
            for k in range(n):
                par[k] += pdelta[k]
                for j in range(nd):
                    P[k][j] = _div(function_sum(xs[j], par) - first[j], pdelta[k])
                par[k] -= pdelta[k]
            for i in range(n):
                for j in range(i, n):
                    for k in range(nd):
                        a[i][j] += P[i][k] * (ws[k] * P[j][k])
            for i in range(n):
                for k in range(nd):
                    g[i] += P[i][k] * ws[k] * (ys[k] - first[k])
            for k in range(n):
                a[k][k] += lam[k] * a[k][k]
                for j in range(k + 1, n):
                    a[j][k] = a[k][j]
            for j in range(n - 1):
                pivot = a[j][j]
                for i in range(j + 1, n):
                    mult = _div(a[i][j], pivot)
                    for k in range(j + 1, n):
                        a[i][k] = float(np.float64(a[i][k]) - np.float64(mult) * np.float64(a[j][k]))
                    g[i] = float(np.float64(g[i]) - np.float64(mult) * np.float64(g[j]))
            change[n - 1] = _div(g[n - 1], a[n - 1][n - 1])
            for i in range(n - 2, -1, -1):
                top = g[i]
                for k in range(i + 1, n):
                    top = float(np.float64(top) - np.float64(a[i][k]) * np.float64(change[k]))
                change[i] = _div(top, a[i][i])
            for j in range(n):
                fresh[j] = par[j] + change[j]
                if fresh[j] > pmax[j] and lam[j] < 1000:
                    fresh[j] = pmax[j]
                    clamped_max = True
                    if lam[j] < 1000:
                        lam[j] *= 10
                if fresh[j] < pmin[j]:
                    fresh[j] = pmin[j]
                    clamped_min = True
                    if lam[j] < 1000:
                        lam[j] *= 10
            new_sse = 0.0
            for i in range(nd):
                error = ys[i] - function_sum(xs[i], fresh)
                new_sse += error * error * ws[i] * ws[i]
            if new_sse == NODATA:
                return
            diff = sse - new_sse
            if diff > 0:
                sse = new_sse
                for j in range(n):
                    par[j] = fresh[j]
                    lam[j] /= 10
            else:
                for j in range(n):
                    lam[j] *= 10
            iteration += 1
            if not (abs(diff) > FIT_EPSILON and iteration <= MAX_ITERATIONS):
                break
    if arms is not None:
        def note(key):
            arms[key] = arms.get(key, 0) + 1
        note("the proxies' fit ends on |diffSSE| <= epsilon" if abs(diff) <= FIT_EPSILON else
             "the proxies' fit ends on a NaN diffSSE" if diff != diff else "the proxies' fit ends on the iteration cap")
        if clamped_min:
            note("a proxy parameter clamped at its minimum")
        if clamped_max:
            note("a proxy parameter clamped at its maximum")


def other_proxies(rows, val, weights, slots, others, min_points_local: int, arms: dict | None = None):
    """multipleDetrendingOtherProxiesFitting and detrendingOtherProxies (interpolation.cpp:1975-2236) over a selected list: rows[slot]: the
    float proxy values of the list's stations; val: their values (detrended by the elevation), changed in place; slots: the active
    proxies that are not the height.  Returns (the list positions still interpolated, {slot: (slope, intercept)} of the significant)"""
    n = len(val)

    def note(key):
        if arms is not None:
            arms[key] = arms.get(key, 0) + 1
    keep = list(range(n))
    if not slots:
        return keep, {}
    first = {}
    for p in slots:
        ok, why = proxy_validity(rows[p], others[p].get("stdDevThreshold", NODATA))
        first[p] = ok
        if not ok:
            note(f"a proxy fails the first pass for {why}")
    if not any(first.values()):
        note("every proxy fails the first pass: the list untouched")
        return keep, {}
    sig = [p for p in slots if first[p]]
    fit_list, keep = [], []
    for i in range(n):
        if not any(f32(rows[p][i]) == f32(NODATA) for p in sig):
            fit_list.append(i)
        nodata = any(_eqf(rows[p][i], NODATA) for p in sig)
        at_least_one = any(not _eqf(rows[p][i], 0) for p in sig)
        if not nodata and at_least_one:
            keep.append(i)
        elif nodata:
            note("a station pruned for NODATA")
        else:
            note("a station pruned from interpolation only: all significant values 0")
    second = {p: proxy_validity([rows[p][i] for i in fit_list], others[p].get("stdDevThreshold", NODATA))[0] for p in slots}
    for p in slots:
        if first[p] and not second[p]:
            note("a proxy fails only the second pass")
        if second[p] and not first[p]:
            note("a proxy passes only the second pass")
    if not any(second.values()):
        return keep, {}
    if len(fit_list) < min_points_local:
        note("too few fit points")
        return keep, {}
    sig = [p for p in slots if second[p]]
    pmin, pmax, pdelta, par = [], [], [], []
    for p in sig:
        for t in range(2):
            lo, hi = float(others[p]["min"][t]), float(others[p]["max"][t])
            pmin.append(lo)
            pmax.append(hi)
            d = (hi - lo) / RATIO_DELTA
            pdelta.append(EPSILON if d < EPSILON else d)
            par.append((hi + lo) / 2)
    xs = [[float(rows[p][i]) for p in sig] for i in fit_list]
    ys = [float(val[i]) for i in fit_list]
    ws = [1.0 if weights is None else float(weights[i]) for i in fit_list]
    marquardt_others(par, pmin, pmax, pdelta, xs, ys, ws, arms)
    left = []
    for i in keep:
        if any(_eqf(rows[p][i], NODATA) for p in sig):
            note("a station erased by detrendingOtherProxies: NODATA entered the fit as a predictor")
            continue
        val[i] = val[i] - f32(function_sum([float(rows[p][i]) for p in sig], par))
        left.append(i)
    return left, {p: (par[2 * k], par[2 * k + 1]) for k, p in enumerate(sig)}


def interpolate_cell(method: int, x, y, z, cell_values, sx, sy, proxy_values, sv, bounding_box_area, fit: dict, proxies, others, use_detrending: bool = True,
                     arms: dict | None = None) -> dict:
    """one DEM cell of height z at the float (x, y); cell_values: the cell's value per proxy slot as getProxyValuesXY leaves it (NODATA
    where the raster holds its flag).  value, count, radius, significant, r2, parameters as localdetrend.interpolate_cell, and interpolated,
    proxy_significant, slope, intercept per slot, ties (of the interpolated list)"""
    x, y = f32(x), f32(y)
    def note(key):
        if arms is not None:
            arms[key] = arms.get(key, 0) + 1
    heights = [p for p, q in enumerate(proxies) if q.get("isHeight")]
    height = heights[0] if heights and proxies[heights[0]].get("active") else None
    slots = [p for p, q in enumerate(proxies) if q.get("active") and not q.get("isHeight")]
    function, n_par = raster.index(fit["function"], ld.FUNCTIONS), len(fit["min"])
    sel, d, weights, radius = ld.local_selection(x, y, sx, sy, fit["minPointsLocalDetrending"], bounding_box_area, arms)
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    if d is None:
        dx, dy = sx.astype(np.float32) - x, sy.astype(np.float32) - y
        d = list(np.sqrt(dx * dx + dy * dy))
    d = np.array(d, np.float32)
    pv = np.asarray(proxy_values, np.float32).reshape(len(proxies), -1)
    rows = {p: pv[p][sel] for p in range(len(proxies))}
    val = np.asarray(sv, np.float32)[sel].copy()
    out = dict(count=len(sel), radius=f32(radius), significant=False, r2=f32(NODATA), parameters=[NODATA] * ld.MAX_PARAMETERS,
               proxy_significant=[False] * MAX_PROXIES, slope=[NODATA] * MAX_PROXIES, intercept=[NODATA] * MAX_PROXIES)
    par = None
    if height is not None:
        r2, par = elevation_fit(rows[height], val, weights, function, fit, arms)
        out["r2"] = f32(r2)
        if par is not None:
            out["significant"] = True
            out["parameters"] = list(par) + [NODATA] * (ld.MAX_PARAMETERS - n_par)
    else:
        note("the height not active")
    left, lines = other_proxies(rows, val, weights, slots, others, fit["minPointsLocalDetrending"], arms)
    if par is None and height is not None and lines:
        note("the height not significant with others significant")
    note(f"{len(slots)} other proxies active")
    for p, (a, b) in lines.items():
        out["proxy_significant"][p], out["slope"][p], out["intercept"][p] = True, a, b
    out["interpolated"] = len(left)
    d, val = d[left], val[left]
    lx, ly = sx[sel][left], sy[sel][left]
    out["ties"] = len(set(d.tolist())) < len(d)
    if method == meteo.IDW:
        res = ld._idw(d, val)
    elif method == meteo.SHEPARD:
        near, r = meteo._neighbours(d, meteo.shepard_initial_radius(bounding_box_area, len(left)))
        res = meteo._shepard(near, r, d, lx, ly, val, x, y)
    else:
        res = meteo._shepard_modified(list(range(len(left))), f32(radius), d, lx, ly, val, x, y) if len(left) else f32(NODATA)
    if abs(float(res) - NODATA) < EPSILON:
        out["value"] = f32(NODATA)
        return out
    if use_detrending:
        # retrend (:1298-1313) through getMultipleDetrendingValues (:2563-2617)
        add = 0.0
        used = ([height] if par is not None else []) + sorted(lines)
        missing = [p for p in used if float(cell_values[p]) == NODATA]
        for p in slots:
            if float(cell_values[p]) == NODATA:
                note("the cell's proxy NODATA for a significant proxy: retrend 0" if p in lines else "the cell's proxy NODATA for a proxy that is not significant")
        if used and not missing:
            total = 0.0
            if par is not None:
                total += ld.lapse_rate(function, float(cell_values[height]), par)
            for p in sorted(lines):
                total += lines[p][0] * float(cell_values[p]) + lines[p][1]
            add = float(f32(total))
        res = f32(res + f32(add))
    out["value"] = f32(res)
    return out


def elevation_fit(h, val, weights, function: int, fit: dict, arms: dict | None = None):
    """multipleDetrendingElevationFitting and detrendingElevation over a selected list, as localdetrend.interpolate_cell holds them: h: the
    list's float heights; val: detrended in place where the height is significant.  (R2, the parameters or None)"""
    n = len(val)
    elevation = [i for i in range(n) if h[i] != f32(NODATA)]
    total = 0.0
    for i in elevation:
        total += float(h[i])
    valid = len(elevation) >= MIN_NR
    if valid:
        avg = total / len(elevation)
        total = 0.0
        for i in elevation:
            total += (float(h[i]) - avg) * (float(h[i]) - avg)
        std_dev = _sqrt(total / (len(elevation) - 1))
        if f32(fit.get("stdDevThreshold", NODATA)) != f32(NODATA):
            valid = std_dev > float(f32(fit["stdDevThreshold"]))
    if valid and len(elevation) < fit["minPointsLocalDetrending"]:
        valid = False
    if not valid:
        return NODATA, None
    xs, ys = [float(h[i]) for i in elevation], [float(val[i]) for i in elevation]
    ws = [1.0 if weights is None else float(weights[i]) for i in elevation]
    r2, par = ld.best_fit(function, fit["min"], fit["max"], fit["delta"], fit["first_guess"], xs, ys, ws, arms)
    zero = any(_eq(p, NODATA) or _eq(p, 0) for p in par)
    if not _eq(r2, NODATA) or not zero:
        for i in range(n):
            val[i] = val[i] - f32(ld.lapse_rate(function, float(h[i]), par))
        return r2, par
    return r2, None


def cell_proxy_values(dem, proxy_maps, flag) -> np.ndarray:
    """getProxyValuesXY on every cell: [rows, cols, len(proxy_maps)] doubles; None in the place of a raster: the DEM's values"""
    dem = np.asarray(dem, np.float32)
    out = np.empty(dem.shape + (len(proxy_maps),), np.float64)
    for p, m in enumerate(proxy_maps):
        grid = dem if m is None else np.asarray(m, np.float32)
        out[..., p] = np.where(grid != f32(flag), grid.astype(np.float64), NODATA)
    return out


def restate_interpolate(dem, xll, yll, cell_size, proxy_maps, var, method, x, y, value, proxy_values, bounding_box_area, fit: dict, proxies, others,
                        settings: dict | None = None, flag: float = NODATA, mine=None, arms: dict | None = None) -> dict:
    """interpolate_cell on every DEM cell (isEqual(dem, flag): the flag), `mine` (bool map): the cells computed.  Maps by name"""
    if raster.index(var, VARIABLES) not in ld.LOCAL_VARIABLES:
        raise ValueError("local detrending is for the two temperatures")
    method = raster.index(method, METHODS)
    dem = np.asarray(dem, np.float32)
    fl = f32(flag)
    shape = dem.shape
    out = dict(value=np.full(shape, fl, np.float32), count=np.zeros(shape, np.uint32), interpolated=np.zeros(shape, np.uint32), radius=np.full(shape, NODATA, np.float32),
               significant=np.zeros(shape, bool), r2=np.full(shape, NODATA, np.float32), parameters=np.full(shape + (ld.MAX_PARAMETERS,), NODATA, np.float64),
               proxy_significant=np.zeros(shape + (MAX_PROXIES,), bool), slope=np.full(shape + (MAX_PROXIES,), NODATA, np.float64),
               intercept=np.full(shape + (MAX_PROXIES,), NODATA, np.float64), ties=np.zeros(shape, bool))
    cx, cy = meteo.cell_centres(shape, float(xll), float(yll), float(cell_size))
    cells = cell_proxy_values(dem, proxy_maps, flag)
    valid = np.abs(dem.astype(np.float64) - float(fl)) >= EPSILON
    if mine is not None:
        valid &= np.asarray(mine, bool)
    use = bool((settings or {}).get("useDetrending", 1))
    with np.errstate(all="ignore"):
        for r, c in np.argwhere(valid):
            cell = interpolate_cell(method, f32(cx[r, c]), f32(cy[r, c]), dem[r, c], cells[r, c], x, y, proxy_values, value, bounding_box_area, fit, proxies, others,
                                    use, arms)
            for k in out:
                out[k][r, c] = cell[k]
    return out
