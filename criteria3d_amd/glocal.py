"""Air and dew-point temperature with glocal detrending on the device (include/sf3d_glocal.h, criteria3d_amd/csrc/sf3d_glocal.inc), on the
raster of the meteo block (`meteo.initialize` with one raster per proxy comes first): what `Project::interpolationDemGlocalDetrending`
(agrolib/project/project.cpp:3267-3384) does - a fit per macro area, every cell interpolated once per area that covers it and blended by
the areas' weights, the areas visited in index order.  `localproxies` is the per-cell sibling; this module stands on it and on
`localdetrend`.

Four parts:
  * the binding (`bind`, `set_areas`, `interpolate`, `get_area_fit`, `interpolate_hour` ...): one launch of k_glocal_areas and one of
    k_glocal_cells per variable; a missing kernel or library is an error;
  * `areas_from_maps`: the restatement of loadGlocalStationsAndCells / loadGlocalWeightMaps for a DEM (project.cpp:2555-2716), and
    `read_areas` for the application's glocal folder (glocalWeight_<i>.flt) and `read_stations_csv` for its area / station csv
    (loadGlocalStationsCsv: the area number, then the station ids, a line);
  * the restatements `marquardt_unweighted`, `r2_adjusted`, `rmse`, `best_fit_unweighted`, `fit_area`, `detrend_area`, `blend_cells` and
    `restate_interpolate`: steps 1 to 3 in Python floats and numpy float32 scalars with the reference's types and operation order, with
    an `arms` counter - the checkers of the CPU tests against the compiled-reference pin (tests/golden/glocal.npz).  Checkers, never a
    fallback.  `marquardt_unweighted` is the reference's unweighted text; the device runs the weighted text with every weight 1.

With the caller stay lapse-rate codes, topographic distance inside an area, the meteo-grid variant, cross validation and output points.
multipleDetrending without areas is `multidetrend`."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import capi, esri, localdetrend as ld, localproxies as lp, meteo, raster
from .capi import pf32, pf64
from .localdetrend import _div, _eq, _sqrt
from .localproxies import _eqf
from .meteo import EPSILON, NODATA, VARIABLES, METHODS, f32

MAX_PROXIES = meteo.MAX_PROXIES
MAX_CELLS = 1 << 24                             # the float cell number is exact up to here
KERNELS = ("k_glocal_areas", "k_glocal_cells")

pi32, pu8, pu32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
# name -> (restype, argtypes): every symbol include/sf3d_glocal.h declares
SIGNATURES = {
    "sf3d_glocal_set_areas": (capi.u8, [capi.u32, pu32, pf32, pf32, pu32, pi32]),
    "sf3d_glocal_interpolate": (capi.u8, [capi.i32, capi.i32, capi.u32, pi32, pf64, pf64, pf32, capi.u32, pf32, capi.f32, meteo.psettings, ld.pfit, lp.pothers, pf32]),
    "sf3d_glocal_get_area_fit": (capi.u8, [capi.u32, capi.u32, pu8, pf32, pf64, pu8, pf64, pf64, pu32, pu32, pf32, pu8]),
    "sf3d_glocal_kernel_ms": (capi.f64, [capi.i32]),
    "sf3d_glocal_bytes": (capi.u64, []),
    "sf3d_glocal_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_glocal.h (and of the headers it stands on) to a loaded product library"""
    lp.bind(sf)
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def flat_areas(areas) -> dict:
    """areas: per area dict(cells=[float cell numbers], weights=[...], stations=[point indices]) -> the arrays of sf3d_glocal_set_areas"""
    cell_offset, station_offset = [0], [0]
    for a in areas:
        if len(a["cells"]) != len(a["weights"]):
            raise ValueError("an area's cells and weights differ in length")
        cell_offset.append(cell_offset[-1] + len(a["cells"]))
        station_offset.append(station_offset[-1] + len(a["stations"]))
    cat = lambda key, dtype: np.ascontiguousarray(np.concatenate([np.asarray(a[key], dtype).ravel() for a in areas]) if areas else np.zeros(0, dtype), dtype)
    return dict(cell_offset=np.array(cell_offset, np.uint32), cell=cat("cells", np.float32), weight=cat("weights", np.float32),
                station_offset=np.array(station_offset, np.uint32), station_index=cat("stations", np.int32))


def set_areas(sf: capi.SF3D, areas) -> None:
    """the project's macro areas (see flat_areas) on the raster of the meteo block"""
    bind(sf)
    f = flat_areas(areas)
    sf.check(sf.lib.sf3d_glocal_set_areas(len(areas), f["cell_offset"].ctypes.data_as(pu32), f["cell"].ctypes.data_as(pf32), f["weight"].ctypes.data_as(pf32),
                                          f["station_offset"].ctypes.data_as(pu32), f["station_index"].ctypes.data_as(pi32)), "glocal_set_areas")
    sf._glocal_areas, sf._glocal_list = len(areas), int(f["station_offset"][-1])


def glocal_settings(proxies, settings: dict | None = None) -> dict:
    """the settings of a call: `proxies` (dicts with active, isHeight), useMultipleDetrending set, useLocalDetrending clear"""
    s = dict(settings or {})
    s["proxies"] = [dict(p) for p in proxies]
    s["useMultipleDetrending"] = s.get("useMultipleDetrending", 1)
    s["useLocalDetrending"] = s.get("useLocalDetrending", 0)
    return s


def interpolate(sf: capi.SF3D, var, method, point_index, x, y, value, proxy_values, bounding_box_area: float, fit: dict, proxies, others,
                settings: dict | None = None, download: bool = True):
    """one temperature map with glocal detrending from the station list (point_index: the index the areas' station lists name; x, y:
    doubles [m]; value: floats, not detrended; proxy_values: [len(proxies), stations] floats in slot order, NODATA where a station has
    none).  The map lands in the meteo block's slot of the variable; download=False: it stays there"""
    bind(sf)
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    v, idx = np.ascontiguousarray(value, np.float32), np.ascontiguousarray(point_index, np.int32)
    pv = np.ascontiguousarray(proxy_values, np.float32).reshape(len(proxies), -1) if len(proxies) else np.zeros((0, len(x)), np.float32)
    if not (x.shape == y.shape == v.shape == idx.shape and x.ndim == 1 and pv.shape[1] == len(x)):
        raise ValueError("point_index, x, y, value and the rows of proxy_values differ in length")
    st = meteo.settings_struct(glocal_settings(proxies, settings))
    ft, ot = ld.fit_struct(dict(fit, minPointsLocalDetrending=fit.get("minPointsLocalDetrending", 0))), lp.others_struct(others)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_glocal_interpolate(raster.index(var, VARIABLES), raster.index(method, METHODS), len(x), idx.ctypes.data_as(pi32), x.ctypes.data_as(pf64),
                                            y.ctypes.data_as(pf64), v.ctypes.data_as(pf32), len(proxies), pv.ctypes.data_as(pf32), float(np.float32(bounding_box_area)),
                                            C.byref(st), C.byref(ft), C.byref(ot), out.ctypes.data_as(pf32) if download else pf32()), "glocal_interpolate")
    return out


def get_area_fit(sf: capi.SF3D) -> dict:
    """per area of the last call: significant, r2, parameters (the height); proxy_significant, slope, intercept per slot; fitted, kept;
    and per entry of the areas' station lists detrended and station_kept"""
    bind(sf)
    na, nl = getattr(sf, "_glocal_areas", 0), getattr(sf, "_glocal_list", 0)          # before set_areas: the library refuses
    sig, r2, par = np.empty(na, np.uint8), np.empty(na, np.float32), np.empty((na, ld.MAX_PARAMETERS), np.float64)
    psig, slope, icpt = np.empty((na, MAX_PROXIES), np.uint8), np.empty((na, MAX_PROXIES), np.float64), np.empty((na, MAX_PROXIES), np.float64)
    fitted, kept = np.empty(na, np.uint32), np.empty(na, np.uint32)
    det, bit = np.empty(nl, np.float32), np.empty(nl, np.uint8)
    sf.check(sf.lib.sf3d_glocal_get_area_fit(na, nl, sig.ctypes.data_as(pu8), r2.ctypes.data_as(pf32), par.ctypes.data_as(pf64), psig.ctypes.data_as(pu8),
                                             slope.ctypes.data_as(pf64), icpt.ctypes.data_as(pf64), fitted.ctypes.data_as(pu32), kept.ctypes.data_as(pu32),
                                             det.ctypes.data_as(pf32), bit.ctypes.data_as(pu8)), "glocal_get_area_fit")
    return dict(significant=sig.astype(bool), r2=r2, parameters=par, proxy_significant=psig.astype(bool), slope=slope, intercept=icpt, fitted=fitted, kept=kept,
                detrended=det, station_kept=bit.astype(bool))


def interpolate_hour(sf: capi.SF3D, stations: dict, method, fit: dict, proxies, others, settings: dict | None = None) -> dict:
    """the hour's two temperature maps, in the order snow.compute_hour takes them: stations[name] = (point_index, x, y, value,
    proxy_values, bounding_box_area[, fit]) for "airT" and / or "dewT"; they stay in the meteo block's slots, where the radiation, snow,
    ET0 and hour blocks read them"""
    names = [n for n in ("airT", "dewT") if n in stations]
    if not names or set(stations) - set(names):
        raise ValueError(f"stations of airT and / or dewT are needed, got {sorted(stations)}")
    out = {}
    for n in names:
        idx, x, y, v, pv, area, *own = stations[n]
        out[n] = interpolate(sf, n, method, idx, x, y, v, pv, area, own[0] if own else fit, proxies, others, settings)
    return out


def kernel_ms(sf: capi.SF3D) -> tuple:
    """(k_glocal_areas, k_glocal_cells) of the last call"""
    return float(sf.lib.sf3d_glocal_kernel_ms(0)), float(sf.lib.sf3d_glocal_kernel_ms(1))


def bytes_held(sf: capi.SF3D) -> int:
    return int(sf.lib.sf3d_glocal_bytes())


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_glocal_clean(), "glocal_clean")
    sf._glocal_areas = sf._glocal_list = 0


# ------------------------------------------------------------------------------------------------ the areas (with the caller)

def _value_from_xy(grid, hdr: dict, x: float, y: float) -> np.float32:
    """Crit3DRasterGrid::getValueFromXY: the cell that holds (x, y), the grid's flag outside"""
    rows, cols = grid.shape
    cs = float(hdr["cellsize"])
    col = int(np.floor((x - float(hdr["xllcorner"])) / cs))
    row = rows - int(np.floor((y - float(hdr["yllcorner"])) / cs)) - 1
    if row < 0 or row >= rows or col < 0 or col >= cols:
        return f32(hdr.get("nodata_value", NODATA))
    return f32(grid[row, col])


def areas_from_maps(dem_header: dict, weight_maps, station_ids_per_area, point_ids) -> list:
    """loadGlocalStationsAndCells and loadGlocalWeightMaps for a DEM (project.cpp:2555-2716).  dem_header: nrows, ncols, xllcorner,
    yllcorner, cellsize; weight_maps: per area None (no file: the area stays without cells), an array on the DEM's header or (array,
    header); station_ids_per_area: the csv's ids; point_ids: the meteo points' ids in index order.  A map is looked up by the DEM cell's
    centre; 0 and NODATA are skipped; a cell is numbered row * ncols + col as a float"""
    rows, cols = int(dem_header["nrows"]), int(dem_header["ncols"])
    cs, xll, yll = float(dem_header["cellsize"]), float(dem_header["xllcorner"]), float(dem_header["yllcorner"])
    ids = [str(p) for p in point_ids]
    out = []
    for a, wanted in enumerate(station_ids_per_area):
        stations = []
        for w in wanted:
            if str(w) in ids:
                stations.append(ids.index(str(w)))                 # the first meteo point of that id
        area = dict(cells=[], weights=[], stations=stations)
        m = weight_maps[a] if a < len(weight_maps) else None
        if m is not None:
            grid, hdr = m if isinstance(m, tuple) else (m, dem_header)
            grid = np.asarray(grid, np.float32)
            for row in range(rows):
                for col in range(cols):
                    x, y = xll + cs * (col + 0.5), yll + cs * (rows - row - 0.5)           # Crit3DRasterGrid::getXY
                    v = _value_from_xy(grid, hdr, x, y)
                    if not _eqf(v, NODATA) and not _eqf(v, 0):
                        area["cells"].append(f32(row * cols + col))
                        area["weights"].append(v)
        area["cells"], area["weights"] = np.array(area["cells"], np.float32), np.array(area["weights"], np.float32)
        out.append(area)
    return out


def read_stations_csv(path) -> list:
    """loadGlocalStationsCsv (project.cpp:2719-2775): a line is `area number, station id, station id, ...`, split at every comma as it
    stands.  A line with a single field is skipped; the list grows to the largest area number seen and a line is assigned by its number,
    so the lines may come in any order, leave gaps (areas without stations) and overwrite one another; a number that does not parse is 0,
    as QString::toInt leaves it.  A negative number indexes before the reference's vector: refused here.  Per area the station ids"""
    areas = []
    with open(path, newline="") as f:
        for raw in f.read().splitlines():
            line = raw.split(",")
            if len(line) <= 1:
                continue
            try:
                number = int(line[0].strip())
            except ValueError:
                number = 0
            if number < 0:
                raise ValueError(f"{path}: area number {number}")
            if number > len(areas) - 1:
                areas.extend([] for _ in range(number + 1 - len(areas)))
            areas[number] = line[1:]
    return areas


def read_areas(folder, stations_csv, dem_header: dict, point_ids) -> list:
    """the application's glocal folder (glocalWeight_<i>.flt, read through esri.read_grid; area i without a file stays without cells) and
    its area / station csv (read_stations_csv) -> areas_from_maps"""
    wanted = read_stations_csv(stations_csv)
    maps = []
    for a in range(len(wanted)):
        base = Path(folder) / f"glocalWeight_{a}"
        maps.append(esri.read_grid(base) if base.with_suffix(".flt").exists() else None)
    return areas_from_maps(dem_header, maps, wanted, point_ids)


def cell_row_col(cell, n_cols: int) -> tuple:
    """int(areaCells[i] / nrCols), int(areaCells[i]) % nrCols (project.cpp:3348-3349): a float quotient"""
    return int(f32(cell) / f32(n_cols)), int(f32(cell)) % n_cols


# ------------------------------------------------------------------------------------------------ restatement (checker)

def _note(arms, key, n=1):
    if arms is not None:
        arms[key] = arms.get(key, 0) + n


def marquardt_unweighted(function: int, par: list, pmin, pmax, pdelta, xs, ys, arms: dict | None = None) -> bool:
    """fittingMarquardt_nDimension without weights (furtherMathFunctions.cpp:2125-2283), as it stands there: `par` is fitted in place"""
    n, nd = len(par), len(ys)
    change, fresh, lam = [0.0] * n, [0.0] * n, [0.01] * n
    sse = 0.0
    for i in range(nd):
        error = ys[i] - ld.lapse_rate(function, xs[i], par)
        sse += error * error
    iteration, unclamped = 0, False
    while True:
        g = [0.0] * n
        a = [[0.0] * n for _ in range(n)]
        first = [ld.lapse_rate(function, xs[i], par) for i in range(nd)]
        P = [[0.0] * nd for _ in range(n)]
        for k in range(n):
            par[k] += pdelta[k]
            for j in range(nd):
                P[k][j] = _div(ld.lapse_rate(function, xs[j], par) - first[j], pdelta[k])
            par[k] -= pdelta[k]
        for i in range(n):
            for j in range(i, n):
                for k in range(nd):
                    a[i][j] += P[i][k] * P[j][k]
        for i in range(n):
            for k in range(nd):
                g[i] += P[i][k] * (ys[k] - first[k])
        for k in range(n):
            a[k][k] += lam[k] * a[k][k]
            for j in range(k + 1, n):
                a[j][k] = a[k][j]
        for j in range(n - 1):
            pivot = EPSILON if a[j][j] < EPSILON else a[j][j]                     # std::max
            for i in range(j + 1, n):
                mult = _div(a[i][j], pivot)
                for k in range(j + 1, n):
                    a[i][k] -= mult * a[j][k]
                g[i] -= mult * g[j]
        last = a[n - 1][n - 1]
        change[n - 1] = _div(g[n - 1], EPSILON if last < EPSILON else last)
        for i in range(n - 2, -1, -1):
            top = g[i]
            for k in range(i + 1, n):
                top -= a[i][k] * change[k]
            change[i] = _div(top, EPSILON if a[i][i] < EPSILON else a[i][i])
        for j in range(n):
            fresh[j] = par[j] + change[j]
            if fresh[j] > pmax[j] and not lam[j] < 1000:
                unclamped = True
            if fresh[j] > pmax[j] and lam[j] < 1000:
                fresh[j] = pmax[j]
                if lam[j] < 1000:
                    lam[j] *= 10
            if fresh[j] < pmin[j]:
                fresh[j] = pmin[j]
                if lam[j] < 1000:
                    lam[j] *= 10
        new_sse = 0.0
        for i in range(nd):
            error = ys[i] - ld.lapse_rate(function, xs[i], fresh)
            new_sse += error * error
        if new_sse == NODATA:
            return False
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
        if not (abs(diff) > ld.FIT_EPSILON and iteration <= ld.MAX_ITERATIONS):
            break
    _note(arms, "the height's fit ends on |diffSSE| <= epsilon" if abs(diff) <= ld.FIT_EPSILON else "the height's fit ends on the iteration cap")
    if unclamped:
        _note(arms, "the maximum clamp with lambda >= 1000 not clamping")
    return abs(diff) <= ld.FIT_EPSILON


def r2_adjusted(obs, sim) -> float:
    """computeR2adjusted, furtherMathFunctions.cpp:1175-1194"""
    mean = 0.0
    for v in obs:
        mean += v
    mean = _div(mean, len(obs))
    rss = tss = 0.0
    for o, s in zip(obs, sim):
        rss += (o - s) * (o - s)
        tss += (o - mean) * (o - mean)
    return 1 - _div(rss, tss)


def rmse(obs, sim) -> float:
    """computeRMSE, furtherMathFunctions.cpp:1324-1340"""
    total = 0.0
    for o, s in zip(obs, sim):
        total += (o - s) * (o - s)
    return _sqrt(_div(total, len(obs)))


def best_fit_unweighted(function: int, pmin, pmax, pdelta, first_guess, xs, ys, arms: dict | None = None):
    """bestFittingMarquardt_nDimension without weights (furtherMathFunctions.cpp:1433-1529): (bestR2, the parameters)"""
    n = len(pmin)
    best = [0.0] * n
    best_r2 = best_rmse = NODATA
    rmse_index = None
    max_z = xs[0]
    for x in xs:
        if x > max_z:
            max_z = x
    valid = True
    for k, guess in enumerate(first_guess):
        par = [float(v) for v in guess[:n]]
        marquardt_unweighted(function, par, pmin, pmax, pdelta, xs, ys, arms)
        if any(par[i] < pmin[i] or par[i] > pmax[i] for i in range(n)):
            _note(arms, "a first guess skipped for leaving its range")
            continue
        sim = [ld.lapse_rate(function, x, par) for x in xs]
        r2, err = r2_adjusted(ys, sim), rmse(ys, sim)
        if _eq(best_rmse, NODATA) or err < best_rmse:
            best_rmse, rmse_index = err, k
        if n > 4:
            valid = (par[0] + par[2]) < max_z
        if _eq(best_r2, NODATA) or (r2 > (best_r2 + ld.DELTA_R2) and valid):
            best = list(par)
            best_r2 = r2
        elif r2 > (best_r2 + ld.DELTA_R2):
            _note(arms, "the double-inversion rule refuses a better R2")
    par = list(best)
    if best_r2 < 0 and rmse_index is not None:
        _note(arms, "bestR2 < 0 with the refit")
        par = [float(v) for v in first_guess[rmse_index][:n]]
        marquardt_unweighted(function, par, pmin, pmax, pdelta, xs, ys, arms)
    return best_r2, par


def elevation_fit_unweighted(h, val, function: int, fit: dict, arms: dict | None = None):
    """multipleDetrendingElevationFitting(.., isWeighted = false) and detrendingElevation over a subset: h: its float heights; val:
    detrended in place where the height is significant.  (R2, the parameters or None)"""
    elevation = [i for i in range(len(val)) if h[i] != f32(NODATA)]
    valid, _ = lp.proxy_validity([h[i] for i in elevation], fit.get("stdDevThreshold", NODATA))
    if not valid:
        return NODATA, None
    xs, ys = [float(h[i]) for i in elevation], [float(val[i]) for i in elevation]
    r2, par = best_fit_unweighted(function, fit["min"], fit["max"], fit["delta"], fit["first_guess"], xs, ys, arms)
    zero = any(_eq(p, NODATA) or _eq(p, 0) for p in par)
    if not _eq(r2, NODATA) or not zero:
        for i in range(len(val)):
            val[i] = val[i] - f32(ld.lapse_rate(function, float(h[i]), par))
        return r2, par
    return r2, None


def _slots(proxies) -> tuple:
    heights = [p for p, q in enumerate(proxies) if q.get("isHeight")]
    height = heights[0] if heights and proxies[heights[0]].get("active") else None
    return height, [p for p, q in enumerate(proxies) if q.get("active") and not q.get("isHeight")]


def fit_area(points, value, proxy_values, fit: dict, proxies, others, arms: dict | None = None) -> dict:
    """step 1 for one area: points: the places in the call's point table of the area's stations that have a point, in the area's order.
    dict(significant, r2, parameters (None or list), lines {slot: (slope, intercept)}, fitted)"""
    height, slots = _slots(proxies)
    function = raster.index(fit["function"], ld.FUNCTIONS)
    pv = np.asarray(proxy_values, np.float32).reshape(len(proxies), -1)
    rows = {p: pv[p][points] for p in range(len(proxies))}
    val = np.asarray(value, np.float32)[points].copy()
    r2, par = NODATA, None
    if height is not None and len(points):
        r2, par = elevation_fit_unweighted(rows[height], val, function, fit, arms)
        _note(arms, "the height significant" if par is not None else "the height not significant")
    elif height is None:
        _note(arms, "the height not active")
    seen = {}
    left, lines = lp.other_proxies(rows, val, None, slots, others, 0, seen) if len(points) else (list(range(len(points))), {})
    if lines and len(left) < len(points) and arms is not None:
        arms["a station pruned or erased in the fit of step 1"] = arms.get("a station pruned or erased in the fit of step 1", 0) + 1
    if par is not None and lines:
        _note(arms, "the height significant with others significant")
    return dict(significant=par is not None, r2=f32(r2), parameters=par, lines=lines, fitted=len(points), pruned=len(points) - len(left))


def detrend_area(points, value, proxy_values, fit: dict, proxies, area_fit: dict, arms: dict | None = None) -> tuple:
    """step 2, macroAreaDetrending: the subset again from all the area's points, detrended with the area's parameters.
    (kept: positions within `points`, their detrended float values)"""
    height, _ = _slots(proxies)
    function = raster.index(fit["function"], ld.FUNCTIONS)
    pv = np.asarray(proxy_values, np.float32).reshape(len(proxies), -1)
    val = np.asarray(value, np.float32)[points].copy()
    if area_fit["parameters"] is not None:
        par = list(area_fit["parameters"])
        for i in range(len(val)):
            val[i] = val[i] - f32(ld.lapse_rate(function, float(pv[height][points[i]]), par))
    lines = area_fit["lines"]
    if not lines:
        return list(range(len(points))), val
    sig = sorted(lines)
    flat = [v for p in sig for v in lines[p]]
    kept = []
    for i in range(len(val)):
        if any(_eqf(pv[p][points[i]], NODATA) for p in sig):
            _note(arms, "a station erased by detrendingOtherProxies in step 2")
            continue
        val[i] = val[i] - f32(lp.function_sum([float(pv[p][points[i]]) for p in sig], flat))
        kept.append(i)
    return kept, val[kept]


def interpolate_over(method: int, x, y, sx, sy, val, bounding_box_area) -> np.float32:
    """interpolate()'s methods over a subset (sx, sy: doubles; val: floats) with the neighbour search of the meteo block; x, y: floats"""
    n = len(val)
    with np.errstate(all="ignore"):
        dx, dy = np.asarray(sx, np.float64).astype(np.float32) - x, np.asarray(sy, np.float64).astype(np.float32) - y
        d = np.sqrt(dx * dx + dy * dy)
        if method == meteo.IDW:
            return f32(ld._idw(d, val))
        idx, radius = meteo._neighbours(d, meteo.shepard_initial_radius(bounding_box_area, n))
        if method == meteo.SHEPARD:
            return f32(meteo._shepard(idx, radius, d, sx, sy, val, x, y))
        return f32(meteo._shepard_modified(idx, radius, d, sx, sy, val, x, y))


def restate_interpolate(dem, xll, yll, cell_size, proxy_maps, areas, var, method, point_index, x, y, value, proxy_values, bounding_box_area, fit: dict, proxies, others,
                        settings: dict | None = None, flag: float = NODATA, mine=None, arms: dict | None = None) -> dict:
    """steps 1 to 3, the areas in index order.  dict(value: the map; failed: an interpolate() gave NODATA; and get_area_fit's arrays)"""
    if raster.index(var, VARIABLES) not in ld.LOCAL_VARIABLES:
        raise ValueError("glocal detrending is for the two temperatures")
    method = raster.index(method, METHODS)
    dem = np.asarray(dem, np.float32)
    fl = f32(flag)
    shape = dem.shape
    function = raster.index(fit["function"], ld.FUNCTIONS)
    sx, sy, sv = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(value, np.float32)
    pv = np.asarray(proxy_values, np.float32).reshape(len(proxies), -1)
    height, slots = _slots(proxies)
    index = [int(i) for i in point_index]
    na, nl = len(areas), sum(len(a["stations"]) for a in areas)
    out = dict(value=np.full(shape, fl, np.float32), failed=False, significant=np.zeros(na, bool), r2=np.full(na, NODATA, np.float32),
               parameters=np.full((na, ld.MAX_PARAMETERS), NODATA, np.float64), proxy_significant=np.zeros((na, MAX_PROXIES), bool),
               slope=np.full((na, MAX_PROXIES), NODATA, np.float64), intercept=np.full((na, MAX_PROXIES), NODATA, np.float64), fitted=np.zeros(na, np.uint32),
               kept=np.zeros(na, np.uint32), detrended=np.full(nl, NODATA, np.float32), station_kept=np.zeros(nl, bool))
    cx, cy = meteo.cell_centres(shape, float(xll), float(yll), float(cell_size))
    cells = lp.cell_proxy_values(dem, proxy_maps, flag)
    use = bool((settings or {}).get("useDetrending", 1))
    covered = np.zeros(shape, np.int32)
    first = 0
    with np.errstate(all="ignore"):
        for a, area in enumerate(areas):
            entries = [(l, index.index(int(s))) for l, s in enumerate(area["stations"]) if int(s) in index]
            points = [p for _, p in entries]
            if len(area["stations"]) == 0 and len(area["cells"]) == 0:
                first += len(area["stations"])
                continue
            fa = fit_area(points, sv, pv, fit, proxies, others, arms)
            kept, val = detrend_area(points, sv, pv, fit, proxies, fa, arms)
            if fa["pruned"] and len(kept) > len(points) - fa["pruned"]:
                _note(arms, "a station pruned in the fit of step 1 but present in the rebuilt subset")
            out["significant"][a], out["r2"][a], out["fitted"][a], out["kept"][a] = fa["significant"], fa["r2"], fa["fitted"], len(kept)
            if fa["parameters"] is not None:
                out["parameters"][a, :len(fa["parameters"])] = fa["parameters"]
            for p, (s, i) in fa["lines"].items():
                out["proxy_significant"][a, p], out["slope"][a, p], out["intercept"][a, p] = True, s, i
            for k, i in enumerate(kept):
                out["detrended"][first + entries[i][0]], out["station_kept"][first + entries[i][0]] = val[k], True
            first += len(area["stations"])
            kx, ky = sx[[points[i] for i in kept]], sy[[points[i] for i in kept]]
            used = ([height] if fa["parameters"] is not None else []) + sorted(fa["lines"])
            for cell, weight in zip(area["cells"], area["weights"]):
                r, c = cell_row_col(cell, shape[1])
                if abs(float(dem[r, c]) - float(fl)) < EPSILON or (mine is not None and not mine[r, c]):
                    continue
                covered[r, c] += 1
                _note(arms, f"a cell visited by its area number {covered[r, c]}" if covered[r, c] <= 3 else "a cell visited by more than three areas")
                now = out["value"][r, c]
                if any(float(cells[r, c][p]) == NODATA for p in used):
                    _note(arms, "a cell set to NODATA by a later area" if covered[r, c] > 1 and not _eqf(now, NODATA) else "a cell set to NODATA")
                    out["value"][r, c] = NODATA
                    continue
                if covered[r, c] > 1 and _eqf(now, NODATA):
                    _note(arms, "a cell set to NODATA by an earlier area and then refilled")
                res = interpolate_over(method, f32(cx[r, c]), f32(cy[r, c]), kx, ky, val, bounding_box_area)
                if abs(float(res) - NODATA) < EPSILON:
                    out["failed"] = True
                    res = f32(NODATA)
                elif use and used:
                    total = 0.0
                    if fa["parameters"] is not None:
                        total += ld.lapse_rate(function, float(cells[r, c][height]), list(fa["parameters"]))
                    for p in sorted(fa["lines"]):
                        total += fa["lines"][p][0] * float(cells[r, c][p]) + fa["lines"][p][1]
                    res = f32(res + f32(float(f32(total))))
                product = float(res) * float(f32(weight))
                out["value"][r, c] = f32(product) if _eqf(now, NODATA) else f32(float(now) + product)
    if arms is not None:
        inside = np.abs(dem.astype(np.float64) - float(fl)) >= EPSILON
        _note(arms, "a DEM cell covered by no area", int((inside & (covered == 0)).sum()))
    return out
