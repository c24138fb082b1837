"""Topographic distance on the device (include/sf3d_topodist.h, criteria3d_amd/csrc/sf3d_topodist.inc), on the raster of the meteo block
(`meteo.initialize` comes first): the maps of `gis::topographicDistanceMap` (agrolib/gis/gis.cpp:1650-1675), `interpolate()` with the
distances of `computeDistances` under `getUseTD()` (agrolib/interpolation/interpolation.cpp:208-256), and the station matrix the caller's
Kh search (`topographicDistanceOptimize`, :2297-2368) evaluates `interpolate()` with.

Three parts:
  * the binding (`bind`, `compute`, `get_map`, `set_map`, `drop_map`, `station_matrix`, `interpolate`, `interpolate_hour`): a missing
    kernel or library is an error;
  * `save_maps` / `load_maps`: the application's TD_<dem>_<id>.flt files (agrolib/project/project.cpp:2362, 2412) over `esri.py`;
  * the restatements `restate_map`, `restate_distances`, `restate_interpolate`, `restate_station_matrix` and `optimize_kh`: the same
    arithmetic in numpy float32 / float64 with the reference's types and operation order, feeding `meteo.py`'s `_shepard`,
    `_shepard_modified`, `_retrend` and `_tail` - the checkers of the CPU tests against the compiled-reference pin
    (tests/golden/topodist.npz).  Checkers, never a fallback."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import capi, esri, meteo, raster
from .capi import pf32, pf64, pi32
from .meteo import EPSILON, NODATA, VARIABLES, METHODS, f32

MAX_STEPS = 65536                               # SF3D_TOPODIST_MAX_STEPS
MAX_STATIONS = meteo.MAX_STATIONS
GOLDEN_SECTION = 1.6180339887499                # commonConstants.h:258
# getUseTdVar (interpolation.cpp:1220-1234) among meteo.VARIABLES
TD_VARIABLES = (meteo.AIR_TEMPERATURE, meteo.AIR_REL_HUMIDITY, meteo.WIND_SCALAR_INTENSITY, meteo.AIR_DEW_TEMPERATURE)
# what sf3d_topodist_interpolate still refuses of sf3d_meteo_settings_t
UNSUPPORTED = tuple(n for n in meteo.UNSUPPORTED if n != "useTopographicDistance")

# name -> (restype, argtypes): every symbol include/sf3d_topodist.h declares
SIGNATURES = {
    "sf3d_topodist_compute": (capi.u8, [capi.u32, pf64, pf64, pf64]),
    "sf3d_topodist_bytes": (capi.u64, []),
    "sf3d_topodist_get_map": (capi.u8, [capi.u32, capi.u32, pf32]),
    "sf3d_topodist_set_map": (capi.u8, [capi.u32, capi.u32, pf32]),
    "sf3d_topodist_drop_map": (capi.u8, [capi.u32]),
    "sf3d_topodist_interpolate": (capi.u8, [capi.i32, capi.i32, capi.u32, pf64, pf64, pf64, pf32, pi32, capi.f32, meteo.psettings, capi.i32, pf32]),
    "sf3d_topodist_station_matrix": (capi.u8, [capi.u32, pf64, pf64, pf64, pi32, pf32]),
    "sf3d_topodist_kernel_ms": (capi.f64, [capi.i32]),
    "sf3d_topodist_clean": (capi.u8, []),
}
KERNELS = ("k_topodist_maps", "k_meteo_idw_td", "k_topodist_matrix")       # the order of sf3d_topodist_kernel_ms


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_topodist.h (and of sf3d_meteo.h) to a loaded product library (AttributeError if a symbol is missing)"""
    meteo.bind(sf)
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def _points(x, y, z):
    x, y, z = (np.ascontiguousarray(a, np.float64) for a in (x, y, z))
    if not (x.shape == y.shape == z.shape and x.ndim == 1):
        raise ValueError("x, y and z differ in length")
    return x, y, z


def _indices(map_index, n):
    """None: no station carries a map"""
    m = np.full(n, -1, np.int32) if map_index is None else np.ascontiguousarray(map_index, np.int32)
    if m.shape != (n,):
        raise ValueError("map_index and the stations differ in length")
    return m


def compute(sf: capi.SF3D, x, y, z) -> None:
    """gis::topographicDistanceMap for every point (x, y: utm [m]; z: height [m]): the maps stay on the device (get_map)"""
    bind(sf)
    x, y, z = _points(x, y, z)
    sf.check(sf.lib.sf3d_topodist_compute(len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64), z.ctypes.data_as(pf64)), "topodist_compute")


def bytes_held(sf: capi.SF3D) -> int:
    return int(sf.lib.sf3d_topodist_bytes())


def get_map(sf: capi.SF3D, index: int) -> np.ndarray:
    out = np.empty(sf._meteo_shape, np.float32)
    sf.check(sf.lib.sf3d_topodist_get_map(int(index), out.size, out.ctypes.data_as(pf32)), "topodist_get_map")
    return out


def set_map(sf: capi.SF3D, index: int, values) -> None:
    """a map the caller holds (load_maps) in the place of map `index`"""
    v = raster.f32(values, sf._meteo_shape, "topodist")
    sf.check(sf.lib.sf3d_topodist_set_map(int(index), v.size, v.ctypes.data_as(pf32)), "topodist_set_map")


def drop_map(sf: capi.SF3D, index: int) -> None:
    """the station of map `index` has no map from now on (topographicDistance == nullptr)"""
    sf.check(sf.lib.sf3d_topodist_drop_map(int(index)), "topodist_drop_map")


def station_matrix(sf: capi.SF3D, x, y, z, map_index=None) -> np.ndarray:
    """matrix[j, i]: the topoDistance computeDistances uses for station i at station j's (float x, float y, float z)"""
    bind(sf)
    x, y, z = _points(x, y, z)
    m = _indices(map_index, len(x))
    out = np.empty((len(x), len(x)), np.float32)
    sf.check(sf.lib.sf3d_topodist_station_matrix(len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64), z.ctypes.data_as(pf64), m.ctypes.data_as(pi32),
                                                 out.ctypes.data_as(pf32)), "topodist_station_matrix")
    return out


def interpolate(sf: capi.SF3D, var, method, x, y, z, value, map_index, bounding_box_area: float, settings: dict | None = None, kh: int = 0,
                download: bool = True):
    """meteo.interpolate under getUseTD(): z the stations' heights, map_index per station the map it carries (-1 or None: none),
    settings["useTopographicDistance"] 0 or 1, kh = getTopoDist_Kh().  The map lands in the meteo block's slot of the variable."""
    bind(sf)
    x, y, z = _points(x, y, z)
    v = np.ascontiguousarray(value, np.float32)
    if v.shape != x.shape:
        raise ValueError("x, y, z and value differ in length")
    m = _indices(map_index, len(x))
    st = meteo.settings_struct(settings)
    out = np.empty(sf._meteo_shape, np.float32) if download else None
    sf.check(sf.lib.sf3d_topodist_interpolate(raster.index(var, VARIABLES), raster.index(method, METHODS), len(x), x.ctypes.data_as(pf64), y.ctypes.data_as(pf64),
                                              z.ctypes.data_as(pf64), v.ctypes.data_as(pf32), m.ctypes.data_as(pi32), float(np.float32(bounding_box_area)),
                                              C.byref(st), int(kh), out.ctypes.data_as(pf32) if download else pf32()), "topodist_interpolate")
    return out


def interpolate_hour(sf: capi.SF3D, stations: dict, method, settings: dict | None = None, kh: dict | None = None) -> dict:
    """the hour's maps, as meteo.interpolate_hour: stations[name] = (x, y, z, value, map_index, bounding_box_area[, settings]) for "airT",
    "prec", "relHum", "windInt" and, optionally, "globalRad"; kh[name]: the Kh of a TD variable (0 where it is missing)"""
    names = [n for n in VARIABLES[:5] if n in stations]
    if names[:4] != list(VARIABLES[:4]):
        raise ValueError(f"stations of {VARIABLES[:4]} are needed, got {sorted(stations)}")
    out = {}
    for n in names:
        x, y, z, v, m, area, *own = stations[n]
        out[n] = interpolate(sf, n, method, x, y, z, v, m, area, own[0] if own else settings, int((kh or {}).get(n, 0)))
    return out


def kernel_ms(sf: capi.SF3D, kernel) -> float:
    return float(sf.lib.sf3d_topodist_kernel_ms(raster.index(kernel, KERNELS)))


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_topodist_clean(), "topodist_clean")


# ------------------------------------------------------------------------------------------------ the application's files

def map_path(directory, dem_name: str, point_id) -> Path:
    """<directory>/TD_<dem base name>_<id> (project.cpp:2362): .flt and .hdr beside each other"""
    return Path(directory) / f"TD_{Path(dem_name).stem}_{point_id}"


def save_maps(directory, dem_name: str, ids, maps, hdr: dict) -> list:
    """one ESRI float grid per station, named as Project::writeTopographicDistanceMap names them"""
    Path(directory).mkdir(parents=True, exist_ok=True)
    paths = []
    for point_id, m in zip(ids, maps):
        p = map_path(directory, dem_name, point_id)
        esri.write_grid(p, m, hdr)
        paths.append(p)
    return paths


def load_maps(directory, dem_name: str, ids) -> list:
    """the maps of the stations `ids` as Project::loadTopographicDistanceMaps reads them; None where a station has no file"""
    out = []
    for point_id in ids:
        p = map_path(directory, dem_name, point_id)
        out.append(esri.read_grid(p)[0] if Path(str(p) + ".flt").exists() else None)
    return out


# ------------------------------------------------------------------------------------------------ restatements (checkers)

def _is_equal(a, b):
    """isEqual(float, float), basicMath.h:25"""
    return np.abs(np.asarray(a, np.float64) - np.float64(b)) < EPSILON


def _distance(x, y, sx, sy):
    """gis::computeDistance on floats (gis.cpp:685-691); broadcasts"""
    dx, dy = f32(sx) - f32(x), f32(sy) - f32(y)
    return np.sqrt(dx * dx + dy * dy, dtype=np.float32)


def _dem_at(dem, xll, yll, cell_size, flag, x, y):
    """Crit3DRasterGrid::getValueFromXY (gis.cpp:533-546) for float arrays x, y: int() truncates"""
    inv = 1.0 / cell_size
    rows, cols = dem.shape
    r = np.trunc((y.astype(np.float64) - yll) * inv).astype(np.int64)
    row = (rows - 1) - r
    col = np.trunc((x.astype(np.float64) - xll) * inv).astype(np.int64)
    inside = (row >= 0) & (row < rows) & (col >= 0) & (col < cols)
    out = np.full(x.shape, f32(flag), np.float32)
    out[inside] = dem[row[inside], col[inside]]
    return out, inside


def _walk(dem, xll, yll, cell_size, flag, x1, y1, z1, x2, y2, z2, distance, arms=None):
    """gis::topographicDistance (gis.cpp:1595-1647) for arrays of float32 (all of one shape)"""
    dem = np.asarray(dem, np.float32)
    shape = np.shape(distance)
    x1, y1, z1, x2, y2, z2, distance = (np.broadcast_to(f32(a), shape).astype(np.float32).ravel() for a in (x1, y1, z1, x2, y2, z2, distance))
    step = f32(cell_size)
    out = np.zeros(distance.shape, np.float32)
    go = ~(distance < step)
    with np.errstate(all="ignore"):
        nr = np.where(go, np.trunc(distance / step), 0).astype(np.int64)
        first = z1 < z2
        xi, yi, zi = np.where(first, x1, x2), np.where(first, y1, y2), np.where(first, z1, z2)
        xf, yf = np.where(first, x2, x1), np.where(first, y2, y1)
        nrf = nr.astype(np.float32)
        dx, dy = (xf - xi) / nrf, (yf - yi) / nrf
    if arms is not None:
        arms["below"] = arms.get("below", 0) + int((~go).sum())
        arms["first"] = arms.get("first", 0) + int((go & first).sum())
        arms["second"] = arms.get("second", 0) + int((go & ~first).sum())
    x, y = xi.copy(), yi.copy()
    for i in range(1, int(nr.max()) + 1 if nr.size else 1):
        live = np.nonzero(nr >= i)[0]
        x[live] = x[live] + dx[live]
        y[live] = y[live] + dy[live]
        v, inside = _dem_at(dem, xll, yll, cell_size, flag, x[live], y[live])
        valid = ~_is_equal(v, flag)
        if arms is not None:
            arms["outside"] = arms.get("outside", 0) + int((~inside).sum())
            arms["flag"] = arms.get("flag", 0) + int((inside & ~valid).sum())
        up = valid & (v > zi[live])
        rise = v - zi[live]
        cur = out[live]
        out[live] = np.where(up & ~(cur > rise), rise, cur)
    return out.reshape(shape)


def restate_map(dem, xll, yll, cell_size, px, py, pz, flag: float = NODATA, mine=None, arms=None) -> np.ndarray:
    """gis::topographicDistanceMap (gis.cpp:1650-1675) for the point (px, py, pz); `mine` (bool map): the cells computed"""
    dem = np.asarray(dem, np.float32)
    out = np.full(dem.shape, f32(flag), np.float32)
    valid = ~_is_equal(dem, flag)
    if mine is not None:
        valid &= np.asarray(mine, bool)
    cx, cy = meteo.cell_centres(dem.shape, float(xll), float(yll), float(cell_size))
    gx, gy = cx[valid].astype(np.float32), cy[valid].astype(np.float32)
    sx, sy, sz = f32(np.float64(px)), f32(np.float64(py)), f32(np.float64(pz))
    d = _distance(gx, gy, sx, sy)
    out[valid] = _walk(dem, float(xll), float(yll), float(cell_size), flag, gx, gy, dem[valid], sx, sy, sz, d, arms)
    return out


def _lookup(maps, map_index, shape, xll, yll, cell_size, x, y):
    """the station maps at the float points (x[k], y[k]) as computeDistances reads them: isOutOfGridXY (gis.cpp:840-845), getRowColFromXY with
    floor (:735-739) -> [points, stations] float32, NODATA where there is no map or the point is outside"""
    rows, cols = shape
    inv = 1.0 / cell_size
    xd, yd = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    outside = (xd < xll) | (yd < yll) | (xd >= (xll + cols * cell_size)) | (yd >= (yll + rows * cell_size))
    row = (rows - 1) - np.floor((yd - yll) * inv).astype(np.int64)
    col = np.floor((xd - xll) * inv).astype(np.int64)
    ok = ~outside & (row >= 0) & (row < rows) & (col >= 0) & (col < cols)
    t = np.full((len(xd), len(map_index)), f32(NODATA), np.float32)
    for i, m in enumerate(map_index):
        if m >= 0:
            t[ok, i] = np.asarray(maps[m], np.float32)[row[ok], col[ok]]
    return t, row, col, ok


def restate_topo(dem, xll, yll, cell_size, flag, x, y, z, sx, sy, sz, maps=None, map_index=None, arms=None) -> np.ndarray:
    """topoDistance of computeDistances (interpolation.cpp:232-247) for the float points (x, y, z) and every station -> [points, stations]"""
    dem = np.asarray(dem, np.float32)
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    sxf, syf, szf = (np.asarray(a, np.float64).astype(np.float32) for a in (sx, sy, sz))
    index = np.full(len(sxf), -1, np.int64) if map_index is None else np.asarray(map_index, np.int64)
    t, _, _, _ = _lookup(maps, index, dem.shape, float(xll), float(yll), float(cell_size), x, y)
    d = _distance(x[:, None], y[:, None], sxf[None, :], syf[None, :])
    miss = _is_equal(t, NODATA)
    if arms is not None:
        arms["map hit"] = arms.get("map hit", 0) + int((~miss).sum())
        arms["map miss"] = arms.get("map miss", 0) + int((miss & (index >= 0)[None, :]).sum())
    if miss.any():
        p, s = np.nonzero(miss)
        t[p, s] = _walk(dem, float(xll), float(yll), float(cell_size), flag, x[p], y[p], z[p], sxf[s], syf[s], szf[s], d[p, s])
    return t


def restate_distances(dem, xll, yll, cell_size, flag, x, y, z, sx, sy, sz, var, kh: int, maps=None, map_index=None, use_td: bool = True, topo=None):
    """computeDistances (interpolation.cpp:208-256) for the float points (x, y, z): [points, stations] float32.  distance += kh *
    topoDistance (an int times a float) for a TD variable under use_td and kh != 0; topo: a ready [points, stations] topoDistance"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    sxf, syf = np.asarray(sx, np.float64).astype(np.float32), np.asarray(sy, np.float64).astype(np.float32)
    d = _distance(x[:, None], y[:, None], sxf[None, :], syf[None, :])
    if use_td and raster.index(var, VARIABLES) in TD_VARIABLES and int(kh) != 0:
        if topo is None:
            topo = restate_topo(dem, xll, yll, cell_size, flag, x, y, z, sx, sy, sz, maps, map_index)
        with np.errstate(all="ignore"):
            d = d + (f32(int(kh)) * np.asarray(topo, np.float32))
    return d


def restate_station_matrix(dem, xll, yll, cell_size, flag, sx, sy, sz, maps=None, map_index=None) -> np.ndarray:
    """what sf3d_topodist_station_matrix returns: matrix[j, i], station i seen from station j's float position"""
    xf, yf, zf = (np.asarray(a, np.float64).astype(np.float32) for a in (sx, sy, sz))
    return restate_topo(dem, xll, yll, cell_size, flag, xf, yf, zf, sx, sy, sz, maps, map_index)


def _idw(d, sv) -> np.float32:
    """inverseDistanceWeighted (interpolation.cpp:1031-1051) on one distance vector"""
    s = sw = 0.0
    for i in range(len(d)):
        di = float(d[i])
        if di > EPSILON:
            km = di / 10000.
            w = 1.0 / (km * km * km)
            sw += w
            s += float(sv[i]) * w
    return f32(s / sw) if sw > 0.0 else f32(NODATA)


def _interpolate_point(var: int, method: int, d, sx, sy, sv, x, y, radius0, settings: dict, proxy_values, threshold, arms=None) -> np.float32:
    """interpolate() (interpolation.cpp:2502-2560) after its distance vector `d`, at the float point (x, y)"""
    if var == meteo.PRECIPITATION and settings.get("allZero", 0):
        return f32(0)
    with np.errstate(all="ignore"):
        if method == meteo.IDW:
            res = _idw(d, sv)
        else:
            idx, radius = meteo._neighbours(d, radius0)
            if arms is not None:
                inside = sum(1 for i in range(len(d)) if d[i] <= radius0 and d[i] > 0)
                key = "input order" if meteo.SHEPARD_MIN <= inside <= meteo.SHEPARD_MAX else "insertion"
                arms[key] = arms.get(key, 0) + 1
            res = (meteo._shepard if method == meteo.SHEPARD else meteo._shepard_modified)(idx, radius, d, sx, sy, sv, x, y)
        if abs(float(res) - NODATA) < EPSILON:
            return f32(NODATA)
        if settings.get("useDetrending", 1):
            res = f32(res + meteo._retrend(var, settings, proxy_values))
        return meteo._tail(var, res, threshold)


def restate_interpolate(dem, xll, yll, cell_size, proxy_maps, var, method, x, y, z, value, bounding_box_area, settings: dict | None = None, kh: int = 0,
                        maps=None, map_index=None, flag: float = NODATA, mine=None, arms=None) -> np.ndarray:
    """what sf3d_topodist_interpolate computes: interpolate() on every DEM cell with the distances of restate_distances"""
    settings = settings or {}
    var, method = raster.index(var, VARIABLES), raster.index(method, METHODS)
    dem = np.asarray(dem, np.float32)
    fl = f32(flag)
    out = np.full(dem.shape, fl, np.float32)
    sx, sy = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sv = np.asarray(value, np.float32)
    valid = ~_is_equal(dem, flag)
    if mine is not None:
        valid &= np.asarray(mine, bool)
    cells = np.argwhere(valid)
    if var == meteo.PRECIPITATION and settings.get("allZero", 0):
        out[valid] = 0.
        return out
    cx, cy = meteo.cell_centres(dem.shape, float(xll), float(yll), float(cell_size))
    xf, yf = cx[valid].astype(np.float32), cy[valid].astype(np.float32)
    topo = None
    if settings.get("useTopographicDistance", 0) and var in TD_VARIABLES and int(kh) != 0:
        topo = restate_topo(dem, xll, yll, cell_size, flag, xf, yf, dem[valid], sx, sy, z, maps, map_index, arms)
    dist = restate_distances(dem, xll, yll, cell_size, flag, xf, yf, dem[valid], sx, sy, z, var, kh, use_td=topo is not None, topo=topo)
    radius0 = meteo.shepard_initial_radius(bounding_box_area, len(sx))
    threshold = f32(settings.get("rainfallThreshold", 0.0))
    for k, (r, c) in enumerate(cells):
        pv = []
        for q, p in enumerate(settings.get("proxies", [])):
            m = dem if (q >= len(proxy_maps) or proxy_maps[q] is None) else np.asarray(proxy_maps[q], np.float32)
            pv.append(float(m[r, c]) if (p.get("active", 0) and m[r, c] != fl) else NODATA)
        out[r, c] = _interpolate_point(var, method, dist[k], sx, sy, sv, xf[k], yf[k], radius0, settings, pv, threshold, arms)
    return out


def optimize_kh(var, method, x, y, z, value, observed, matrix, bounding_box_area, settings: dict | None = None, max_kh: int = 128, proxy_values=None,
                inside_dem=None):
    """topographicDistanceOptimize (interpolation.cpp:2297-2368): goldenSectionSearch over kh in [0, max_kh] of the cross-validation error of
    interpolate() at the stations - computeResiduals(excludeOutsideDem = true, excludeSupplemental = true; spatialControl.cpp:102-160),
    computeErrorCrossValidation (:310-333), statistics::meanAbsoluteError (statistics.cpp:201-220).  value: the interpolation points'
    (detrended) values; observed: the meteo points' currentValue; matrix: a station matrix (station_matrix / restate_station_matrix);
    proxy_values[j]: the meteo point's proxy values for retrend; inside_dem[j]: isInsideDem.  Every station is active, accepted and primary.
    -> (Kh as the int setTopoDist_Kh gets, the Kh series as [(float kh, float error)])"""
    settings = dict(settings or {}, useTopographicDistance=1)
    var, method = raster.index(var, VARIABLES), raster.index(method, METHODS)
    sx, sy = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xf, yf = sx.astype(np.float32), sy.astype(np.float32)
    sv, obs = np.asarray(value, np.float32), np.asarray(observed, np.float32)
    n = len(sx)
    matrix = np.asarray(matrix, np.float32).reshape(n, n)
    inside = np.ones(n, bool) if inside_dem is None else np.asarray(inside_dem, bool)
    radius0 = meteo.shepard_initial_radius(bounding_box_area, n)
    threshold = f32(settings.get("rainfallThreshold", 0.0))
    plain = _distance(xf[:, None], yf[:, None], xf[None, :], yf[None, :])
    nodata = f32(NODATA)

    def error(kh_float: float) -> float:
        """topographicDistanceInternalFunction: a float error returned as double"""
        kh = int(kh_float)
        d = plain
        if var in TD_VARIABLES and kh != 0:
            with np.errstate(all="ignore"):
                d = plain + (f32(kh) * matrix)
        total, count = 0.0, 0
        for j in range(n):
            if not inside[j]:
                continue
            my = obs[j]
            est = _interpolate_point(var, method, d[j], sx, sy, sv, xf[j], yf[j], radius0, settings, proxy_values[j] if proxy_values is not None else [], threshold)
            if var == meteo.PRECIPITATION:
                if my != nodata and my < threshold:
                    my = f32(0)
                if est != nodata and est < threshold:
                    est = f32(0)
            if est == nodata or my == nodata:
                continue
            residual = f32(my - est)
            value_j = obs[j]
            if value_j == nodata or residual == nodata:
                continue
            simulated = f32(value_j - residual)
            if simulated == nodata:
                continue
            total += abs(float(f32(value_j - simulated)))
            count += 1
        if count == 0:
            return float(nodata)
        return float(f32(total / count))

    series = []
    a, b = 0.0, float(max_kh)
    x1 = b - (b - a) / GOLDEN_SECTION
    x2 = a + (b - a) / GOLDEN_SECTION
    counter = 0
    while abs(b - a) > 1 and counter < 100:
        counter += 1
        if error(x1) < error(x2):
            b = x2
            x2 = x1
            x1 = b - (b - a) / GOLDEN_SECTION
            series.append((f32(x1), f32(error(x1))))
        else:
            a = x1
            x1 = x2
            x2 = a + (b - a) / GOLDEN_SECTION
            series.append((f32(x2), f32(error(x2))))
    series.append((f32((a + b) / 2), f32(error((a + b) / 2))))
    return int((a + b) / 2), series
