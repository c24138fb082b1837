"""What tests/test_hour_host.py, tests/test_gpu_hour.py and scripts/multirank_hour_worker.py share (no tests here): the pins
tests/golden/relhum_dew.npz and pond_day.npz, the host build of the per-cell text (tests/hour_host.cpp), and a small "world" - every raster
block and a node model on one small raster - with the hour driven through it in two ways: every stage's maps downloaded and handed to the
next stage through the host-pointer entry points, and in place through include/sf3d_hour.h."""
from pathlib import Path

import numpy as np

from criteria3d_amd import catchment as cm, crop, hour, meteo, radiation as rad, root, sinks, snow
from tests import crop_cases as cc
from tests import root_cases as rc
from tests import sink_cases as sc

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SHAPES = ((7, 37), (3, 11), (1, 300))          # 259 cells: one block and three lanes; 33: less than a wave; 300: a partial second block
TWO_POW_MINUS_53 = 2.0 ** -53


def load_relhum_pin():
    z = np.load(GOLDEN / "relhum_dew.npz")
    return {k: z[k] for k in z.files}


def load_pond_pin():
    z = np.load(GOLDEN / "pond_day.npz")
    p = {k: z[k] for k in z.files}
    p["unit"] = np.where(p["unit_index"] == int(p["flag"]), -1, p["unit_index"]).astype(np.int32)      # getLandUnitIndexRowCol, -1 for NODATA
    return p


def run_host(exe, tmp_path, rh, pd, case, tag="x"):
    """the pins' inputs through the host program -> (relHum of the pairs, the raster's map, the pond map of `case` (0: computeCrop on, 1: off))"""
    from tests.raster_helpers import Reader, run_host_program
    parts = [np.array([rh["dew_t"].size, rh["map_air_t"].size], np.int32), np.array([rh["flag"]], np.float32)]
    parts += [np.asarray(rh[name], np.float32) for name in ("dew_t", "air_t", "map_air_t", "map_dew_t")]
    parts += [np.array([pd["slope"].size, len(pd["maximum_pond"]), int(pd["compute_crop"][case])], np.int32), np.array([pd["slope_flag"], pd["flag"]], np.float32),
              np.asarray(pd["slope"], np.float32), np.asarray(pd["unit"], np.int32), np.asarray(pd["lai"], np.float32),
              np.stack([pd["maximum_pond"], pd["lai_max"]], axis=1).astype(np.float64), np.asarray(pd["is_crop"], np.int32)]
    out = Reader(run_host_program(exe, tmp_path, tag, parts))
    got = out.take(np.float32, rh["dew_t"].size), out.take(np.float32, *rh["map_air_t"].shape), out.take(np.float32, *pd["slope"].shape)
    assert out.done()
    return got


def pond_restated(pd, case, surface_index=None, mine=None):
    return hour.restate_pond(pd["slope"], pd["unit"], pd["maximum_pond"], pd["lai_max"], pd["is_crop"], bool(pd["compute_crop"][case]), pd["lai"],
                             float(pd["slope_flag"]), float(pd["flag"]), surface_index, mine)


# ---- the small world: every block on one raster

GEO = (683768.0, 4928230.0)                    # lower left corner [m, UTM 32]; the cell size is the sink pin's
HOURS = ((2021, 3, 20, 10, 0, 0), (2021, 3, 20, 11, 0, 0))
METHOD = "idw"


def world(pin, shape, seed=None):
    """a small case of tests/sink_cases.py (DEM with flag cells, indices, column table, node model tables) with what the other blocks need on
    the same raster: latitude / longitude / slope / aspect maps, the crop table of the crop pin, and per hour a station list per meteo
    variable.  pin: sink_cases.load_pin()."""
    case = sc.small_case(pin, shape, seed=shape[1] if seed is None else seed)
    rows, cols = shape
    rng = np.random.default_rng(1000 * rows + cols)
    dem, flag, cell = case["dem"], np.float32(case["flag"]), float(case["cell_size"])
    valid = dem != flag
    header = dict(nrows=rows, ncols=cols, xllcorner=GEO[0], yllcorner=GEO[1], cellsize=cell)
    lat, lon = rad.latlon_maps(header, dem=dem, flag=flag)
    slope = (np.round(rng.uniform(0, 40, shape) * 4) / 4).astype(np.float32)
    slope[rng.random(shape) < 0.15] = 0.0
    aspect = np.round(rng.uniform(0, 360, shape)).astype(np.float32)
    static = {k: np.where(valid, v, flag).astype(np.float32) for k, v in dict(lat=lat, lon=lon, slope=slope, aspect=aspect).items()}
    units = cc.load_pin()["unit_list"]
    crop_units = [units[k % len(units)] for k in range(len(case["unit_list"]))]          # one crop entry per land unit of the sink case
    # stations: a dozen around the raster, values chosen so that the hours melt snow, evaporate and rain
    ns = 12
    w, h = cols * cell, rows * cell
    sx = GEO[0] + rng.uniform(-0.5 * w - 40, 1.5 * w + 40, ns)
    sy = GEO[1] + rng.uniform(-0.5 * h - 40, 1.5 * h + 40, ns)
    area = np.float32((sx.max() - sx.min()) * (sy.max() - sy.min()))
    q = lambda v, step: (np.round(np.asarray(v) / step) * step).astype(np.float32)
    stations = []
    for k in range(len(HOURS)):
        air = q(rng.uniform(6.0, 14.0, ns) + 2 * k, 1 / 16)
        stations.append(dict(airT=(sx, sy, air, area), prec=(sx, sy, q(rng.uniform(0.0, 3.0, ns), 1 / 8), area),
                             relHum=(sx, sy, q(rng.uniform(35.0, 95.0, ns), 1), area), dewT=(sx, sy, q(air - rng.uniform(0.5, 12.0, ns), 1 / 16), area),
                             windInt=(sx, sy, q(rng.uniform(0.0, 6.0, ns), 1 / 4), area),
                             transmissivity=(sx, sy, q(rng.uniform(0.3, 0.72, ns), 1 / 64), area)))
    # the snow the first hour melts: SWE on two thirds of the cells
    swe = np.where(rng.random(shape) < 0.66, q(rng.uniform(2.0, 40.0, shape), 1 / 4), np.float32(0)).astype(np.float32)
    swe[~valid] = flag
    case.update(static, header=header, crop_units=crop_units, stations=stations, swe=swe, shape=shape)
    return case


def build_model(sf, case):
    m = sc.node_model(case)
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1)
    sc.set_state(sf, case, m)
    return m


def initialize_blocks(sf, case, with_snow=True):
    """meteo, radiation, (snow,) crop, root and sink blocks on the case's raster; the crop block starts from the case's first degree-day map"""
    dem, flag = case["dem"], float(case["flag"])
    cell = float(case["cell_size"])
    meteo.initialize(sf, dem, GEO[0], GEO[1], cell, [None], flag)
    rad.initialize(sf, dem, GEO[0], GEO[1], cell, case["lat"], case["lon"], case["slope"], case["aspect"], flag=flag)
    if with_snow:
        snow.initialize(sf, dem, flag)
        snow.set_state(sf, "swe", case["swe"])
        snow.reset(sf)
    crop.initialize(sf, dem, case["crop_index"], case["crop_units"], 44.5, flag)
    crop.set_degree_days(sf, case["sink_degree_days"][0], 120)
    rc.initialize(sf, case, dem, case["crop_index"], case["soil_index"])
    sc.initialize(sf, case)


SETTINGS = dict(proxies=[dict(active=1, isHeight=1, slope=-0.006)])


def _interpolate(sf, st, name, download):
    x, y, v, area = st[name]
    return meteo.interpolate(sf, name, METHOD, x, y, v, area, SETTINGS, download=download)


def hour_host_fed(sf, case, k, with_snow, dew_point):
    """hour k with every stage's maps downloaded and handed to the next stage through the host-pointer entry points"""
    st = case["stations"][k]
    air = _interpolate(sf, st, "airT", True)
    prec = _interpolate(sf, st, "prec", True)
    if dew_point:
        dew = _interpolate(sf, st, "dewT", True)
        rh = hour.restate_relative_humidity(air, dew, float(case["flag"]))
    else:
        rh = _interpolate(sf, st, "relHum", True)
    wind = _interpolate(sf, st, "windInt", True)
    trans = _interpolate(sf, st, "transmissivity", True)
    rad.compute_hour(sf, HOURS[k], trans)
    glob, beam = rad.get_map(sf, "global"), rad.get_map(sf, "beam")
    met = dict(airT=air, prec=prec, relHum=rh, windInt=wind, globalRad=glob, beamRad=beam, transmissivity=trans, clearSkyTransmissivity=0.75)
    if with_snow:
        snow.compute_hour(sf, met)
        liquid = snow.get_output(sf, "liquid")
    else:
        liquid = prec
    crop.compute_hour(sf, met, 0.75)
    et0, lai, dd = crop.get_et0(sf), crop.get_state(sf, "lai"), crop.get_state(sf, "degreeDays")
    root.compute(sf, dd)
    sinks.compute_hour(sf, et0, lai, dd, liquid)


def hour_in_place(sf, case, k, with_snow, dew_point):
    """hour k through include/sf3d_hour.h: nothing is handed over"""
    st = case["stations"][k]
    _interpolate(sf, st, "airT", False)
    _interpolate(sf, st, "prec", False)
    if dew_point:
        _interpolate(sf, st, "dewT", False)
        hour.relative_humidity(sf, download=False)
    else:
        _interpolate(sf, st, "relHum", False)
    _interpolate(sf, st, "windInt", False)
    _interpolate(sf, st, "transmissivity", False)
    rad.compute_hour(sf, HOURS[k], None)
    if with_snow:
        hour.snow_hour(sf, None, 0.75)
        crop.compute_hour(sf, None, 0.75)
    else:
        hour.et0_hour(sf, 0.75)
    root.compute(sf, None)
    hour.sink_hour(sf)


def all_maps(sf, case, m, with_snow):
    """every map the hour leaves, by name"""
    res = {}
    if with_snow:
        res.update(snow.all_maps(sf))
    res.update(crop.all_maps(sf))
    res.update({"root_" + n: v for n, v in root.all_maps(sf).items()})
    res["root_keys"] = root.get_keys(sf)
    e, t = sinks.get_actual(sf)
    res.update(sinks=sinks.get_node_sinks(sf, m.n), evaporation=e, transpiration=t)
    return res


def clean_blocks(sf):
    for mod in (hour, sinks, root, crop, snow, rad, meteo):
        mod.clean(sf)


def totals_restated(case, liquid, evaporation, transpiration, mine=None):
    """(sequential totals, sum of |term| per total) on downloaded maps"""
    area = float(case["cell_size"]) ** 2
    terms = hour.total_terms(case["columns"][0], case["dem"], float(case["flag"]), area, liquid, evaporation, transpiration, mine)
    seq = hour.restate_totals(case["columns"][0], case["dem"], float(case["flag"]), area, liquid, evaporation, transpiration, mine)
    return seq, np.abs(terms).sum(axis=1)


# ---- what the single rank and the ranks of scripts/multirank_hour_worker.py both run

def pond_tables(case):
    """per land unit of the case: maximum pond [m], LAImax and isCrop, from the crop table the crop block holds"""
    nu = len(case["crop_units"])
    return (np.array([0.002 + 0.003 * (u % 4) for u in range(nu)]), np.array([max(float(c["LAImax"]), 0.5) for c in case["crop_units"]]),
            np.array([int(c["isCrop"]) for c in case["crop_units"]], np.int32))


def chain(sf, case, m):
    """hour 0 in place with snow and the humidity from the dew point, its totals, then the day's ponds: every map by name, "humidity",
    "totals", "liquid_read", and the ponds of the surface nodes before and after update_ponds with the pond map"""
    initialize_blocks(sf, case, with_snow=True)
    hour_in_place(sf, case, 0, True, True)
    res = all_maps(sf, case, m, True)
    res["humidity"] = meteo.get_map(sf, "relHum")
    res["totals"] = hour.totals(sf)
    mp, lm, ic = pond_tables(case)
    hour.set_ponds(sf, case["slope"], case["crop_index"], mp, lm, ic, True, float(case["flag"]))
    res["pond_before"] = np.array([sf.lib.sf3d_get_node_pond(i) for i in range(m.ns)])
    res["pond_map"] = hour.update_ponds(sf)
    res["pond_after"] = np.array([sf.lib.sf3d_get_node_pond(i) for i in range(m.ns)])
    return res


# ---- run_hour

def hour_stations(case, k):
    """the stations of hour k as hour.run_hour takes them: the meteo variables with the case's settings, and six radiation stations with a
    measured global irradiance over a window of three hours"""
    from criteria3d_amd import transmissivity as tr
    st = {name: tuple(v) + (SETTINGS,) for name, v in case["stations"][k].items() if name != "transmissivity"}
    x, y = case["stations"][k]["airT"][0][:6], case["stations"][k]["airT"][1][:6]
    rng = np.random.default_rng(77 + k)
    points = tr.station_points(x, y, np.full(6, -9999.0), None, case["dem"], dict(case["header"]), float(case["flag"]))
    points[:, 2] = np.where(np.abs(points[:, 2] + 9999.0) < 1e-5, 150.0, points[:, 2])      # a station outside the DEM: a height of its own
    measured = (np.round(rng.uniform(150.0, 600.0, (6, 3)))).astype(np.float32)
    st["transmissivity"] = dict(width=3, time_step_second=3600, points=points, measured=measured, area=case["stations"][k]["airT"][3], settings=SETTINGS)
    return st


def run_hour_host_fed(sf, case, m, k, with_snow, dew_point):
    """hour k of hour.run_hour through the host-pointer entry points: every stage's maps downloaded and handed on; the balance from
    restate_totals on the downloaded maps"""
    from criteria3d_amd import transmissivity as tr
    st = hour_stations(case, k)
    one = lambda name: meteo.interpolate(sf, name, METHOD, *st[name][:4], st[name][4], download=True)
    air, prec = one("airT"), one("prec")
    rh = hour.restate_relative_humidity(air, one("dewT"), float(case["flag"])) if dew_point else one("relHum")
    wind = one("windInt")
    t = st["transmissivity"]
    values, _ = tr.points(sf, HOURS[k], t["width"], t["time_step_second"], t["points"], t["measured"])
    has = np.abs(values.astype(np.float64) + 9999.0) >= 1e-5
    trans = meteo.interpolate(sf, "transmissivity", METHOD, t["points"][has, 0], t["points"][has, 1], values[has], t["area"], t["settings"], download=True)
    rad.compute_hour(sf, HOURS[k], trans)
    met = dict(airT=air, prec=prec, relHum=rh, windInt=wind, globalRad=rad.get_map(sf, "global"), beamRad=rad.get_map(sf, "beam"), transmissivity=trans,
               clearSkyTransmissivity=0.75)
    if with_snow:
        snow.compute_hour(sf, met)
        liquid = snow.get_output(sf, "liquid")
    else:
        liquid = prec
    crop.compute_hour(sf, met, 0.75)
    et0, lai, dd = crop.get_et0(sf), crop.get_state(sf, "lai"), crop.get_state(sf, "degreeDays")
    root.compute(sf, dd)
    sinks.compute_hour(sf, et0, lai, dd, liquid)
    sinks.apply(sf)
    e, tr_ = sinks.get_actual(sf)
    seq, _ = totals_restated(case, liquid, e, tr_)
    return hour.run_water_fluxes(sf, seq)
