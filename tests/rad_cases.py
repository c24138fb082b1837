"""Inputs of the radiation tests: the cases of the compiled-reference pin (tests/golden/rad_rsun.npz) and small seeded rasters off the
pin, with the restatement of criteria3d_amd/radiation.py as their reference (tests/test_rad_host.py holds it against the pin bit for bit).

Small rasters: 7 x 37 (a partial second block of 256 threads), 3 x 11 (less than a wave), 1 x 300 (a partial second block in one row), 4 m
cells at the pin's place, relief of tens of metres over a few cells (steep enough for shadows at any sun below 60 degrees), a hole of
flag cells in the middle (on the ray paths of its neighbours), slopes from flat to 70 degrees with flat cells (slope == 0) and one cell
whose slope is NODATA.  The hours put the sun low in the east and low in the west, in all four quadrants (so rays leave by each of
the four edges), at noon and below the horizon; the settings walk through the arms the pin reaches."""
import functools
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import radiation as rad

GOLDEN = Path(__file__).resolve().parent / "golden"
FLAG = np.float32(-9999.0)
SHAPES = ((7, 37), (3, 11), (1, 300))
GEO = (683768.0, 4928230.0, 4.0)          # lower left corner [m, UTM 32] and cell size of the pin's window
MONTHLY = (2.1, 2.2, 8.0, 2.9, 3.2, 3.4, 3.5, 3.3, 2.9, 2.6, 2.3, 2.2)


@functools.lru_cache(maxsize=1)
def load_pin():
    d = np.load(GOLDEN / "rad_rsun.npz")
    pin = {k: d[k] for k in d.files}
    pin["cases"] = json.loads(str(pin["cases"]))
    r, c = pin["nodata_slope_cell"]
    slope = pin["slope_reference"].copy()
    slope[:, r, c] = -9999.0             # the hand-made NODATA slope of make_rad_rsun.py
    pin["slope"] = slope
    return pin


@functools.lru_cache(maxsize=1)
def load_places_pin():
    """tests/golden/rad_rsun_places.npz in the shape of load_pin(): one DEM for the six rasters, geo and gis settings per raster"""
    d = np.load(GOLDEN / "rad_rsun_places.npz")
    pin = {k: d[k] for k in d.files}
    for k in ("cases", "places", "edits", "notes"):
        pin[k] = json.loads(str(pin[k]))
    pin["dem"] = np.broadcast_to(pin["dem"], (len(pin["places"]),) + pin["dem"].shape)
    return pin


def pin_geo(pin, raster):
    """(xll, yll, cell size) of a raster of either pin"""
    return tuple(pin["geo"][raster]) if pin["geo"].ndim == 2 else tuple(pin["geo"])


def pin_chains(pin):
    """the pin's cases as chains of hours that share their maps: [(raster, [case, ...]), ...]"""
    chains = []
    for case in pin["cases"]:
        if case["keep"]:
            chains[-1][1].append(case)
        else:
            chains.append((case["raster"], [case]))
    return chains


def pin_maps(pin, case):
    return pin[f"maps{case['raster']}"][case["index"]]


# the small rasters' places off the pin's: name -> (latitude of the lower edge, longitude of the left edge, cell size [m], time zone).  Their
# latitude and longitude maps are given directly (a degree of latitude is 111 km), not through UTM
PLACES = {"80 N": (80.0, -179.9, 10.0, -12), "80 S": (-80.0, 179.9, 2.5, 12), "equator": (0.0, 179.9, 10.0, 12), "pole row": (80.0, -179.9, 2.5, -12)}
# "pole row": row 0 stands at latitude 90 (left half) and -90 (right half); in row 1, from column 1: three cells S_solpos refuses
# (latitude 90.5, longitude 180.5, aspect 361) and two at latitude 89.9 whose longitudes put the cosine of the azimuth beyond 1 and
# below -1 at 2021-03-20 11:30 UTC (found by search, as tests/golden/make_rad_rsun.py finds those of the pin)
CA_CELLS = ((89.9, 9.275), (89.9, -171.03))


@functools.lru_cache(maxsize=None)
def small_raster(shape, place=None, seed=20261018):
    """place None: the pin's corner (GEO); a name of PLACES otherwise"""
    rows, cols = shape
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    r, c = np.mgrid[0:rows, 0:cols]
    dem = (120 + 35 * np.sin(c / 2.3) * np.cos(r / 1.7) + 12 * np.sin(c / 9.0) + rng.uniform(-4, 4, shape)).astype(np.float32)
    dem = np.round(dem * 8) / 8
    hole = (slice(rows // 2, rows // 2 + 1), slice(cols // 2 - 1, cols // 2 + 2))
    dem[hole] = FLAG
    dem = dem.astype(np.float32)
    valid = dem != FLAG
    slope = np.round(rng.uniform(0, 70, shape) * 4) / 4
    slope[rng.uniform(size=shape) < 0.12] = 0.0
    aspect = np.round(rng.uniform(0, 360, shape))
    slope.flat[3] = -9999.0                # S_solpos refuses this tilt
    if place is None:
        lat, lon = rad.latlon_maps(dict(nrows=rows, ncols=cols, xllcorner=GEO[0], yllcorner=GEO[1], cellsize=GEO[2]), dem=dem, flag=FLAG)
    else:
        lat0, lon0, cell, _ = PLACES[place]
        lat = (lat0 + (rows - 1 - r + 0.5) * cell / 111000.0).astype(np.float32)
        lon = (lon0 + (c + 0.5) * cell / (111000.0 * np.cos(np.radians(lat0)))).astype(np.float32)
        if place == "pole row":
            lat[0, :cols // 2], lat[0, cols // 2:] = 90.0, -90.0
            lat[1, 1], lon[1, 2], aspect[1, 3] = 90.5, 180.5, 361.0
            for k, (la, lo) in enumerate(CA_CELLS):
                lat[1, 4 + k], lon[1, 4 + k] = la, lo
            slope[1, 1:6] = 20.0
    trans = []
    for k in range(2):
        t = (np.round(rng.uniform(0.05, 0.9, shape) * 64) / 64).astype(np.float32)
        t.flat[5 + 4 * k::9] = -9999.0
        t[~valid] = FLAG
        trans.append(t)
    static = tuple(np.where(valid, m, FLAG).astype(np.float32) for m in (lat, lon, slope, aspect))
    geo = GEO if place is None else (GEO[0], GEO[1], PLACES[place][2])
    return dict(dem=dem, lat=static[0], lon=static[1], slope=static[2], aspect=static[3], transmissivity=trans, geo=geo)


def small_chains():
    """[(name, settings, [(when, transmissivity map), ...]), ...]: hours of one chain share their maps"""
    eq, js, ds = (2021, 3, 20), (2021, 6, 21), (2021, 12, 21)
    total = dict(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY)
    return [
        ("night, then the sun low in the east, then mid-morning", {}, [(eq + (2, 30, 0), 0), (eq + (5, 30, 0), 0), (eq + (7, 30, 0), 1)]),
        ("noon, the sun low in the west, after sunset", {}, [(eq + (11, 30, 0), 0), (eq + (17, 15, 0), 1), (eq + (18, 30, 0), 0)]),
        ("June: north-east, north-west", {}, [(js + (4, 30, 0), 0), (js + (18, 0, 0), 1)]),
        ("December: south-east, south-west", {}, [(ds + (8, 30, 0), 0), (ds + (14, 30, 0), 1)]),
        ("total transmissivity, real sky", total, [(eq + (8, 30, 0), 0)]),
        ("total transmissivity, clear sky", dict(total, realSky=0), [(eq + (8, 30, 0), 0)]),
        ("Linke, clear sky", dict(realSky=0), [(eq + (15, 30, 0), 0)]),
        ("no shadowing", dict(shadowing=0), [(eq + (7, 30, 0), 0)]),
        ("fixed tilt", dict(tiltMode=rad.TILT_FIXED, tilt=35.0, aspect=135.0), [(eq + (9, 30, 0), 1)]),
        ("monthly Linke: the A0 patch", dict(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), [(eq + (10, 30, 0), 0)]),
        ("Linke map and albedo map", dict(linkeMode=rad.MODE_MAP, albedoMode=rad.MODE_MAP), [(eq + (12, 30, 0), 1)]),
        ("local time, time zone -12 across the date", dict(timeZone=-12, isUTC=0), [((2021, 3, 19, 18, 30, 0), 0)]),
    ]


def small_chains_places():
    """[(name, place, settings, [(when, transmissivity map), ...]), ...]: the kinds of hours of small_chains() where the sun position takes
    its other arms.  The times are UTC; the longitudes +-179.9 put the true solar noon at 00:00 UTC.  An hour S_solpos refuses leaves the maps"""
    eq, js, ds = (2021, 3, 20), (2021, 6, 21), (2021, 12, 21)
    Z = lambda place, **kw: dict(kw, timeZone=PLACES[place][3])
    n, s, e, p = "80 N", "80 S", "equator", "pole row"
    return [
        ("80 N: midnight sun, morning, noon, evening", n, Z(n), [(js + (12, 5, 0), 0), (js + (18, 30, 0), 1), (js + (23, 55, 0), 0), ((2021, 6, 22, 6, 30, 0), 1)]),
        ("80 N: polar night", n, Z(n), [(ds + (0, 30, 0), 0), (ds + (12, 30, 0), 1)]),
        ("80 N: equinox, the sun low in the east, noon, low in the west", n, Z(n), [(eq + (18, 15, 0), 0), ((2021, 3, 21, 0, 5, 0), 1), ((2021, 3, 21, 5, 45, 0), 0)]),
        ("80 N: the local date steps back over 1 March and 1 January; a refused year", n, Z(n),
         [((2024, 3, 1, 6, 30, 0), 0), ((2022, 1, 1, 0, 30, 0), 1), ((1950, 1, 1, 0, 30, 0), 0)]),
        ("80 S: polar day at noon and at midnight", s, Z(s), [(ds + (0, 30, 0), 0), (ds + (12, 5, 0), 1)]),
        ("80 S: polar night; equinox, low in the west, 00:05 local time before the true solar midnight", s, Z(s), [(js + (0, 30, 0), 0), (eq + (5, 40, 0), 1), (eq + (12, 5, 0), 0)]),
        ("80 S: local time, total transmissivity", s, Z(s, isUTC=0, realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY), [(ds + (9, 30, 0), 0)]),
        ("equator: sunrise, the zenith, sunset, night", e, Z(e), [((2022, 9, 22, 18, 5, 0), 0), ZENITH, ((2022, 9, 23, 5, 40, 0), 1), ((2022, 9, 23, 12, 5, 0), 0)]),
        ("equator: leap years and centuries", e, Z(e), [((2024, 2, 29, 2, 30, 0), 0), ((2024, 12, 30, 23, 30, 0), 1), ((2000, 2, 29, 1, 30, 0), 0),
                                                       ((2100, 3, 1, 3, 30, 0), 1), ((2100, 12, 30, 21, 30, 0), 0)]),
        ("equator: before 2000", e, Z(e), [((1999, 12, 31, 3, 30, 0), 0), ((1951, 1, 1, 2, 30, 0), 1)]),
        # a time zone far from the longitude: the sun stands above the horizon and the wrapped tstfix alone makes the cells dark
        ("80 N: equinox morning sun in time zone 1, dark only by the tstfix < -720 wrap", n, dict(timeZone=1), [(eq + (18, 30, 0), 0)]),
        ("equator: afternoon sun in time zone -1, dark only by the tstfix > 720 wrap", e, dict(timeZone=-1), [(eq + (5, 30, 0), 1)]),
        ("pole row: equinox, June, December", p, Z(p), [(eq + (11, 30, 0), 0), (js + (23, 30, 0), 1), (ds + (11, 30, 0), 0)]),
        ("pole row: fixed tilt, no shadowing", p, Z(p, tiltMode=rad.TILT_FIXED, tilt=35.0, aspect=135.0, shadowing=0), [(js + (2, 30, 0), 1)]),
    ]


ZENITH = ((2022, 9, 22, 23, 52, 55), 1)          # the second of 2022's September equinox at which the sun is within 0.057 degrees of the zenith at 0 N 179.9 E
SHAPES_PLACES = ((7, 37), (3, 11))


def restate_chain(shape, settings, hours, mine=None, place=None, sun_arms=None):
    """the restatement's maps after every hour of a chain -> [(maps, arms), ...]; an hour S_solpos refuses leaves the maps (arms None).
    sun_arms: a list that receives the union of the SUN_ARMS bits of every hour"""
    g = small_raster(shape, place)
    out, prev = [], None
    for when, tk in hours:
        bits = np.zeros(g["dem"].shape, np.int64)
        maps, arms = rad.restate_radiation_hour(g["dem"], FLAG, *g["geo"], g["lat"], g["lon"], g["slope"], g["aspect"], when,
                                                g["transmissivity"][tk], settings, previous=prev, mine=mine, sun_arms=bits)
        if maps is None:
            maps = prev.copy() if prev is not None else np.full((5,) + g["dem"].shape, FLAG, np.float32)
        out.append((maps, arms))
        prev = maps
        if sun_arms is not None:
            sun_arms.append(int(np.bitwise_or.reduce(bits, axis=None)))
    return out


@functools.lru_cache(maxsize=1)
def small_reference():
    """{(shape, chain name): [(maps, arms), ...]} for every small raster and chain: computed once, shared by the tests"""
    return {(shape, name): restate_chain(shape, settings, hours) for shape in SHAPES for name, settings, hours in small_chains()}


@functools.lru_cache(maxsize=1)
def small_reference_places():
    """({(shape, chain name): [(maps, arms), ...]}, the union of the SUN_ARMS bits) for the small rasters at the other places"""
    bits, ref = [], {}
    for shape in SHAPES_PLACES:
        for name, place, settings, hours in small_chains_places():
            ref[(shape, name)] = restate_chain(shape, settings, hours, place=place, sun_arms=bits)
    return ref, int(np.bitwise_or.reduce(bits))
