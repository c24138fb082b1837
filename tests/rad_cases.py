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


def same_bits(a, b):
    """equal float32 maps: the same bits, a nan equals a nan (the sign and payload of a nan are not promised, sf3d_glibcmath.inc)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


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


@functools.lru_cache(maxsize=None)
def small_raster(shape, seed=20261018):
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
    lat, lon = rad.latlon_maps(dict(nrows=rows, ncols=cols, xllcorner=GEO[0], yllcorner=GEO[1], cellsize=GEO[2]), dem=dem, flag=FLAG)
    trans = []
    for k in range(2):
        t = (np.round(rng.uniform(0.05, 0.9, shape) * 64) / 64).astype(np.float32)
        t.flat[5 + 4 * k::9] = -9999.0
        t[~valid] = FLAG
        trans.append(t)
    static = tuple(np.where(valid, m, FLAG).astype(np.float32) for m in (lat, lon, slope, aspect))
    return dict(dem=dem, lat=static[0], lon=static[1], slope=static[2], aspect=static[3], transmissivity=trans)


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


def restate_chain(shape, settings, hours, mine=None):
    """the restatement's maps after every hour of a chain -> [(maps, arms), ...]"""
    g = small_raster(shape)
    out, prev = [], None
    for when, tk in hours:
        maps, arms = rad.restate_radiation_hour(g["dem"], FLAG, GEO[0], GEO[1], GEO[2], g["lat"], g["lon"], g["slope"], g["aspect"], when,
                                                g["transmissivity"][tk], settings, previous=prev, mine=mine)
        out.append((maps, arms))
        prev = maps
    return out


@functools.lru_cache(maxsize=1)
def small_reference():
    """{(shape, chain name): [(maps, arms), ...]} for every small raster and chain: computed once, shared by the tests"""
    return {(shape, name): restate_chain(shape, settings, hours) for shape in SHAPES for name, settings, hours in small_chains()}
