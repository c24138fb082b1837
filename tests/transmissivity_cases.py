"""Inputs of the station transmissivity tests: the cases of the compiled-reference pin (tests/golden/transmissivity.npz), the host build of
the kernel's text (tests/transmissivity_host.cpp) with its input and output formats, and small seeded station sets off the pin with the
restatement of criteria3d_amd/transmissivity.py as their reference (tests/test_transmissivity_host.py holds it against the pin bit for
bit).

Off the pin: nPoints x width of 1 x 1, 3 x 3, 5 x 13, 65 x 23 and 300 x 23 (less than a wave, a partial block, a partial last block) on
the pin's scaled window; the stations are seeded over the raster stretched by a fifth on every side, every third with z = NODATA, the
series walk through the kinds of the pin, and the times and settings are chosen so that the runs together reach every arm of the pin."""
import functools
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import radiation as rad, transmissivity as tr

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NODATA = np.float32(-9999.0)
POINTS, WINDOW = 0, 1
SETTING_INTS = ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")
MONTHLY = (2.1, 2.2, 8.0, 2.9, 3.2, 3.4, 3.5, 3.3, 2.9, 2.6, 2.3, 2.2)


@functools.lru_cache(maxsize=1)
def load_pin():
    d = np.load(GOLDEN / "transmissivity.npz")
    pin = {k: d[k] for k in d.files}
    pin["cases"] = json.loads(str(pin["cases"]))
    pin["rasters"] = json.loads(str(pin["rasters"]))
    return pin


def raster_of(pin, r):
    """(dem, flag, geo) of raster r"""
    return pin[f"dem{r}"], float(pin["flag"]), tuple(pin["rasters"][r]["geo"])


def host_input(dem, flag, geo, calls) -> list:
    """the input of tests/transmissivity_host.cpp, part by part; calls: [(settings, when, mode, width, step, stations [n, 5], measured
    [n, width] or None)]"""
    parts = [np.array(dem.shape, np.int32), np.array([flag], np.float32), np.array(geo, np.float64), np.asarray(dem, np.float32), np.array([len(calls)], np.int32)]
    for settings, when, mode, width, step, stations, measured in calls:
        full = rad.settings_dict(settings)
        parts += [np.array([full[k] for k in SETTING_INTS], np.int32),
                  np.array([full["linke"], *full["linkeMonthly"], full["albedo"], full["tilt"], full["aspect"], full["clearSky"]], np.float32),
                  np.array([*when, mode, width, step, len(stations)], np.int32), np.asarray(stations, np.float64)]
        if mode == POINTS:
            parts.append(np.asarray(measured, np.float32))
    return parts


def write_host_input(path, dem, flag, geo, calls):
    """for scripts/transmissivity_timing.py, which runs the program itself (with a repeat count)"""
    from tests.raster_helpers import write_parts
    write_parts(path, host_input(dem, flag, geo, calls))


def run_host(exe, tmp_path, dem, flag, geo, calls, tag="x"):
    """[dict(status, result, written, elev, glob)] per call"""
    from tests.raster_helpers import Reader, run_host_program
    r, out = Reader(run_host_program(exe, tmp_path, tag, host_input(dem, flag, geo, calls))), []
    for _, _, mode, width, _, stations, _ in calls:
        n = len(stations)
        slots = tr.WINDOW_SLOTS if mode == WINDOW else width
        out.append(dict(status=r.take(np.int32, n), result=r.take(np.float32 if mode == POINTS else np.int32, n), written=r.take(np.uint8, n, slots),
                        elev=r.take(np.float32, n, slots), glob=r.take(np.float64, n, slots)))
    assert r.done()
    return out


def pin_calls(pin, r):
    """the pin's cases on raster r as host calls, with their indices"""
    idx = [k for k, c in enumerate(pin["cases"]) if c["raster"] == r]
    return idx, [(pin["cases"][k]["settings"], pin["cases"][k]["when"], pin["cases"][k]["mode"], pin["cases"][k]["width"], pin["cases"][k]["step"],
                  pin[f"stations{k}"], pin.get(f"measured{k}")) for k in idx]


# ------------------------------------------------------------------------------------------------ off the pin

SHAPES = ((1, 1), (3, 3), (5, 13), (65, 23), (300, 23))          # nPoints x width
KINDS = ("all there", "centre NODATA", "just enough", "one too few", "backward NODATA", "forward NODATA", "above clear sky", "all zeros", "seeded gaps")
# per shape: (settings, when, step) - the hours and settings that, with the window calls below, reach every arm of the pin
SMALL = {
    (1, 1): (dict(), (2021, 3, 20, 11, 30, 0), 3600),
    (3, 3): (dict(timeZone=-12), (1950, 1, 1, 11, 0, 0), 3600),                    # the centre's local year is 1949: NODATA is added
    (5, 13): (dict(timeZone=-12), (1950, 1, 1, 13, 0, 0), 3600),                   # backward slots in 1949: the stale value
    (65, 23): (dict(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY, isUTC=0), (2021, 3, 20, 9, 0, 0), 1800),
    (300, 23): (dict(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), (2021, 3, 20, 6, 30, 0), 3600),
}
# (settings, when, step, stations of the (65, 23) set): noon ends at 1, the morning in between, midnight at 23, and the refused centre of 2101
SMALL_WINDOWS = ((dict(), (2021, 3, 20, 11, 0, 0), 3600, 9), (dict(), (2021, 3, 20, 5, 30, 0), 1800, 9), (dict(), (2021, 12, 21, 23, 30, 0), 1800, 5),
                 (dict(), (2100, 12, 31, 23, 30, 0), 3600, 5))


def small_series(kind, width, rng):
    centre = (width - 1) // 2
    m = np.round(rng.uniform(0.05, 1.0, width) * 600.0).astype(np.float32)
    enough = int(np.ceil(0.66 * width))
    others = np.array([i for i in range(width) if i != centre], np.int64)
    if kind == "centre NODATA":
        m[centre] = NODATA
    elif kind in ("just enough", "one too few"):
        m[rng.permutation(others)[:width - (enough if kind == "just enough" else enough - 1)]] = NODATA
    elif kind == "backward NODATA":
        m[:centre][::2] = NODATA
    elif kind == "forward NODATA":
        m[centre + 1:][::2] = NODATA
    elif kind == "above clear sky":
        m[:] = 3000.0
    elif kind == "all zeros":
        m[:] = 0.0
    elif kind == "seeded gaps":
        m[rng.permutation(others)[:max(0, (width - enough) // 2)]] = NODATA
    return m


@functools.lru_cache(maxsize=None)
def small_set(shape, seed=20261019):
    """(stations [n, 5], measured [n, width]) of a shape, on raster 1 of the pin"""
    pin = load_pin()
    dem, flag, geo = raster_of(pin, 1)
    n, width = shape
    rng = np.random.default_rng(seed + 1000 * n + width)
    rows, cols = dem.shape
    x = geo[0] + geo[2] * cols * rng.uniform(-0.2, 1.2, n)
    y = geo[1] + geo[2] * rows * rng.uniform(-0.2, 1.2, n)
    z = np.where(np.arange(n) % 3 == 0, float(NODATA), 130.0 + rng.uniform(-10, 80, n))
    if n >= 5:                                        # the pin's hollow and a station above every cell are among them
        x[1], y[1], z[1] = pin["xyz0"][5]
        x[2], y[2], z[2] = pin["xyz0"][4]
    r = pin["rasters"][1]
    st = tr.station_points(x, y, z, dict(utmZone=r["utmZone"], startLatitude=r["startLatitude"]), dem, dict(xllcorner=geo[0], yllcorner=geo[1], cellsize=geo[2]), flag)
    measured = np.stack([small_series(KINDS[k % len(KINDS)] if n > 1 else "all there", width, rng) for k in range(n)])
    return st, measured


@functools.lru_cache(maxsize=1)
def small_reference():
    """{shape: (transmissivity, nValid, arms, evaluations)} and [(steps per station, arms)] of SMALL_WINDOWS: computed once, shared"""
    pin = load_pin()
    dem, flag, geo = raster_of(pin, 1)
    grid = tr.grid_of(dem, flag, *geo)
    ref = {}
    for shape in SHAPES:
        st, measured = small_set(shape)
        settings, when, step = SMALL[shape]
        got, n_valid, arms, _, evals = tr.restate_points(grid, settings, when, shape[1], step, st, measured)
        ref[shape] = (got, n_valid, arms, evals)
    st = small_set((65, 23))[0]
    windows = []
    for settings, when, step, count in SMALL_WINDOWS:
        res = [tr.restate_window(grid, settings, when, p, step) for p in st[:count]]
        windows.append(([v[0] for v in res], [v[1] for v in res]))
    return ref, windows
