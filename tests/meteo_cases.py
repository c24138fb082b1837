"""What tests/test_meteo_host.py, tests/test_gpu_meteo.py and scripts/multirank_meteo_worker.py share (no tests here): the pin
tests/golden/meteo_idw.npz decoded into the station sets, the case table and the arguments the binding and the restatement take, the
raster of 257 x 3 cells with 1 024 stations, and two small rasters (3 x 11, 1 x 300 cells) under the first 300 of those stations."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import meteo

PIN = Path(__file__).resolve().parent / "golden" / "meteo_idw.npz"


def load_pin():
    z = np.load(PIN)
    p = {k: z[k] for k in z.files}
    ends = np.cumsum(p["set_sizes"])
    p["sets"] = [(p["set_x"][e - n:e], p["set_y"][e - n:e]) for n, e in zip(p["set_sizes"], ends)]
    settings = json.loads(str(p["case_settings"]))
    p["cases"] = []
    o = 0
    for k in range(len(p["case_var"])):
        s = int(p["case_set"][k])
        n = int(p["set_sizes"][s])
        x, y = p["sets"][s]
        p["cases"].append(dict(var=int(p["case_var"][k]), method=int(p["case_method"][k]), set=s, x=x, y=y, value=p["case_values"][o:o + n],
                               area=np.float32(p["case_area"][k]), settings=settings[k], want=p["maps"][k]))
        o += n
    assert o == len(p["case_values"])
    p["proxy_maps"] = [None, p["other_proxy"]]              # the height proxy reads the DEM
    return p


def case_name(c) -> str:
    return f"{meteo.VARIABLES[c['var']]}-{meteo.METHODS[c['method']]}-{len(c['x'])}st"


def restated(pin, c, mine=None):
    return meteo.restate_interpolate(pin["dem"], float(pin["xll"]), float(pin["yll"]), float(pin["cell_size"]), pin["proxy_maps"], c["var"], c["method"], c["x"], c["y"],
                                     c["value"], c["area"], c["settings"], float(pin["flag"]), mine)


def initialize(sf, pin):
    meteo.initialize(sf, pin["dem"], float(pin["xll"]), float(pin["yll"]), float(pin["cell_size"]), pin["proxy_maps"], float(pin["flag"]))


def interpolate(sf, c, download=True):
    return meteo.interpolate(sf, c["var"], c["method"], c["x"], c["y"], c["value"], c["area"], c["settings"], download)


def cap_raster(pin):
    """257 x 3 = 771 cells (three blocks and three lanes) with SF3D_METEO_MAX_STATIONS stations on a jittered lattice around it: the LDS
    staging loop runs four times per thread and the tail block computes; the height proxy with inversion and a second raster"""
    rng = np.random.default_rng(1024)
    shape = (257, 3)
    flag = np.float32(pin["flag"])
    dem = rng.uniform(-5.0, 300.0, shape).astype(np.float32)
    dem.flat[0] = flag
    dem.flat[400] = flag
    other = np.round(rng.uniform(0.0, 1.0, shape), 3).astype(np.float32)
    other.flat[-1] = flag
    xll, yll, cs = 682000.0, 4923000.0, 4.0
    gx, gy = np.meshgrid(np.arange(32), np.arange(32))
    x = np.round(xll - 400.0 + 26.0 * gx.ravel() + rng.uniform(0.0, 25.0, 1024), 3)
    y = np.round(yll - 50.0 + 36.0 * gy.ravel() + rng.uniform(0.0, 35.0, 1024), 3)
    value = np.round(rng.uniform(2.0, 28.0, 1024), 2).astype(np.float32)
    area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
    settings = dict(allZero=0, rainfallThreshold=0.2, useDetrending=1,
                    proxies=[dict(active=1, isHeight=1, inversion=1, slope=-0.0065, lapseRateH0=20.0, lapseRateH1=150.0, inversionLapseRate=0.004),
                             dict(active=1, isHeight=0, inversion=0, slope=0.6)])
    return dict(dem=dem, xll=xll, yll=yll, cell_size=cs, proxy_maps=[None, other], flag=flag, x=x, y=y, value=value, area=area, settings=settings)


SMALL_SHAPES = ((3, 11), (1, 300))             # 33 cells: less than a wave; one row of 300: a partial second block
SMALL_STATIONS = 300                           # the LDS staging loop's second pass ends at lane 44 (300 = 256 + 44)
# the small rasters' lower left corner relative to the cap raster's: inside the cloud of the 300 stations, and a position at which no cell has
# two stations at equal float distance (x and y near 682 000 and 4 923 000 are multiples of 1/16 and 1/2 as floats, so such pairs are common:
# tests/test_meteo_host.py checks that this position has none)
SMALL_OFFSET = (200.0, 100.0)
# the bounding-box area handed to the Shepard methods, as a multiple of the stations' own bounding box: the initial radius becomes
# sqrt(8 * area / (pi * 300)) = 55.5 m, and the single row of 300 cells, which runs from inside the station cloud to 970 m beyond it, holds
# cells with fewer than 5, with 5 to 10 and with more than 10 stations inside the radius (tests/test_meteo_host.py counts them)
SMALL_AREA_FACTOR = 1.25


def small_raster(pin, shape):
    """a small raster SMALL_OFFSET from the cap raster's corner with the first SMALL_STATIONS stations of its lattice, values and settings: a flag cell
    first, a computing cell last, the second proxy without a value in one cell"""
    r = cap_raster(pin)
    rng = np.random.default_rng(shape[1])
    flag = np.float32(pin["flag"])
    dem = rng.uniform(-5.0, 300.0, shape).astype(np.float32)
    dem.flat[0] = flag
    dem.flat[dem.size // 2] = flag
    other = np.round(rng.uniform(0.0, 1.0, shape), 3).astype(np.float32)
    other.flat[-2] = flag
    x, y, value = r["x"][:SMALL_STATIONS], r["y"][:SMALL_STATIONS], r["value"][:SMALL_STATIONS]
    area = np.float32(SMALL_AREA_FACTOR) * np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
    return dict(r, dem=dem, proxy_maps=[None, other], x=x, y=y, value=value, area=np.float32(area), xll=r["xll"] + SMALL_OFFSET[0],
                yll=r["yll"] + SMALL_OFFSET[1])


def float_distances(r):
    """float32 distance of every cell centre to every station, as meteo.restate_interpolate takes them: [cells, stations]"""
    cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
    xf, yf = cx.astype(np.float32).ravel(), cy.astype(np.float32).ravel()
    dx, dy = r["x"].astype(np.float32)[None, :] - xf[:, None], r["y"].astype(np.float32)[None, :] - yf[:, None]
    return np.sqrt(dx * dx + dy * dy)
