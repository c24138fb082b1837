"""What tests/test_meteo_host.py, tests/test_gpu_meteo.py and scripts/multirank_meteo_worker.py share (no tests here): the pin
tests/golden/meteo_idw.npz decoded into the station sets, the case table and the arguments the binding and the restatement take, and the
raster of 257 x 3 cells with 1 024 stations."""
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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
