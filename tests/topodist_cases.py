"""What tests/test_topodist_host.py, tests/test_gpu_topodist.py and scripts/multirank_topodist_worker.py share (no tests here): the pin
tests/golden/topodist.npz decoded into its two rasters with their stations, maps, cases, station matrices and Kh searches; the host
build of the per-cell text (tests/topodist_host.cpp); and the small and the cap rasters of tests/meteo_cases.py with station heights."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import meteo, topodist

ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "topodist.npz"
RASTERS = ("relief", "tiny")
PORT = 29799                                    # the two-rank test's (clear of tests/ranks.py's table and of test_gpu_multirank.py's ports)


def load_pin():
    z = np.load(PIN)
    p = {k: z[k] for k in z.files}
    p["modes"] = [str(m) for m in p["modes"]]
    out = dict(flag=np.float32(p["flag"]), modes=p["modes"], max_kh=int(p["max_kh"]), arms=dict(zip((str(n) for n in p["arm_names"]), (int(c) for c in p["arm_counts"]))))
    for name in RASTERS:
        g = lambda key: p[f"{name}_{key}"]
        settings = json.loads(str(g("case_settings")))
        r = dict(name=name, dem=g("dem"), xll=float(g("geo")[0]), yll=float(g("geo")[1]), cell_size=float(g("geo")[2]), x=g("x"), y=g("y"), z=g("z"), maps=g("maps"),
                 hand=int(g("hand")), hand_map=g("hand_map"), mixed=g("mixed"), matrices=g("matrices"), flag=out["flag"])
        r["cases"] = [dict(var=int(g("case_var")[k]), method=int(g("case_method")[k]), kh=int(g("case_kh")[k]), mode=p["modes"][int(g("case_mode")[k])],
                           value=g("case_values")[k], settings=settings[k], area=np.float32(g("case_area")[k]), want=g("case_maps")[k])
                      for k in range(len(settings))]
        out[name] = r
    table = json.loads(str(p["opt_table"]))
    out["opt"] = [dict(o, sub=np.array(o["sub"]), kh=int(p["opt_kh"][k]), value=p[f"opt{k}_value"], observed=p[f"opt{k}_observed"], series_kh=p[f"opt{k}_series_kh"],
                       series_error=p[f"opt{k}_series_error"]) for k, o in enumerate(table)]
    return out


def case_name(c) -> str:
    return f"{meteo.VARIABLES[c['var']]}-{meteo.METHODS[c['method']]}-kh{c['kh']}-{c['mode']}"


def mode_maps(r, mode):
    """(the maps held, the map index per station) of a mode of the pin: none, all, mixed, hand"""
    held = [r["hand_map"] if (mode == "hand" and i == r["hand"]) else r["maps"][i] for i in range(len(r["x"]))]
    n = len(held)
    if mode == "none":
        index = np.full(n, -1, np.int32)
    elif mode == "mixed":
        index = np.where(r["mixed"] != 0, np.arange(n), -1).astype(np.int32)
    else:
        index = np.arange(n, dtype=np.int32)
    return held, index


def effective_kh(c) -> int:
    """the Kh the distances see: 0 under useTopographicDistance = 0 and for a variable getUseTdVar excludes"""
    return c["kh"] if (c["settings"].get("useTopographicDistance", 0) and c["var"] in topodist.TD_VARIABLES) else 0


def restated(r, c, mine=None):
    held, index = mode_maps(r, c["mode"])
    return topodist.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], [None], c["var"], c["method"], r["x"], r["y"], r["z"], c["value"], c["area"],
                                        c["settings"], c["kh"], held, index, float(r["flag"]), mine)


def initialize(sf, r):
    meteo.initialize(sf, r["dem"], r["xll"], r["yll"], r["cell_size"], [None], float(r["flag"]))


def hold(sf, r, mode):
    """the device holds the maps of `mode`: computed, with the hand-made one set where the mode says so; returns the map index"""
    topodist.compute(sf, r["x"], r["y"], r["z"])
    if mode == "hand":
        topodist.set_map(sf, r["hand"], r["hand_map"])
    return mode_maps(r, mode)[1]


def interpolate(sf, r, c, index, download=True):
    return topodist.interpolate(sf, c["var"], c["method"], r["x"], r["y"], r["z"], c["value"], index, c["area"], c["settings"], c["kh"], download)


def run_host(exe, r, pin, directory):
    """the host program on one raster of the pin -> (maps, case maps, matrices per mode)"""
    from tests.raster_helpers import Reader, run_host_program
    n = len(r["x"])
    parts = [np.array([r["dem"].shape[0], r["dem"].shape[1], n, len(r["cases"]), len(pin["modes"]), r["hand"]], np.int32), np.array([r["flag"]], np.float32),
             np.array([r["xll"], r["yll"], r["cell_size"]], np.float64), r["dem"].astype(np.float32)]
    parts += [a.astype(np.float64) for a in (r["x"], r["y"], r["z"])] + [r["hand_map"].astype(np.float32)]
    for c in r["cases"]:
        st = c["settings"]
        parts += [np.array([c["var"], c["method"], effective_kh(c), int(c["mode"] == "hand"), st["proxies"][0]["active"], st["useDetrending"]], np.int32),
                  np.array([st["rainfallThreshold"], meteo.shepard_initial_radius(c["area"], n), st["proxies"][0]["slope"]], np.float32),
                  mode_maps(r, c["mode"])[1], c["value"].astype(np.float32)]
    for mode in pin["modes"]:
        parts += [np.array([int(mode == "hand")], np.int32), mode_maps(r, mode)[1]]
    out = Reader(run_host_program(exe, directory, r["name"], parts))
    got = out.take(np.float32, n, *r["dem"].shape), out.take(np.float32, len(r["cases"]), *r["dem"].shape), out.take(np.float32, len(pin["modes"]), n, n)
    assert out.done()
    return got


def with_heights(r, seed):
    """a raster of tests/meteo_cases.py (cap_raster, small_raster) with station heights and a mixed map index (every third station map-less)"""
    rng = np.random.default_rng(seed)
    n = len(r["x"])
    z = np.round(rng.uniform(-20.0, 330.0, n), 2)
    return dict(r, z=z, proxy_maps=[None, r["proxy_maps"][1]], index=np.where(np.arange(n) % 3 != 1, np.arange(n), -1).astype(np.int32),
                settings=dict(r["settings"], useTopographicDistance=1))
