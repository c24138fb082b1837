"""What tests/test_root_host.py, tests/test_gpu_root.py and scripts/multirank_root_worker.py share (no tests here): the pin
tests/golden/root_density.npz decoded into the tables the binding and the restatement take, and a small raster of any shape."""
from pathlib import Path

import numpy as np

from criteria3d_amd import root

PIN = Path(__file__).resolve().parent / "golden" / "root_density.npz"
OUTPUTS = ("length", "depth", "first", "last", "density")


def load_pin():
    z = np.load(PIN)
    p = {k: z[k] for k in z.files}
    names = [str(n) for n in p["unit_fields"]]
    p["unit_list"] = [dict(zip(names, row)) for row in p["units"]]
    p["soil_list"] = []
    for s, nh in enumerate(p["soil_nr_horizons"]):
        hz = p["soil_horizons"][s, :int(nh)]
        p["soil_list"].append(dict(totalDepth=float(p["soil_total_depth"][s]), upperDepth=[float(v) for v in hz[:, 0]], lowerDepth=[float(v) for v in hz[:, 1]],
                                   soilFraction=[1.0 - float(v) for v in hz[:, 2]]))                      # getSoilFraction(): 1.0 - coarseFragments
    return p


def restated(pin, k):
    """the restatement of both functions on the pin's k-th degree-day map"""
    return root.restate_root_maps(pin["dem"], pin["crop_index"], pin["soil_index"], pin["unit_list"], pin["soil_list"], pin["layer_depth"],
                                  pin["layer_thickness"], pin["degree_days"][k], float(pin["flag"]))


def initialize(sf, pin, dem=None, crop_index=None, soil_index=None):
    root.initialize(sf, pin["dem"] if dem is None else dem, pin["crop_index"] if crop_index is None else crop_index,
                    pin["soil_index"] if soil_index is None else soil_index, pin["unit_list"], pin["soil_list"], pin["layer_depth"], pin["layer_thickness"],
                    float(pin["flag"]))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def small_raster(pin, shape, seed):
    """a raster of any shape on the pin's tables: DEM with flag cells, random unit and soil indices (some missing), degree days over all phases"""
    rng = np.random.default_rng(seed)
    flag = np.float32(pin["flag"])
    dem = rng.uniform(50.0, 400.0, shape).astype(np.float32)
    dem.flat[0] = flag
    dem.flat[dem.size // 2] = flag
    ci = rng.integers(-1, len(pin["unit_list"]), shape).astype(np.int32)
    si = rng.integers(-1, len(pin["soil_list"]), shape).astype(np.int32)
    ci.flat[-1], si.flat[-1] = 3, 0                          # the last lane computes: a tree on the deepest soil
    dd = (np.round(rng.uniform(-20.0, 1500.0, shape) * 4) / 4).astype(np.float32)
    dd.flat[1] = flag
    dd.flat[-1] = np.float32(700.0)
    return dem, ci, si, dd
