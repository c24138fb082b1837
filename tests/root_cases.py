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


# ---- the host build of the kernels' text behind the table builder of sf3d_root_initialize (tests/root_host.cpp)

SHAPES = ((7, 37), (3, 11), (1, 300))          # 259 cells: one block and three lanes; 33: less than a wave; 300: a partial second block
SEEDS = (31, 32, 33, 34)                        # of the random rasters, per shape; the device runs the first two
TABLES = ("flag", "unit_list", "soil_list", "layer_depth", "layer_thickness")
ROOTED_SHARE = 0.25                             # the least share of the cells that hold a root length > 0 and a key: a cell needs a DEM value, a
                                                # unit, a soil and degree days (about 0.96 x 0.89 x 0.83 x 0.97), and grows roots above 0 degree days


def case_of(pin, dem, crop_index, soil_index, degree_days, **tables):
    """the tables of the pin (or those given) with a raster and a list of degree-day maps"""
    c = {k: pin[k] for k in TABLES}
    c.update(tables)
    c.update(dem=dem, crop_index=crop_index, soil_index=soil_index, degree_days=list(degree_days))
    return c


def random_case(pin, shape, seed, continuous=True):
    """small_raster with a second degree-day map; continuous: both maps drawn from -20 to 3000 without rounding, 4 % at the flag"""
    dem, ci, si, dd = small_raster(pin, shape, seed)
    rng = np.random.default_rng(seed + 9000)
    flag = np.float32(pin["flag"])
    if continuous:
        maps = [rng.uniform(-20.0, 3000.0, shape).astype(np.float32) for _ in range(2)]
        for m in maps:
            m[rng.random(shape) < 0.04] = flag
        maps[0].flat[-1] = np.float32(700.0)
    else:
        maps = [dd, (dd * np.float32(0.5)).astype(np.float32)]
        maps[1][dd == flag] = flag
    return case_of(pin, dem, ci, si, maps)


def restated_case(case, k):
    return root.restate_root_maps(case["dem"], case["crop_index"], case["soil_index"], case["unit_list"], case["soil_list"], case["layer_depth"],
                                  case["layer_thickness"], case["degree_days"][k], float(case["flag"]))


def edge_cases(pin):
    """(name, case) of valid inputs at the edges of the tables.
    caps: CROP_MAX_UNITS land units with cells on the last one; a last soil of ROOT_MAX_HORIZONS horizons and 0.995 m (nrAtoms = 100 =
          round(totalDepth / 0.01)), the deepest soil of its raster, so a unit rooting from the surface (top = 0) to the soil's depth asks for
          m = lunetteMax rooted atoms, the last row of its pair; the units are put in an order that makes that pair the table's last, so its key is
          the last table row.  A unit rooting from 0 gives firstRootLayer = 0.
    clamp: rootDepthMin 0.3 m and 0.05 m on the soils of 0.29 m and 0.04 m: top + n > nrAtoms clamps m, and to m <= 0 where top >= nrAtoms.
    deep: the static 3 m root system on the 1.5 m soil under a layer grid that ends at 0.95 m: lastRootLayer = nrLayers - 1.
    one-layer: nrLayers = 1.   1x8: one row of eight cells."""
    flag = np.float32(pin["flag"])
    rng = np.random.default_rng(640)
    shape = (3, 11)
    dem, ci, si, dd = small_raster(pin, shape, 35)
    units = [dict(pin["unit_list"][k % len(pin["unit_list"])]) for k in range(root.MAX_UNITS)]
    units[root.MAX_UNITS - 1] = dict(pin["unit_list"][1], rootDepthMax=2.0)                       # cylinder, linear, rootDepthMin 0
    hz = np.linspace(0.0, 0.995, root.MAX_HORIZONS + 1)
    last_soil = dict(totalDepth=0.995, upperDepth=[float(v) for v in hz[:-1]], lowerDepth=[float(v) for v in hz[1:]],
                     soilFraction=[1.0 - 0.02 * h for h in range(root.MAX_HORIZONS)])
    soils = [pin["soil_list"][k] for k in (2, 3, 4)] + [last_soil]                             # 0.6 m, 0.29 m, 0.04 m, 0.995 m
    ci = rng.integers(-1, root.MAX_UNITS, shape).astype(np.int32)
    si = rng.integers(-1, len(soils), shape).astype(np.int32)
    ci.flat[5:9], si.flat[5:9] = root.MAX_UNITS - 1, len(soils) - 1
    maps = [np.full(shape, np.float32(2500.0)), dd]
    maps[0].flat[6], maps[0].flat[7] = np.float32(300.0), np.float32(1.0)
    yield "caps", case_of(pin, dem, ci, si, maps, unit_list=units, soil_list=soils)

    dem, ci, si, dd = small_raster(pin, shape, 36)
    units = [dict(pin["unit_list"][2], rootDepthMin=0.3, rootDepthMax=0.5), dict(pin["unit_list"][0]), dict(pin["unit_list"][3])]
    ci = rng.integers(0, len(units), shape).astype(np.int32)
    si = rng.integers(3, 5, shape).astype(np.int32)                                             # the soils of 0.29 m and 0.04 m
    yield "clamp", case_of(pin, dem, ci, si, [dd, np.full(shape, np.float32(900.0))], unit_list=units)

    dem, ci, si, dd = small_raster(pin, shape, 37)
    ci.flat[5:9], si.flat[5:9] = 7, 0
    yield "deep", case_of(pin, dem, ci, si, [dd, np.full(shape, np.float32(900.0))])

    dem, ci, si, dd = small_raster(pin, shape, 38)
    yield "one-layer", case_of(pin, dem, ci, si, [dd], layer_depth=pin["layer_depth"][:1], layer_thickness=pin["layer_thickness"][:1])

    dem, ci, si, dd = small_raster(pin, (1, 8), 39)
    yield "1x8", case_of(pin, dem, ci, si, [dd, np.full((1, 8), np.float32(900.0))])


def accepted(sf, case):
    """sf3d_root_initialize takes the case: its validation passes (without a device the call then fails on the device, with another code)"""
    from criteria3d_amd import capi
    root.bind(sf)
    dem = np.ascontiguousarray(case["dem"], np.float32)
    ci, si = np.ascontiguousarray(case["crop_index"], np.int32), np.ascontiguousarray(case["soil_index"], np.int32)
    ld, lt = np.ascontiguousarray(case["layer_depth"], np.float64), np.ascontiguousarray(case["layer_thickness"], np.float64)
    code = sf.lib.sf3d_root_initialize(dem.shape[0], dem.shape[1], dem.ctypes.data_as(root.pf32), float(case["flag"]), len(ld), ld.ctypes.data_as(root.pf64),
                                       lt.ctypes.data_as(root.pf64), ci.ctypes.data_as(root.pi32), si.ctypes.data_as(root.pi32), len(case["unit_list"]),
                                       root.unit_array(case["unit_list"]), len(case["soil_list"]), root.soil_array(case["soil_list"]))
    sf.lib.sf3d_root_clean()
    return code not in (capi.PARAMETER_ERROR, capi.INDEX_ERROR)


def run_host(exe, directory, name, case, layer0=0):
    """the host program on a case -> dict(status, rows, table [layer][row], row_layers [row][2], maps: per degree-day map length, depth, first,
    last, key and density of the layers layer0 .. nrLayers - 1)"""
    import ctypes
    from tests.raster_helpers import Reader, run_host_program
    dem = np.asarray(case["dem"], np.float32)
    n, nl, units, soils = dem.size, len(case["layer_depth"]), case["unit_list"], case["soil_list"]
    parts = [np.array([n, nl, len(units), len(soils), len(case["degree_days"])], np.int32), np.array([case["flag"]], np.float32), dem,
             np.asarray(case["crop_index"], np.int32), np.asarray(case["soil_index"], np.int32), np.asarray(case["layer_depth"], np.float64),
             np.asarray(case["layer_thickness"], np.float64), bytes(root.unit_array(units))[:len(units) * ctypes.sizeof(root.Unit)],
             bytes(root.soil_array(soils))[:len(soils) * ctypes.sizeof(root.Soil)]]
    for dd in case["degree_days"]:
        parts += [np.array([layer0, nl - layer0], np.int32), np.asarray(dd, np.float32)]
    r = Reader(run_host_program(exe, directory, name, parts))
    status, rows = (int(v) for v in r.take(np.int32, 2))
    out = dict(status=status, rows=rows, maps=[])
    if status == 0:
        out["table"], out["row_layers"] = r.take(np.float64, nl, rows), r.take(np.int32, rows, 2)
        for _ in case["degree_days"]:
            out["maps"].append(dict(length=r.take(np.float64, *dem.shape), depth=r.take(np.float64, *dem.shape), first=r.take(np.int32, *dem.shape),
                                    last=r.take(np.int32, *dem.shape), key=r.take(np.int32, *dem.shape), density=r.take(np.float64, nl - layer0, *dem.shape)))
    assert r.done()
    return out
