"""What tests/test_sink_host.py, tests/test_gpu_sink.py and scripts/multirank_sink_worker.py share (no tests here): the pin
tests/golden/water_sinks.npz (on the raster, units, soils and layer grid of the root pin) decoded into the tables the binding and the
restatement take, the node model the fixture's water contents belong to, and the set-up of the blocks on a loaded product."""
from pathlib import Path

import numpy as np

from criteria3d_amd import catchment as cm, root, sinks
from tests import root_cases as rc

PIN = Path(__file__).resolve().parent / "golden" / "water_sinks.npz"
OUTPUTS = ("sinks_et", "sinks", "evaporation", "transpiration")


def load_pin():
    p = rc.load_pin()
    z = np.load(PIN)
    p.update({("sink_" + k if k == "degree_days" else k): z[k] for k in z.files})
    p["sink_units"] = [dict(kcMax=float(kc), fRAW=float(fr), isWaterSurplusResistant=int(rice)) for kc, fr, rice in p["unit_extra"]]
    p["sink_soils"] = []
    for s, so in enumerate(p["soil_list"]):
        nh = len(so["upperDepth"])
        w = p["soil_water"][s, :nh]
        p["sink_soils"].append(dict(so, waterContentHH=[float(v) for v in w[:, 0]], waterContentFC=[float(v) for v in w[:, 1]],
                                    waterContentWP=[float(v) for v in w[:, 2]], waterContentSAT=[float(v) for v in w[:, 3]]))
    return p


def roots_of(pin, hour):
    k = int(pin["root_map"][hour])
    return dict(length=pin["length"][k], first=pin["first"][k], last=pin["last"][k], density=pin["density"][k])


def restated(pin, hour, arms=None, one_layer=False):
    nl = 1 if one_layer else len(pin["layer_depth"])
    r = roots_of(pin, hour)
    r["density"] = r["density"][:nl]
    return sinks.restate_sink_hour(pin["dem"], float(pin["flag"]), float(pin["cell_size"]), pin["columns"][:nl], pin["vwc"], pin["crop_index"], pin["soil_index"],
                                   pin["sink_units"], pin["sink_soils"], pin["layer_depth"][:nl], pin["layer_thickness"][:nl],
                                   0.0 if one_layer else float(pin["computation_depth"]), pin["et0"][hour], pin["lai"][hour], pin["sink_degree_days"][hour],
                                   pin["liquid_water"][hour], r, len(pin["vwc"]), arms)


def node_model(pin):
    """catchment_model(32, 24, 14) with the fixture's soil classes per node: what the fixture's water contents were read from"""
    rows, cols = pin["dem"].shape
    m = cm.catchment_model(cols, rows, len(pin["layer_depth"]))
    table = []
    for s in range(pin["soil_vg"].shape[0]):
        for h in range(int(pin["soil_nr_horizons"][s])):
            a, n, he, tr, ts, ks, L = (float(v) for v in pin["soil_vg"][s, h])
            table.append((s, h, (a, n, 1.0 - 1.0 / n, he, tr, ts, ks, L, 0.01, 0.2)))
    m.soils, m.soil_table, m.lv_ratio = [], table, 4.0
    m.soil_index = pin["node_soil"][m.ns:].astype(np.uint16)
    m.horizon_index = pin["node_horizon"][m.ns:].astype(np.uint16)
    return m


def set_state(sf, pin, m):
    """the fixture's matric potentials and its column table"""
    sf.set_matric_potential_bulk(0, pin["psi"])
    sinks.set_columns(sf, pin["columns"], pin["layer_thickness"])


def initialize(sf, pin, one_layer=False):
    nl = 1 if one_layer else len(pin["layer_depth"])
    sinks.initialize(sf, pin["dem"], float(pin["cell_size"]), pin["crop_index"], pin["soil_index"], pin["sink_units"], pin["sink_soils"], pin["layer_depth"][:nl],
                     pin["layer_thickness"][:nl], 0.0 if one_layer else float(pin["computation_depth"]), float(pin["flag"]))


def hour(sf, pin, k, null=()):
    """root compute and sink compute of hour k with every map passed in, but those named in `null`"""
    root.compute(sf, pin["sink_degree_days"][k])
    given = dict(et0=pin["et0"][k], lai=pin["lai"][k], degree_days=pin["sink_degree_days"][k], liquid_water=pin["liquid_water"][k])
    for name in null:
        given[name] = None
    sinks.compute_hour(sf, **given)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- a raster of any shape on the pin's tables

SHAPES = ((7, 37), (3, 11), (1, 300))          # 259 cells: one block and three lanes; 33: less than a wave; 300: a partial second block
TABLES = ("flag", "cell_size", "computation_depth", "unit_list", "soil_list", "sink_units", "sink_soils", "layer_depth", "layer_thickness", "soil_vg",
          "soil_nr_horizons")
ET0 = (0.0, 0.000004, 0.006, 0.05, 0.2, 0.45, 0.8, 1.2)        # [mm]: none, below EPSILON, residual < EPSILON behind the surface term, ordinary
LAI = (0.0, 0.000005, 0.3, 1.0, 2.5, 4.0, 8.0)
LIQUID = (0.0, 0.000002, 0.4, 1.2, 2.8)
# the least share of the soil nodes under computing cells that hold a sink: the restatement reaches 0.142 to 0.232 on the three shapes and
# two hours with the seeds the tests use (a quarter of the maps' values ask for no evaporation, and most roots end above the deep layers)
SINK_SHARE = 0.125
RICE, TREE = 6, 3                                # the water-surplus-resistant unit; a static root system of 2 m


def _column(case, cell, potentials=None, surface_water=None, **maps):
    """a cell placed by hand: a valid DEM cell with its whole column, the given potential in every soil node (one value or one per layer),
    and the given crop / soil index or hourly map values (a value, or one per hour)"""
    nl = len(case["layer_depth"])
    n = case["dem"].size
    case["dem"].flat[cell] = np.float32(120.0 + cell)
    case["columns"].reshape(nl, n)[:, cell] = np.arange(nl) * n + cell
    if potentials is not None:
        case["psi"][n + cell::n] = potentials
    if surface_water is not None:
        case["psi"][cell] = surface_water
    for name, v in maps.items():
        if case[name].ndim == 2:
            case[name].flat[cell] = v
        else:
            case[name].reshape(len(case[name]), n)[:, cell] = v


def small_case(pin, shape, seed, hours=2):
    """everything one hour needs on a raster of any shape, under the pin's keys and on the pin's units, soils, layer grid, cell size and
    computation depth: DEM with flag cells (the first, the middle one, a few more), crop and soil indices (some missing), `hours` sets of
    ET0 / LAI / degree-day / liquid-water maps that hold the flag, 0, values below EPSILON and ordinary ones, the column table over
    catchment_model(cols, rows, 14) with surface nodes, evaporation-layer nodes and root-range nodes missing and the whole column of the
    valid cell 2 left out, soil class and horizon per node as node_model takes them, and potentials drawn from the fixture generator's
    lists.  Cells placed by hand (cells 3 to 9, and the last cell, which evaporates and transpires) reach the arms chance does not."""
    from tests.golden.make_water_sinks import PSI, SURFACE_WATER
    rng = np.random.default_rng(seed)
    case = {k: pin[k] for k in TABLES}
    flag = np.float32(pin["flag"])
    rows, cols = shape
    n, nl = rows * cols, len(pin["layer_depth"])
    assert n >= 33, "the hand-placed cells need 33 cells"
    dem = rng.uniform(50.0, 400.0, shape).astype(np.float32)
    dem[rng.random(shape) < 0.04] = flag
    dem.flat[0] = flag
    dem.flat[n // 2] = flag
    dem.flat[2] = np.float32(77.0)
    ci = rng.integers(-1, len(pin["unit_list"]), shape).astype(np.int32)
    si = rng.integers(-1, len(pin["soil_list"]), shape).astype(np.int32)

    def drawn(values, p_flag):
        v = np.array(values, np.float32)[rng.integers(0, len(values), (hours,) + shape)]
        v[rng.random(v.shape) < p_flag] = flag
        return v
    et0, lai, liquid = drawn(ET0, 0.03), drawn(LAI, 0.05), drawn(LIQUID, 0.05)
    dd = (np.round(rng.uniform(-20.0, 1500.0, (hours,) + shape) * 4) / 4).astype(np.float32)
    dd[rng.random(dd.shape) < 0.04] = flag
    columns = np.arange(nl * n, dtype=np.int32).reshape(nl, rows, cols)       # catchment_model(cols, rows, nl).meta["index"]
    columns[0][rng.random(shape) < 0.04] = -1                                  # DEM cells without a surface node
    columns[1:][rng.random((nl - 1,) + shape) < 0.05] = -1                     # missing nodes inside the evaporation layers and the root ranges
    columns[:, dem == flag] = -1
    columns[:, 0, 0] = np.arange(nl) * n                                       # a flag cell that keeps its column: its nodes hold 0
    columns.reshape(nl, n)[:, 2] = -1                                          # a valid cell without any node
    psi = np.array(PSI)[rng.integers(0, len(PSI), nl * n)]
    psi[:n] = np.array(SURFACE_WATER)[rng.integers(0, len(SURFACE_WATER), n)]
    case.update(dem=dem, crop_index=ci, soil_index=si, et0=et0, lai=lai, sink_degree_days=dd, liquid_water=liquid, columns=columns, psi=psi)
    # ---- by hand.  A large demand over a dry surface and a profile that is dry in every other layer: the evaporation loop runs three times
    layers = np.arange(1, nl)
    _column(case, 3, potentials=np.where(layers % 2 == 1, -800.0, -0.3), surface_water=0.0, crop_index=-1, soil_index=0, et0=np.float32(1.2), lai=np.float32(0.0))
    # the first soil layer of the sand holds less than its share of a large demand, the others enough: the second iteration ends the loop
    _column(case, 4, potentials=np.where(layers == 1, -40.0, -0.3), surface_water=0.0, crop_index=-1, soil_index=1, et0=np.float32(1.2), lai=np.float32(0.0))
    # a profile at saturation: no stress for the rice unit, "water surplus" for the crop next to it
    crop_hour = dict(et0=np.float32(0.45), lai=np.float32(2.5))
    _column(case, 5, potentials=0.05, crop_index=RICE, soil_index=1, sink_degree_days=np.float32(900.0), **crop_hour)
    _column(case, 6, potentials=0.05, crop_index=0, soil_index=1, sink_degree_days=np.float32(900.0), **crop_hour)
    # the tree on the deepest soil.  Between the scarcity and the surplus threshold of its three horizons lie -12 m, -40 m and -800 m
    unstressed = np.where(layers <= 8, -12.0, np.where(layers <= 11, -40.0, -800.0))
    # ... its upper ten layers dry: the redistribution is limited by rootDensityWithoutStress, and the dry layers' flow is <= DBL_EPSILON
    _column(case, 7, potentials=np.where(layers <= 10, -800.0, unstressed), crop_index=TREE, soil_index=0, sink_degree_days=np.float32(700.0), **crop_hour)
    # ... one dry layer: limited by waterStress
    _column(case, 8, potentials=np.where(layers == 5, -800.0, unstressed), crop_index=TREE, soil_index=0, sink_degree_days=np.float32(700.0), **crop_hour)
    # the 4 cm soil: the evaporation layers below it have no horizon, and nothing roots
    _column(case, 9, potentials=-2.0, crop_index=TREE, soil_index=4, sink_degree_days=np.float32(700.0), **crop_hour)
    # the last lane computes: the tree again, unstressed, under a partly open canopy, less water on the surface than the demand, rain
    _column(case, n - 1, potentials=unstressed, surface_water=0.0001, crop_index=TREE, soil_index=0, et0=np.float32(0.45), lai=np.float32(1.0),
            sink_degree_days=np.float32(700.0), liquid_water=np.float32(1.2))
    set_node_classes(case)
    return case


def set_node_classes(case):
    """per node: soil and horizon of its cell and layer; cells without a soil take soil 0, layers below the soil horizon 0 (the fixture's
    rule).  Called again by whoever places further cells by hand (tests/map_cases.py)."""
    si = case["soil_index"]
    nl, n = len(case["layer_depth"]), si.size
    hz_of = sinks.horizon_table(case["sink_soils"], case["layer_depth"])
    node_soil = np.broadcast_to(np.where(si < 0, 0, si)[None], (nl,) + si.shape).ravel().astype(np.int32)
    layer = np.repeat(np.arange(nl), n)
    case["node_soil"], case["node_horizon"] = node_soil, np.where(hz_of[node_soil, layer] < 0, 0, hz_of[node_soil, layer]).astype(np.int32)


def roots_restated(case, k):
    """the root maps of hour k by root.restate_root_maps, as restate_sink_hour takes them"""
    r = root.restate_root_maps(case["dem"], case["crop_index"], case["soil_index"], case["unit_list"], case["soil_list"], case["layer_depth"],
                               case["layer_thickness"], case["sink_degree_days"][k], float(case["flag"]))
    return dict(length=r["length"], first=r["first"], last=r["last"], density=r["density"])


def restated_case(case, k, vwc, columns=None, arms=None):
    """the restatement of hour k of a small case on the water contents `vwc`, on the case's column table or another one"""
    return sinks.restate_sink_hour(case["dem"], float(case["flag"]), float(case["cell_size"]), case["columns"] if columns is None else columns, vwc,
                                   case["crop_index"], case["soil_index"], case["sink_units"], case["sink_soils"], case["layer_depth"], case["layer_thickness"],
                                   float(case["computation_depth"]), case["et0"][k], case["lai"][k], case["sink_degree_days"][k], case["liquid_water"][k],
                                   roots_restated(case, k), case["columns"].size, arms)


def computing_cells(case, columns=None):
    """the cells the hour computes: a DEM value and a surface node"""
    col = case["columns"] if columns is None else columns
    return (np.abs(case["dem"].astype(np.float64) - float(case["flag"])) >= 1e-5) & (col[0] >= 0)


def host_water_content(checker, case):
    """the water contents of the case's potentials from a checker library (the CPU oracle): the same node model and setter the device test uses"""
    m = node_model(case)
    checker.check(checker.lib.sf3d_reset_solver_state(), "reset")
    cm.build(checker, m, threads=1)
    checker.set_matric_potential_bulk(0, case["psi"])
    vwc = checker.water_content(0, m.n)
    checker.lib.sf3d_clean()
    return vwc


def soil_nodes_of_computing_cells(case, columns=None):
    """how many soil nodes lie in columns of computing cells"""
    col = case["columns"] if columns is None else columns
    return int(np.count_nonzero(col[1:][:, computing_cells(case, col)] >= 0))
