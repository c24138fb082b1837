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


# ---- the host build of the per-cell text behind the table builders of sf3d_sink_initialize / sf3d_sink_set_cracking (tests/sink_host.cpp)

SEEDS = (41, 42, 43, 44)                        # of the random cases, per shape; the device runs the first two
HAND_CELLS = tuple(range(3, 19))                # the cells small_case (3 to 9) and tests/crack_cases.py (10 to 18) place by hand; and the last one


def continuous_case(case, seed):
    """a small case (sc.small_case, kc.small_case) with the hourly maps and the potentials of every cell not placed by hand drawn from
    continuous ranges: ET0 0 to 1.5 mm, LAI 0 to 8, liquid water (with cracking: precipitation) 0 to 5 mm, degree days -20 to 3000, soil
    potentials log-uniform from -1000 to -0.01 m with 5 % ponded (0 to 0.1 m).  The flags of the maps and the missing nodes stay where
    they are (3 to 5 %)."""
    rng = np.random.default_rng(seed + 11000)
    flag = np.float32(case["flag"])
    n, nl = case["dem"].size, len(case["layer_depth"])
    hours = len(case["et0"])
    free = np.ones(n, bool)
    free[list(HAND_CELLS) + [n - 1]] = False
    free = free.reshape(case["dem"].shape)

    def redraw(name, lo, hi):
        m = case[name]
        new = rng.uniform(lo, hi, m.shape).astype(np.float32)
        keep = (m == flag) | ~free[None]
        case[name] = np.where(keep, m, new).astype(np.float32)
    redraw("et0", 0.0, 1.5)
    redraw("lai", 0.0, 8.0)
    redraw("sink_degree_days", -20.0, 3000.0)
    if "precipitation" in case:
        from tests import crack_cases as kc
        redraw("precipitation", 0.0, 5.0)
        case["liquid_water"] = np.stack([kc.liquid_water(case["precipitation"][k], case["snow_fall"][k], case["snow_melt"][k], bool(case["snow"][k]), flag)
                                         for k in range(hours)])
    else:
        redraw("liquid_water", 0.0, 5.0)
    psi = case["psi"].reshape(nl, n)
    soil = -np.exp(rng.uniform(np.log(0.01), np.log(1000.0), (nl - 1, n)))
    ponded = rng.random((nl - 1, n)) < 0.05
    soil[ponded] = rng.uniform(0.0, 0.1, int(ponded.sum()))
    psi[1:, free.ravel()] = soil[:, free.ravel()]
    return case


def read_state(lib, m, case):
    """what the kernel reads of the solver's state, through a library's getters on the built model m: H, Se, z, the soil class of every
    node and thetaS / thetaR of every class, the ponds"""
    classes = {(s, h): k for k, (s, h, _) in enumerate(m.soil_table)}
    cls = np.zeros(m.n, np.uint16)
    cls[m.ns:] = [classes[(int(s), int(h))] for s, h in zip(m.soil_index, m.horizon_index)]
    pond = np.zeros(m.n)
    if "pond" in case:
        pond[:len(case["pond"])] = case["pond"]
    return dict(H=lib.total_potential(0, m.n), Se=lib.degree_of_saturation(0, m.n), vwc=lib.water_content(0, m.n), z=np.asarray(m.z, np.float64), cls=cls,
                theta_s=np.array([a[5] for _, _, a in m.soil_table]), theta_r=np.array([a[4] for _, _, a in m.soil_table]), n=m.n, ns=m.ns, pond=pond)


def node_state(checker, case):
    """read_state from a checker library (the CPU oracle): the model of node_model under the case's potentials (and ponds)"""
    m = node_model(case)
    checker.check(checker.lib.sf3d_reset_solver_state(), "reset")
    cm.build(checker, m, threads=1)
    if "pond" in case:
        checker.set_pond_bulk(0, case["pond"])
    checker.set_matric_potential_bulk(0, case["psi"])
    state = read_state(checker, m, case)
    checker.lib.sf3d_clean()
    return state


def device_run(sf, case, one_layer=False, crack=False):
    """the module chain on a loaded product: node_model with set_matric_potential_bulk (and the ponds), the column table, the root block, the
    sink block (with cracking), then every hour of the case with its maps passed in -> (read_state of the device's own state, the outputs
    of every hour)"""
    nl = 1 if one_layer else len(case["layer_depth"])
    m = node_model(case)
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1)
    if "pond" in case:
        sf.set_pond_bulk(0, case["pond"])
    sf.set_matric_potential_bulk(0, case["psi"])
    sinks.set_columns(sf, case["columns"][:nl], case["layer_thickness"][:nl])
    state = read_state(sf, m, case)
    root.initialize(sf, case["dem"], case["crop_index"], case["soil_index"], case["unit_list"], case["soil_list"], case["layer_depth"][:nl], case["layer_thickness"][:nl],
                    float(case["flag"]))
    initialize(sf, case, one_layer)
    if crack:
        sinks.set_cracking(sf, case["crack_soils"])
    out = []
    for k in range(len(case["et0"])):
        hour(sf, case, k)
        e, t = sinks.get_actual(sf)
        got = dict(sinks=sinks.get_node_sinks(sf, m.n), evaporation=e, transpiration=t)
        if crack:
            got["prec_surface_water"], got["crack_water"] = sinks.get_crack(sf)
        out.append(got)
    sf.lib.sf3d_clean()
    return state, out


HOST_PROGRAMS = ("root", "sink")                # run_host's `exes`, in this order: the sink program takes the root program's outputs


def run_host(exes, directory, name, case, k, state, one_layer=False, crack=False):
    """hour k of a case (the pin, a small case) on the host programs: the root program on the hour's degree days, then the sink program
    without and, with `crack`, with soil cracking -> dict(status, last_evap_layer, plain=dict(sinks, evaporation, transpiration)[,
    crack=dict(sinks, evaporation, transpiration, prec_surface_water, crack_water), max_depth, last_layer])"""
    import ctypes
    from tests.raster_helpers import Reader, run_host_program
    nl = 1 if one_layer else len(case["layer_depth"])
    dem = np.asarray(case["dem"], np.float32)
    n, N = dem.size, state["n"]
    ld, lt = np.asarray(case["layer_depth"][:nl], np.float64), np.asarray(case["layer_thickness"][:nl], np.float64)
    rcase = rc.case_of(case, dem, case["crop_index"], case["soil_index"], [case["sink_degree_days"][k]], layer_depth=ld, layer_thickness=lt)
    roots = rc.run_host(exes[0], directory, name + "-root", rcase)
    assert roots["status"] == 0
    rm = roots["maps"][0]
    units, soils = case["sink_units"], case["sink_soils"]
    columns = np.asarray(case["columns"], np.int32)[:nl]
    parts = [np.array([n, nl, len(units), len(soils), N, state["ns"], len(state["theta_s"]), roots["rows"], int(crack)], np.int32), np.array([case["flag"]], np.float32),
             np.array([case["cell_size"], 0.0 if one_layer else case["computation_depth"]], np.float64), dem, np.asarray(case["crop_index"], np.int32),
             np.asarray(case["soil_index"], np.int32), ld, lt, bytes(sinks.unit_array(units))[:len(units) * ctypes.sizeof(sinks.Unit)],
             bytes(sinks.soil_array(soils))[:len(soils) * ctypes.sizeof(sinks.Soil)], columns,
             np.asarray(state["H"], np.float64), np.asarray(state["z"], np.float64), np.asarray(state["Se"], np.float64), np.asarray(state["cls"], np.uint16),
             np.asarray(state["theta_s"], np.float64), np.asarray(state["theta_r"], np.float64)]
    parts += [np.asarray(case[key][k], np.float32) for key in ("et0", "lai", "sink_degree_days", "liquid_water")]
    parts += [rm["length"], rm["first"], rm["last"], rm["key"], roots["table"]]
    if crack:
        cs = case["crack_soils"]
        parts += [bytes(sinks.crack_soil_array(cs))[:len(cs) * ctypes.sizeof(sinks.CrackSoil)], np.asarray(state["pond"], np.float64)]
    r = Reader(run_host_program(exes[1], directory, name, parts))
    status, last_evap = (int(v) for v in r.take(np.int32, 2))
    out = dict(status=status, last_evap_layer=last_evap, roots=roots)
    if status == 0:
        take = lambda: dict(sinks=r.take(np.float64, N), evaporation=r.take(np.float64, *dem.shape), transpiration=r.take(np.float64, *dem.shape))
        out["plain"] = take()
        if crack:
            out["max_depth"], out["last_layer"] = r.take(np.float64, len(soils)), r.take(np.int32, len(soils))
            out["crack"] = take()
            out["crack"].update(prec_surface_water=r.take(np.float32, *dem.shape), crack_water=r.take(np.float64, *dem.shape))
    assert r.done()
    return out


def crack_state(checker, case):
    """(VWC, maxVWC, pond [mm]) of every node as getCriteria3DVar returns them, for the restatement with cracking"""
    from tests import crack_cases as kc
    m = node_model(case)
    checker.check(checker.lib.sf3d_reset_solver_state(), "reset")
    cm.build(checker, m, threads=1)
    checker.set_pond_bulk(0, case["pond"])
    checker.set_matric_potential_bulk(0, case["psi"])
    state = kc.node_state(checker, m.n)
    checker.lib.sf3d_clean()
    return state


def shorter_grid(pin, layers, **other):
    """the pin's tables on its first `layers` layers"""
    return dict(pin, layer_depth=pin["layer_depth"][:layers], layer_thickness=pin["layer_thickness"][:layers], **other)


def tiny_case(pin, seed, crack=False):
    """one row of eight cells on the pin's tables (small_case needs 33 cells for the cells it places by hand): cell 0 holds the flag, cell 1
    has no surface node, the others compute on drawn maps and potentials; the last one is the tree on the deepest soil, unstressed, in rain"""
    from tests.golden.make_water_sinks import PSI, SURFACE_WATER
    rng = np.random.default_rng(seed)
    case = {k: pin[k] for k in TABLES}
    flag = np.float32(pin["flag"])
    shape, n, nl, hours = (1, 8), 8, len(pin["layer_depth"]), 2
    dem = rng.uniform(50.0, 400.0, shape).astype(np.float32)
    dem.flat[0] = flag
    ci = rng.integers(0, len(pin["unit_list"]), shape).astype(np.int32)
    si = rng.integers(0, len(pin["soil_list"]), shape).astype(np.int32)
    draw = lambda values: np.array(values, np.float32)[rng.integers(0, len(values), (hours,) + shape)]
    columns = np.arange(nl * n, dtype=np.int32).reshape(nl, *shape)
    columns[:, 0, 0] = -1
    columns[0, 0, 1] = -1
    if nl > 3:
        columns[3, 0, 4] = -1
    psi = np.array(PSI)[rng.integers(0, len(PSI), nl * n)]
    psi[:n] = np.array(SURFACE_WATER)[rng.integers(0, len(SURFACE_WATER), n)]
    case.update(dem=dem, crop_index=ci, soil_index=si, et0=draw(ET0[3:]), lai=draw(LAI[2:]), liquid_water=draw(LIQUID),
                sink_degree_days=np.full((hours,) + shape, np.float32(900.0)), columns=columns, psi=psi)
    _column(case, n - 1, potentials=-12.0, surface_water=0.0001, crop_index=TREE, soil_index=0, et0=np.float32(0.45), lai=np.float32(1.0),
            sink_degree_days=np.float32(700.0), liquid_water=np.float32(1.2))
    if crack:
        from tests import crack_cases as kc
        case["crack_soils"] = pin["crack_soils"]
        case["pond"] = np.array(kc.POND)[rng.integers(0, len(kc.POND), n)]
        _column(case, 5, potentials=-800.0, soil_index=0, crop_index=-1, et0=np.float32(0.0), lai=np.float32(0.0), liquid_water=np.float32(14.0))      # the dry clay cracks
    set_node_classes(case)
    return case


def accepted(sf, case, one_layer=False, crack=False):
    """sf3d_sink_initialize (and sf3d_sink_set_cracking) take the case; neither needs a device"""
    from criteria3d_amd import capi
    try:
        initialize(sf, case, one_layer)
        if crack:
            sinks.set_cracking(sf, case["crack_soils"])
    except capi.SF3DError:
        return False
    finally:
        sinks.clean(sf)
    nl = 1 if one_layer else len(case["layer_depth"])
    return rc.accepted(sf, rc.case_of(case, case["dem"], case["crop_index"], case["soil_index"], [], layer_depth=case["layer_depth"][:nl],
                                      layer_thickness=case["layer_thickness"][:nl]))


def caps_tables(pin):
    """the pin's tables with CROP_MAX_UNITS land units (the pin's, repeated; the last one roots from the surface to 2 m, statically) and
    a further, last soil of ROOT_MAX_HORIZONS horizons and 0.995 m"""
    units = [dict(pin["unit_list"][k % len(pin["unit_list"])]) for k in range(sinks.MAX_UNITS)]
    units[-1] = dict(pin["unit_list"][1], rootDepthMax=2.0, isRootStatic=1)
    sink_units = [dict(pin["sink_units"][k % len(pin["sink_units"])]) for k in range(sinks.MAX_UNITS)]
    hz = np.linspace(0.0, 0.995, sinks.MAX_HORIZONS + 1)
    first = pin["sink_soils"][0]
    geometry = dict(totalDepth=0.995, upperDepth=[float(v) for v in hz[:-1]], lowerDepth=[float(v) for v in hz[1:]], soilFraction=[1.0 - 0.01 * h for h in range(sinks.MAX_HORIZONS)])
    water = {k: [first[k][0] - 0.001 * h for h in range(sinks.MAX_HORIZONS)] for k in ("waterContentHH", "waterContentFC", "waterContentWP", "waterContentSAT")}
    ns = len(pin["soil_list"])
    vg = np.zeros((ns + 1, sinks.MAX_HORIZONS) + pin["soil_vg"].shape[2:])
    vg[:ns, :pin["soil_vg"].shape[1]] = pin["soil_vg"]
    vg[ns, :] = pin["soil_vg"][0, 0]
    out = dict(pin, unit_list=units, sink_units=sink_units, soil_list=list(pin["soil_list"]) + [geometry], sink_soils=list(pin["sink_soils"]) + [dict(geometry, **water)],
               soil_vg=vg, soil_nr_horizons=np.append(pin["soil_nr_horizons"], sinks.MAX_HORIZONS))
    if "crack_soils" in pin:
        cs = pin["crack_soils"][0]
        out["crack_soils"] = list(pin["crack_soils"]) + [dict(totalDepth=0.995, **{k: [cs[k][0]] * sinks.MAX_HORIZONS for k in sinks.CRACK_FIELDS})]
    return out


def edge_cases(pin, crack_pin):
    """(name, case, one_layer, crack) of valid inputs at the edges of the tables.
    caps: caps_tables, with cell 19 on unit 63 and the last soil (its key is the last table row, its first root layer 0, its horizons reach
          the last of ROOT_MAX_HORIZONS) and cell 20 with the 3 m root system on the 1.5 m soil (lastRootLayer = nrLayers - 1); with cracking.
    evap-bottom: the first seven layers: lastEvapLayer = nrLayers - 1.
    crack-bottom: the first ten layers under a computation depth of 0.55 m: maxDepth = 0.55 m lies below the centre of the deepest layer
          (0.50 m), so computeSoilCracking's first loop stops at layerIndex = nrLayers.
    one-layer: nrLayers = 1, without and with cracking.   1x8: one row of eight cells, without and with cracking."""
    from tests import crack_cases as kc
    tables = caps_tables(crack_pin)
    case = kc.small_case(tables, (3, 12), 45)
    crop_hour = dict(et0=np.float32(0.45), lai=np.float32(2.5))
    _column(case, 19, potentials=-12.0, crop_index=sinks.MAX_UNITS - 1, soil_index=len(tables["soil_list"]) - 1, sink_degree_days=np.float32(2500.0), **crop_hour)
    _column(case, 20, potentials=-12.0, crop_index=7, soil_index=0, sink_degree_days=np.float32(700.0), **crop_hour)
    _column(case, 21, potentials=-800.0, crop_index=-1, soil_index=len(tables["soil_list"]) - 1, et0=np.float32(1.2), lai=np.float32(0.0))
    set_node_classes(case)
    yield "caps", case, False, True
    yield "evap-bottom", small_case(shorter_grid(pin, 7), (3, 11), 46), False, False
    yield "crack-bottom", kc.small_case(shorter_grid(crack_pin, 10, computation_depth=np.float64(0.55)), (4, 10), 47), False, True
    yield "one-layer", kc.small_case(crack_pin, (3, 11), 48), True, True
    yield "1x8", tiny_case(crack_pin, 49, crack=True), False, True
    yield "1x8-one-layer", tiny_case(crack_pin, 50, crack=True), True, True


def random_cases(pin, small=None):
    """(name, case): `small` (small_case, or tests/crack_cases.py's) on every shape and seed, with the value lists and with continuous_case"""
    small = small_case if small is None else small
    for shape in SHAPES:
        for seed in SEEDS:
            for continuous in (False, True):
                case = small(pin, shape, seed)
                if continuous:
                    continuous_case(case, seed)
                yield f"{'continuous' if continuous else 'lists'}-{shape[0]}x{shape[1]}-{seed}", case


def compare_host(got, want, names, what, exact=True):
    """the host program's arrays against the restatement's (or a pin's), bit for bit; not exact (another C library under the restatement's
    exp): to the last places of a double.  Returns how many values differ."""
    from tests.raster_helpers import differing
    differ = 0
    for n in names:
        g = got[n]
        w = np.asarray(want[n], g.dtype).reshape(g.shape)
        bad = differing(g, w)
        differ += int(bad.sum())
        if exact:
            assert not bad.any(), (what, n, int(bad.sum()), g[bad][:4], w[bad][:4])
        else:
            assert np.allclose(g, w, rtol=1e-9, atol=1e-15, equal_nan=True), (what, n)
    return differ
