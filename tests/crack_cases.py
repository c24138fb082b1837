"""What tests/test_crack_host.py, tests/test_gpu_crack.py and scripts/multirank_crack_worker.py share (no tests here): the pin
tests/golden/soil_cracking.npz (on the raster, units, layer grid and root maps of the sink pin, with seven soils) decoded into the tables
the binding and the restatement take, the set-up of the blocks on a loaded product, and small rasters of any shape that reach the arms of
Crit3DProject::computeSoilCracking."""
from pathlib import Path

import numpy as np

from criteria3d_amd import maps, sinks
from tests import sink_cases as sc

PIN = Path(__file__).resolve().parent / "golden" / "soil_cracking.npz"
OUTPUTS = ("sinks", "evaporation", "transpiration", "prec_surface_water", "crack_water")
PORT = 29797                                    # of the two-rank test: clear of tests/ranks.py PORTS and of what test_gpu_multirank.py reaches

def load_pin():
    """the sink pin's dictionary with the cracking pin's arrays in place of the sink pin's, and its own beside them"""
    p = sc.load_pin()
    for k in ("arm_names", "arm_counts", "horizon", "one_layer_sinks_et"):
        p.pop(k, None)
    z = np.load(PIN)
    for k in z.files:
        p["sink_degree_days" if k == "degree_days" else k] = z[k]
    p["soil_list"], p["sink_soils"], p["crack_soils"] = [], [], []
    for s, nh in enumerate(int(v) for v in p["soil_nr_horizons"]):
        hz, w, tx = p["soil_horizons"][s, :nh], p["soil_water"][s, :nh], p["soil_texture"][s, :nh]
        so = dict(totalDepth=float(p["soil_total_depth"][s]), upperDepth=[float(v) for v in hz[:, 0]], lowerDepth=[float(v) for v in hz[:, 1]],
                  soilFraction=[1.0 - float(v) for v in hz[:, 2]])
        p["soil_list"].append(so)
        p["sink_soils"].append(dict(so, waterContentHH=[float(v) for v in w[:, 0]], waterContentFC=[float(v) for v in w[:, 1]],
                                    waterContentWP=[float(v) for v in w[:, 2]], waterContentSAT=[float(v) for v in w[:, 3]]))
        p["crack_soils"].append(dict(totalDepth=so["totalDepth"], clay=[float(v) for v in tx[:, 0]], silt=[float(v) for v in tx[:, 1]],
                                     coarseFragments=[float(v) for v in hz[:, 2]], organicMatter=[float(v) for v in tx[:, 2]]))
    return p


def cracking(pin):
    """the `cracking` argument of sinks.restate_sink_hour on the pin's recorded state"""
    return dict(crack_soils=pin["crack_soils"], max_vwc=pin["max_vwc"], pond=pin["pond_mm"])


def restated(pin, hour, arms=None, one_layer=False):
    nl = 1 if one_layer else len(pin["layer_depth"])
    r = sc.roots_of(pin, hour)
    r["density"] = r["density"][:nl]
    return sinks.restate_sink_hour(pin["dem"], float(pin["flag"]), float(pin["cell_size"]), pin["columns"][:nl], pin["vwc"], pin["crop_index"], pin["soil_index"],
                                   pin["sink_units"], pin["sink_soils"], pin["layer_depth"][:nl], pin["layer_thickness"][:nl],
                                   0.0 if one_layer else float(pin["computation_depth"]), pin["et0"][hour], pin["lai"][hour], pin["sink_degree_days"][hour],
                                   pin["liquid_water"][hour], r, len(pin["vwc"]), arms, cracking(pin))


def liquid_water(prec, fall, melt, snow, flag, arms=None):
    """liquidWater of assignPrecipitation (criteria3DProject.cpp:939-953) in float arithmetic; counts its two snow arms"""
    fl = np.float32(flag)
    liquid = prec.astype(np.float32).copy()
    if snow:
        both = (prec != fl) & (fall != fl) & (melt != fl)
        liquid[both] = (prec[both] - fall[both]) + melt[both]
        if arms is not None:
            for name, count in (("crack: snowfall or snowmelt at the flag", np.count_nonzero((prec != fl) & ~both)),
                                ("crack: liquidWater changed by snow", np.count_nonzero((prec != fl) & (liquid != prec)))):
                arms[name] = arms.get(name, 0) + int(count)
    return liquid


def set_state(sf, pin, columns=True):
    """the fixture's matric potentials, ponds and (on the product) column table; the model of sc.node_model is built"""
    sf.set_pond_bulk(0, pin["pond"])
    sf.set_matric_potential_bulk(0, pin["psi"])
    if columns:
        sinks.set_columns(sf, pin["columns"], pin["layer_thickness"])


def node_state(sf, n):
    """(VWC, maxVWC, pond [mm]) of every node as getCriteria3DVar returns them, from the library's per-node getters"""
    wanted = (maps.VOLUMETRIC_WATER_CONTENT, maps.MAX_VOLUMETRIC_WATER_CONTENT, maps.SURFACE_POND)
    g = maps.node_getter_values(sf, n, wanted)
    return tuple(maps.criteria3d_var(var, g[var]) for var in wanted)


def initialize(sf, pin, one_layer=False, crack=True):
    """the root and the sink block on the pin's (or a small case's) raster, with cracking on"""
    nl = 1 if one_layer else len(pin["layer_depth"])
    from criteria3d_amd import root
    root.initialize(sf, pin["dem"], pin["crop_index"], pin["soil_index"], pin["unit_list"], pin["soil_list"], pin["layer_depth"][:nl], pin["layer_thickness"][:nl],
                    float(pin["flag"]))
    sc.initialize(sf, pin, one_layer)
    if crack:
        sinks.set_cracking(sf, pin["crack_soils"])


def outputs(sf, n):
    e, t = sinks.get_actual(sf)
    p, w = sinks.get_crack(sf)
    return dict(sinks=sinks.get_node_sinks(sf, n), evaporation=e, transpiration=t, prec_surface_water=p, crack_water=w)


# ---- a raster of any shape on the pin's tables

PREC = (0.0, 0.05, 0.6, 3.0, 14.0, 60.0)       # [mm]: none, below the smallest pond, between the ponds, ordinary, more than a crack of 0.6 m takes
POND = (0.0001, 0.0005, 0.002, 0.005)          # [m]
SHALLOW = (3, 11)                               # the shape whose computationSoilDepth is 0.15 m: no soil is deep enough to crack
DRY = (-800.0, -150.0)


def small_case(pin, shape, seed, hours=2):
    """sc.small_case on the cracking pin's seven soils, with ponds, rain drawn from PREC with snowfall and snowmelt in the second hour, half
    of the columns dry, and cells placed by hand (cells 10 to 17) for the arms chance may miss on 33 cells"""
    case = sc.small_case(pin, shape, seed, hours)
    case["crack_soils"] = pin["crack_soils"]
    rng = np.random.default_rng(seed + 1000)
    flag = np.float32(pin["flag"])
    n, nl = case["dem"].size, len(pin["layer_depth"])
    if tuple(shape) == SHALLOW:
        case["computation_depth"] = np.float64(0.15)
    psi = case["psi"].reshape(nl, n)
    dry = rng.random(n) < 0.5
    psi[1:, dry] = np.array(DRY)[rng.integers(0, 2, (nl - 1, int(dry.sum())))]
    case["pond"] = np.array(POND)[rng.integers(0, len(POND), n)]
    prec = np.array(PREC, np.float32)[rng.integers(0, len(PREC), (hours,) + tuple(shape))]
    prec[rng.random(prec.shape) < 0.04] = flag
    fall, melt = np.zeros_like(prec), np.zeros_like(prec)
    fall[1][rng.random(shape) < 0.3] = np.float32(2.5)
    fall[1][rng.random(shape) < 0.1] = np.float32(80.0)
    melt[1][rng.random(shape) < 0.3] = np.float32(0.7)
    fall[1].flat[20], melt[1].flat[21] = flag, flag
    layers = np.arange(1, nl)
    hand = dict(crop_index=-1, et0=np.float32(0.0), lai=np.float32(0.0))
    # the deep clay, dry: the ratio clamped to 1; 60 mm leave a residual after layer 1, 3 mm are used up before it
    sc._column(case, 10, potentials=-800.0, soil_index=0, **hand)
    sc._column(case, 11, potentials=-800.0, soil_index=0, **hand)
    # ... moist at the top and dry below: storage below the cap in one layer and capped in another
    sc._column(case, 12, potentials=np.where(layers <= 3, -2.0, -800.0), soil_index=0, **hand)
    # ... a hole at layer 1, and a hole inside the range
    sc._column(case, 13, potentials=-800.0, soil_index=0, **hand)
    sc._column(case, 14, potentials=-800.0, soil_index=0, **hand)
    case["columns"].reshape(nl, n)[1, 13] = -1
    case["columns"].reshape(nl, n)[4, 14] = -1
    # the thin fine horizon, the gap between two fine horizons, the fine range ended by a second horizon
    sc._column(case, 15, potentials=-800.0, soil_index=5, **hand)
    sc._column(case, 16, potentials=-800.0, soil_index=6, **hand)
    sc._column(case, 17, potentials=-150.0, soil_index=1, **hand)
    # ... evaporating: the crack's upper layers already carry a subtraction
    sc._column(case, 18, potentials=np.where(layers <= 4, -0.3, -800.0), soil_index=0, crop_index=-1, et0=np.float32(1.2), lai=np.float32(0.0))
    for cell, p in ((10, 60.0), (11, 3.0), (12, 14.0), (13, 14.0), (14, 14.0), (15, 14.0), (16, 14.0), (17, 14.0), (18, 14.0)):
        prec[:, cell // shape[1], cell % shape[1]] = np.float32(p)
        fall[:, cell // shape[1], cell % shape[1]] = melt[:, cell // shape[1], cell % shape[1]] = 0
    case["pond"][10:19] = 0.0005
    case["precipitation"], case["snow_fall"], case["snow_melt"] = prec, fall, melt
    case["snow"] = np.array([0, 1][:hours] + [0] * max(0, hours - 2), np.int32)
    case["liquid_water"] = np.stack([liquid_water(prec[k], fall[k], melt[k], bool(case["snow"][k]), flag) for k in range(hours)])
    sc.set_node_classes(case)
    return case


def restated_case(case, k, state, columns=None, arms=None, crack=True):
    """the restatement of hour k of a small case on the node state (VWC, maxVWC, pond [mm]) a library holds"""
    vwc, max_vwc, pond_mm = state
    return sinks.restate_sink_hour(case["dem"], float(case["flag"]), float(case["cell_size"]), case["columns"] if columns is None else columns, vwc,
                                   case["crop_index"], case["soil_index"], case["sink_units"], case["sink_soils"], case["layer_depth"], case["layer_thickness"],
                                   float(case["computation_depth"]), case["et0"][k], case["lai"][k], case["sink_degree_days"][k], case["liquid_water"][k],
                                   sc.roots_restated(case, k), case["columns"].size, arms,
                                   dict(crack_soils=case["crack_soils"], max_vwc=max_vwc, pond=pond_mm) if crack else None)


def snow_arms(case, arms):
    """counts the arms of assignPrecipitation's own lines over the case's hours"""
    for k in range(len(case["precipitation"])):
        liquid_water(case["precipitation"][k], case["snow_fall"][k], case["snow_melt"][k], bool(case["snow"][k]), np.float32(case["flag"]), arms)
