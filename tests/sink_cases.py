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
