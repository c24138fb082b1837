"""Soil cracking without a GPU: the restatement of Crit3DProject::computeSoilCracking inside the rain term (criteria3d_amd/sinks.py) against
the compiled-reference pin tests/golden/soil_cracking.npz - node sinks, both actual maps, computeSoilCracking's return value and the crack
water of every hour bit for bit, zero excluded; the fixture's arm table; the small rasters of tests/crack_cases.py reach every arm too;
the per-soil tables of sf3d_sink_set_cracking against the recorded ones; its refusals and its off-switch, which need no device; and the host build of
the kernel's per-cell text with cracking (tests/sink_host.cpp): equal to the pin and to the restatement bit for bit, clean under the sanitizers."""
import ctypes as C

import numpy as np
import pytest

from criteria3d_amd import capi, sinks
from tests import crack_cases as kc
from tests import sink_cases as sc
from tests.golden import make_soil_cracking as gen
from tests.raster_helpers import bits, build_host_program


@pytest.fixture(scope="module")
def pin():
    return kc.load_pin()


@pytest.fixture(scope="module")
def restated(pin):
    arms = {}
    return [kc.restated(pin, k, arms) for k in range(len(pin["et0"]))], arms


def test_restatement_equals_the_pin(pin, restated):
    for k, got in enumerate(restated[0]):
        for name in ("sinks_et",) + kc.OUTPUTS:
            bad = bits(got[name]) != bits(pin[name][k])
            assert not bad.any(), (k, name, int(bad.sum()))
        plain = sinks.restate_sink_hour(pin["dem"], float(pin["flag"]), float(pin["cell_size"]), pin["columns"], pin["vwc"], pin["crop_index"], pin["soil_index"],
                                        pin["sink_units"], pin["sink_soils"], pin["layer_depth"], pin["layer_thickness"], float(pin["computation_depth"]),
                                        pin["et0"][k], pin["lai"][k], pin["sink_degree_days"][k], pin["liquid_water"][k], sc.roots_of(pin, k), len(pin["vwc"]))
        assert np.count_nonzero(plain["sinks"] != got["sinks"]) > 100, k                  # cracking changes the hour
        assert np.array_equal(bits(plain["sinks_et"]), bits(got["sinks_et"]))
    ns = pin["dem"].size
    flag = float(pin["flag"])
    assert np.all(pin["crack_water"][:, pin["columns"][0] < 0] == flag) and np.all(pin["prec_surface_water"][:, pin["columns"][0] < 0] == np.float32(flag))
    filled = pin["sinks"][:, ns:] > pin["sinks_et"][:, ns:]
    assert np.count_nonzero(filled) > 1000 and np.count_nonzero(filled & (pin["sinks_et"][:, ns:] < 0)) > 100      # additions on top of subtractions


def test_one_layer_case(pin):
    for j, k in enumerate(int(v) for v in pin["one_layer_hours"]):
        got = kc.restated(pin, k, one_layer=True)
        for name in kc.OUTPUTS:
            assert np.array_equal(bits(got[name]), bits(pin["one_layer_" + name][j])), (k, name)
        w = pin["one_layer_crack_water"][j]
        assert not pin["one_layer_sinks"][j][pin["dem"].size:].any() and np.all(w[w != float(pin["flag"])] == 0)
        assert np.array_equal(bits(pin["one_layer_prec_surface_water"][j]), bits(np.where(pin["columns"][0] < 0, np.float32(pin["flag"]), pin["liquid_water"][k])))


def test_no_arm_is_empty(pin, restated):
    recorded = dict(zip((str(n) for n in pin["arm_names"]), (int(v) for v in pin["arm_counts"])))
    for arm in gen.REQUIRED_ARMS:
        assert recorded.get(arm, 0) > 0, arm
    counted = {k: v for k, v in restated[1].items() if k.startswith("crack")}
    outside = ("crack: snowfall or snowmelt at the flag", "crack: liquidWater changed by snow", "crack: soilDepth <= 0.2 by computationSoilDepth")
    assert counted == {k: v for k, v in recorded.items() if k not in outside}      # the restatement walks the same arms as often
    arms1 = {}
    for k in pin["one_layer_hours"]:
        kc.restated(pin, int(k), arms1, one_layer=True)
    assert arms1["crack: soilDepth <= 0.2 by computationSoilDepth"] == recorded["crack: soilDepth <= 0.2 by computationSoilDepth"]
    snow = {}
    for k in range(len(pin["et0"])):
        computed = pin["evaporation"][k] != float(pin["flag"])
        flag = np.float32(pin["flag"])
        kc.liquid_water(np.where(computed, pin["precipitation"][k], flag), pin["snow_fall"][k], pin["snow_melt"][k], bool(pin["snow"][k]), flag, snow)
    assert snow == {k: recorded[k] for k in outside[:2]}
    for k in range(len(pin["et0"])):
        want = kc.liquid_water(pin["precipitation"][k], pin["snow_fall"][k], pin["snow_melt"][k], bool(pin["snow"][k]), pin["flag"])
        assert np.array_equal(bits(want), bits(pin["liquid_water"][k]))


def test_small_cases_reach_every_arm(pin, oracle):
    """the rasters tests/test_gpu_crack.py runs off the fixture: 259, 33 and 300 cells, on the CPU oracle's node state"""
    from criteria3d_amd import catchment as cm
    union = {}
    for shape in sc.SHAPES:
        case = kc.small_case(pin, shape, seed=shape[1])
        m = sc.node_model(case)
        oracle.check(oracle.lib.sf3d_reset_solver_state(), "reset")
        cm.build(oracle, m, threads=1)
        oracle.set_pond_bulk(0, case["pond"])
        oracle.set_matric_potential_bulk(0, case["psi"])
        state = kc.node_state(oracle, m.n)
        oracle.lib.sf3d_clean()
        for k in range(len(case["et0"])):
            got = kc.restated_case(case, k, state, arms=union)
            assert np.count_nonzero((got["crack_water"] != float(case["flag"])) & (got["crack_water"] > 0)) > 0 or tuple(shape) == kc.SHALLOW, (shape, k)
        kc.snow_arms(case, union)
    missing = [arm for arm in gen.REQUIRED_ARMS if union.get(arm, 0) == 0]
    assert not missing, missing


def test_crack_tables_equal_the_recorded_ones(pin):
    reasons = []
    md, ll = sinks.crack_tables(pin["sink_soils"], pin["crack_soils"], pin["layer_depth"], pin["layer_thickness"], float(pin["computation_depth"]), reasons)
    assert np.array_equal(bits(md), bits(pin["crack_max_depth"])) and np.array_equal(ll, pin["crack_last_layer"])      # lastLayer: the compiled getSoilLayerIndex
    assert (ll == -9999).sum() == 3 and len(set(reasons)) == 6 and md[0] == 0.6 and md[1] == 0.4
    sf = capi.load_product()
    sc.initialize(sf, pin)                                        # no device needed
    sinks.set_cracking(sf, pin["crack_soils"])
    md2, ll2 = sinks.get_crack_tables(sf)
    assert np.array_equal(bits(md2), bits(pin["crack_max_depth"])) and np.array_equal(ll2, pin["crack_last_layer"])
    sc.initialize(sf, pin, one_layer=True)
    sinks.set_cracking(sf, pin["crack_soils"])
    md1, ll1 = sinks.get_crack_tables(sf)
    assert np.array_equal(bits(md1), bits(pin["one_layer_crack_max_depth"])) and np.array_equal(ll1, pin["one_layer_crack_last_layer"]) and np.all(ll1 == -9999)
    sinks.clean(sf)


def test_set_cracking_refusals_and_off_switch(pin):
    sf = capi.load_product()
    sinks.bind(sf)
    lib = sf.lib
    lib.sf3d_clean()
    soils = sinks.crack_soil_array(pin["crack_soils"])
    ns = len(pin["crack_soils"])
    n = pin["dem"].size
    p, w = np.zeros(n, np.float32), np.zeros(n)
    get = lambda: lib.sf3d_sink_get_crack(n, p.ctypes.data_as(sinks.pf32), w.ctypes.data_as(sinks.pf64))
    assert lib.sf3d_sink_set_cracking(ns, soils) == capi.MEMORY_ERROR and lib.sf3d_sink_set_cracking(0, None) == capi.MEMORY_ERROR      # before initialize
    assert lib.sf3d_sink_get_crack_tables(None, None) == capi.MEMORY_ERROR and get() == capi.MEMORY_ERROR
    sc.initialize(sf, pin)
    assert lib.sf3d_sink_get_crack_tables(None, None) == capi.MEMORY_ERROR                          # cracking is off unless asked for
    assert lib.sf3d_sink_set_cracking(ns - 1, soils) == capi.PARAMETER_ERROR and lib.sf3d_sink_set_cracking(ns + 1, soils) == capi.PARAMETER_ERROR
    assert lib.sf3d_sink_get_crack_tables(None, None) == capi.MEMORY_ERROR                          # a refused call leaves it off
    many = sinks.crack_soil_array(pin["crack_soils"])
    many[0].nrHorizons = sinks.MAX_HORIZONS + 1
    assert lib.sf3d_sink_set_cracking(ns, many) == capi.PARAMETER_ERROR
    many[0].nrHorizons = -1
    assert lib.sf3d_sink_set_cracking(ns, many) == capi.PARAMETER_ERROR
    many[0].nrHorizons = 1
    many[3].nrHorizons = 2                                                                          # more horizons than the soil of sf3d_sink_initialize has
    assert lib.sf3d_sink_set_cracking(ns, many) == capi.PARAMETER_ERROR
    assert lib.sf3d_sink_set_cracking(ns, soils) == capi.OK and lib.sf3d_sink_get_crack_tables(None, None) == capi.OK
    assert get() == capi.MEMORY_ERROR                                                               # before the first hour
    assert lib.sf3d_sink_set_cracking(0, None) == capi.OK and lib.sf3d_sink_get_crack_tables(None, None) == capi.MEMORY_ERROR       # the off-switch
    assert lib.sf3d_sink_set_cracking(ns, None) == capi.OK and lib.sf3d_sink_set_cracking(0, soils) == capi.OK
    assert lib.sf3d_sink_set_cracking(ns, soils) == capi.OK
    sc.initialize(sf, pin)                                                                          # a new raster: off again
    assert lib.sf3d_sink_get_crack_tables(None, None) == capi.MEMORY_ERROR
    assert lib.sf3d_sink_clean() == capi.OK and lib.sf3d_sink_set_cracking(ns, soils) == capi.MEMORY_ERROR
    lib.sf3d_clean()


def test_soil_crack_table_reads_the_soils_of_load_all_soils():
    from criteria3d_amd import project3d
    soils = [dict(total_depth=0.9, horizons=[dict(clay=55.0, silt=30.0, coarse=0.05, organic_matter=0.02, upper=0.0, lower=0.5),
                                             dict(clay=20.0, silt=40.0, coarse=0.0, organic_matter=0.01, upper=0.5, lower=0.9)])]
    t = project3d.soil_crack_table(soils)
    assert t == [dict(totalDepth=0.9, clay=[55.0, 20.0], silt=[30.0, 40.0], coarseFragments=[0.05, 0.0], organicMatter=[0.02, 0.01])]
    arr = sinks.crack_soil_array(t)
    assert arr[0].nrHorizons == 2 and arr[0].totalDepth == 0.9 and arr[0].silt[1] == 40.0 and C.sizeof(sinks.CrackSoil) == 16 + 32 * sinks.MAX_HORIZONS


# ---- the host build of the per-cell text of k_sink_hour_crack behind sf3d_sink_set_cracking's table builder (tests/sink_host.cpp): the
# text == the pin, the text == the restatement.  The edge cases of the tables run in tests/test_sink_host.py, with cracking.

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from types import SimpleNamespace
    d = tmp_path_factory.mktemp("crack_host")
    return SimpleNamespace(dir=d, exes=[build_host_program(b, d) for b in sc.HOST_PROGRAMS], san=[build_host_program(b, d, sanitize=True) for b in sc.HOST_PROGRAMS])


def test_host_text_equals_the_pin_on_every_hour_and_on_one_layer(pin, oracle, host):
    """H, Se and the ponds come from the checker on the pin's potentials; no libm escape: the text carries its own exp"""
    state = sc.node_state(oracle, pin)
    assert np.array_equal(bits(state["vwc"]), bits(pin["vwc"]))
    for k in range(len(pin["et0"])):
        got = sc.run_host(host.exes, host.dir, "pin", pin, k, state, crack=True)
        assert np.array_equal(bits(got["max_depth"]), bits(pin["crack_max_depth"])) and np.array_equal(got["last_layer"], pin["crack_last_layer"])
        print(f"host text, hour {k}: values differ: {sc.compare_host(got['crack'], {n: pin[n][k] for n in kc.OUTPUTS}, kc.OUTPUTS, k)}")
    for j, k in enumerate(int(v) for v in pin["one_layer_hours"]):
        got = sc.run_host(host.exes, host.dir, "pin-one-layer", pin, k, state, one_layer=True, crack=True)
        assert np.array_equal(got["last_layer"], pin["one_layer_crack_last_layer"])
        print(f"host text, one layer, hour {k}: values differ: {sc.compare_host(got['crack'], {n: pin['one_layer_' + n][j] for n in kc.OUTPUTS}, kc.OUTPUTS, k)}")


def test_host_text_equals_the_restatement_on_random_cases(pin, oracle, host):
    from tests import tolerances
    exact, why = tolerances.libm_probe()
    print(why)
    for name, case in sc.random_cases(pin, kc.small_case):
        state, node_state = sc.node_state(oracle, case), sc.crack_state(oracle, case)
        differ = 0
        for k in range(len(case["et0"])):
            got = sc.run_host(host.exes, host.dir, name, case, k, state, crack=True)
            differ += sc.compare_host(got["crack"], kc.restated_case(case, k, node_state), kc.OUTPUTS, (name, k), exact)
            differ += sc.compare_host(got["plain"], kc.restated_case(case, k, node_state, crack=False), kc.OUTPUTS[:3], (name, k, "off"), exact)
        print(f"{name}: values differ: {differ}")


def test_random_cases_reach_every_arm_of_the_pin(pin, oracle):
    """the restatement's own counters over the union of the random cases: every arm the pin's census lists"""
    union = {}
    for name, case in sc.random_cases(pin, kc.small_case):
        node_state = sc.crack_state(oracle, case)
        filled = 0
        for k in range(len(case["et0"])):
            got = kc.restated_case(case, k, node_state, arms=union)
            filled += np.count_nonzero((got["crack_water"] != float(case["flag"])) & (got["crack_water"] > 0))
        assert filled > 0 or case["dem"].shape == kc.SHALLOW, name
        kc.snow_arms(case, union)
    unreachable = {}                                                 # arm -> why the random cases cannot reach it (the pin covers it); three at the most
    missing = [str(arm) for arm in pin["arm_names"] if union.get(str(arm), 0) == 0 and str(arm) not in unreachable]
    assert not missing and len(unreachable) <= 3, missing


def test_sanitized_host_build_reports_nothing(pin, oracle, host):
    """address and undefined-behaviour sanitizers on the pin and on every random case, with cracking: exit 0, nothing on stderr"""
    state = sc.node_state(oracle, pin)
    for k in range(len(pin["et0"])):
        sc.run_host(host.san, host.dir, "san-pin", pin, k, state, crack=True)
    for k in (int(v) for v in pin["one_layer_hours"]):
        sc.run_host(host.san, host.dir, "san-pin-one-layer", pin, k, state, one_layer=True, crack=True)
    runs = len(pin["et0"]) + len(pin["one_layer_hours"])
    for name, case in sc.random_cases(pin, kc.small_case):
        state = sc.node_state(oracle, case)
        for k in range(len(case["et0"])):
            sc.run_host(host.san, host.dir, "san-" + name, case, k, state, crack=True)
            runs += 1
    print(f"sink_host_san with cracking: {runs} runs, nothing reported")
