"""Soil cracking on the device (sf3d_sink_set_cracking, k_sink_hour_crack) against the compiled-reference pin
tests/golden/soil_cracking.npz: node sinks, both actual maps and both cracking maps of every hour bit for bit, zero cells excluded, on a
state whose water content, maximum water content and pond equal the recorded ones; the nrLayers = 1 case; rasters with a partial block,
less than a wave and a single row against the restatement, reaching every arm; cracking off after on; a column table changed between two
hours; sf3d_sink_apply against the node-by-node setter with one computeStep against the CPU oracle given the same sinks; two ranks
sharing the GPU; the device against the host build of the same text (tests/sink_host.cpp) with cracking, bit for bit."""
import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, sinks
from tests import crack_cases as kc
from tests import ranks as mr
from tests import sink_cases as sc
from tests.golden import make_soil_cracking as gen
from tests.raster_helpers import bits, build_host_program, need_glibc_set as _need_glibc_set
from tests.tolerances import assert_water_nodes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return kc.load_pin()


def _model(lib, case, columns=True):
    m = sc.node_model(case)
    lib.check(lib.lib.sf3d_reset_solver_state(), "reset")
    cm.build(lib, m, threads=1)
    kc.set_state(lib, case, columns)
    return m


def _same(got, want, what):
    for name in want:
        bad = bits(got[name]) != bits(want[name])
        print(f"{what} {name}: {int(bad.sum())} values differ")
        assert not bad.any(), (what, name, int(bad.sum()), np.asarray(got[name])[bad][:4], np.asarray(want[name])[bad][:4])


def test_every_hour_equals_the_pin(product, pin):
    _need_glibc_set(product)
    m = _model(product, pin)
    for got, name in zip(kc.node_state(product, m.n), ("vwc", "max_vwc", "pond_mm")):              # the state the reference read
        assert np.array_equal(bits(got), bits(pin[name])), name
    kc.initialize(product, pin)
    for k in range(len(pin["et0"])):
        sc.hour(product, pin, k)
        _same(kc.outputs(product, m.n), {name: pin[name][k] for name in kc.OUTPUTS}, f"hour {k}")
    sc.hour(product, pin, 0)                                                                        # an earlier hour again: nothing is left over
    _same(kc.outputs(product, m.n), {name: pin[name][0] for name in kc.OUTPUTS}, "hour 0 again")
    product.lib.sf3d_clean()


def test_one_layer(product, pin):
    _need_glibc_set(product)
    m = _model(product, pin)
    sinks.set_columns(product, pin["columns"][:1], pin["layer_thickness"][:1])
    kc.initialize(product, pin, one_layer=True)
    for j, k in enumerate(int(v) for v in pin["one_layer_hours"]):
        sc.hour(product, pin, k)
        _same(kc.outputs(product, m.n), {name: pin["one_layer_" + name][j] for name in kc.OUTPUTS}, f"one layer, hour {k}")
    product.lib.sf3d_clean()


def _small(product, pin, shape):
    case = kc.small_case(pin, shape, seed=shape[1])
    m = _model(product, case)
    state = kc.node_state(product, m.n)
    kc.initialize(product, case)
    return case, m, state


def _wanted(case, k, state, columns=None, arms=None, crack=True):
    want = kc.restated_case(case, k, state, columns, arms, crack)
    return {name: want[name] for name in (kc.OUTPUTS if crack else kc.OUTPUTS[:3])}


ARMS = {}                                       # shape -> the arms its two hours reach, counted by the restatement on the device's node state


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_other_raster_shapes_against_the_restatement(product, pin, shape):
    """259 cells: one block plus three lanes; 33 cells: less than a wave (and a computation depth under which no soil cracks); one row of
    300: a partial second block.  Two hours against the restatement on the node state the device holds."""
    _need_glibc_set(product)
    case, m, state = _small(product, pin, shape)
    flag, n, nl = float(case["flag"]), case["dem"].size, len(case["layer_depth"])
    arms = ARMS.setdefault(tuple(shape), {})
    arms.clear()
    for k in range(len(case["et0"])):
        sc.hour(product, case, k)
        got = kc.outputs(product, m.n)
        _same(got, _wanted(case, k, state, arms=arms), f"raster {shape}, hour {k}")
        p, w = got["prec_surface_water"], got["crack_water"]
        assert p.flat[0] == np.float32(flag) and w.flat[0] == flag and p.flat[2] == np.float32(flag) and w.flat[2] == flag      # a flag cell, a cell without a column
        assert not got["sinks"][np.arange(nl) * n + 2].any() and not got["sinks"][np.arange(nl) * n].any()
        assert p.flat[-1] != np.float32(flag) and w.flat[-1] != flag                                # the last lane computes
        if tuple(shape) != kc.SHALLOW:
            assert w.flat[10] > 0 and p.flat[10] < np.float32(60.0) and got["sinks"][n + 10] > 0   # the dry clay takes water
    kc.snow_arms(case, arms)
    product.lib.sf3d_clean()


def test_the_small_rasters_reach_every_arm(product, pin):
    """the arms the three rasters above reached, together; a shape whose test did not run in this session is walked here"""
    _need_glibc_set(product)
    for shape in sc.SHAPES:
        if tuple(shape) not in ARMS:
            case, m, state = _small(product, pin, shape)
            arms = ARMS.setdefault(tuple(shape), {})
            for k in range(len(case["et0"])):
                _wanted(case, k, state, arms=arms)
            kc.snow_arms(case, arms)
            product.lib.sf3d_clean()
    missing = [arm for arm in gen.REQUIRED_ARMS if not any(a.get(arm, 0) for a in ARMS.values())]
    assert not missing, missing


def test_cracking_off_after_on_equals_a_block_that_never_had_it(product, pin):
    _need_glibc_set(product)
    shape = (7, 37)
    case = kc.small_case(pin, shape, seed=shape[1])
    m = _model(product, case)
    state = kc.node_state(product, m.n)
    kc.initialize(product, case, crack=False)
    sc.hour(product, case, 0)
    e, t = sinks.get_actual(product)
    never = dict(sinks=sinks.get_node_sinks(product, m.n), evaporation=e, transpiration=t)
    n = case["dem"].size
    assert product.lib.sf3d_sink_get_crack(n, None, None) == capi.MEMORY_ERROR                     # cracking is off
    sinks.set_cracking(product, case["crack_soils"])
    assert product.lib.sf3d_sink_get_crack(n, None, None) == capi.MEMORY_ERROR                     # no cracked hour yet
    sc.hour(product, case, 0)
    cracked = kc.outputs(product, m.n)
    _same(cracked, _wanted(case, 0, state), "on")
    assert np.count_nonzero(cracked["sinks"] != never["sinks"]) > 50
    sinks.set_cracking(product, None)
    sc.hour(product, case, 0)
    e, t = sinks.get_actual(product)
    _same(dict(sinks=sinks.get_node_sinks(product, m.n), evaporation=e, transpiration=t), never, "off after on")
    _same(never, _wanted(case, 0, state, crack=False), "off, against the restatement")
    assert product.lib.sf3d_sink_get_crack(n, None, None) == capi.MEMORY_ERROR
    product.lib.sf3d_clean()


def _changed_columns(case):
    """the case's column table in which some computing cells have lost their whole column and others their nodes from layer 3 down"""
    n, nl = case["dem"].size, len(case["layer_depth"])
    columns = case["columns"].copy().reshape(nl, n)
    computing = np.flatnonzero(sc.computing_cells(case).ravel())
    columns[:, computing[1::5]] = -1
    columns[3:, computing[3::5]] = -1
    columns[3:, 10:12] = -1                                               # (the dry clay cells whose deep layers fill)
    return columns.reshape(case["columns"].shape)


def _one_step(lib, case, feed, columns=True):
    """the first computeStep of the case's model after `feed` has handed the sinks over: what the step took, H and Se"""
    m = _model(lib, case, columns)
    feed(m)
    dt = lib.lib.sf3d_compute_step(3600.0)
    s = cm.snapshot(lib, m)
    return dt, s["H"], s["Se"]


def test_a_changed_column_table_leaves_no_crack_water_behind_and_apply_is_the_setter(product, oracle, pin):
    """Hour A on the full column table, then the same maps on a table in which cells have lost their column or its deep part: a node
    outside this hour's table holds 0.  Then the hand-over: sf3d_sink_compute_hour leaves the solver's state untouched, sf3d_sink_apply
    equals N setter calls, and one computeStep gives the H of the CPU oracle given the same sinks."""
    _need_glibc_set(product)
    shape = (7, 37)
    case, m, state = _small(product, pin, shape)
    before = cm.snapshot(product, m)
    sc.hour(product, case, 0)
    hour_a = kc.outputs(product, m.n)
    _same(hour_a, _wanted(case, 0, state), "hour A")
    after = cm.snapshot(product, m)
    assert np.array_equal(before["H"], after["H"]) and np.array_equal(before["Se"], after["Se"])   # the compute call leaves the state alone
    columns = _changed_columns(case)
    outside = np.ones(m.n, bool)
    outside[columns[columns >= 0]] = False
    inside_a = np.zeros(m.n, bool)
    inside_a[case["columns"][case["columns"] >= 0]] = True
    left = outside & inside_a & (hour_a["sinks"] > 0)
    assert np.count_nonzero(left[m.ns:]) > 20                                                      # soil nodes that leave the table held crack water in hour A
    sinks.set_columns(product, columns, case["layer_thickness"])
    sc.hour(product, case, 0)
    hour_b = kc.outputs(product, m.n)
    stale = outside & (hour_b["sinks"] != 0)
    print(f"{int(stale.sum())} of {int(outside.sum())} nodes outside the new table hold a sink")
    _same(hour_b, _wanted(case, 0, state, columns), "hour B")
    assert not stale.any() and np.count_nonzero(hour_b["sinks"][m.ns:] > 0) > 50
    sinks.apply(product)
    assert np.array_equal(bits(sinks.get_node_sinks(product, m.n)), bits(hour_b["sinks"]))
    dt0 = product.lib.sf3d_compute_step(3600.0)
    s0 = cm.snapshot(product, m)
    q = hour_b["sinks"]

    def setter(lib):
        def feed(m):
            for i in range(m.n):
                lib.lib.sf3d_set_node_water_sink_source(i, float(q[i]))
        return feed
    dt1, h1, se1 = _one_step(product, case, setter(product))
    dt2, h2, _ = _one_step(product, case, lambda m: None)
    assert dt0 == dt1 > 0.0 and np.array_equal(s0["H"], h1) and np.array_equal(s0["Se"], se1)
    assert dt2 > 0.0 and not np.array_equal(h1, h2)                      # the sinks did reach the solver
    dt3, h3, _ = _one_step(oracle, case, setter(oracle), columns=False)      # (the checker has no column table)
    oracle.lib.sf3d_clean()
    assert dt3 == dt1
    assert_water_nodes(h1, h3, "H after one step with the cracked sinks")      # the oracle given the same sinks
    product.lib.sf3d_clean()


def test_two_ranks_merge_to_the_single_rank_sinks_and_maps(product, pin, tmp_path):
    _need_glibc_set(product)
    which = 1
    ranks = mr.run("scripts/multirank_crack_worker.py", 2, kc.PORT, [which], tmp_path, env={"SF3D_BENCH_SHARE_GPU": "1"})
    flag = float(pin["flag"])
    n = len(pin["vwc"])
    owner = mr.cell_owner(ranks, np.arange(n), n)
    cell_owner = mr.cell_owner(ranks, np.arange(pin["dem"].size).reshape(pin["dem"].shape), n)      # a column goes with its surface node
    merged = dict(sinks=mr.merge([res["sinks"] for res in ranks], owner, 0.0, others=0.0, what="sinks"))      # another rank's nodes: 0
    for name in kc.OUTPUTS[1:]:
        merged[name] = mr.merge([res[name] for res in ranks], cell_owner, np.float32(flag) if name == "prec_surface_water" else flag)
        for r, res in enumerate(ranks):
            computed = (cell_owner == r) & (pin["columns"][0] >= 0)
            assert np.all(res[name][~computed] == flag), (name, r)      # another rank's cells: the flag
    _same(merged, {name: pin[name][which] for name in kc.OUTPUTS}, "merged ranks")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crack_host")
    return d, [build_host_program(b, d) for b in sc.HOST_PROGRAMS]


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_device_equals_the_host_build_of_the_same_text(product, pin, host, shape):
    """k_sink_hour_crack against tests/sink_host.cpp, the same sink_cell<true> compiled for the CPU, on the continuous cases of two seeds
    and on the edge cases of the tables, cracking on: node sinks, both actual maps, precSurfaceWater and crackWater of every hour, bit for
    bit, on the H, Se and ponds the device holds.  tests/test_crack_host.py and tests/test_sink_host.py have run these cases under the
    sanitizers and shown that they reach every arm."""
    _need_glibc_set(product)
    directory, exes = host
    cases = [(f"{shape[1]}-{seed}", sc.continuous_case(kc.small_case(pin, shape, seed), seed), False) for seed in sc.SEEDS[:2]]
    if shape == sc.SHAPES[0]:
        cases += [(name, case, one_layer) for name, case, one_layer, crack in sc.edge_cases(sc.load_pin(), pin) if crack]
    for name, case, one_layer in cases:
        state, hours = sc.device_run(product, case, one_layer, crack=True)
        for k, got in enumerate(hours):
            want = sc.run_host(exes, directory, "gpu-" + name, case, k, state, one_layer=one_layer, crack=True)
            print(f"{name}, hour {k}: values differ: {sc.compare_host(got, want['crack'], kc.OUTPUTS, (name, k))}")
        assert any(np.count_nonzero(got["sinks"]) > 0 for got in hours), name                      # some sinks are non-zero
