"""The hourly water sinks on the device (include/sf3d_sink.h, k_sink_hour) against the compiled-reference pin
tests/golden/water_sinks.npz: node sinks and both actual maps of every hour bit for bit, zero cells excluded, with every map passed in and
with NULL maps read from the crop and snow blocks; the nrLayers = 1 case; sf3d_sink_apply against the node-by-node setter and the compute
call without apply against the run without it (C2's F20 hour); the crop, snow and root blocks undisturbed; two ranks sharing the GPU;
rasters with a partial block, less than a wave and a single row against the restatement, a column table changed between two hours, and the
output maps driven alternately with the sink hour under a table that changes; the device against the host build of the same text
(tests/sink_host.cpp) on continuous cases and on the edges of the tables, bit for bit."""
import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, crop, maps, root, sinks, snow
from tests import ranks as mr
from tests import crop_cases as cc
from tests import root_cases as rc
from tests import sink_cases as sc
from tests.snow_cases import melt_forcing
from tests.raster_helpers import bits as _bits, build_host_program, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return sc.load_pin()


def _model(product, pin):
    m = sc.node_model(pin)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)
    sc.set_state(product, pin, m)
    return m


def _same(got, want, what):
    for name in want:
        bad = _bits(got[name]) != _bits(want[name])
        print(f"{what} {name}: {int(bad.sum())} values differ")
        assert not bad.any(), (what, name, int(bad.sum()), np.asarray(got[name])[bad][:4], np.asarray(want[name])[bad][:4])


def _outputs(product, n):
    e, t = sinks.get_actual(product)
    return dict(sinks=sinks.get_node_sinks(product, n), evaporation=e, transpiration=t)


def test_every_hour_equals_the_pin(product, pin):
    _need_glibc_set(product)
    m = _model(product, pin)
    assert np.array_equal(_bits(product.water_content(0, m.n)), _bits(pin["vwc"]))             # the state the fixture's water contents were read from
    rc.initialize(product, pin)
    sc.initialize(product, pin)
    for k in range(len(pin["et0"])):
        sc.hour(product, pin, k)
        _same(_outputs(product, m.n), {name: pin[name][k] for name in ("sinks", "evaporation", "transpiration")}, f"hour {k}")
    sc.hour(product, pin, 0)                                                                        # an earlier hour again: nothing is left over
    _same(_outputs(product, m.n), {name: pin[name][0] for name in ("sinks", "evaporation", "transpiration")}, "hour 0 again")
    product.lib.sf3d_clean()


def test_one_layer(product, pin):
    _need_glibc_set(product)
    m = _model(product, pin)
    sinks.set_columns(product, pin["columns"][:1], pin["layer_thickness"][:1])
    root.initialize(product, pin["dem"], pin["crop_index"], pin["soil_index"], pin["unit_list"], pin["soil_list"], pin["layer_depth"][:1], pin["layer_thickness"][:1],
                    float(pin["flag"]))
    sc.initialize(product, pin, one_layer=True)
    for j, k in enumerate(int(v) for v in pin["one_layer_hours"]):
        sc.hour(product, pin, k)
        got = _outputs(product, m.n)
        _same(got, dict(sinks=pin["one_layer_sinks"][j], evaporation=pin["one_layer_evaporation"][j], transpiration=pin["one_layer_transpiration"][j]), f"one layer, hour {k}")
        assert not got["sinks"][m.ns:].any() and np.all(got["transpiration"][got["transpiration"] != float(pin["flag"])] == 0)
    product.lib.sf3d_clean()


def test_null_maps_read_the_blocks_and_leave_them_undisturbed(product, pin):
    _need_glibc_set(product)
    m = _model(product, pin)
    dem, flag = pin["dem"], float(pin["flag"])
    k = 3
    rc.initialize(product, pin)
    sc.initialize(product, pin)
    units = cc.load_pin()["unit_list"]
    unit_index = np.where(pin["crop_index"] < 0, 0, pin["crop_index"]) % len(units)
    snow.initialize(product, dem, flag)
    crop.initialize(product, dem, unit_index, units, 44.5, flag)
    for met in melt_forcing(dem.shape, dem, flag)[11:13]:
        snow.compute_hour(product, met)
        crop.compute_hour(product, None)
    crop.set_state(product, "degreeDays", pin["sink_degree_days"][k])
    crop.set_state(product, "lai", pin["lai"][k])
    root.compute(product, None)
    before = dict(snow.all_maps(product)); before.update(crop.all_maps(product)); before.update({"root_" + n: v for n, v in root.all_maps(product).items()})
    et0, liquid = crop.get_et0(product), snow.get_output(product, "liquid")
    assert np.count_nonzero((et0 != flag) & (et0 > 0)) > 300 and np.count_nonzero((liquid != flag) & (liquid > 0)) > 300
    sinks.compute_hour(product, None, None, None, None)
    null_form = _outputs(product, m.n)
    sinks.compute_hour(product, et0, pin["lai"][k], pin["sink_degree_days"][k], liquid)
    _same(null_form, _outputs(product, m.n), "NULL form against the same maps passed in")
    want = sinks.restate_sink_hour(dem, flag, float(pin["cell_size"]), pin["columns"], pin["vwc"], pin["crop_index"], pin["soil_index"], pin["sink_units"], pin["sink_soils"],
                                   pin["layer_depth"], pin["layer_thickness"], float(pin["computation_depth"]), et0, pin["lai"][k], pin["sink_degree_days"][k], liquid,
                                   sc.roots_of(pin, k), m.n)
    _same(null_form, {name: want[name] for name in ("sinks", "evaporation", "transpiration")}, "NULL form against the restatement")
    assert np.count_nonzero(null_form["sinks"][m.ns:] < 0) > 1000 and np.count_nonzero(null_form["sinks"][:m.ns] > 0) > 100
    after = dict(snow.all_maps(product)); after.update(crop.all_maps(product)); after.update({"root_" + n: v for n, v in root.all_maps(product).items()})
    for name, v in before.items():
        assert np.array_equal(v, after[name], equal_nan=True), name
    snow.clean(product); crop.clean(product)
    assert product.lib.sf3d_sink_compute_hour(dem.size, None, None, None, None) == capi.PARAMETER_ERROR
    product.lib.sf3d_clean()


def _small(product, pin, shape):
    """a small case on the device: its node model, potentials and column table, the root and sink blocks on its raster; the water contents the device holds"""
    case = sc.small_case(pin, shape, seed=shape[1])
    m = _model(product, case)
    vwc = product.water_content(0, m.n)
    rc.initialize(product, case, case["dem"], case["crop_index"], case["soil_index"])
    sc.initialize(product, case)
    return case, m, vwc


def _wanted(case, k, vwc, columns=None):
    want = sc.restated_case(case, k, vwc, columns)
    return {name: want[name] for name in ("sinks", "evaporation", "transpiration")}


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_other_raster_shapes_against_the_restatement(product, pin, shape):
    """259 cells: one block plus three lanes; 33 cells: less than a wave; one row of 300: a partial second block.  Two hours with maps of
    their own against restate_sink_hour on the water contents the device holds: nothing of the first hour is left in the second."""
    _need_glibc_set(product)
    case, m, vwc = _small(product, pin, shape)
    flag, n, nl = float(case["flag"]), case["dem"].size, len(case["layer_depth"])
    soil_nodes = sc.soil_nodes_of_computing_cells(case)
    for k in range(len(case["et0"])):
        sc.hour(product, case, k)
        got = _outputs(product, m.n)
        _same(got, _wanted(case, k, vwc), f"raster {shape}, hour {k}")
        e, t = got["evaporation"], got["transpiration"]
        assert e.flat[-1] > 0 and t.flat[-1] > 0                                                    # the last lane computes
        assert e.flat[0] == flag and t.flat[0] == flag and e.flat[n // 2] == flag and t.flat[n // 2] == flag      # flag cells
        assert e.flat[2] == flag and not got["sinks"][np.arange(nl) * n + 2].any()                  # the column left out under a valid cell
        assert not got["sinks"][np.arange(nl) * n].any()                                            # the column under a flag cell
        # (the restatement reaches 0.142 to 0.232 on the host's water contents: sc.SINK_SHARE, tests/test_sink_host.py)
        assert np.count_nonzero(got["sinks"][m.ns:] < 0) >= sc.SINK_SHARE * soil_nodes
    product.lib.sf3d_clean()


def _one_step(product, case, feed):
    """the first computeStep of the case's model after `feed` has handed the sinks over: what the step took, H and Se"""
    m = _model(product, case)
    feed(m)
    dt = product.lib.sf3d_compute_step(3600.0)
    s = cm.snapshot(product, m)
    return dt, s["H"], s["Se"]


def _changed_columns(case):
    """the case's column table on the same layer grid, in which some computing cells have lost their whole column and others their
    nodes from layer 3 down"""
    n, nl = case["dem"].size, len(case["layer_depth"])
    columns = case["columns"].copy().reshape(nl, n)
    computing = np.flatnonzero(sc.computing_cells(case).ravel())
    columns[:, computing[1::5]] = -1                                      # the whole column gone
    columns[3:, computing[3::5]] = -1                                     # the nodes from layer 3 down gone
    columns[3:, 7:9] = -1                                                 # (the trees whose deep layers transpire)
    return columns.reshape(case["columns"].shape)


def test_a_changed_column_table_leaves_no_sinks_behind(product, pin):
    """Hour A on the full column table, then the same maps on a table of the same layer grid in which some computing cells have lost
    their whole column and others their nodes from layer 3 down: a node outside this hour's table holds 0, as the reference starts
    every hour with waterSinkSource = 0 in every node (runModelHour); and what sf3d_sink_apply hands to the solver is that array."""
    _need_glibc_set(product)
    shape = (7, 37)
    case, m, vwc = _small(product, pin, shape)
    sc.hour(product, case, 0)
    hour_a = _outputs(product, m.n)
    _same(hour_a, _wanted(case, 0, vwc), "hour A")
    columns = _changed_columns(case)
    outside = np.ones(m.n, bool)
    outside[case["columns"][case["columns"] >= 0]] = False
    was_outside = outside.copy()
    outside[:] = True
    outside[columns[columns >= 0]] = False
    left = outside & ~was_outside & (hour_a["sinks"] != 0)
    assert np.count_nonzero(left) > 100 and np.count_nonzero(left[:m.ns]) > 10      # the nodes that leave the table held sinks in hour A
    sinks.set_columns(product, columns, case["layer_thickness"])
    sc.hour(product, case, 0)
    hour_b = _outputs(product, m.n)
    stale = outside & (hour_b["sinks"] != 0)
    print(f"{int(stale.sum())} of {int(outside.sum())} nodes outside the new table hold a sink", hour_b["sinks"][stale][:3], np.flatnonzero(stale)[:3])
    _same(hour_b, _wanted(case, 0, vwc, columns), "hour B")
    assert not stale.any() and np.count_nonzero(hour_b["sinks"]) > 300
    # the hand-over: apply leaves the array as it is, and the solver steps as after the node-by-node setter
    sinks.apply(product)
    assert np.array_equal(_bits(sinks.get_node_sinks(product, m.n)), _bits(hour_b["sinks"]))
    dt0 = product.lib.sf3d_compute_step(3600.0)
    s0 = cm.snapshot(product, m)
    q = hour_b["sinks"]

    def setter(m):
        for i in range(m.n):
            product.lib.sf3d_set_node_water_sink_source(i, float(q[i]))
    dt1, h1, se1 = _one_step(product, case, setter)
    dt2, h2, se2 = _one_step(product, case, lambda m: None)
    assert dt0 == dt1 > 0.0 and np.array_equal(s0["H"], h1) and np.array_equal(s0["Se"], se1)
    assert dt2 > 0.0 and not np.array_equal(h1, h2)                      # the sinks did reach the solver
    product.lib.sf3d_clean()


@pytest.mark.parametrize("shape", ((3, 11), (7, 37)))
def test_output_maps_and_sinks_share_one_column_table_on_the_device(product, pin, shape):
    """The output maps and the sink hour upload the column table through one function and keep one version of it on the device.  Driven
    alternately - map, sink hour, map, another table, sink hour, map - each call works on the table in force: the sinks equal the
    restatement on it, a map is not disturbed by the sink hour between two of them, and the map after the change holds the flag exactly
    where the new table has no node and the earlier bits wherever both tables name the same node."""
    _need_glibc_set(product)
    case, m, vwc = _small(product, pin, shape)
    flag = np.float32(maps.NODATA)
    water_content = lambda: maps.output_maps(product, m, maps.VOLUMETRIC_WATER_CONTENT)
    first = water_content()
    sc.hour(product, case, 0)
    _same(_outputs(product, m.n), _wanted(case, 0, vwc), f"raster {shape}, the case's table")
    second = water_content()
    assert np.array_equal(_bits(first), _bits(second))
    assert np.array_equal(first == flag, case["columns"] < 0)
    columns = _changed_columns(case)
    gone = (columns < 0) & (case["columns"] >= 0)
    assert np.count_nonzero(gone) > 100                                  # the change takes nodes away
    sinks.set_columns(product, columns, case["layer_thickness"])
    sc.hour(product, case, 1)
    _same(_outputs(product, m.n), _wanted(case, 1, vwc, columns), f"raster {shape}, the changed table")
    third = water_content()
    print(f"raster {shape}: {int(np.count_nonzero(gone))} nodes left the table, {int(np.count_nonzero(third == flag))} flag values in the third map")
    assert np.array_equal(third == flag, columns < 0)
    same_node = (columns >= 0) & (columns == case["columns"])
    assert np.array_equal(_bits(third)[same_node], _bits(first)[same_node]) and np.count_nonzero(same_node) > columns.size // 3
    product.lib.sf3d_clean()


def _c2_run(product, pin, mode):
    """C2 in its F20 hour with the column table of its own grid; mode: "none", "apply" (compute + apply before every step), "setter" (the
    downloaded array through sf3d_set_node_water_sink_source node by node), "compute" (compute without apply between every two steps)"""
    m = cm.catchment_model(32, 24, 14)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)
    if mode != "none":
        cols = np.asarray(m.meta["index"]).astype(np.int32)
        sinks.set_columns(product, cols, pin["layer_thickness"])
        rc.initialize(product, pin)
        sc.initialize(product, pin)
    rain = np.zeros(m.n)
    rain[:m.ns] = cm.rain_rate(20.0, m.cell_area)
    product.set_sink_source_bulk(0, rain)
    t, k = 0.0, 0
    while t < 3600.0 and k < 40:
        if mode in ("apply", "setter"):
            sc.hour(product, pin, k % len(pin["et0"]))
            if mode == "apply":
                sinks.apply(product)
            else:
                q = sinks.get_node_sinks(product, m.n)
                for i in range(m.n):
                    product.lib.sf3d_set_node_water_sink_source(i, float(q[i]))
        dt = product.lib.sf3d_compute_step(3600.0 - t)
        assert dt > 0.0
        t += dt
        if mode == "compute":
            sc.hour(product, pin, k % len(pin["et0"]))
            sinks.get_node_sinks(product, m.n)
        k += 1
    s, c = cm.snapshot(product, m), product.counters()
    product.lib.sf3d_clean()
    return s, c


def test_apply_is_the_setter_and_compute_leaves_the_solver_untouched(product, pin):
    (s0, c0), (s1, c1) = _c2_run(product, pin, "apply"), _c2_run(product, pin, "setter")
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"]) and c0 == c1
    (s2, c2), (s3, c3) = _c2_run(product, pin, "none"), _c2_run(product, pin, "compute")
    assert np.array_equal(s2["H"], s3["H"]) and np.array_equal(s2["Se"], s3["Se"]) and c2 == c3
    assert not np.array_equal(s0["H"], s2["H"])                   # the sinks did reach the solver


def test_two_ranks_merge_to_the_single_rank_sinks(product, pin, tmp_path):
    _need_glibc_set(product)
    which = 4
    ranks = mr.run("scripts/multirank_sink_worker.py", 2, mr.PORTS["sink"], [which], tmp_path, env={"SF3D_BENCH_SHARE_GPU": "1"})
    flag = float(pin["flag"])
    n = len(pin["vwc"])
    owner = mr.cell_owner(ranks, np.arange(n), n)
    cell_owner = mr.cell_owner(ranks, np.arange(pin["dem"].size).reshape(pin["dem"].shape), n)      # a column goes with its surface node
    merged = dict(sinks=mr.merge([res["sinks"] for res in ranks], owner, 0.0, others=0.0, what="sinks"))      # another rank's nodes: 0
    for name in ("evaporation", "transpiration"):
        merged[name] = mr.merge([res[name] for res in ranks], cell_owner, flag)
        for r, res in enumerate(ranks):
            computed = (cell_owner == r) & (pin["columns"][0] >= 0)
            assert np.all(res[name][~computed] == flag), (name, r)      # another rank's cells: the flag
    assert [a.shape for a in merged.values()] == [(n,), pin["dem"].shape, pin["dem"].shape] and all(a.dtype == np.float64 for a in merged.values())
    _same(merged, {name: pin[name][which] for name in ("sinks", "evaporation", "transpiration")}, "merged ranks")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("sink_host")
    return d, [build_host_program(b, d) for b in sc.HOST_PROGRAMS]


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_device_equals_the_host_build_of_the_same_text(product, pin, host, shape):
    """k_sink_hour (behind k_root_table, k_root_cell) against tests/sink_host.cpp fed by tests/root_host.cpp, the same sink_cell<false>
    compiled for the CPU, on the continuous cases of two seeds and on the edge cases of the tables, cracking off: node sinks and both
    actual maps of every hour, bit for bit, on the H and Se the device's getters return.  tests/test_sink_host.py has run these cases
    under the sanitizers and shown that they reach every arm.  (The ownership mask is reached through the rank launcher only: the two-rank
    tests hold it.)"""
    _need_glibc_set(product)
    from tests import crack_cases as kc
    directory, exes = host
    cases = [(f"{shape[1]}-{seed}", sc.continuous_case(sc.small_case(pin, shape, seed), seed), False) for seed in sc.SEEDS[:2]]
    if shape == sc.SHAPES[0]:
        cases += [(name, case, one_layer) for name, case, one_layer, crack in sc.edge_cases(pin, kc.load_pin())]
    for name, case, one_layer in cases:
        state, hours = sc.device_run(product, case, one_layer)
        for k, got in enumerate(hours):
            want = sc.run_host(exes, directory, "gpu-" + name, case, k, state, one_layer=one_layer)
            print(f"{name}, hour {k}: values differ: {sc.compare_host(got, want['plain'], ('sinks', 'evaporation', 'transpiration'), (name, k))}")
        assert any(np.count_nonzero(got["sinks"]) > 0 for got in hours), name                      # some sinks are non-zero
