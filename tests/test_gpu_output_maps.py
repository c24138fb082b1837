"""Output maps on the device (include/sf3d_maps.h, k_output_map): every variable the application maps, on a window of the Ravone project in
its 25 mm hour, against the reference's loops (criteria3d_amd/maps.py restate_*, gathered in tests/map_cases.py restated) over per-node
getter values - bit for bit on the product's own getters, and on the oracle's; the kernel did the work; the solver does not notice the
call; the error codes; two ranks sharing the GPU give the single-GPU maps.  Off that fixture, on the small ragged rasters of
tests/map_cases.py (7 x 37, 3 x 11 and 1 x 300 cells: a partial block, less than a wave, a single row; the modified and the plain van
Genuchten curve; hand-placed columns for the arms a run does not reach): every map with and without increaseSlope against the restated
loops over the product's getters bit for bit; another flag, one-layer calls against slices of the all-layer call, a call repeated after
another variable; a column table of another size taken up and given back inside one model; geotechnics missing for one deep horizon."""
import copy

import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, maps
from tests import ranks as mr
from tests import map_cases as mpc
from tests import sink_cases as sc
from tests.map_cases import restated as _restated
from tests.scenarios import ravone_project_model
from tests.raster_helpers import bits as _bits, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu
WINDOW = (980, 1108, 300, 428)          # the catchment's edge, four soils, short BSC columns
STEPS = 300                             # of the 25 mm hour: ponding and runoff cells appear
FLAG = -9999.0


def _device(sf, model, increase_slope=False):
    maps.set_slopes(sf, model, increase_slope)
    out = {var: maps.output_maps(sf, model, var, flag=FLAG) for var in maps.LAYER_VARIABLES + maps.COLUMN_VARIABLES}
    out[maps.FACTOR_OF_SAFETY] = maps.output_maps(sf, model, maps.FACTOR_OF_SAFETY, flag=FLAG)
    return out


@pytest.fixture(scope="module")
def window_run(product, oracle):
    m = ravone_project_model(WINDOW)
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=16)
        cm.run_hour(sf, m, 25.0, max_steps=STEPS)
    maps.set_output(product, m)
    dev = {inc: _device(product, m, inc) for inc in (False, True)}
    g_prod = maps.node_getter_values(product, m.n)
    g_ora = maps.node_getter_values(oracle, m.n)
    yield m, dev, g_prod, g_ora
    oracle.lib.sf3d_clean(); product.lib.sf3d_clean()


def test_window_maps_equal_the_restated_loops_bit_for_bit(window_run):
    m, dev, g_prod, g_ora = window_run
    wc = g_prod[maps.VOLUMETRIC_WATER_CONTENT]
    assert np.count_nonzero(wc[:m.ns] > 0) > 0, "no ponding yet"                      # surface water
    assert np.count_nonzero(g_prod[maps.WATER_OUTFLOW] < 0) > 0                          # lateral flow
    print(f"ponded cells {np.count_nonzero(wc[:m.ns] > 0)}, soil nodes with psi > 0 {np.count_nonzero(g_prod[maps.WATER_MATRIC_POTENTIAL][m.ns:] > 0)}")
    for inc in (False, True):
        want = _restated(m, g_prod, FLAG, inc)
        for var, w in want.items():
            got = dev[inc][var]
            assert got.shape == w.shape, (var, got.shape, w.shape)
            bad = np.count_nonzero(_bits(got) != _bits(w))
            assert bad == 0, (var, inc, bad, got[_bits(got) != _bits(w)][:5], w[_bits(got) != _bits(w)][:5])
    fos = dev[False][maps.FACTOR_OF_SAFETY]
    assert np.all(fos[0] == np.float32(FLAG)) and np.count_nonzero(fos[1:] != np.float32(FLAG)) > 10000
    assert not np.array_equal(dev[False][maps.MINIMUM_FACTOR_OF_SAFETY], dev[True][maps.MINIMUM_FACTOR_OF_SAFETY])


def test_window_maps_against_the_oracles_getters(window_run):
    """the same loops over the ORACLE's getters: the two states agree to the trajectory tolerance of tests/tolerances.py, so the float
    maps agree to the bit wherever the states do; flag positions everywhere"""
    m, dev, g_prod, g_ora = window_run
    same_state = all(np.array_equal(g_prod[v], g_ora[v]) for v in maps.GETTERS)
    want = _restated(m, g_ora)
    for var, w in want.items():
        got = dev[False][var]
        assert np.array_equal(got == np.float32(FLAG), w == np.float32(FLAG)), var
        if same_state:
            assert np.array_equal(_bits(got), _bits(w)), var
        else:
            np.testing.assert_allclose(got, w, rtol=2e-6, atol=1e-6 if var in (maps.WATER_INFLOW, maps.WATER_OUTFLOW) else 0, err_msg=str(var))
    print(f"product and oracle per-node getters bit-identical: {same_state}")


def _small(sf):
    m = ravone_project_model()
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1)
    return m


def test_the_map_kernel_runs_once_per_call(product):
    m = _small(product)
    cm.run_hour(product, m, 25.0, max_steps=20)
    maps.set_output(product, m)
    product.check(product.lib.sf3d_kernel_timing(1), "timing")
    try:
        before = product.kernel_stats()["k_output_map"][0]
        maps.output_maps(product, m, maps.DEGREE_OF_SATURATION)
        maps.output_maps(product, m, maps.FACTOR_OF_SAFETY, layers=3)
        after = product.kernel_stats()["k_output_map"]
        assert after[0] == before + 2 and after[1] > 0
    finally:
        product.lib.sf3d_kernel_timing(0)
    product.lib.sf3d_clean()


def test_maps_leave_the_solver_untouched(product):
    def run(take_maps):
        m = _small(product)
        cm.run_hour(product, m, 25.0)
        if take_maps:
            maps.set_output(product, m)
            for var in (maps.FACTOR_OF_SAFETY, maps.WATER_INFLOW, maps.AVAILABLE_WATER_CONTENT, maps.AVG_DEGREE_OF_SATURATION):
                maps.output_maps(product, m, var)
        cm.run_hour(product, m, 0.0)
        s = cm.snapshot(product, m)
        c = product.counters()
        product.lib.sf3d_clean()
        return s, c
    (s0, c0), (s1, c1) = run(False), run(True)
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"])
    assert c0 == c1


def test_error_paths(product):
    out = np.empty(64 * 1024, np.float32)
    p = out.ctypes.data_as(maps.pf32)
    maps.bind(product)
    product.lib.sf3d_clean()
    assert product.lib.sf3d_compute_output_map(0, 0, FLAG, p) == capi.MEMORY_ERROR                  # not initialised
    m = _small(product)
    assert product.lib.sf3d_compute_output_map(0, 0, FLAG, p) == capi.TOPOGRAPHY_ERROR              # no column table
    col, thick = maps.columns(m)
    bad = col.copy(); bad[0, 0] = m.n
    assert product.lib.sf3d_set_output_columns(col.shape[1], col.shape[0], bad.ctypes.data_as(maps.pi32), thick.ctypes.data_as(capi.pd)) == capi.INDEX_ERROR
    assert product.lib.sf3d_set_output_columns(col.shape[1], col.shape[0], col.ctypes.data_as(maps.pi32), thick.ctypes.data_as(capi.pd)) == capi.OK
    cm.run_hour(product, m, 25.0, max_steps=5)
    for var in (-1, 6, 7, 8, 17):
        assert product.lib.sf3d_compute_output_map(var, 0, FLAG, p) == capi.PARAMETER_ERROR, var
    assert product.lib.sf3d_compute_output_map(0, 0, FLAG, None) == capi.PARAMETER_ERROR
    for layer in (-2, col.shape[0]):
        assert product.lib.sf3d_compute_output_map(0, layer, FLAG, p) == capi.INDEX_ERROR, layer
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, 2, FLAG, p) == capi.MISSING_DATA_ERROR        # no slopes
    maps.set_slopes(product, m, False)
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, 2, FLAG, p) == capi.MISSING_DATA_ERROR        # no geotechnics
    assert product.lib.sf3d_compute_output_map(maps.DEGREE_OF_SATURATION, 2, FLAG, p) == capi.OK
    maps.set_output(product, m)
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, 2, FLAG, p) == capi.OK
    product.lib.sf3d_clean()
    assert product.lib.sf3d_compute_output_map(0, 0, FLAG, p) == capi.MEMORY_ERROR


# ------------------------------------------------------------------------------------------------ small ragged rasters (tests/map_cases.py)

ALL_VARIABLES = maps.LAYER_VARIABLES + (maps.FACTOR_OF_SAFETY,) + maps.COLUMN_VARIABLES


@pytest.fixture(scope="module")
def sink_pin():
    return sc.load_pin()


def _small_run(product, pin, shape, curve):
    """a small case after mpc.prepare on the product, its setters called: (case, model, the product's per-node getter values)"""
    case = mpc.small_map_case(pin, shape, seed=shape[1])
    mpc.prepare(product, case, mpc.CURVES[curve])
    m = case["model"]
    maps.set_output(product, m)
    return case, m, maps.node_getter_values(product, m.n)


def _all_maps(product, model, increase_slope=False, flag=FLAG):
    maps.set_slopes(product, model, increase_slope)
    return {var: maps.output_maps(product, model, var, flag=flag) for var in ALL_VARIABLES}


def _same(got, want, what):
    """every variable of `want` bit for bit; the count of differing values per variable is printed first"""
    for var, w in want.items():
        assert got[var].shape == w.shape and got[var].dtype == w.dtype == np.float32, (what, var, got[var].shape, w.shape)
        bad = _bits(got[var]) != _bits(w)
        print(f"{what} variable {var}: {int(bad.sum())} of {w.size} values differ")
    for var, w in want.items():
        bad = _bits(got[var]) != _bits(w)
        assert not bad.any(), (what, var, int(bad.sum()), got[var][bad][:5], w[bad][:5], np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("curve", list(mpc.CURVES))
@pytest.mark.parametrize("shape", mpc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_rasters_equal_the_restated_loops_bit_for_bit(product, sink_pin, shape, curve):
    """259 cells: one block and three lanes; 33: less than a wave, a 64-node chunk straddles two layers and almost every node is an edge
    node; one row of 300: a partial second block.  The yardstick is the product's own per-node getters and numpy (mpc.restated); which
    arms the cases reach is asserted on the CPU oracle in tests/test_output_maps_host.py."""
    _need_glibc_set(product)
    case, m, g = _small_run(product, sink_pin, shape, curve)
    n = m.ns
    flag = np.float32(FLAG)
    for inc in (False, True):
        got = _all_maps(product, m, inc)
        _same(got, _restated(m, g, FLAG, inc), f"raster {shape}, {curve} curve, increaseSlope {inc}:")
        for var, v in got.items():
            v = v.reshape(-1, n)
            assert np.all(v[:, 2] == flag), var                                                     # the valid cell without any node
            if var in (maps.SURFACE_POND, maps.MIN_VOLUMETRIC_WATER_CONTENT, maps.MAX_VOLUMETRIC_WATER_CONTENT):
                continue                                                                            # (defined on one kind of node only)
            assert np.all(v[1 if var == maps.FACTOR_OF_SAFETY else 0:, n - 1] != flag), var         # the last cell, its whole column
        assert np.all(got[maps.FACTOR_OF_SAFETY][0] == flag)
        assert got[maps.SURFACE_POND].reshape(-1, n)[0, n - 1] != flag
        assert np.all(got[maps.MAX_VOLUMETRIC_WATER_CONTENT].reshape(-1, n)[1:, n - 1] != flag)
    product.lib.sf3d_clean()


def test_call_forms_on_7_x_37(product, sink_pin):
    """another flag; one-layer calls of layers 0, 1, 7 and 13 (7 and 13 lie directly under a hole of the hand-placed column) against the
    slices of the all-layer call; the same variable twice with another one between"""
    _need_glibc_set(product)
    case, m, g = _small_run(product, sink_pin, (7, 37), "plain")
    first = _all_maps(product, m)
    _same(first, _restated(m, g, FLAG), "raster (7, 37), flag -9999:")
    other = _all_maps(product, m, flag=-1.0)
    _same(other, _restated(m, g, -1.0), "raster (7, 37), flag -1:")
    for var, v in first.items():
        assert not np.any(v == np.float32(-1.0)), var                       # (no value of the state is the other flag)
        assert np.array_equal(_bits(other[var]), _bits(np.where(v == np.float32(FLAG), np.float32(-1.0), v))), var
    for var in (maps.VOLUMETRIC_WATER_CONTENT, maps.FACTOR_OF_SAFETY, maps.WATER_OUTFLOW):
        for layer in mpc.LAYER_CALLS:
            one = maps.output_maps(product, m, var, layers=layer, flag=FLAG)
            assert one.shape == (1,) + first[var].shape[1:] and np.array_equal(_bits(one[0]), _bits(first[var][layer])), (var, layer)
        several = maps.output_maps(product, m, var, layers=list(reversed(mpc.LAYER_CALLS)), flag=FLAG)
        assert np.array_equal(_bits(several), _bits(first[var][list(reversed(mpc.LAYER_CALLS))])), var
    for var, between in ((maps.WATER_INFLOW, maps.MINIMUM_FACTOR_OF_SAFETY), (maps.FACTOR_OF_SAFETY, maps.AVAILABLE_WATER_CONTENT),
                         (maps.AVG_DEGREE_OF_SATURATION, maps.WATER_DEFICIT)):
        a = maps.output_maps(product, m, var, flag=FLAG)
        maps.output_maps(product, m, between, flag=FLAG)
        b = maps.output_maps(product, m, var, flag=FLAG)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(first[var])), var
    product.lib.sf3d_clean()


def test_a_column_table_of_another_size_is_taken_up(product, sink_pin):
    """the table of the first two raster rows (74 cells of 259) inside the initialised model, then the full one again: the column, slope
    and output buffers on the device shrink and grow with their versions"""
    _need_glibc_set(product)
    case, m, g = _small_run(product, sink_pin, (7, 37), "modified")
    first = _all_maps(product, m)
    _same(first, _restated(m, g, FLAG), "raster (7, 37), full table:")
    sub = copy.copy(m)
    sub.meta = dict(m.meta, index=np.ascontiguousarray(m.meta["index"][:, :2]), slope=np.ascontiguousarray(m.meta["slope"][:2]))
    maps.set_columns(product, *maps.columns(sub))
    out = np.empty(first[maps.FACTOR_OF_SAFETY].size, np.float32)
    p = out.ctypes.data_as(maps.pf32)
    for var, layer in ((maps.FACTOR_OF_SAFETY, 2), (maps.FACTOR_OF_SAFETY, -1), (maps.MINIMUM_FACTOR_OF_SAFETY, -1)):      # the slopes are the full raster's
        assert product.lib.sf3d_compute_output_map(var, layer, FLAG, p) == capi.MISSING_DATA_ERROR, (var, layer)
    before_slopes = maps.output_maps(product, sub, maps.WATER_TOTAL_POTENTIAL, flag=FLAG)                                  # (needs none)
    want = _restated(sub, g, FLAG)
    assert np.array_equal(_bits(before_slopes), _bits(want[maps.WATER_TOTAL_POTENTIAL]))
    for inc in (False, True):
        _same(_all_maps(product, sub, inc), _restated(sub, g, FLAG, inc), f"the first two rows, increaseSlope {inc}:")
    assert want[maps.FACTOR_OF_SAFETY].shape == (14, 2, 37) and np.count_nonzero(want[maps.FACTOR_OF_SAFETY] != np.float32(FLAG)) > 500
    maps.set_columns(product, *maps.columns(m))
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, 2, FLAG, p) == capi.MISSING_DATA_ERROR              # slopes of 74 cells
    again = _all_maps(product, m)
    for var, v in first.items():
        assert np.array_equal(_bits(again[var]), _bits(v)), var
    product.lib.sf3d_clean()


def test_geotechnics_missing_for_one_deep_horizon(product, sink_pin):
    """the third horizon of soil 0 occurs from layer 12 down only.  Without its row, the factor of safety of a layer above it is computed
    and equals the restatement; the all-layer call and the column minimum, which walk through it, are refused.  (computeFactorOfSafety
    reads the horizon of the layer asked for and of every layer above it, never a deeper one.)"""
    _need_glibc_set(product)
    product.lib.sf3d_clean()                                            # (no row left over from a model before)
    case = mpc.small_map_case(sink_pin, (7, 37), seed=37)
    m = case["model"]
    gone = (0, 2)
    layer_of = np.repeat(np.arange(14), m.ns)[m.ns:]
    on_gone = (m.soil_index == gone[0]) & (m.horizon_index == gone[1])
    first_layer = int(layer_of[on_gone].min())
    assert first_layer == 12 and np.count_nonzero(on_gone) > 50
    mpc.prepare(product, case, mpc.CURVES["modified"])
    partial = copy.copy(m)
    partial.meta = dict(m.meta, geotechnics=[row for row in m.meta["geotechnics"] if tuple(row[:2]) != gone])
    assert len(partial.meta["geotechnics"]) == len(m.meta["geotechnics"]) - 1
    maps.set_output(product, partial)
    g = maps.node_getter_values(product, m.n)
    want = _restated(partial, g, FLAG)[maps.FACTOR_OF_SAFETY]
    out = np.empty(want.size, np.float32)
    p = out.ctypes.data_as(maps.pf32)
    for layer in (1, 7, first_layer - 1):
        got = maps.output_maps(product, partial, maps.FACTOR_OF_SAFETY, layers=layer, flag=FLAG)
        assert np.array_equal(_bits(got[0]), _bits(want[layer])) and np.isfinite(want[layer]).all(), layer
        assert np.count_nonzero(got[0] != np.float32(FLAG)) > 200
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, first_layer, FLAG, p) == capi.MISSING_DATA_ERROR
    assert product.lib.sf3d_compute_output_map(maps.FACTOR_OF_SAFETY, -1, FLAG, p) == capi.MISSING_DATA_ERROR
    assert product.lib.sf3d_compute_output_map(maps.MINIMUM_FACTOR_OF_SAFETY, -1, FLAG, p) == capi.MISSING_DATA_ERROR
    assert product.lib.sf3d_compute_output_map(maps.AVG_DEGREE_OF_SATURATION, -1, FLAG, p) == capi.OK      # (reads no geotechnics)
    maps.set_output(product, m)                                                                            # the row given: everything again
    _same({maps.FACTOR_OF_SAFETY: maps.output_maps(product, m, maps.FACTOR_OF_SAFETY, flag=FLAG)},
          {maps.FACTOR_OF_SAFETY: _restated(m, g, FLAG)[maps.FACTOR_OF_SAFETY]}, "with the row:")
    product.lib.sf3d_clean()


@pytest.mark.parametrize("sparse,port", [(False, mr.PORTS["output_maps"][0]), (True, mr.PORTS["output_maps"][1])])
def test_two_ranks_merge_to_the_single_gpu_maps(product, tmp_path, sparse, port):
    steps = 150
    ranks = mr.run("scripts/multirank_maps_worker.py", 2, port, [steps], tmp_path, env={"SF3D_TEST_SPARSE_BUILD": "1" if sparse else "0"})
    m = ravone_project_model((980, 1060, 330, 420))
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)
    cm.run_hour(product, m, 25.0, max_steps=steps)
    maps.set_output(product, m)
    single = {var: maps.output_maps(product, m, var, flag=FLAG) for var in maps.LAYER_VARIABLES + (maps.FACTOR_OF_SAFETY,) + maps.COLUMN_VARIABLES}
    g_single = maps.node_getter_values(product, m.n)
    product.lib.sf3d_clean()
    mr.cell_owner(ranks, np.arange(m.n), m.n)               # every node has an owner (a strip-local build knows the owner of the nodes it staged only)
    index = np.asarray(m.meta["index"])
    first = np.where(index[0] >= 0, index[0], index.max(axis=0))               # a column's owner is its surface node's
    cell_owner = mr.cell_owner(ranks, first, m.n)
    g = {var: np.full(m.n, np.nan) for var in maps.GETTERS}
    for r, res in enumerate(ranks):
        for var in maps.GETTERS:
            g[var][res["mine"]] = res[f"get_{var}"]
    want = _restated(m, g)
    for var, s in single.items():
        merged = mr.merge([res[f"map_{var}"] for res in ranks], cell_owner, np.float32(FLAG), others=np.float32(FLAG), what=f"map_{var}")      # another rank's cells: the flag
        assert merged.shape == s.shape and merged.dtype == np.float32
        assert np.array_equal(_bits(merged), _bits(want[var])), var                       # each rank's maps: its own state, restated
        assert np.array_equal(merged == np.float32(FLAG), s == np.float32(FLAG)), var
        if all(np.array_equal(g[v], g_single[v]) for v in maps.GETTERS):                  # the same state: the single-GPU maps' bits
            assert np.array_equal(_bits(merged), _bits(s)), var
        else:
            np.testing.assert_allclose(merged, s, rtol=2e-6, atol=1e-6, err_msg=str(var))
