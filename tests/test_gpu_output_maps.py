"""Output maps on the device (include/sf3d_maps.h, k_output_map): every variable the application maps, on a window of the Ravone project in
its 25 mm hour, against the reference's loops (criteria3d_amd/maps.py restate_*) over per-node getter values - bit for bit on the
product's own getters, and on the oracle's; the kernel did the work; the solver does not notice the call; the error codes; two ranks
sharing the GPU give the single-GPU maps."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, maps
from tests.scenarios import ravone_project_model
from tests.raster_helpers import bits as _bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WINDOW = (980, 1108, 300, 428)          # the catchment's edge, four soils, short BSC columns
STEPS = 300                             # of the 25 mm hour: ponding and runoff cells appear
FLAG = -9999.0


def _restated(model, g, increase_slope=False):
    """variable -> list of float32 maps [layer] (or one whole-column map) from per-node getter values g"""
    index = np.asarray(model.meta["index"])
    thick = [0.0] + list(model.meta["layers"])
    out = {}
    for var in maps.LAYER_VARIABLES:
        out[var] = np.stack([maps.restate_layer_map(index, var, l, g[var], FLAG) for l in range(index.shape[0])])
    tan_a, sin2 = maps.slope_terms(model.meta["slope"], increase_slope)
    geo = maps.node_geotechnics(model)
    args = (tan_a, sin2, geo, g[maps.VOLUMETRIC_WATER_CONTENT], g[maps.DEGREE_OF_SATURATION], g[maps.WATER_MATRIC_POTENTIAL])
    out[maps.FACTOR_OF_SAFETY] = np.stack([maps.restate_fos_map(index, thick, l, *args, flag=FLAG) for l in range(index.shape[0])])
    out[maps.MINIMUM_FACTOR_OF_SAFETY] = maps.restate_minimum_fos(index, thick, *args, flag=FLAG)[None]
    out[maps.AVG_DEGREE_OF_SATURATION] = maps.restate_avg_degree_of_saturation(
        index, thick, g[maps.VOLUMETRIC_WATER_CONTENT], g[maps.MIN_VOLUMETRIC_WATER_CONTENT], g[maps.MAX_VOLUMETRIC_WATER_CONTENT], FLAG)[None]
    return out


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
        want = _restated(m, g_prod, inc)
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


def _ranks(world, port, tmp_path, steps, sparse):
    import os
    outs = [tmp_path / f"maps_r{r}_{port}.npz" for r in range(world)]
    env = {**os.environ, "SF3D_DIST_TIMEOUT_S": os.environ.get("SF3D_DIST_TIMEOUT_S", "60"), "SF3D_TEST_SPARSE_BUILD": "1" if sparse else "0"}
    procs = [subprocess.Popen([sys.executable, str(ROOT / "scripts" / "multirank_maps_worker.py"), str(r), str(world), str(port), str(steps),
                               str(outs[r])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(pr.returncode == 0 for pr in procs), "\n".join(logs)
    return [np.load(o) for o in outs]


@pytest.mark.parametrize("sparse,port", [(False, 29751), (True, 29753)])
def test_two_ranks_merge_to_the_single_gpu_maps(product, tmp_path, sparse, port):
    steps = 150
    ranks = _ranks(2, port, tmp_path, steps, sparse)
    m = ravone_project_model((980, 1060, 330, 420))
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)
    cm.run_hour(product, m, 25.0, max_steps=steps)
    maps.set_output(product, m)
    single = {var: maps.output_maps(product, m, var, flag=FLAG) for var in maps.LAYER_VARIABLES + (maps.FACTOR_OF_SAFETY,) + maps.COLUMN_VARIABLES}
    g_single = maps.node_getter_values(product, m.n)
    product.lib.sf3d_clean()
    owner = np.full(m.n, 255, np.int64)                   # (a strip-local build knows the owner of the nodes it staged only)
    for r, res in enumerate(ranks):
        owner[res["owner"] == r] = r
    assert np.all(owner < 2)
    index = np.asarray(m.meta["index"])
    first = np.where(index[0] >= 0, index[0], index.max(axis=0))               # a column's owner is its surface node's
    cell_owner = np.where(first >= 0, owner[np.maximum(first, 0)], 255)
    g = {var: np.full(m.n, np.nan) for var in maps.GETTERS}
    for r, res in enumerate(ranks):
        for var in maps.GETTERS:
            g[var][res["mine"]] = res[f"get_{var}"]
    want = _restated(m, g)
    for var, s in single.items():
        merged = np.full(s.shape, np.float32(FLAG), np.float32)
        for r, res in enumerate(ranks):
            mp = res[f"map_{var}"]
            assert np.all(mp[:, cell_owner != r] == np.float32(FLAG)), (var, r)          # another rank's cells: the flag
            merged[:, cell_owner == r] = mp[:, cell_owner == r]
        assert np.array_equal(_bits(merged), _bits(want[var])), var                       # each rank's maps: its own state, restated
        assert np.array_equal(merged == np.float32(FLAG), s == np.float32(FLAG)), var
        if all(np.array_equal(g[v], g_single[v]) for v in maps.GETTERS):                  # the same state: the single-GPU maps' bits
            assert np.array_equal(_bits(merged), _bits(s)), var
        else:
            np.testing.assert_allclose(merged, s, rtol=2e-6, atol=1e-6, err_msg=str(var))
