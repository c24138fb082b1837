"""Root length, depth, first / last root layer and root density on the device (include/sf3d_root.h, k_root_cell / k_root_table /
k_root_gather) against the compiled-reference pin tests/golden/root_density.npz: every output of every degree-day map bit for bit, zero
cells excluded; degreeDays == NULL reads the crop block's map; rasters with a partial block, less than a wave and a single row against
the restatement; sf3d_clean and re-initialise; the solver does not notice the calls; two ranks sharing the GPU merge to the single-rank
maps; the error codes; the device against the host build of the same text (tests/root_host.cpp) on random rasters and on the edges of
the tables, bit for bit."""
import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, crop, root
from tests import ranks as mr
from tests import root_cases as rc
from tests.raster_helpers import bits, build_host_program, differing, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return rc.load_pin()


def _same(got, want, what):
    for n in rc.OUTPUTS:
        bad = bits(got[n]) != bits(want[n])
        print(f"{what} {n}: {int(bad.sum())} values differ")
        assert not bad.any(), (what, n, int(bad.sum()), got[n][bad][:4], want[n][bad][:4])


def test_every_output_of_every_map_equals_the_pin(product, pin):
    _need_glibc_set(product)
    rc.initialize(product, pin)
    flag = float(pin["flag"])
    first = root.all_maps(product)
    assert np.all(first["length"] == flag) and np.all(first["density"] == flag) and np.all(first["first"] == int(flag))      # before the first compute: the flag
    for k in range(len(pin["degree_days"])):
        root.compute(product, pin["degree_days"][k])
        got = root.all_maps(product)
        _same(got, {n: pin[n][k] for n in rc.OUTPUTS}, f"map {k}")
        for layer in (0, 5, len(pin["layer_depth"]) - 1):                   # the one-layer getter
            assert np.array_equal(bits(root.get_density(product, layer)), bits(pin["density"][k][layer])), (k, layer)
        keys = root.get_keys(product)
        assert np.array_equal(keys >= 0, pin["length"][k] != flag) and keys.max() < root.table_rows(product)
    # the keyed form: far fewer distinct density vectors than computed cells
    assert len(np.unique(keys[keys >= 0])) < int((keys >= 0).sum()) // 4
    root.clean(product)


def test_null_degree_days_read_the_crop_block(product, pin):
    _need_glibc_set(product)
    dem, flag = pin["dem"], float(pin["flag"])
    n = dem.size
    root.bind(product); crop.bind(product)
    lib = product.lib
    crop.clean(product)
    rc.initialize(product, pin)
    assert lib.sf3d_root_compute(n, None) == capi.PARAMETER_ERROR                                   # no crop block
    units = [dict(type=crop.TREE, isCrop=1, sowingDoy=-9999, plantCycle=365, LAImin=1.0, LAImax=4.0, LAIgrass=0.0, LAIcurve_a=4.1, LAIcurve_b=-0.014,
                  thermalThreshold=0.0, upperThermalThreshold=35.0, degreeDaysIncrease=2500, degreeDaysDecrease=1000, degreeDaysEmergence=0)] * len(pin["unit_list"])
    crop.initialize(product, dem[:, :16], pin["crop_index"][:, :16], units, 44.5, flag)             # another raster
    assert lib.sf3d_root_compute(n, None) == capi.PARAMETER_ERROR
    crop.initialize(product, dem.reshape(32, 24), pin["crop_index"].reshape(32, 24), units, 44.5, flag)      # as many cells, other rows x columns
    assert lib.sf3d_root_compute(n, None) == capi.PARAMETER_ERROR
    every = np.where(pin["crop_index"] < 0, 0, pin["crop_index"])                                   # the crop block keeps degree days on its own crop cells: all of them
    crop.initialize(product, dem, every, units, 44.5, flag)
    k = 2
    crop.set_degree_days(product, pin["degree_days"][k], 150)
    dd = crop.get_state(product, "degreeDays")
    lai = crop.get_state(product, "lai")
    root.compute(product, dd)
    uploaded = root.all_maps(product)
    root.compute(product, np.full(dem.shape, flag, np.float32))                                     # forget
    assert np.all(root.get_length(product) == flag)
    root.compute(product, None)
    _same(root.all_maps(product), uploaded, "NULL form")
    _same(uploaded, {m: pin[m][k] for m in rc.OUTPUTS}, "crop block's map")                         # the crop block holds the map on every cell root computes
    assert np.array_equal(crop.get_state(product, "degreeDays"), dd) and np.array_equal(crop.get_state(product, "lai"), lai)      # crop's maps are untouched
    crop.clean(product)
    assert lib.sf3d_root_compute(n, None) == capi.PARAMETER_ERROR
    root.clean(product)


@pytest.mark.parametrize("shape", [(7, 37), (3, 11), (1, 300)])
def test_other_raster_shapes_against_the_restatement(product, pin, shape):
    """259 cells: one block plus three lanes; 33 cells: less than a wave; one row of 300: a partial second block"""
    _need_glibc_set(product)
    dem, ci, si, dd = rc.small_raster(pin, shape, seed=shape[1])
    rc.initialize(product, pin, dem, ci, si)
    root.compute(product, dd)
    got = root.all_maps(product)
    want = root.restate_root_maps(dem, ci, si, pin["unit_list"], pin["soil_list"], pin["layer_depth"], pin["layer_thickness"], dd, float(pin["flag"]))
    _same(got, want, f"raster {shape}")
    assert got["length"].flat[-1] > 0 and got["density"][:, -1, -1].max() > 0 and got["length"].flat[0] == float(pin["flag"])
    root.clean(product)


def test_clean_and_reinitialise(product, pin):
    _need_glibc_set(product)
    n = pin["dem"].size
    buf = np.zeros(n, np.float64)
    rc.initialize(product, pin)
    root.compute(product, pin["degree_days"][1])
    before = root.all_maps(product)
    m = cm.catchment_model(16, 16, 4)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)                                   # sf3d_initialize inside: the root state survives it
    _same(root.all_maps(product), before, "after sf3d_initialize")
    product.lib.sf3d_clean()
    assert product.lib.sf3d_root_get_length(n, buf.ctypes.data_as(root.pf64)) == capi.MEMORY_ERROR
    assert product.lib.sf3d_root_table_rows() == 0
    rc.initialize(product, pin, pin["dem"][:, :20], pin["crop_index"][:, :20], pin["soil_index"][:, :20])      # another raster first
    rc.initialize(product, pin)
    root.compute(product, pin["degree_days"][1])
    _same(root.all_maps(product), before, "re-initialised")
    root.clean(product)
    assert product.lib.sf3d_root_get_length(n, buf.ctypes.data_as(root.pf64)) == capi.MEMORY_ERROR


def test_root_calls_leave_the_solver_untouched(product, pin):
    """C2 in its F20 hour, a root call and its getters between every two computeSteps: H, Se and the work counters of the run without"""
    def run(with_root):
        m = cm.catchment_model(64, 64, 10)
        product.check(product.lib.sf3d_reset_solver_state(), "reset")
        cm.build(product, m, threads=1)
        if with_root:
            rc.initialize(product, pin)
        product.set_sink_source_bulk(0, np.full(m.ns, cm.rain_rate(20.0, m.cell_area)))
        t, k = 0.0, 0
        while t < 3600.0:
            dt = product.lib.sf3d_compute_step(3600.0 - t)
            assert dt > 0.0
            t += dt
            if with_root:
                root.compute(product, pin["degree_days"][k % len(pin["degree_days"])])
                if k % 5 == 0:
                    root.get_density(product, -1)
                    root.get_layers(product)
            k += 1
        s, c = cm.snapshot(product, m), product.counters()
        if with_root:
            assert np.count_nonzero(root.get_length(product) > 0) > 0
        product.lib.sf3d_clean()
        return s, c
    (s0, c0), (s1, c1) = run(False), run(True)
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"])
    assert c0 == c1


def test_two_ranks_merge_to_the_single_rank_maps(product, pin, tmp_path):
    _need_glibc_set(product)
    which = 2
    ranks = mr.run("scripts/multirank_root_worker.py", 2, mr.PORTS["root"], [which], tmp_path)
    rows, cols = pin["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = float(pin["flag"])
    single = {n: pin[n][which] for n in rc.OUTPUTS}                       # what the single rank gives (the first test): the pin
    others = dict(length=flag, density=flag, first=int(flag), last=int(flag))      # another rank's cells: the flag
    merged = {n: mr.merge([res[n] for res in ranks], cell_owner, flag, others=others.get(n), what=n) for n in rc.OUTPUTS}
    mr.merge([res["keys"] for res in ranks], cell_owner, -1, others=-1, what="keys")
    assert all(merged[n].shape == single[n].shape and merged[n].dtype == single[n].dtype for n in rc.OUTPUTS)
    _same(merged, single, "merged ranks")
    assert np.count_nonzero(merged["length"] > 0) > 300


def test_error_paths(product, pin):
    root.bind(product)
    lib = product.lib
    n = pin["dem"].size
    nl = len(pin["layer_depth"])
    buf = np.zeros(n * nl, np.float64)
    d = buf.ctypes.data_as(root.pf64)
    i = np.zeros(n, np.int32)
    pi = i.ctypes.data_as(root.pi32)
    f = np.zeros(n, np.float32)
    pf = f.ctypes.data_as(root.pf32)
    lib.sf3d_root_clean()
    assert lib.sf3d_root_compute(n, pf) == capi.MEMORY_ERROR and lib.sf3d_root_get_density(0, n, d) == capi.MEMORY_ERROR
    units = list(pin["unit_list"])
    with pytest.raises(capi.SF3DError):
        root.initialize(product, pin["dem"], pin["crop_index"], pin["soil_index"], units[:3], pin["soil_list"], pin["layer_depth"], pin["layer_thickness"])      # a crop index >= nUnits
    with pytest.raises(capi.SF3DError):
        root.initialize(product, pin["dem"], pin["crop_index"], pin["soil_index"], units, pin["soil_list"][:2], pin["layer_depth"], pin["layer_thickness"])       # a soil index >= nSoils
    assert lib.sf3d_root_get_length(n, d) == capi.MEMORY_ERROR                                       # a refused initialise leaves no raster
    root.initialize(product, pin["dem"], pin["crop_index"] % 2, pin["soil_index"], (units * 8)[:root.MAX_UNITS], pin["soil_list"], pin["layer_depth"],
                    pin["layer_thickness"])                                                          # the unit cap itself
    rc.initialize(product, pin)
    assert lib.sf3d_root_compute(n - 1, pf) == capi.PARAMETER_ERROR                                  # wrong size
    assert lib.sf3d_root_get_length(n + 1, d) == capi.PARAMETER_ERROR and lib.sf3d_root_get_depth(n // 2, d) == capi.PARAMETER_ERROR
    assert lib.sf3d_root_get_layers(n - 1, pi, pi) == capi.PARAMETER_ERROR and lib.sf3d_root_get_keys(n - 1, pi) == capi.PARAMETER_ERROR
    assert lib.sf3d_root_get_density(0, n - 1, d) == capi.PARAMETER_ERROR
    assert lib.sf3d_root_get_length(n, None) == capi.PARAMETER_ERROR and lib.sf3d_root_get_layers(n, pi, None) == capi.PARAMETER_ERROR      # null pointer
    assert lib.sf3d_root_get_density(nl, n, d) == capi.INDEX_ERROR and lib.sf3d_root_get_density(-2, n, d) == capi.INDEX_ERROR
    assert lib.sf3d_root_get_density(-1, n, d) == capi.OK and np.all(buf == float(pin["flag"]))     # before the first compute: the flag
    with pytest.raises(ValueError):
        root.compute(product, np.zeros((3, 3), np.float32))
    assert lib.sf3d_root_clean() == capi.OK
    assert lib.sf3d_root_get_length(n, d) == capi.MEMORY_ERROR                                       # after clean


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("root_host")
    return d, build_host_program("root", d)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_of_the_same_text(product, pin, host, shape):
    """k_root_table, k_root_cell and k_root_gather against tests/root_host.cpp, the same root_table_row, root_cell and root_gather_cell
    compiled for the CPU behind the same table builder, on the continuous rasters of two seeds and on the edge cases of the tables: the
    number of table rows, length, depth, first and last root layer, the key, the density of every layer (the rows of the table the cells
    reach) and the one-layer gather of the layers 1, 5 and the last, bit for bit.  tests/test_root_host.py has run these cases under the
    sanitizers and shown that they are not vacuous."""
    _need_glibc_set(product)
    directory, exe = host
    cases = [(f"{shape[1]}-{seed}", rc.random_case(pin, shape, seed)) for seed in rc.SEEDS[:2]]
    if shape == rc.SHAPES[0]:
        cases += list(rc.edge_cases(pin))
    for name, case in cases:
        want = rc.run_host(exe, directory, "gpu-" + name, case)
        nl = len(case["layer_depth"])
        root.initialize(product, case["dem"], case["crop_index"], case["soil_index"], case["unit_list"], case["soil_list"], case["layer_depth"],
                        case["layer_thickness"], float(case["flag"]))
        assert root.table_rows(product) == want["rows"], name
        for k, dd in enumerate(case["degree_days"]):
            root.compute(product, dd)
            got = dict(root.all_maps(product), key=root.get_keys(product))
            for n in rc.OUTPUTS + ("key",):
                g, w = np.asarray(got[n]), want["maps"][k][n]
                bad = differing(g, w.astype(g.dtype))
                print(f"{name} map {k} {n}: values differ: {int(bad.sum())}")
                assert not bad.any(), (name, k, n, int(bad.sum()), g[bad][:4], w[bad][:4])
            for layer in sorted({min(1, nl - 1), min(5, nl - 1), nl - 1}):                  # layer0 > 0, one layer
                assert not differing(root.get_density(product, layer), want["maps"][k]["density"][layer]).any(), (name, k, layer)
        assert np.count_nonzero(want["maps"][0]["length"] > 0) > 0
        root.clean(product)
