"""The hourly snow model on the device (include/sf3d_snow.h, k_snow_hour) against the compiled-reference pin tests/golden/snow_brooks.npz:
all thirteen maps after every checkpoint hour bit for bit, zero cells excluded; the same run interrupted at hour 48 through get_state /
set_state and through the application's snow/ state folder; the solver does not notice the calls; a melt hour's liquid water drives the
product and the oracle to the same state; two ranks sharing the GPU merge to the single-rank maps; the error codes; rasters with a
partial block, less than a wave and a single row, and a parameter set away from the defaults, against the restatement; and the device against the host build of the same
text (tests/snow_host.cpp) on continuous forcing, bit for bit."""
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, maps, snow
from tests import ranks as mr
from tests import tolerances
from tests.scenarios import ravone_project_model
from tests import snow_cases
from tests.snow_cases import melt_forcing
from tests.raster_helpers import bits as _bits, build_host_program, differing, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "snow_brooks.npz"
WINDOW = (980, 1108, 300, 428)          # the 128 x 128 project window of the output-map tests


@pytest.fixture(scope="module")
def pin():
    z = np.load(PIN)
    return {k: z[k] for k in z.files}


def _meteo(pin, h):
    m = {n: pin["inputs"][h, k] for k, n in enumerate(snow.INPUT)}
    m["clearSkyTransmissivity"] = float(pin["clear_sky"])
    return m


def _start(product, pin):
    flag = float(pin["flag"])
    snow.initialize(product, pin["dem"], flag)
    edit = pin["swe_edit"]
    swe = snow.get_state(product, "swe")
    snow.set_state(product, "swe", np.where(edit == np.float32(flag), swe, edit))      # the hand-edited SWE map of the pin, no reset
    edit = pin["surface_temp_edit"]
    snow.set_state(product, "surfaceTemp", np.where(edit == np.float32(flag), snow.get_state(product, "surfaceTemp"), edit))


def _compare(product, pin, k, what):
    names = [str(n) for n in pin["map_names"]]
    got = snow.all_maps(product)
    for j, n in enumerate(names):
        want = pin["maps"][k][j]
        bad = _bits(got[n]) != _bits(want)
        print(f"{what} hour {int(pin['checkpoints'][k])} {n}: {int(bad.sum())} cells differ")
        assert not bad.any(), (what, int(pin["checkpoints"][k]), n, int(bad.sum()), got[n][bad][:4], want[bad][:4])


def test_initial_maps_equal_the_reference(product, pin):
    snow.initialize(product, pin["dem"], float(pin["flag"]))
    got = snow.all_maps(product)
    for j, n in enumerate(str(n) for n in pin["map_names"][:12]):
        assert np.array_equal(_bits(got[n]), _bits(pin["initial"][j])), n
    snow.clean(product)


def test_all_thirteen_maps_equal_the_pin_at_every_checkpoint(product, pin):
    _need_glibc_set(product)
    _start(product, pin)
    cps = [int(c) for c in pin["checkpoints"]]
    for h in range(int(cps[-1])):
        snow.compute_hour(product, _meteo(pin, h))
        if h + 1 in cps:
            _compare(product, pin, cps.index(h + 1), "uninterrupted")
    snow.clean(product)


@pytest.mark.parametrize("how", ["get_set_state", "state_directory"])
def test_interrupted_run_equals_the_uninterrupted_one(product, pin, tmp_path, how):
    _need_glibc_set(product)
    _start(product, pin)
    for h in range(48):
        snow.compute_hour(product, _meteo(pin, h))
    header = dict(xllcorner=0.0, yllcorner=0.0, cellsize=4.0, nodata=float(pin["flag"]))
    if how == "get_set_state":
        saved = {n: snow.get_state(product, n) for n in snow.STATE}
    else:
        d = snow.save_snow_state(product, tmp_path, header)
        assert sorted(p.name for p in d.iterdir()) == sorted(f"{s}{e}" for s in snow.STATE_FILES.values() for e in (".flt", ".hdr"))
    snow.clean(product)
    snow.initialize(product, pin["dem"], float(pin["flag"]))
    if how == "get_set_state":
        for n, v in saved.items():
            snow.set_state(product, n, v)
    else:
        snow.load_snow_state(product, tmp_path)
    cps = [int(c) for c in pin["checkpoints"]]
    for h in range(48, 96):
        snow.compute_hour(product, _meteo(pin, h))
        if h + 1 in cps:
            _compare(product, pin, cps.index(h + 1), how)
    snow.clean(product)


def test_snow_calls_leave_the_solver_untouched(product, pin):
    """C2 in its F20 hour, a snow hour between every two computeSteps: H, Se and the work counters of the run without"""
    def run(with_snow):
        m = cm.catchment_model(64, 64, 10)
        product.check(product.lib.sf3d_reset_solver_state(), "reset")
        cm.build(product, m, threads=1)
        if with_snow:
            _start(product, pin)
        product.set_sink_source_bulk(0, np.full(m.ns, cm.rain_rate(20.0, m.cell_area)))
        t, k = 0.0, 0
        while t < 3600.0:
            dt = product.lib.sf3d_compute_step(3600.0 - t)
            assert dt > 0.0
            t += dt
            if with_snow:
                snow.compute_hour(product, _meteo(pin, k % 96))
                if k % 5 == 0:
                    snow.get_output(product, "liquid")
            k += 1
        s, c = cm.snapshot(product, m), product.counters()
        if with_snow:
            assert np.count_nonzero(snow.get_state(product, "swe") > 0) > 0
        product.lib.sf3d_clean()
        return s, c
    (s0, c0), (s1, c1) = run(False), run(True)
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"])
    assert c0 == c1


def test_snow_state_survives_sf3d_initialize_and_goes_with_sf3d_clean(product, pin):
    _start(product, pin)
    snow.compute_hour(product, _meteo(pin, 0))
    before = snow.get_state(product, "surfaceTemp")
    m = cm.catchment_model(16, 16, 4)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)                                   # sf3d_initialize inside
    assert np.array_equal(_bits(snow.get_state(product, "surfaceTemp")), _bits(before))
    product.lib.sf3d_clean()
    out = np.empty(before.size, np.float32)
    assert product.lib.sf3d_snow_get_state(0, out.size, out.ctypes.data_as(snow.pf32)) == capi.MEMORY_ERROR


def test_melt_hour_drives_product_and_oracle_to_the_same_state(product, oracle):
    m = ravone_project_model(WINDOW)
    idx = np.asarray(m.meta["index"])[0]
    flag = -9999.0
    dem = np.where(idx >= 0, m.z[np.maximum(idx, 0)], flag).astype(np.float32)
    snow.initialize(product, dem, flag)
    for met in melt_forcing(dem.shape, dem, flag):
        snow.compute_hour(product, met)
    liquid, melt = snow.get_output(product, "liquid"), snow.get_output(product, "snowMelt")
    assert np.count_nonzero(melt[idx >= 0] > 0) > 0.9 * np.count_nonzero(idx >= 0)
    assert np.all(liquid[idx < 0] == np.float32(flag))
    q = snow.surface_sources(m, liquid, flag)
    assert np.count_nonzero(q) == np.count_nonzero((idx >= 0) & (liquid > 0)) and np.all(q[m.ns:] == 0)
    snow.clean(product)
    snaps = []
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=16)
        cm.run_hour_sinks(sf, m, q, max_steps=150)
        snaps.append(cm.snapshot(sf, m))
        sf.lib.sf3d_clean()
    tolerances.assert_water_nodes(snaps[0]["H"], snaps[1]["H"], "H after the melt hour")
    tolerances.assert_water_nodes(snaps[0]["Se"], snaps[1]["Se"], "Se after the melt hour")


def test_two_ranks_merge_to_the_single_rank_maps(product, tmp_path):
    hours = 16
    ranks = mr.run("scripts/multirank_snow_worker.py", 2, mr.PORTS["snow"], [hours], tmp_path)
    m = ravone_project_model((980, 1060, 330, 420))
    idx = np.asarray(m.meta["index"])[0]
    flag = -9999.0
    dem = np.where(idx >= 0, m.z[np.maximum(idx, 0)], flag).astype(np.float32)
    snow.initialize(product, dem, flag)
    for met in melt_forcing(dem.shape, dem, flag)[:hours]:
        snow.compute_hour(product, met)
    single = snow.all_maps(product)
    snow.clean(product)
    cell_owner = mr.cell_owner(ranks, idx, m.n)
    for n in snow.OUTPUT:
        merged = mr.merge([res[n] for res in ranks], cell_owner, np.float32(flag), others=np.float32(flag), what=n)      # another rank's cells: the flag
        assert merged.shape == dem.shape and merged.dtype == np.float32 and np.array_equal(_bits(merged), _bits(single[n])), n
    for n in snow.STATE:
        for r, res in enumerate(ranks):
            mine = cell_owner == r
            assert np.array_equal(_bits(res[n][mine]), _bits(single[n][mine])), (n, r)
            assert np.array_equal(_bits(res[n][~mine]), _bits(ranks[r]["initial_" + n][~mine])), (n, r)      # untouched elsewhere


def _same_maps(got, want, what):
    for n in snow.STATE + snow.OUTPUT:
        bad = _bits(got[n]) != _bits(want[n])
        print(f"{what} {n}: {int(bad.sum())} cells differ")
        assert not bad.any(), (what, n, int(bad.sum()), got[n][bad][:4], want[n][bad][:4])


@pytest.mark.parametrize("shape", snow_cases.SHAPES)
def test_other_raster_shapes_against_the_restatement(product, shape):
    """259 cells: one block plus three lanes; 33 cells: less than a wave; one row of 300: a partial second block.  Six hours (snow builds,
    falls mixed, melts; flags in relHum and transmissivity, free water) with snow.restate_snow_hour carried along: all thirteen maps after
    every hour.  tests/test_snow_host.py checks that the forcing does what it says."""
    _need_glibc_set(product)
    dem, flag, hours = snow_cases.small_forcing(shape, seed=shape[1])
    want = snow_cases.restated_run(dem, flag, hours)
    snow.initialize(product, dem, flag)
    for h, met in enumerate(hours):
        snow.compute_hour(product, met)
        got = snow.all_maps(product)
        _same_maps(got, want[h], f"raster {shape}, hour {h}")
        assert np.all(got["swe"][dem == np.float32(flag)] == np.float32(flag))
    assert want[1]["swe"].flat[-1] > 0 and max(want[3]["snowMelt"].flat[-1], want[4]["snowMelt"].flat[-1]) > 0      # the last lane built snow and melted it
    assert any(np.count_nonzero(w["liquid"] > 0) > 0 for w in want)
    snow.clean(product)


def test_non_default_parameters_against_the_restatement(product):
    """Every one of the seven parameters away from its default (snow_cases.OTHER_PARAMETERS), once passed to sf3d_snow_initialize and once
    set by sf3d_snow_set_parameters (and sf3d_snow_reset, whose surface energy reads skinThickness) on a raster initialised with the defaults.
    No run of the compiled reference pins these values: snow.restate_snow_hour, which equals it on the defaults, is the only authority
    here.  tests/test_snow_host.py checks that each parameter alone changes the result of this forcing."""
    _need_glibc_set(product)
    shape = (7, 37)
    p = snow_cases.OTHER_PARAMETERS
    dem, flag, hours = snow_cases.small_forcing(shape, seed=shape[1])
    want = snow_cases.restated_run(dem, flag, hours, p)
    default = snow_cases.restated_run(dem, flag, hours[:1])
    runs = []
    for how in ("initialize", "set_parameters"):
        if how == "initialize":
            snow.initialize(product, dem, flag, p)
        else:
            snow.initialize(product, dem, flag)
            snow.set_parameters(product, p)
            snow.reset(product)
        runs.append([])
        for h, met in enumerate(hours):
            snow.compute_hour(product, met)
            runs[-1].append(snow.all_maps(product))
            _same_maps(runs[-1][h], want[h], f"{how}, hour {h}")
        snow.clean(product)
    for h in range(len(hours)):
        _same_maps(runs[0][h], runs[1][h], f"both ways, hour {h}")
    assert not np.array_equal(_bits(want[0]["surfaceTemp"]), _bits(default[0]["surfaceTemp"]))      # (not the default run)


def test_error_paths(product, pin):
    snow.bind(product)
    lib = product.lib
    n = pin["dem"].size
    buf = np.zeros(n, np.float32)
    p = buf.ctypes.data_as(snow.pf32)
    lib.sf3d_snow_clean()
    seven = [p] * 7
    assert lib.sf3d_snow_get_state(0, n, p) == capi.MEMORY_ERROR                                    # before initialise
    assert lib.sf3d_snow_set_state(0, n, p) == capi.MEMORY_ERROR
    assert lib.sf3d_snow_get_output(0, n, p) == capi.MEMORY_ERROR
    assert lib.sf3d_snow_compute_hour(n, *seven, None, 0.75) == capi.MEMORY_ERROR
    assert lib.sf3d_snow_reset() == capi.MEMORY_ERROR
    assert lib.sf3d_snow_initialize(0, 4, p, -9999.0, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_snow_initialize(4, 4, None, -9999.0, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_snow_default_parameters(None) == capi.PARAMETER_ERROR
    snow.initialize(product, pin["dem"], float(pin["flag"]))
    assert lib.sf3d_snow_get_state(0, n - 1, p) == capi.PARAMETER_ERROR                             # wrong size
    assert lib.sf3d_snow_set_state(0, n + 1, p) == capi.PARAMETER_ERROR
    assert lib.sf3d_snow_compute_hour(n // 2, *seven, None, 0.75) == capi.PARAMETER_ERROR
    assert lib.sf3d_snow_get_state(0, n, None) == capi.PARAMETER_ERROR                              # null pointer
    assert lib.sf3d_snow_compute_hour(n, *seven[:6], None, None, 0.75) == capi.PARAMETER_ERROR
    assert lib.sf3d_snow_get_state(7, n, p) == capi.INDEX_ERROR
    assert lib.sf3d_snow_get_output(6, n, p) == capi.INDEX_ERROR
    assert lib.sf3d_snow_set_state(-1, n, p) == capi.INDEX_ERROR
    assert lib.sf3d_snow_get_state(0, n, p) == capi.OK
    with pytest.raises(ValueError):
        snow.set_state(product, "swe", np.zeros((3, 3), np.float32))
    assert lib.sf3d_snow_clean() == capi.OK
    assert lib.sf3d_snow_get_state(0, n, p) == capi.MEMORY_ERROR                                    # after clean
    assert lib.sf3d_snow_compute_hour(n, *seven, None, 0.75) == capi.MEMORY_ERROR


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("snow_host")
    return d, build_host_program("snow", d)


@pytest.mark.parametrize("shape", snow_cases.SHAPES)
def test_device_equals_the_host_build_of_the_same_text(product, host, shape):
    """k_snow_hour against tests/snow_host.cpp, the same snow_cell compiled for the CPU, on the continuous forcing of two seeds (seven hours,
    the state carried along) under the default and the other parameters, and on one row of eight cells: all thirteen maps after every hour,
    bit for bit.  tests/test_snow_host.py has run these cases under the sanitizers and shown that they are not vacuous."""
    _need_glibc_set(product)
    directory, exe = host
    cases = [(seed, snow_cases.continuous_forcing(shape, seed), par) for seed in snow_cases.SEEDS[:2] for par in (None, snow_cases.OTHER_PARAMETERS)]
    if shape == snow_cases.SHAPES[0]:
        cases.append(("1x8", snow_cases.small_forcing((1, 8), 3), None))
    for seed, (dem, flag, hours), par in cases:
        snow.initialize(product, dem, flag, par)
        start = {n: snow.get_state(product, n) for n in snow.STATE}
        want = snow_cases.run_host(exe, directory, f"gpu-{shape[1]}-{seed}-{par is not None}", dem, flag, start, hours, par)
        for h, met in enumerate(hours):
            snow.compute_hour(product, met)
            got = snow.all_maps(product)
            for n in snow.STATE + snow.OUTPUT:
                bad = differing(got[n], want[h][n])
                if bad.any() or h == len(hours) - 1:
                    print(f"raster {dem.shape}, seed {seed}, hour {h} {n}: values differ: {int(bad.sum())}")
                assert not bad.any(), (shape, seed, h, n, int(bad.sum()), got[n][bad][:4], want[h][n][bad][:4])
        assert np.count_nonzero(want[1]["swe"] > 0) > 0 and any(np.count_nonzero(w["liquid"] > 0) > 0 for w in want)
        snow.clean(product)
