"""Hourly ET0, daily extremes and daily crop maps on the device (include/sf3d_crop.h, k_et0_hour / k_crop_day) against the
compiled-reference pin tests/golden/crop_et0.npz: all five maps at every checkpoint of the calendar bit for bit, zero cells excluded; a
raster with a partial wave and a partial block, one of less than a wave and a single row of 300 cells against the restatement; the run interrupted through get_state / set_state and through
the crop/ state folder; NULL inputs read what the snow hour uploaded; the solver does not notice the calls; two ranks sharing the GPU
merge to the single-rank maps; the error codes; the device against the host build of the same text (tests/crop_host.cpp) on random scripts
over both hemispheres, bit for bit."""
import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, crop, snow
from tests import ranks as mr
from tests import crop_cases as cc
from tests.scenarios import ravone_project_model
from tests.raster_helpers import bits as _bits, build_host_program, differing, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return cc.load_pin()


def _checker(pin, what):
    def at(k, maps):
        for j, n in enumerate(crop.MAPS):
            want = pin["maps"][k][j]
            bad = _bits(maps[n]) != _bits(want)
            print(f"{what} checkpoint {k} {n}: {int(bad.sum())} cells differ")
            assert not bad.any(), (what, k, n, int(bad.sum()), maps[n][bad][:4], want[bad][:4])
    return at


def test_all_five_maps_equal_the_pin_at_every_checkpoint(product, pin):
    _need_glibc_set(product)
    n = cc.replay(pin, cc.Device(product, pin), _checker(pin, "uninterrupted"))
    assert n == pin["maps"].shape[0]
    crop.clean(product)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_partial_wave_and_partial_block_against_the_restatement(product, pin, shape):
    """7 x 37 = 259 cells: one full block plus three lanes; 3 x 11: less than a wave; one row of 300: a partial second block.  The degree-day
    map, one hour and one daily update against the restatement (cc.small_raster_stages); the shares of cells that must hold ET0 and LAI
    are asserted on the restatement in tests/test_crop_host.py"""
    _need_glibc_set(product)
    r = cc.small_raster(pin, shape)
    dem, idx, units, lat, flag = r["dem"], r["idx"], r["units"], r["latitude"], r["flag"]
    after_degree_days, after_hour, after_day = cc.small_raster_stages(r)
    crop.initialize(product, dem, idx, units, lat, flag)
    crop.set_degree_days(product, r["dd0"], cc.DOY)
    got = crop.all_maps(product)
    for n in crop.MAPS:
        assert np.array_equal(_bits(got[n]), _bits(after_degree_days[n])), ("degree-day map", n)
    crop.compute_hour(product, r["met"])
    got = crop.all_maps(product)
    assert np.count_nonzero(got["et0"] > 0) > cc.ET0_SHARE * r["dem_cells"] and got["et0"].flat[-2] > 0 and got["et0"][r["inner"]] == np.float32(flag)
    assert got["et0"].flat[-1] == np.float32(flag)
    for n in crop.MAPS:
        assert np.array_equal(_bits(got[n]), _bits(after_hour[n])), ("hour", n)
    crop.daily_update(product, cc.DOY)
    got = crop.all_maps(product)
    assert np.count_nonzero(got["lai"] > 0) > cc.LAI_SHARE * r["dem_cells"]
    for n in crop.MAPS:
        assert np.array_equal(_bits(got[n]), _bits(after_day[n])), ("day", n)
    crop.clean(product)


@pytest.mark.parametrize("how", ["get_set_state", "state_directory"])
def test_interrupted_run_equals_the_uninterrupted_one(product, pin, tmp_path, how):
    _need_glibc_set(product)
    ops = pin["ops"]
    hours = [n for n, o in enumerate(ops) if o[0] == cc.OP_HOUR]
    stops = {hours[30], hours[120]}                         # mid-day in spring (extremes in flight), mid-day in autumn
    header = dict(xllcorner=0.0, yllcorner=0.0, cellsize=4.0, nodata=float(pin["flag"]))
    done = []

    def interrupt(n, backend):
        if n not in stops:
            return
        if how == "get_set_state":
            saved = {s: crop.get_state(product, s) for s in crop.STATE}
        else:
            d = crop.save_crop_state(product, tmp_path, header)
            assert sorted(p.name for p in d.iterdir()) == sorted(f"{s}{e}" for s in crop.STATE_FILES.values() for e in (".flt", ".hdr"))
        crop.clean(product)
        backend.initialize(44.5)
        if how == "get_set_state":
            for s, v in saved.items():
                crop.set_state(product, s, v)
        else:
            crop.load_crop_state(product, tmp_path)
        done.append(n)

    last = max(n for n, o in enumerate(ops) if o[0] == cc.OP_LATITUDE)          # the northern part of the calendar
    short = dict(pin, ops=ops[:last])
    cc.replay(short, cc.Device(product, pin), _checker(pin, how), interrupt)
    assert len(done) == 2
    crop.clean(product)


def _snow_meteo(met, dem, flag, clear_sky):
    valid = dem != np.float32(flag)
    f = lambda v: np.where(valid, np.float32(v), np.float32(flag)).astype(np.float32)
    return dict(airT=met["airT"], prec=f(0.5), relHum=met["relHum"], windInt=met["windInt"], globalRad=met["globalRad"], beamRad=f(10.0),
                transmissivity=met["transmissivity"], clearSkyTransmissivity=clear_sky)


def test_null_inputs_read_the_maps_the_snow_hour_uploaded(product, pin):
    dem, flag, clear = pin["dem"], float(pin["flag"]), float(pin["clear_sky"])
    hours = (10, 11, 12)

    def run(reuse):
        crop.initialize(product, dem, pin["unit_index"], pin["unit_list"], 44.5, flag)
        if reuse:
            snow.initialize(product, dem, flag)
        out = []
        for h in hours:
            met = cc.meteo(pin, h)
            if reuse:
                snow.compute_hour(product, _snow_meteo(met, dem, flag, clear))
                crop.compute_hour(product, None, clear)
            else:
                crop.compute_hour(product, met, clear)
            out.append(crop.all_maps(product))
        if reuse:
            swe = snow.get_state(product, "swe")
            snow.clean(product)
            assert np.isfinite(swe).all()
        crop.clean(product)
        return out
    explicit, reused = run(False), run(True)
    assert np.count_nonzero(explicit[-1]["et0"] > 0) > 100
    for a, b in zip(explicit, reused):
        for n in crop.MAPS:
            assert np.array_equal(_bits(a[n]), _bits(b[n])), n


def test_null_inputs_need_a_snow_hour_on_the_same_raster(product, pin):
    crop.bind(product); snow.bind(product)
    lib = product.lib
    dem, flag = pin["dem"], float(pin["flag"])
    n = dem.size
    snow.clean(product)
    crop.initialize(product, dem, pin["unit_index"], pin["unit_list"], 44.5, flag)
    null = crop.pf32()
    p = np.zeros(n, np.float32).ctypes.data_as(crop.pf32)
    assert lib.sf3d_crop_compute_hour(n, null, null, null, null, null, 0.75) == capi.PARAMETER_ERROR          # no snow raster
    snow.initialize(product, dem, flag)
    assert lib.sf3d_crop_compute_hour(n, null, null, null, null, null, 0.75) == capi.PARAMETER_ERROR          # snow has not computed an hour
    snow.compute_hour(product, _snow_meteo(cc.meteo(pin, 10), dem, flag, 0.75))
    assert lib.sf3d_crop_compute_hour(n, null, null, null, null, null, 0.75) == capi.OK
    assert lib.sf3d_crop_compute_hour(n, p, null, p, p, p, 0.75) == capi.PARAMETER_ERROR                      # a mix
    assert lib.sf3d_crop_compute_hour(n, null, p, p, p, p, 0.75) == capi.PARAMETER_ERROR
    snow.initialize(product, dem[:, :16], flag)                                                                # another raster
    m = _snow_meteo({k: v[:, :16] for k, v in cc.meteo(pin, 10).items()}, dem[:, :16], flag, 0.75)
    snow.compute_hour(product, m)
    assert lib.sf3d_crop_compute_hour(n, null, null, null, null, null, 0.75) == capi.PARAMETER_ERROR
    snow.initialize(product, dem.reshape(32, 24), flag)                                                        # as many cells, other rows x columns
    snow.compute_hour(product, {k: (v.reshape(32, 24) if isinstance(v, np.ndarray) else v) for k, v in _snow_meteo(cc.meteo(pin, 10), dem, flag, 0.75).items()})
    assert lib.sf3d_crop_compute_hour(n, null, null, null, null, null, 0.75) == capi.PARAMETER_ERROR
    snow.clean(product)
    crop.clean(product)


def test_crop_calls_leave_the_solver_untouched(product, pin):
    """C2 in its F20 hour, an hourly and a daily call between every two computeSteps: H, Se and the work counters of the run without"""
    def run(with_crop):
        m = cm.catchment_model(64, 64, 10)
        product.check(product.lib.sf3d_reset_solver_state(), "reset")
        cm.build(product, m, threads=1)
        if with_crop:
            crop.initialize(product, pin["dem"], pin["unit_index"], pin["unit_list"], 44.5, float(pin["flag"]))
        product.set_sink_source_bulk(0, np.full(m.ns, cm.rain_rate(20.0, m.cell_area)))
        t, k = 0.0, 0
        while t < 3600.0:
            dt = product.lib.sf3d_compute_step(3600.0 - t)
            assert dt > 0.0
            t += dt
            if with_crop:
                crop.compute_hour(product, cc.meteo(pin, k % 72), float(pin["clear_sky"]))
                crop.daily_update(product, 100 + k % 50)
                if k % 5 == 0:
                    crop.get_et0(product)
            k += 1
        s, c = cm.snapshot(product, m), product.counters()
        if with_crop:
            assert np.count_nonzero(crop.get_state(product, "lai") > 0) > 0
        product.lib.sf3d_clean()
        return s, c
    (s0, c0), (s1, c1) = run(False), run(True)
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"])
    assert c0 == c1


def test_crop_state_survives_sf3d_initialize_and_goes_with_sf3d_clean(product, pin):
    crop.initialize(product, pin["dem"], pin["unit_index"], pin["unit_list"], 44.5, float(pin["flag"]))
    crop.compute_hour(product, cc.meteo(pin, 12), float(pin["clear_sky"]))
    before = crop.get_state(product, "dailyTmax")
    assert np.count_nonzero(before > -100) > 0
    m = cm.catchment_model(16, 16, 4)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)                                   # sf3d_initialize inside
    assert np.array_equal(_bits(crop.get_state(product, "dailyTmax")), _bits(before))
    product.lib.sf3d_clean()
    out = np.empty(before.size, np.float32)
    assert product.lib.sf3d_crop_get_state(0, out.size, out.ctypes.data_as(crop.pf32)) == capi.MEMORY_ERROR


def test_two_ranks_merge_to_the_single_rank_maps(product, pin, tmp_path):
    hours = 4
    ranks = mr.run("scripts/multirank_crop_worker.py", 2, mr.PORTS["crop"], [hours], tmp_path)
    m = ravone_project_model((980, 1060, 330, 420))
    idx = np.asarray(m.meta["index"])[0]
    flag = -9999.0
    dem = np.where(idx >= 0, m.z[np.maximum(idx, 0)], flag).astype(np.float32)
    units = pin["unit_list"]
    unit_index = (np.arange(dem.size).reshape(dem.shape) % len(units)).astype(np.int32)
    crop.initialize(product, dem, unit_index, units, 44.5, flag)
    crop.set_degree_days(product, np.where(idx >= 0, np.float32(800.0), np.float32(flag)), 200)
    for met in cc.small_forcing(dem.shape, dem, flag)[:hours]:
        crop.compute_hour(product, met)
    single_hour = crop.all_maps(product)
    crop.daily_update(product, 200)
    single = crop.all_maps(product)
    crop.clean(product)
    cell_owner = mr.cell_owner(ranks, idx, m.n)
    merged = mr.merge([res["et0"] for res in ranks], cell_owner, np.float32(flag), others=np.float32(flag), what="et0")      # another rank's cells: the flag
    assert merged.shape == dem.shape and merged.dtype == np.float32 and np.array_equal(_bits(merged), _bits(single["et0"])) and np.count_nonzero(merged > 0) > 1000
    for n in crop.STATE:
        for r, res in enumerate(ranks):
            mine = cell_owner == r
            assert np.array_equal(_bits(res["hour_" + n][mine]), _bits(single_hour[n][mine])), (n, r)
            assert np.array_equal(_bits(res[n][mine]), _bits(single[n][mine])), (n, r)
            assert np.array_equal(_bits(res[n][~mine]), _bits(res["initial_" + n][~mine])), (n, r)      # untouched elsewhere


def test_error_paths(product, pin):
    crop.bind(product)
    lib = product.lib
    dem, flag = pin["dem"], float(pin["flag"])
    n = dem.size
    buf = np.zeros(n, np.float32)
    p = buf.ctypes.data_as(crop.pf32)
    lib.sf3d_crop_clean()
    five = [p] * 5
    assert lib.sf3d_crop_get_state(0, n, p) == capi.MEMORY_ERROR                                    # before initialise
    assert lib.sf3d_crop_set_state(0, n, p) == capi.MEMORY_ERROR
    assert lib.sf3d_crop_get_et0(n, p) == capi.MEMORY_ERROR
    assert lib.sf3d_crop_compute_hour(n, *five, 0.75) == capi.MEMORY_ERROR
    assert lib.sf3d_crop_daily_update(10, 10) == capi.MEMORY_ERROR
    assert lib.sf3d_crop_set_degree_days(n, p, 10) == capi.MEMORY_ERROR
    idx = np.ascontiguousarray(pin["unit_index"], np.int32)
    pi = idx.ctypes.data_as(crop.pi32)
    units = pin["unit_list"]
    demp = np.ascontiguousarray(dem, np.float32).ctypes.data_as(crop.pf32)
    many = crop.unit_array([units[0]] * (crop.MAX_UNITS + 1))
    assert lib.sf3d_crop_initialize(24, 32, demp, flag, pi, crop.MAX_UNITS + 1, many, 44.5) == capi.PARAMETER_ERROR      # more units than the cap
    assert lib.sf3d_crop_initialize(24, 32, demp, flag, pi, 3, crop.unit_array(units[:3]), 44.5) == capi.PARAMETER_ERROR  # a crop index >= nUnits
    assert lib.sf3d_crop_initialize(24, 32, demp, flag, pi, len(units), None, 44.5) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_get_state(0, n, p) == capi.MEMORY_ERROR                                    # a refused initialise leaves no raster
    assert lib.sf3d_crop_initialize(24, 32, demp, flag, pi, crop.MAX_UNITS, crop.unit_array((units * 8)[:crop.MAX_UNITS]), 44.5) == capi.OK      # the cap itself
    crop.initialize(product, dem, idx, units, 44.5, flag)
    assert lib.sf3d_crop_get_state(0, n - 1, p) == capi.PARAMETER_ERROR                             # wrong size
    assert lib.sf3d_crop_set_state(0, n + 1, p) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_get_et0(n // 2, p) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_compute_hour(n // 2, *five, 0.75) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_set_degree_days(n - 1, p, 10) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_get_state(0, n, None) == capi.PARAMETER_ERROR                              # null pointer
    assert lib.sf3d_crop_daily_update(0, 10) == capi.PARAMETER_ERROR and lib.sf3d_crop_daily_update(10, 367) == capi.PARAMETER_ERROR
    assert lib.sf3d_crop_get_state(4, n, p) == capi.INDEX_ERROR                                     # a map number out of range
    assert lib.sf3d_crop_set_state(-1, n, p) == capi.INDEX_ERROR
    assert lib.sf3d_crop_get_state(0, n, p) == capi.OK and np.all(buf == np.float32(flag))          # initializeCropMaps: the flag
    assert lib.sf3d_crop_get_et0(n, p) == capi.OK and np.all(buf == np.float32(flag))
    with pytest.raises(ValueError):
        crop.set_state(product, "lai", np.zeros((3, 3), np.float32))
    assert lib.sf3d_crop_clean() == capi.OK
    assert lib.sf3d_crop_get_state(0, n, p) == capi.MEMORY_ERROR                                    # after clean


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crop_host")
    return d, build_host_program("crop", d)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_of_the_same_text(product, pin, host, shape):
    """k_et0_hour and k_crop_day against tests/crop_host.cpp, the same crop_et0_cell and crop_day_cell compiled for the CPU, on the
    continuous scripts of two seeds (the degree-day map, hours by day and by night, daily updates on both hemispheres) and on the edge
    cases (64 land units, one row of eight cells): all five maps at every checkpoint, bit for bit.  tests/test_crop_host.py has run these
    scripts under the sanitizers and shown that they are not vacuous."""
    _need_glibc_set(product)
    directory, exe = host
    scripts = [(f"{shape[1]}-{seed}",) + cc.random_script(pin, shape, seed) for seed in cc.SEEDS[:2]]
    if shape == cc.SHAPES[0]:
        scripts += list(cc.edge_scripts(pin))
    for name, r, ops in scripts:
        p = cc.as_pin(r, pin)
        want = cc.run_host(exe, directory, "gpu-" + name, p, ops)
        got = cc.run_script(cc.Device(product, p), ops)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            for n in crop.MAPS:
                bad = differing(g[n], w[n])
                if bad.any() or k == len(got) - 1:
                    print(f"{name} checkpoint {k} {n}: values differ: {int(bad.sum())}")
                assert not bad.any(), (name, k, n, int(bad.sum()), g[n][bad][:4], w[n][bad][:4])
        # (the share tests/test_crop_host.py asserts of the random scripts; the edge rasters hold a handful of cells)
        assert np.count_nonzero(got[1]["et0"] > 0) > (cc.ET0_SHARE * r["dem_cells"] if r["dem"].shape == shape else 0)
        crop.clean(product)
