"""The hourly r.sun radiation maps on the device (include/sf3d_rad.h, k_rad_hour) against the compiled-reference pin
tests/golden/rad_rsun.npz: every cell of every map and case bit for bit, both hours of the two-hour cases included; the same property
off the pin against the restatement on 7 x 37, 3 x 11 and 1 x 300 rasters (a partial second block, less than a wave, a partial second
block in one row) that together reach the arms of the pin; the device build of sf3d_trig.inc against its host build bit for bit;
transmissivity taken from the meteo block on the device against the same map passed from the host; no side effect on the solver; two
ranks sharing the GPU merge to the single-rank maps; the maps survive sf3d_initialize and go with sf3d_clean.

Away from 44 N 11 E and from 2021 (tests/golden/rad_rsun_places.npz, the second pin of the compiled reference): every cell of its 39
cases at 69.67 N, 0.23 N, 33.93 S, 122.4 W and 178.9 W with 4, 10 and 2.5 m cells, cells edited to the poles, the date line and out of
validate()'s range, leap years, the century rules, dates before 2000 and a refused local year, with the latitude and longitude maps of
the pin; 7 x 37 and 3 x 11 rasters at 80 N, 80 S, the equator and a pole row against the restatement, whose chains reach every
sun-position arm (rad.SUN_ARMS) the pin reaches; two ranks on the southern raster merge to the pin."""
import ctypes

import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm, meteo, radiation as rad
from tests import ranks as mr
from tests import rad_cases
from tests.raster_helpers import differing
from tests.test_trig_host import acos_ranges, build_trig_host, ptr, trig_ranges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return rad_cases.load_pin()


def _same(got, want, what):
    same = ~differing(got, want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), np.asarray(got)[~same][:4], np.asarray(want)[~same][:4])


def _maps(product):
    return np.stack([rad.get_map(product, n) for n in rad.MAPS])


@pytest.fixture(scope="module")
def places():
    return rad_cases.load_places_pin()


def _start_pin(product, pin, raster, settings):
    geo = rad_cases.pin_geo(pin, raster)
    dummy = pin["dem"][raster]                   # map mode needs a map; the reference never reads it inside the grid
    s = rad.settings_dict(settings)
    rad.initialize(product, pin["dem"][raster], geo[0], geo[1], geo[2], pin["lat"][raster], pin["lon"][raster], pin["slope"][raster], pin["aspect"][raster],
                   linke_map=dummy if s["linkeMode"] == rad.MODE_MAP else None, albedo_map=dummy if s["albedoMode"] == rad.MODE_MAP else None,
                   settings=settings, flag=float(pin["flag"]))


def _every_cell(product, pin):
    checked = 0
    for raster, chain in rad_cases.pin_chains(pin):
        _start_pin(product, pin, raster, chain[0]["settings"])
        for case in chain:
            t = np.ascontiguousarray(pin["transmissivity"][case["transmissivity"]])
            if "refuses" in case["name"]:
                assert product.lib.sf3d_rad_compute_hour(*case["when"], t.size, t.ctypes.data_as(capi.pf32)) == capi.PARAMETER_ERROR
            else:
                rad.compute_hour(product, case["when"], t)
            _same(_maps(product), rad_cases.pin_maps(pin, case), case["name"])
            checked += 1
    rad.clean(product)
    return checked


def test_every_cell_of_every_map_and_case_equals_the_pin(product, pin):
    assert _every_cell(product, pin) == len(pin["cases"])


def test_every_cell_of_the_places_pin(product, places):
    """five other places (polar, equator, southern, two western), cells edited to the poles, the date line and out of validate()'s range,
    leap years and centuries: the latitude and longitude maps are the pin's; the refused hour is SF3D_PARAMETER_ERROR and leaves the maps"""
    refused = [c for c in places["cases"] if "refuses" in c["name"]]
    assert len(refused) == 1 and refused[0]["keep"] == 1
    assert _every_cell(product, places) == len(places["cases"]) >= 36


@pytest.mark.parametrize("shape", rad_cases.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_rasters_equal_the_restatement(product, shape):
    ref = rad_cases.small_reference()
    g = rad_cases.small_raster(shape)
    reached = 0
    for name, settings, hours in rad_cases.small_chains():
        s = rad.settings_dict(settings)
        rad.initialize(product, g["dem"], *rad_cases.GEO, g["lat"], g["lon"], g["slope"], g["aspect"],
                       linke_map=g["dem"] if s["linkeMode"] == rad.MODE_MAP else None, albedo_map=g["dem"] if s["albedoMode"] == rad.MODE_MAP else None,
                       settings=settings, flag=float(rad_cases.FLAG))
        for k, (when, tk) in enumerate(hours):
            rad.compute_hour(product, when, g["transmissivity"][tk])
            want, arms = ref[(shape, name)][k]
            _same(_maps(product), want, (shape, name, k))
            reached |= int(np.bitwise_or.reduce(arms, axis=None))
    rad.clean(product)
    assert reached != 0
    every = 0
    for (_, _), hours in ref.items():
        for _, arms in hours:
            every |= int(np.bitwise_or.reduce(arms, axis=None))
    assert every == (1 << len(rad.ARMS)) - 1                              # together the three rasters reach the arms of the pin


@pytest.mark.parametrize("shape", rad_cases.SHAPES_PLACES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_rasters_at_other_places_equal_the_restatement(product, shape):
    ref, reached = rad_cases.small_reference_places()
    refused = 0
    for name, place, settings, hours in rad_cases.small_chains_places():
        g = rad_cases.small_raster(shape, place)
        s = rad.settings_dict(settings)
        rad.initialize(product, g["dem"], *g["geo"], g["lat"], g["lon"], g["slope"], g["aspect"], settings=settings, flag=float(rad_cases.FLAG))
        for k, (when, tk) in enumerate(hours):
            t = g["transmissivity"][tk]
            if rad.hour_setup(when, s["timeZone"], bool(s["isUTC"])) is None:             # S_solpos refuses the date: the maps stay
                assert product.lib.sf3d_rad_compute_hour(*when, t.size, t.ctypes.data_as(capi.pf32)) == capi.PARAMETER_ERROR
                refused += 1
            else:
                rad.compute_hour(product, when, t)
            _same(_maps(product), ref[(shape, name)][k][0], (shape, name, k))
    rad.clean(product)
    assert refused == 1
    # what the kernel ran here is what tests/test_rad_host.py counts on the CPU: every sun-position arm the places pin reaches
    pin = rad_cases.load_places_pin()
    assert {n for k, n in enumerate(rad.SUN_ARMS) if reached >> k & 1} == {n for n, k in zip(pin["sun_arm_names"], pin["sun_arm_counts"]) if k > 0}


def test_device_trig_equals_the_host_build_bit_for_bit(product, tmp_path):
    lib = build_trig_host(tmp_path)
    n = 1_000_000
    for which, name in enumerate(("sin", "cos", "tan", "acos")):
        ranges = acos_ranges(60 + which) if which == 3 else trig_ranges(60 + which)
        x = np.concatenate([np.asarray(v)[:n // len(ranges)] for v in ranges.values()])
        x = np.concatenate([x, [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 200.0, -200.0, 5e-324]])
        host = np.empty_like(x)
        lib.tr_eval(which, ptr(x), ptr(host), ctypes.c_size_t(x.size))
        dev = rad.device_trig(product, which, x)
        nan = np.isnan(host) & np.isnan(dev)
        assert x.size >= n and np.array_equal(dev.view(np.int64)[~nan], host.view(np.int64)[~nan]), name
    rng = np.random.default_rng(66)
    x = np.concatenate([rng.uniform(-1, 1, n), [1.0, -1.0, 0.5, -0.5, 0.0, 2.0 ** -26, 2.0 ** -27]]).astype(np.float32)
    host = np.empty_like(x)
    lib.tr_eval_acosf(ptr(x), ptr(host), ctypes.c_size_t(x.size))
    assert np.array_equal(rad.device_trig(product, 4, x.astype(np.float64)).astype(np.float32).view(np.int32), host.view(np.int32))
    x = rng.uniform(3.0, 97.0, n).astype(np.float32)
    e = np.where(rng.uniform(size=n) < 0.5, np.float32(-1.6364), rng.uniform(-4, 4, n)).astype(np.float32)
    host = np.empty_like(x)
    lib.tr_eval_powf(ptr(x), ptr(e), ptr(host), ctypes.c_size_t(x.size))
    dev = rad.device_trig(product, 5, x.astype(np.float64), e.astype(np.float64)).astype(np.float32)
    nan = np.isnan(host) & np.isnan(dev)
    assert np.array_equal(dev.view(np.int32)[~nan], host.view(np.int32)[~nan])


def test_transmissivity_from_the_meteo_block_equals_the_map_passed_from_the_host(product, pin):
    raster, when = 1, (2021, 3, 20, 7, 30, 0)
    dem, geo, flag = pin["dem"][raster], pin["geo"], float(pin["flag"])
    _start_pin(product, pin, raster, None)
    n = dem.size
    null = lambda: product.lib.sf3d_rad_compute_hour(*when, n, None)
    meteo.clean(product)
    assert null() == capi.PARAMETER_ERROR                                 # no meteo block
    meteo.initialize(product, dem[:, :16], geo[0], geo[1], geo[2], flag=flag)
    rng = np.random.default_rng(5)
    sx, sy = geo[0] + rng.uniform(-200, 400, 12), geo[1] + rng.uniform(-200, 300, 12)
    sv = rng.uniform(0.1, 0.8, 12).astype(np.float32)
    meteo.interpolate(product, "transmissivity", "idw", sx, sy, sv, 600.0 * 500.0, download=False)
    assert null() == capi.PARAMETER_ERROR                                 # the meteo block is on another raster
    meteo.initialize(product, dem, geo[0], geo[1], geo[2], flag=flag)
    meteo.interpolate(product, "airT", "idw", sx, sy, sv, 600.0 * 500.0, download=False)
    assert null() == capi.PARAMETER_ERROR                                 # on this raster, but no transmissivity yet
    t = meteo.interpolate(product, "transmissivity", "idw", sx, sy, sv, 600.0 * 500.0)
    assert ((t > 0.1) & (t < 0.8))[dem != pin["flag"]].all()
    assert null() == capi.OK
    from_device = _maps(product)
    _start_pin(product, pin, raster, None)
    rad.compute_hour(product, when, t)
    _same(from_device, _maps(product), "meteo hand-over")
    assert np.count_nonzero(from_device[1] > 0) > 600                      # not vacuous: global irradiance on the lit cells of the window
    meteo.clean(product)
    rad.clean(product)


def test_rad_calls_leave_the_solver_untouched(product, pin):
    """C2 in its F20 hour, a radiation hour between every two computeSteps: H, Se and the work counters of the run without"""
    def run(with_rad):
        m = cm.catchment_model(64, 64, 10)
        product.check(product.lib.sf3d_reset_solver_state(), "reset")
        cm.build(product, m, threads=1)
        if with_rad:
            _start_pin(product, pin, 1, None)
        product.set_sink_source_bulk(0, np.full(m.ns, cm.rain_rate(20.0, m.cell_area)))
        t, k = 0.0, 0
        while t < 3600.0:
            dt = product.lib.sf3d_compute_step(3600.0 - t)
            assert dt > 0.0
            t += dt
            if with_rad:
                rad.compute_hour(product, (2021, 3, 20, 6 + k % 10, 30, 0), pin["transmissivity"][k % 2])
                if k % 5 == 0:
                    rad.get_map(product, "global")
            k += 1
        s, c = cm.snapshot(product, m), product.counters()
        if with_rad:
            assert np.count_nonzero(rad.get_map(product, "global") > 0) > 0
        product.lib.sf3d_clean()
        return s, c
    (s0, c0), (s1, c1) = run(False), run(True)
    assert np.array_equal(s0["H"], s1["H"]) and np.array_equal(s0["Se"], s1["Se"])
    assert c0 == c1


def test_maps_survive_sf3d_initialize_and_go_with_sf3d_clean(product, pin):
    _start_pin(product, pin, 0, None)
    rad.compute_hour(product, (2021, 3, 20, 11, 30, 0), pin["transmissivity"][0])
    before = _maps(product)
    m = cm.catchment_model(16, 16, 4)
    product.check(product.lib.sf3d_reset_solver_state(), "reset")
    cm.build(product, m, threads=1)                                   # sf3d_initialize inside
    _same(_maps(product), before, "after sf3d_initialize")
    out = np.empty(before[0].size, np.float32)
    assert product.lib.sf3d_rad_get_map(5, out.size, out.ctypes.data_as(capi.pf32)) == capi.INDEX_ERROR
    assert product.lib.sf3d_rad_get_map(0, out.size + 1, out.ctypes.data_as(capi.pf32)) == capi.PARAMETER_ERROR
    assert product.lib.sf3d_rad_compute_hour(2021, 3, 20, 11, 30, 0, out.size + 1, out.ctypes.data_as(capi.pf32)) == capi.PARAMETER_ERROR
    product.lib.sf3d_clean()
    assert product.lib.sf3d_rad_get_map(0, out.size, out.ctypes.data_as(capi.pf32)) == capi.MEMORY_ERROR


def test_two_ranks_merge_to_the_single_rank_maps(product, pin, tmp_path):
    which = next(k for k, c in enumerate(pin["cases"]) if c["raster"] == 1 and c["name"].endswith("equinox morning"))
    first, second = pin["cases"][which], pin["cases"][which + 1]
    ranks = mr.run("scripts/multirank_rad_worker.py", 2, mr.PORTS["rad"], [which], tmp_path)
    rows, cols = pin["dem"][1].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(pin["flag"])
    for k, case in enumerate((first, second)):
        merged = mr.merge([res[f"hour{k}"] for res in ranks], cell_owner, flag, others=flag, what=f"hour{k}")      # another rank's cells: the flag
        assert merged.shape == (5, rows, cols) and merged.dtype == np.float32
        _same(merged, rad_cases.pin_maps(pin, case), f"merged ranks, hour {k}")      # what the single rank gives (the first test): the pin
    assert np.count_nonzero(merged[1] > 0) > 500


def test_two_ranks_merge_to_the_places_pin_on_the_southern_raster(product, places, tmp_path):
    pin = places
    which = next(k for k, c in enumerate(pin["cases"]) if c["name"].startswith("south: 21 June 2021, morning"))
    first, second = pin["cases"][which], pin["cases"][which + 1]
    assert second["keep"] and pin["places"][first["raster"]]["startLatitude"] < 0
    ranks = mr.run("scripts/multirank_rad_worker.py", 2, mr.PORTS["rad_places"], [which, "places"], tmp_path)
    rows, cols = pin["dem"][first["raster"]].shape
    idx = np.arange(rows * cols).reshape(rows, cols)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(pin["flag"])
    for k, case in enumerate((first, second)):
        merged = mr.merge([res[f"hour{k}"] for res in ranks], cell_owner, flag, others=flag, what=f"hour{k}")
        assert merged.shape == (5, rows, cols) and merged.dtype == np.float32
        _same(merged, rad_cases.pin_maps(pin, case), f"merged ranks, hour {k}")
    assert np.count_nonzero(merged[1] > 0) > 200
