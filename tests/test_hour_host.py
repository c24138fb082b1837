"""The hour, device to device, the parts that need no GPU: the ABI of include/sf3d_hour.h against the binding, the Python restatements of
relHumFromTdew / computeRelativeHumidityMap and of computeCurrentPond / dailyUpdatePond equal to the compiled-reference pins
tests/golden/relhum_dew.npz and pond_day.npz bit for bit, the pins' arms, the per-cell text of k_hour_relhum and k_hour_pond compiled for
the host (tests/hour_host.cpp) equal to the pins on every value - and once more as a stand-alone program under the address and
undefined-behaviour sanitizers -, the order of restate_totals, and every refusal of the entry points through the C ABI without a device."""
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, catchment as cm, hour, sinks
from tests import hour_cases as hc
from tests import sink_cases as sc
from tests.raster_helpers import bits, build_host_program, declared_entry_points, exported_names, header_text

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def rh():
    return hc.load_relhum_pin()


@pytest.fixture(scope="module")
def pd():
    return hc.load_pond_pin()


def test_hour_header_and_binding_table_agree():
    text, declared = header_text("sf3d_hour.h"), declared_entry_points("sf3d_hour.h", "sf3d_hour_")
    assert declared == sorted(hour.SIGNATURES)
    for k, n in enumerate(("RELHUM", "TOTALS", "POND")):
        assert re.search(rf"SF3D_HOUR_KERNEL_{n} = {k}\b", text) and getattr(hour, "KERNEL_" + n) == k
    args = lambda name: len([a for a in re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1).split(",") if a.strip() and a.strip() != "void"])
    for name, (_, argtypes) in hour.SIGNATURES.items():
        assert args(name) == len(argtypes), name


def test_product_library_exports_the_hour_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(hour.SIGNATURES) <= names
    assert "sf3d_hour" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("sf3d_hour" in n for n in capi.SIGNATURES)
    assert not any("sf3d_hour" in n for n in exported_names(build.build_shim()))


def test_the_pins_reach_every_arm(rh, pd):
    for p in (rh, pd):
        arms = dict(zip((str(n) for n in p["arm_names"]), (int(c) for c in p["arm_counts"])))
        assert all(c > 0 for c in arms.values()), {k: c for k, c in arms.items() if c == 0}
    assert list(rh["arm_names"]) == ["NODATA in", "100", "floor", "between", "flag cell"] and all(int(c) > 0 for c in rh["map_arm_counts"])
    assert float(rh["flag"]) != -9999.0 and float(pd["slope_flag"]) != -9999.0
    assert np.isfinite(rh["rel_hum"]).all() and np.isfinite(rh["map_rel_hum"]).all() and np.isfinite(pd["cell_pond"]).all() and np.isfinite(pd["node_pond"]).all()
    assert rh["map_air_t"].shape == pd["slope"].shape == (7, 37)
    assert list(pd["compute_crop"]) == [1, 0] and len(pd["arm_names"]) == 20
    crops = pd["is_crop"] != 0
    assert crops.any() and (~crops).any() and np.all(pd["lai_max"][crops] > 0)
    assert np.count_nonzero(pd["slope"] == 0) > 10 and float(pd["slope"].max()) > 75.0            # from flat to steep
    assert np.count_nonzero(pd["slope"] == np.float32(-9999.0)) == 1                             # (under the slope map's own flag -9999 is a slope like any other)
    for name in ("relhum_dew.npz", "pond_day.npz"):
        assert (hc.GOLDEN / name).stat().st_size < 100_000


def test_restatements_equal_the_pins(rh, pd):
    assert np.array_equal(bits(hour.rel_hum_from_tdew(rh["dew_t"], rh["air_t"])), bits(rh["rel_hum"]))
    assert np.array_equal(bits(hour.restate_relative_humidity(rh["map_air_t"], rh["map_dew_t"], float(rh["flag"]))), bits(rh["map_rel_hum"]))
    for case in range(2):
        cell = hc.pond_restated(pd, case)
        assert np.array_equal(bits(cell), bits(pd["cell_pond"][case])), case
        # dailyUpdatePond: the node of a cell takes the value unless it is NODATA; the others keep theirs
        on_nodes = hc.pond_restated(pd, case, surface_index=pd["index"])
        node = pd["initial_pond"].copy()
        put = on_nodes != np.float32(-9999.0)
        node[pd["index"][put]] = on_nodes[put].astype(np.float64)
        assert np.array_equal(bits(node), bits(pd["node_pond"][case])), case
        assert np.count_nonzero(node != pd["initial_pond"]) > 200 and np.count_nonzero(node == pd["initial_pond"]) > 10
    assert not np.array_equal(pd["cell_pond"][0], pd["cell_pond"][1])


def test_other_ranks_cells_keep_the_flag_in_the_restatements(rh, pd):
    mine = (np.arange(rh["map_air_t"].size).reshape(rh["map_air_t"].shape) % 3) != 0
    got = hour.restate_relative_humidity(rh["map_air_t"], rh["map_dew_t"], float(rh["flag"]), mine)
    assert np.all(got[~mine] == rh["flag"]) and np.array_equal(bits(got[mine]), bits(rh["map_rel_hum"][mine]))
    pond = hc.pond_restated(pd, 0, mine=mine)
    assert np.all(pond[~mine] == np.float32(-9999.0)) and np.array_equal(bits(pond[mine]), bits(pd["cell_pond"][0][mine]))


def test_host_build_of_the_kernels_text_equals_the_pins(rh, pd, tmp_path):
    exe = build_host_program("hour", tmp_path)
    for case in range(2):
        pairs, raster, pond = hc.run_host(exe, tmp_path, rh, pd, case, tag=str(case))
        assert np.array_equal(bits(pairs), bits(rh["rel_hum"]))
        assert np.array_equal(bits(raster), bits(rh["map_rel_hum"]))
        assert np.array_equal(bits(pond), bits(pd["cell_pond"][case])), case


def test_host_build_runs_clean_under_the_sanitizers(rh, pd, tmp_path):
    """the program has its own main and is not loaded into python; a sanitizer report ends it with a non-zero status"""
    exe = build_host_program("hour", tmp_path, sanitize=True)
    for case in range(2):
        pairs, _, pond = hc.run_host(exe, tmp_path, rh, pd, case, tag=f"san{case}")
        assert np.array_equal(bits(pairs), bits(rh["rel_hum"])) and np.array_equal(bits(pond), bits(pd["cell_pond"][case]))


def test_restate_totals_is_the_sequential_sum_of_the_terms():
    rng = np.random.default_rng(5)
    shape, flag, area = (3, 11), -9999.0, 16.0
    idx = np.arange(33, dtype=np.int32).reshape(shape)
    idx[0, 3] = -1
    dem = np.full(shape, 100.0, np.float32)
    dem[1, 1] = flag
    liquid = rng.uniform(0.0, 3.0, shape).astype(np.float32)
    liquid[2, 2], liquid[2, 3], liquid[0, 3] = flag, -1.0, 2.0
    e, t = rng.uniform(0.0, 0.5, shape), rng.uniform(0.0, 0.4, shape)
    e[1, 1] = t[1, 1] = flag
    terms = hour.total_terms(idx, dem, flag, area, liquid, e, t)
    assert terms.shape == (3, 33) and terms[0, 3] == 0 and terms[0, 2 * 11 + 2] == 0 and terms[0, 2 * 11 + 3] == 0 and not terms[:, 12][1:].any()
    assert terms[0, 12] == area * (float(liquid[1, 1]) / 1000.)              # the rain term does not look at the DEM (criteria3DProject.cpp:939-957)
    assert terms[1, 5] == area * (e[0, 5] / 1000.) and terms[2, 5] == area * (t[0, 5] / 1000.)
    want = np.zeros(3)
    for q in range(3):
        for v in terms[q]:
            want[q] = want[q] + v
    assert np.array_equal(hour.restate_totals(idx, dem, flag, area, liquid, e, t), want)
    mine = np.arange(33).reshape(shape) % 2 == 0
    part = hour.restate_totals(idx, dem, flag, area, liquid, e, t, mine) + hour.restate_totals(idx, dem, flag, area, liquid, e, t, ~mine)
    assert np.allclose(part, want, rtol=1e-14, atol=0)


def test_error_codes_without_a_device():
    pin = sc.load_pin()
    sf = hour.bind(sinks.bind(capi.load_product()))
    lib = sf.lib
    lib.sf3d_clean()
    dem = pin["dem"]
    rows, cols = dem.shape
    n = dem.size
    f = np.zeros(n, np.float32)
    pf = f.ctypes.data_as(hour.pf32)
    tot = np.zeros(3)
    pt = tot.ctypes.data_as(hour.pf64)
    # before the consuming block is initialised
    assert lib.sf3d_hour_relative_humidity(n, pf) == capi.MEMORY_ERROR and lib.sf3d_hour_relative_humidity(n, None) == capi.MEMORY_ERROR
    assert lib.sf3d_hour_snow(n, None, 0.75) == capi.MEMORY_ERROR and lib.sf3d_hour_et0(n, 0.75) == capi.MEMORY_ERROR
    assert lib.sf3d_hour_sinks(n) == capi.MEMORY_ERROR and lib.sf3d_hour_totals(n, pt) == capi.MEMORY_ERROR
    assert lib.sf3d_hour_update_ponds(n, pf) == capi.MEMORY_ERROR and lib.sf3d_hour_update_ponds(n, None) == capi.MEMORY_ERROR
    assert lib.sf3d_hour_kernel_ms(0) == 0.0 and lib.sf3d_hour_kernel_ms(2) == 0.0 and lib.sf3d_hour_kernel_ms(3) == 0.0
    # sf3d_hour_set_ponds: null pointers, sizes, the caps
    slope = np.full(dem.shape, 10.0, np.float32)
    unit = np.zeros(dem.shape, np.int32)
    unit[3, 3] = -1
    many = hour.MAX_UNITS + 1
    mp, lm, ic = np.full(many, 0.01), np.full(many, 4.0), np.ones(many, np.int32)

    def ponds(rows_=rows, cols_=cols, slope_=slope, unit_=unit, nu=2, mp_=mp, lm_=lm, ic_=ic, crop=0):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib.sf3d_hour_set_ponds(rows_, cols_, p(slope_, hour.pf32), -9999.0, p(unit_, hour.pi32), nu, p(mp_, hour.pf64), p(lm_, hour.pf64), p(ic_, hour.pi32), crop)
    assert ponds(rows_=0) == capi.PARAMETER_ERROR and ponds(cols_=0) == capi.PARAMETER_ERROR
    assert ponds(slope_=None) == capi.PARAMETER_ERROR and ponds(unit_=None) == capi.PARAMETER_ERROR
    assert ponds(mp_=None) == capi.PARAMETER_ERROR and ponds(lm_=None) == capi.PARAMETER_ERROR and ponds(ic_=None) == capi.PARAMETER_ERROR
    assert ponds(nu=many) == capi.PARAMETER_ERROR                          # the cap ...
    assert ponds(nu=hour.MAX_UNITS) == capi.OK                             # ... itself is allowed
    beyond = unit.copy()
    beyond[5, 5] = 2
    assert ponds(unit_=beyond) == capi.PARAMETER_ERROR                     # a unit index beyond nUnits
    assert ponds(crop=1) == capi.PARAMETER_ERROR                           # computeCrop without the crop block on this raster
    assert lib.sf3d_hour_clean() == capi.OK and lib.sf3d_hour_update_ponds(n, pf) == capi.MEMORY_ERROR
    assert ponds(nu=0, mp_=None, lm_=None, ic_=None, unit_=np.full(dem.shape, -1, np.int32)) == capi.OK      # no land unit at all
    assert ponds() == capi.OK
    assert lib.sf3d_hour_update_ponds(n - 1, pf) == capi.PARAMETER_ERROR   # wrong nrCells
    assert lib.sf3d_hour_update_ponds(n, pf) == capi.MEMORY_ERROR          # no model
    # the sink block (it needs no device before its first hour)
    sc.initialize(sf, pin)
    assert lib.sf3d_hour_sinks(n - 1) == capi.PARAMETER_ERROR and lib.sf3d_hour_totals(n - 1, pt) == capi.PARAMETER_ERROR
    assert lib.sf3d_hour_totals(n, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_hour_sinks(n) == capi.MEMORY_ERROR and lib.sf3d_hour_totals(n, pt) == capi.MEMORY_ERROR          # no model
    m = cm.catchment_model(cols, rows, len(pin["layer_depth"]))
    cm.build(sf, m, finalize=False)                                        # host-side staging only
    assert lib.sf3d_hour_sinks(n) == capi.TOPOGRAPHY_ERROR and lib.sf3d_hour_totals(n, pt) == capi.TOPOGRAPHY_ERROR  # no column table
    assert lib.sf3d_hour_update_ponds(n, pf) == capi.TOPOGRAPHY_ERROR
    sinks.set_columns(sf, pin["columns"][:4], pin["layer_thickness"][:4])
    assert lib.sf3d_hour_sinks(n) == capi.TOPOGRAPHY_ERROR and lib.sf3d_hour_totals(n, pt) == capi.TOPOGRAPHY_ERROR  # one of another layer grid
    sinks.set_columns(sf, pin["columns"], pin["layer_thickness"])
    assert lib.sf3d_hour_sinks(n) == capi.PARAMETER_ERROR                  # no crop block to read
    assert lib.sf3d_hour_totals(n, pt) == capi.PARAMETER_ERROR             # no sink hour computed
    assert lib.sf3d_sink_compute_hour(n, pf, pf, pf, None) == capi.PARAMETER_ERROR      # the existing call does not take the meteo block's rain
    assert lib.sf3d_clean() == capi.OK
    assert lib.sf3d_hour_update_ponds(n, pf) == capi.MEMORY_ERROR          # sf3d_clean forgets sf3d_hour_set_ponds
