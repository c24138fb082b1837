"""Hourly ET0, daily extremes and the daily crop maps, the parts that need no GPU: the numpy restatements equal the compiled-reference
pin tests/golden/crop_et0.npz bit for bit at every checkpoint, the pin reaches every arm, the small rasters of the GPU test hold ET0 and
LAI on the shares of cells it asks for, the crop-table reader and isCrop on the
Ravone project's crop rows, the C entry points of include/sf3d_crop.h and the binding table, the crop/ state folder; and the host build of the kernels' per-cell
text (tests/crop_host.cpp): equal to the pin and to the restatement bit for bit, clean under the address and undefined-behaviour sanitizers."""
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from criteria3d_amd import build, capi, crop, esri, project3d as p3
from tests import crop_cases as cc
from tests import tolerances
from tests.raster_helpers import bits as _bits, build_host_program, declared_entry_points, differing, exported_names, header_text

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return cc.load_pin()


def test_crop_header_and_binding_table_agree():
    text, declared = header_text("sf3d_crop.h"), declared_entry_points("sf3d_crop.h", "sf3d_crop_")
    assert declared == sorted(crop.SIGNATURES)
    assert not set(declared) & set(capi.SIGNATURES)          # sf3d.h (the drop-in ABI) is unchanged
    for k, n in enumerate(("DEGREE_DAYS", "LAI", "DAILY_TMIN", "DAILY_TMAX")):
        assert re.search(rf"SF3D_CROP_{n} = {k}\b", text) and getattr(crop, n) == k
    assert re.search(rf"#define SF3D_CROP_MAX_UNITS {crop.MAX_UNITS}\b", text)
    import ctypes
    assert ctypes.sizeof(crop.Unit) == 96


def test_product_library_exports_the_crop_entry_points():
    names = exported_names(build.build_product())
    assert set(crop.SIGNATURES) <= names


def test_error_codes_without_a_raster():
    sf = crop.bind(capi.load_product())
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data_as(crop.pf32)
    assert sf.lib.sf3d_crop_get_state(0, 16, p) == capi.MEMORY_ERROR
    assert sf.lib.sf3d_crop_set_state(0, 16, p) == capi.MEMORY_ERROR
    assert sf.lib.sf3d_crop_get_et0(16, p) == capi.MEMORY_ERROR
    assert sf.lib.sf3d_crop_set_degree_days(16, p, 100) == capi.MEMORY_ERROR
    assert sf.lib.sf3d_crop_compute_hour(16, p, p, p, p, p, 0.75) == capi.MEMORY_ERROR
    assert sf.lib.sf3d_crop_daily_update(1, 1) == capi.MEMORY_ERROR
    idx = np.zeros(16, np.int32)
    pi = idx.ctypes.data_as(crop.pi32)
    units = crop.unit_array([])
    assert sf.lib.sf3d_crop_initialize(0, 4, p, -9999.0, pi, 0, units, 44.5) == capi.PARAMETER_ERROR
    assert sf.lib.sf3d_crop_initialize(4, 4, None, -9999.0, pi, 0, units, 44.5) == capi.PARAMETER_ERROR
    assert sf.lib.sf3d_crop_initialize(4, 4, p, -9999.0, None, 0, units, 44.5) == capi.PARAMETER_ERROR
    assert sf.lib.sf3d_crop_initialize(4, 4, p, -9999.0, pi, crop.MAX_UNITS + 1, units, 44.5) == capi.PARAMETER_ERROR      # more units than the cap
    assert sf.lib.sf3d_crop_initialize(4, 4, p, -9999.0, pi, 0, units, 44.5) == capi.PARAMETER_ERROR                       # crop index 0 >= nUnits 0
    assert sf.lib.sf3d_crop_clean() == capi.OK
    assert sf.lib.sf3d_crop_kernel_ms(0) == 0.0 and sf.lib.sf3d_crop_kernel_ms(1) == 0.0


def test_the_pin_reaches_every_arm(pin):
    dem, flag = pin["dem"], pin["flag"]
    assert dem.shape == (24, 32) and cc.PIN.stat().st_size <= (ROOT / "tests" / "golden" / "snow_brooks.npz").stat().st_size
    assert list(pin["window"]) == [8, 280, 24, 32]                      # the snow pin's window
    valid = np.abs(dem.astype(np.float64) - float(flag)) >= 1e-5
    assert 0 < int(valid.sum()) < dem.size
    odd = valid & (np.trunc(dem.astype(np.float64)) == float(flag))
    assert int(odd.sum()) == 1                                           # the cell where the two validity tests disagree
    assert [str(n) for n in pin["map_names"]] == list(crop.MAPS) and [str(n) for n in pin["input_names"]] == list(crop.INPUT)
    assert [str(n) for n in pin["unit_fields"]] == list(crop.UNIT_FIELDS)
    ops = pin["ops"]
    assert int((ops[:, 0] == cc.OP_HOUR).sum()) == pin["input_codes"].shape[0] <= 400
    assert int((ops[:, 0] == cc.OP_CHECKPOINT).sum()) == pin["maps"].shape[0] >= 10
    assert np.isfinite(pin["maps"]).all() and np.isfinite(pin["inputs"]).all() and np.isfinite(pin["set_maps"]).all()
    types = {int(u["type"]) for u in pin["unit_list"] if int(u["isCrop"])}
    assert {crop.HERBACEOUS_ANNUAL, crop.HORTICULTURAL, crop.GRASS, crop.TREE} <= types
    assert any(not int(u["isCrop"]) for u in pin["unit_list"]) and (pin["unit_index"] < 0).any()
    days = sorted({int(a) for op, a, b in ops if op == cc.OP_DAY})
    assert set(range(300, 341)) <= set(days) and {364, 1, 2} <= set(days)
    arms = dict(zip((str(n) for n in pin["arm_names"]), (int(c) for c in pin["arm_counts"])))
    assert len(arms) >= 40 and all(c > 0 for c in arms.values()), {k: c for k, c in arms.items() if c == 0}
    for must in ("ET0: net radiation <= 0 (night)", "ET0: transmissivity above clear sky (min with 1)", "ET0: cloud factor clipped at 0", "ET0: sum clipped at 0",
                 "ET0: no air temperature", "ET0: no relative humidity", "ET0: no wind", "ET0: no global radiation", "ET0: no transmissivity",
                 "ET0: DEM cell by isEqual, not by int()", "day: reset (first doy) per cell", "day: inside the cycle across the year end",
                 "LAI: tree in the 30-day senescence", "LAI: tree after the senescence", "LAI: sown crop falling", "LAI: perennial falling"):
        assert arms[must] > 0, must
    calls = json.loads(str(pin["library_calls"]))
    assert "pow" in calls["ET0_Penman_hourly"] and "pow" in calls["pressureFromAltitude"] and {"exp", "pow"} <= set(calls["getLAICriteria"])


def test_restatements_equal_the_compiled_reference_at_every_checkpoint(pin):
    exact, why = tolerances.libm_probe()
    print(why)
    seen = []

    def at(k, maps):
        for j, n in enumerate(crop.MAPS):
            want = pin["maps"][k][j]
            assert np.isfinite(maps[n]).all() and np.isfinite(want).all()
            bad = _bits(maps[n]) != _bits(want)
            print(f"checkpoint {k} {n}: {int(bad.sum())} cells differ")
            if exact:
                assert not bad.any(), (k, n, int(bad.sum()), maps[n][bad][:4], want[bad][:4])
            else:           # another C library: its exp / log / pow may differ in the last place of a double, far below the float the maps hold
                assert np.allclose(maps[n], want, rtol=1e-6, atol=1e-6), (k, n)
        seen.append(k)

    n = cc.replay(pin, cc.Restated(pin), at)
    assert n == pin["maps"].shape[0] and seen == list(range(n))
    # not vacuous: ET0 positive somewhere at some checkpoint, LAI and degree days present, extremes present before a day closes
    names = list(crop.MAPS)
    assert (pin["maps"][:, names.index("et0")] > 0).any() and (pin["maps"][:, names.index("lai")] > 0).any()
    assert (pin["maps"][:, names.index("dailyTmax")] > -100).any()


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_rasters_hold_et0_and_lai_on_the_shares_the_gpu_test_asks_for(pin, shape):
    """the bounds of tests/test_gpu_crop.py's small-raster test are the restatement's: 200 and 50 cells of the 255 DEM cells of 7 x 37"""
    r = cc.small_raster(pin, shape)
    dem, flag = r["dem"], np.float32(r["flag"])
    assert dem.shape == shape and np.all(dem.flat[:3] == flag) and dem.flat[-1] == flag and dem[r["inner"]] == np.float32(-9999.5)
    assert np.all(r["idx"].flat[-4:-1] == 3) and int(pin["unit_list"][3]["type"]) == crop.TREE
    assert r["dem_cells"] == dem.size - 4
    if shape == (7, 37):
        assert cc.ET0_SHARE * r["dem_cells"] == 200 and cc.LAI_SHARE * r["dem_cells"] == 50
    after_degree_days, after_hour, after_day = cc.small_raster_stages(r)
    assert np.all(after_degree_days["et0"] == flag) and np.count_nonzero(after_degree_days["degreeDays"] != flag) > 0
    et0 = after_hour["et0"]
    assert np.count_nonzero(et0 > 0) > cc.ET0_SHARE * r["dem_cells"] and et0.flat[-2] > 0 and et0[r["inner"]] == flag and et0.flat[-1] == flag
    assert np.count_nonzero(after_day["lai"] > 0) > cc.LAI_SHARE * r["dem_cells"]
    for stage in (after_degree_days, after_hour, after_day):
        assert sorted(stage) == sorted(crop.MAPS) and all(np.isfinite(v).all() for v in stage.values())


def test_point_models_by_hand():
    u = dict(type=crop.HERBACEOUS_ANNUAL, isCrop=1, sowingDoy=300, plantCycle=200, LAImin=0.0, LAImax=5.0, LAIgrass=0.0, LAIcurve_a=4.0, LAIcurve_b=-0.006,
             thermalThreshold=0.0, upperThermalThreshold=30.0, degreeDaysIncrease=1400.0, degreeDaysDecrease=1200.0, degreeDaysEmergence=120.0)
    assert crop.is_inside_typical_cycle(u, 300) and crop.is_inside_typical_cycle(u, 1) and crop.is_inside_typical_cycle(u, 134)
    assert not crop.is_inside_typical_cycle(u, 135) and not crop.is_inside_typical_cycle(u, 299)
    assert crop.simple_lai(u, np.array([119.0]), 44.5, 10)[0] == 0.0                           # before emergence
    tree = dict(u, type=crop.TREE, LAImin=1.0, LAImax=4.0, LAIgrass=0.5)
    assert crop.simple_lai(tree, np.array([0.0]), 44.5, 100)[0] == 1.5                        # LAImin + LAIgrass
    assert crop.simple_lai(tree, np.array([500.0]), 44.5, 336)[0] == 1.5                      # 31 days after the start of the leaf fall
    assert abs(crop.simple_lai(tree, np.array([500.0]), 44.5, 305)[0] - 3.5) < 1e-12          # day 0: LAImax * 0.75 + LAIgrass
    assert crop.simple_lai(tree, np.array([500.0]), -35.0, 182)[0] > 1.5                      # south: no leaf fall from doy 182 on
    flag = np.float32(-9999.0)
    tmin, tmax = crop.restate_daily_temperatures(np.array([flag, 5.0, 5.0], np.float32), np.array([flag, 9.0, 9.0], np.float32), np.array([3.0, flag, 12.0], np.float32))
    assert list(tmin) == [3.0, 5.0, 5.0] and list(tmax) == [3.0, 9.0, 12.0]
    # ET0: a cell at -9999.5 is no DEM cell for computeET0PMMap
    met = {k: np.full((1, 2), v, np.float32) for k, v in zip(crop.INPUT, (20.0, 50.0, 2.0, 500.0, 0.6))}
    et0 = crop.restate_et0_hour(np.array([[100.0, -9999.5]], np.float32), met)
    assert 0.1 < et0[0, 0] < 1.0 and et0[0, 1] == flag


def test_crop_table_reader_and_is_crop():
    rows = json.loads((ROOT / "tests" / "golden" / "ravone_crops.json").read_text())
    assert rows["columns"][:3] == ["id_crop", "crop_name", "type"]
    inp = p3.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz")
    table = p3.crop_table(rows["crop"], inp.land_units)
    assert [t["id_crop"] for t in table] == [u["id_crop"] for u in inp.land_units] == ["SHRUB", "BROADLEAF", "BARE"]
    assert [t["isCrop"] for t in table] == [1, 1, 0]
    shrub, broad, bare = table
    assert shrub["type"] == crop.TREE and broad["type"] == crop.TREE and bare["type"] == crop.BARESOIL
    assert (shrub["LAImin"], shrub["LAImax"], shrub["LAIgrass"], shrub["thermalThreshold"], shrub["upperThermalThreshold"]) == (0.5, 3.0, 0.0, 3.0, 35.0)
    assert (broad["degreeDaysIncrease"], broad["degreeDaysDecrease"], broad["degreeDaysEmergence"]) == (2500.0, 1000.0, 0.0)
    assert (broad["LAIcurve_a"], broad["LAIcurve_b"], broad["plantCycle"], broad["sowingDoy"]) == (4.1, -0.014, 365, -9999)      # '' -> NODATA (getValue)
    assert set(crop.UNIT_FIELDS) <= set(shrub)
    crop.unit_array(table)                                               # the binding takes the reader's entries as they are
    for cid, want in (("", False), (None, False), ("BARE", False), ("bare", False), ("SHRUB", True), ("Bare soil", True)):
        assert p3.is_crop(cid) is want, cid
    with pytest.raises(ValueError):
        p3.crop_table(rows["crop"], [dict(id=9, id_crop="NOSUCHCROP")])
    # the index map the table is indexed by is the one project_model derives
    idx = p3.land_unit_index(inp)
    assert idx.shape == inp.dem.shape and set(np.unique(idx)) <= {-1, 0, 1, 2} and (idx >= 0).any()


def test_state_directory_round_trip(tmp_path, pin):
    names = list(crop.MAPS)
    maps = {n: pin["maps"][3][names.index(n)] for n in crop.STATE}
    got = {}
    shape = pin["dem"].shape
    sf = SimpleNamespace(_crop_shape=shape, check=lambda code, what="": None, lib=SimpleNamespace())

    def get_state(which, size, ptr):
        np.ctypeslib.as_array(ptr, shape=(size,))[:] = maps[crop.STATE[which]].ravel()
        return 0

    def set_state(which, size, ptr):
        got[crop.STATE[which]] = np.ctypeslib.as_array(ptr, shape=(size,)).copy().reshape(shape)
        return 0
    sf.lib.sf3d_crop_get_state, sf.lib.sf3d_crop_set_state = get_state, set_state
    header = dict(xllcorner=683768.0, yllcorner=4928326.0, cellsize=4.0, nodata=-9999.0)
    d = crop.save_crop_state(sf, tmp_path, header)
    assert d == tmp_path / "crop"
    assert sorted(p.name for p in d.iterdir()) == sorted(f"{s}{e}" for s in crop.STATE_FILES.values() for e in (".flt", ".hdr"))
    grid, hdr = esri.read_grid(d / "LAI")
    assert hdr["cellsize"] == 4.0 and np.array_equal(_bits(grid), _bits(maps["lai"]))
    crop.load_crop_state(sf, tmp_path)
    assert sorted(got) == sorted(crop.STATE)
    for n in crop.STATE:
        assert np.array_equal(_bits(got[n]), _bits(maps[n])), n


# ---- the host build of the per-cell text of k_et0_hour and k_crop_day (tests/crop_host.cpp): the text == the pin, the text == the restatement

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crop_host")
    return SimpleNamespace(dir=d, exe=build_host_program("crop", d), san=build_host_program("crop", d, sanitize=True))


def _random_scripts(pin):
    for shape in cc.SHAPES:
        for seed in cc.SEEDS:
            for continuous in (False, True):
                r, ops = cc.random_script(pin, shape, seed, continuous)
                yield f"{'continuous' if continuous else 'lists'}-{shape[0]}x{shape[1]}-{seed}", r, ops


def test_host_text_equals_the_pin_at_every_checkpoint(pin, host):
    """no libm escape: the text carries its own exp, log and pow"""
    got = cc.run_host(host.exe, host.dir, "pin", pin, cc.pin_script(pin))
    assert len(got) == pin["maps"].shape[0]
    for k, maps in enumerate(got):
        for j, n in enumerate(crop.MAPS):
            bad = differing(maps[n], pin["maps"][k][j])
            print(f"host text, checkpoint {k} {n}: values differ: {int(bad.sum())}")
            assert not bad.any(), (k, n, int(bad.sum()), maps[n][bad][:4], pin["maps"][k][j][bad][:4])


def test_host_text_equals_the_restatement_on_random_scripts(pin, host):
    """both hemispheres, the leaf fall of the south (days 119 to 152), the year's first day at 182, night hours; the value lists of
    small_forcing and continuous ranges, four seeds per shape"""
    exact, why = tolerances.libm_probe()
    print(why)
    for name, r, ops in _random_scripts(pin):
        p = cc.as_pin(r, pin)
        want, got = cc.run_script(cc.Restated(p), ops), cc.run_host(host.exe, host.dir, name, p, ops)
        assert len(got) == len(want) == 15
        differ = 0
        for k, (g, w) in enumerate(zip(got, want)):
            for n in crop.MAPS:
                bad = differing(g[n], w[n])
                differ += int(bad.sum())
                if exact:
                    assert not bad.any(), (name, k, n, int(bad.sum()), g[n][bad][:4], w[n][bad][:4])
                else:           # another C library under the restatement: the tolerance of the restatement's own test above
                    assert np.allclose(g[n], w[n], rtol=1e-6, atol=1e-6), (name, k, n)
        print(f"{name}: values differ: {differ}")


def test_random_scripts_are_not_vacuous(pin):
    """the shares tests/test_gpu_crop.py asks of its small rasters, from the restatement; the south loses its leaves and starts its year"""
    flag = np.float32(-9999.0)
    for name, r, ops in _random_scripts(pin):
        cps = cc.run_script(cc.Restated(cc.as_pin(r, pin)), ops)
        after_dd, after_hour, after_day, after_night, after_next = cps[:5]
        cells = r["dem_cells"]
        assert np.count_nonzero(after_hour["et0"] > 0) > cc.ET0_SHARE * cells, name
        assert np.count_nonzero(after_day["lai"] > 0) > cc.LAI_SHARE * cells and np.count_nonzero(after_next["lai"] > 0) > cc.LAI_SHARE * cells, name
        assert np.count_nonzero(after_night["et0"] != flag) > 0 and np.count_nonzero(after_hour["dailyTmax"] != flag) > 0, name
        south = cps[5:]
        tree = (r["idx"] == 3) & (south[0]["lai"] != flag)
        assert tree.sum() >= 3, name                                                      # the three lanes before the last hold a tree
        day119, day120, day121, day150, day151, day152, day181, day182, day183 = south[1:]
        # (a tree without a temperature that day keeps its LAI, so these are counts)
        assert np.count_nonzero(day121["lai"][tree] < day120["lai"][tree]) > tree.sum() // 2, name      # the leaves fall from day 120 on
        assert np.count_nonzero(day150["lai"][tree] > day151["lai"][tree]) > 0 and np.count_nonzero(day152["lai"][tree] == day151["lai"][tree]) > 0, name      # 30 days, then LAImin
        held = lambda m: np.count_nonzero(m["degreeDays"] != flag)
        assert held(day181) > 0 and np.all(day182["degreeDays"][day182["degreeDays"] != flag] <= 40.0), name      # day 182 starts the year: one day's degrees at the most
        assert np.count_nonzero(day181["degreeDays"] > 40.0) > 0, name


def test_sanitized_host_build_reports_nothing(pin, host):
    """address and undefined-behaviour sanitizers on the pin, on every random script and on the edge cases: exit 0, nothing on stderr"""
    cc.run_host(host.san, host.dir, "san-pin", pin, cc.pin_script(pin))
    runs = 1
    for name, r, ops in _random_scripts(pin):
        cc.run_host(host.san, host.dir, "san-" + name, cc.as_pin(r, pin), ops)
        runs += 1
    sf = capi.load_product()
    for name, r, ops in cc.edge_scripts(pin):
        p = cc.as_pin(r, pin)
        assert cc.accepted(sf, p), name
        want, got = cc.run_script(cc.Restated(p), ops), cc.run_host(host.san, host.dir, "san-" + name, p, ops)
        if tolerances.libm_probe()[0]:
            assert all(not differing(g[n], w[n]).any() for g, w in zip(got, want) for n in crop.MAPS), name
        runs += 1
    assert np.count_nonzero(r["dem"] != np.float32(r["flag"])) > 0
    print(f"crop_host_san: {runs} runs, nothing reported")
