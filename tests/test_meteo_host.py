"""The hourly meteo maps from station data, the parts that need no GPU: the ABI of include/sf3d_meteo.h against the binding, the Python
restatement of interpolate() equal to the compiled-reference pin tests/golden/meteo_idw.npz bit for bit in every cell of every case, the
pin's arms and cases, the neighbourhood sizes and the distinct distances of the small rasters of the GPU test, the caps and the options that stay with the caller refused through the C ABI without a device, and the entry
points absent from sf3d.h and the drop-in shim."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, meteo
from tests import meteo_cases as mc
from tests.raster_helpers import bits, declared_entry_points, exported_names, header_text

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return mc.load_pin()


def test_meteo_header_and_binding_table_agree():
    text, declared = header_text("sf3d_meteo.h"), declared_entry_points("sf3d_meteo.h", "sf3d_meteo_")
    assert declared == sorted(meteo.SIGNATURES)
    assert re.search(rf"#define SF3D_METEO_MAX_STATIONS {meteo.MAX_STATIONS}\b", text) and re.search(rf"#define SF3D_METEO_MAX_PROXIES {meteo.MAX_PROXIES}\b", text)
    for k, n in enumerate(("AIR_TEMPERATURE", "PRECIPITATION", "AIR_REL_HUMIDITY", "WIND_SCALAR_INTENSITY", "GLOBAL_IRRADIANCE", "ATM_TRANSMISSIVITY",
                           "AIR_DEW_TEMPERATURE")):
        assert re.search(rf"SF3D_METEO_{n} = {k}\b", text) and getattr(meteo, n) == k
    assert re.search(r"SF3D_METEO_VARIABLES = 7\b", text) and len(meteo.VARIABLES) == 7
    for k, n in enumerate(("IDW", "SHEPARD", "SHEPARD_MODIFIED")):
        assert re.search(rf"SF3D_METEO_{n} = {k}\b", text) and getattr(meteo, n) == k
    proxy = re.search(r"typedef struct \{([^}]*)\} sf3d_meteo_proxy_t;", text).group(1)
    assert re.findall(r"int32_t (\w+);", proxy) == list(meteo.PROXY_INT_FIELDS) + ["reserved"]
    assert [n.strip() for n in re.search(r"float ([\w, ]+);", proxy).group(1).split(",")] == list(meteo.PROXY_FLOAT_FIELDS)
    settings = re.search(r"typedef struct \{([^}]*)\} sf3d_meteo_settings_t;", text).group(1)
    assert re.findall(r"(?:int32_t|float) (\w+);", settings) == [n for n, _ in meteo.Settings._fields_[:-1]]
    assert ctypes.sizeof(meteo.Proxy) == 32 and ctypes.sizeof(meteo.Settings) == 48 + 32 * meteo.MAX_PROXIES and meteo.Settings.proxy.offset == 48


def test_product_library_exports_the_meteo_entry_points():
    names = exported_names(build.build_product())
    assert set(meteo.SIGNATURES) <= names


def test_meteo_entry_points_are_not_part_of_the_drop_in_abi():
    assert "sf3d_meteo" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("meteo" in n.lower() for n in capi.SIGNATURES) and not any("meteo" in n.lower() for n in capi.REFERENCE_API)
    assert not any("meteo" in n.lower() for n in exported_names(build.build_shim()))


def test_the_pin_reaches_every_arm_and_case(pin):
    assert pin["dem"].shape == (24, 32) and list(pin["window"]) == [8, 280, 24, 32] and mc.PIN.stat().st_size < (1 << 20)
    assert float(pin["cell_size"]) == 4.0                              # the project's cell size
    arms = dict(zip((str(n) for n in pin["arm_names"]), (int(c) for c in pin["arm_counts"])))
    assert len(arms) >= 30 and all(c > 0 for c in arms.values()), {k: c for k, c in arms.items() if c == 0}
    for must in ("cell: no stations", "list: a station on the cell centre (distance 0)", "list: fewer than 5 in the radius (the 5 nearest, sorted)",
                 "list: the sorted list is shorter than 5", "list: 5 to 10 in the radius (input order)", "list: more than 10 in the radius (the 10 nearest, sorted)",
                 "retrend: height below 0", "retrend: inversion, height in (H0, H1]", "retrend: inversion, height above H1", "retrend: another proxy without value",
                 "retrend: a variable that is not detrended, proxy active", "tail: precipitation all zero", "tail: precipitation below the threshold",
                 "tail: precipitation above the threshold", "tail: humidity clamped at 0", "tail: humidity clamped at 100", "tail: clamped at 0"):
        assert arms[must] > 0, must
    assert list(pin["set_sizes"]) == [0, 1, 4, 7, 12, 40]
    combos = {(c["set"], c["method"]) for c in pin["cases"]}
    assert combos >= {(s, m) for s in range(6) for m in range(3)}           # each method on each station set
    assert {c["var"] for c in pin["cases"]} == set(range(7))
    x, y = pin["sets"][5]
    w, h = 32 * 4.0, 24 * 4.0
    outside = (x < float(pin["xll"])) | (x > float(pin["xll"]) + w) | (y < float(pin["yll"])) | (y > float(pin["yll"]) + h)
    assert outside.any() and (~outside).any()                               # stations outside the window and inside
    cx, cy = meteo.cell_centres((24, 32), float(pin["xll"]), float(pin["yll"]), 4.0)
    r, c = pin["centre_cell"]
    assert any(x[i] == cx[r, c] and y[i] == cy[r, c] for i in range(len(x)))
    assert (pin["dem"][pin["dem"] != pin["flag"]] < 0).any() and (pin["other_proxy"][pin["dem"] != pin["flag"]] == pin["flag"]).any()
    assert np.isfinite(pin["maps"]).all()


def test_no_cell_has_two_stations_at_equal_float_distances(pin):
    """the condition under which the order of std::sort among equal keys cannot show (checked here on the restatement's distances)"""
    cx, cy = meteo.cell_centres(pin["dem"].shape, float(pin["xll"]), float(pin["yll"]), float(pin["cell_size"]))
    xf, yf = cx.astype(np.float32).ravel(), cy.astype(np.float32).ravel()
    for x, y in pin["sets"]:
        if len(x) < 2:
            continue
        dx, dy = x.astype(np.float32)[None, :] - xf[:, None], y.astype(np.float32)[None, :] - yf[:, None]
        d = np.sort(np.sqrt(dx * dx + dy * dy), axis=1)
        assert not (d[:, 1:] == d[:, :-1]).any(), len(x)


def test_small_rasters_hold_every_neighbourhood_size_and_no_equal_distances(pin):
    """3 x 11 and 1 x 300 cells under 300 stations (tests/test_gpu_meteo.py): counted with float distances as meteo._neighbours counts
    them, the single row holds cells with fewer than 5 stations inside the initial radius (the 5 nearest of all, sorted), with 5 to 10
    (input order) and with more than 10 (the 10 nearest, sorted); no cell of either raster has two stations at equal float distance"""
    for shape in mc.SMALL_SHAPES:
        r = mc.small_raster(pin, shape)
        assert r["dem"].shape == shape and len(r["x"]) == len(r["y"]) == len(r["value"]) == mc.SMALL_STATIONS == 256 + 44
        assert np.array_equal(r["x"], mc.cap_raster(pin)["x"][:300]) and r["dem"].flat[0] == r["flag"] and r["dem"].flat[-1] != r["flag"]
        d = mc.float_distances(r)
        assert d.dtype == np.float32 and d.shape == (r["dem"].size, 300)
        radius = meteo.shepard_initial_radius(r["area"], 300)
        inside = np.count_nonzero((d <= radius) & (d > 0), axis=1)
        few, some, many = (int(np.count_nonzero(k)) for k in (inside < meteo.SHEPARD_MIN, (inside >= meteo.SHEPARD_MIN) & (inside <= meteo.SHEPARD_MAX),
                                                             inside > meteo.SHEPARD_MAX))
        print(f"{shape}: radius {radius}, cells with < 5 stations inside {few}, with 5 to 10 {some}, with more {many}")
        for cell in (1, r["dem"].size - 1):                                  # the counts are _neighbours' own
            idx, rad = meteo._neighbours(d[cell], radius)
            assert len(idx) == (meteo.SHEPARD_MIN if inside[cell] < meteo.SHEPARD_MIN else min(inside[cell], meteo.SHEPARD_MAX))
            assert (rad == radius) == (meteo.SHEPARD_MIN <= inside[cell] <= meteo.SHEPARD_MAX)
        if shape == (1, 300):
            assert few > 0 and some > 0 and many > 0, (few, some, many)
        else:
            assert some > 0 and many > 0, (few, some, many)
        ds = np.sort(d, axis=1)
        assert not (ds[:, 1:] == ds[:, :-1]).any() and ds.min() > meteo.EPSILON, shape


def test_restatement_equals_the_compiled_reference_in_every_cell_of_every_case(pin):
    flag = float(pin["flag"])
    computed = 0
    for k, c in enumerate(pin["cases"]):
        got = mc.restated(pin, c)
        bad = bits(got) != bits(c["want"])
        if bad.any():
            print(f"case {k} {mc.case_name(c)}: {int(bad.sum())} values differ")
        assert np.array_equal(bits(got), bits(c["want"])), (k, mc.case_name(c), int(bad.sum()), got[bad][:4], c["want"][bad][:4])
        computed += int((got != flag).sum())
    assert computed > 30000                                                 # not vacuous
    # the methods differ from each other where they should
    a, b, c3 = (pin["cases"][15 + m]["want"] for m in range(3))             # the 40-station set, air temperature
    valid = pin["dem"] != pin["flag"]
    assert (a[valid] != b[valid]).any() and (b[valid] != c3[valid]).any()


def test_restatement_by_hand():
    dem = np.array([[10.0, -9999.0]], np.float32)
    cx, cy = meteo.cell_centres(dem.shape, 100.0, 200.0, 2.0)
    assert cx[0, 0] == 101.0 and cx[0, 1] == 103.0 and cy[0, 0] == 201.0
    one = lambda method, **kw: meteo.restate_interpolate(dem, 100.0, 200.0, 2.0, [None], "airT", method, [104.0, 101.0], [205.0, 201.0], [7.5, 99.0], 12.0, **kw)
    for method in meteo.METHODS:                                            # the second station lies on the cell: it is left out, the first alone decides
        out = one(method)
        assert out[0, 0] == np.float32(7.5) and out[0, 1] == np.float32(-9999.0), method
    st = dict(proxies=[dict(active=1, isHeight=1, inversion=0, slope=-0.5)])
    assert one("idw", settings=st)[0, 0] == np.float32(2.5)                 # 7.5 + 10 * -0.5
    assert one("idw", settings=dict(st, useDetrending=0))[0, 0] == np.float32(7.5)
    none = meteo.restate_interpolate(dem, 100.0, 200.0, 2.0, [], "prec", "shepard", [], [], [], 0.0)
    assert none[0, 0] == np.float32(-9999.0)
    assert meteo.shepard_initial_radius(np.float32(100.0), 8) == np.float32(np.sqrt(np.float64(np.float32(800.0) / (np.float32(meteo.PI) * np.float32(8)))))
    assert meteo._tail(meteo.AIR_REL_HUMIDITY, np.float32(120.0), np.float32(0)) == 100 and meteo._tail(meteo.AIR_REL_HUMIDITY, np.float32(-3.0), np.float32(0)) == 0
    assert meteo._tail(meteo.PRECIPITATION, np.float32(0.1), np.float32(0.2)) == 0 and meteo._tail(meteo.PRECIPITATION, np.float32(0.2), np.float32(0.2)) == np.float32(0.2)
    assert meteo._tail(meteo.WIND_SCALAR_INTENSITY, np.float32(-1.0), np.float32(0)) == 0 and meteo._tail(meteo.AIR_TEMPERATURE, np.float32(-1.0), np.float32(0)) == -1


def test_caps_and_unsupported_options_without_a_device(pin):
    sf = meteo.bind(capi.load_product())
    lib = sf.lib
    n = 16
    f = np.zeros(n, np.float32)
    pf = f.ctypes.data_as(meteo.pf32)
    assert lib.sf3d_meteo_get_map(0, n, pf) == capi.MEMORY_ERROR            # before initialise
    assert lib.sf3d_meteo_kernel_ms() == 0.0
    # sf3d_meteo_initialize: refused before any device work
    maps9 = (meteo.pf32 * 9)(*[pf] * 9)
    assert lib.sf3d_meteo_initialize(0, 4, pf, -9999.0, 0.0, 0.0, 4.0, 0, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_meteo_initialize(4, 0, pf, -9999.0, 0.0, 0.0, 4.0, 0, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_meteo_initialize(4, 4, None, -9999.0, 0.0, 0.0, 4.0, 0, None) == capi.PARAMETER_ERROR
    assert lib.sf3d_meteo_initialize(4, 4, pf, -9999.0, 0.0, 0.0, 0.0, 0, None) == capi.PARAMETER_ERROR           # cell size
    assert lib.sf3d_meteo_initialize(4, 4, pf, -9999.0, 0.0, 0.0, 4.0, meteo.MAX_PROXIES + 1, maps9) == capi.PARAMETER_ERROR   # the proxy cap
    assert lib.sf3d_meteo_initialize(4, 4, pf, -9999.0, 0.0, 0.0, 4.0, 2, None) == capi.PARAMETER_ERROR
    # sf3d_meteo_interpolate
    many = meteo.MAX_STATIONS + 1
    x = np.zeros(many, np.float64)
    v = np.zeros(many, np.float32)
    px, pv = x.ctypes.data_as(meteo.pf64), v.ctypes.data_as(meteo.pf32)
    ok = meteo.settings_struct(dict(proxies=[dict(active=1, isHeight=1, slope=-0.006)]))
    call = lambda var=0, method=0, ns=4, st=ok, xs=px: lib.sf3d_meteo_interpolate(var, method, ns, xs, px, pv, 100.0, ctypes.byref(st) if st is not None else None, None)
    assert call() == capi.MEMORY_ERROR                                      # a valid call, no raster yet
    assert call(ns=meteo.MAX_STATIONS) == capi.MEMORY_ERROR                 # the cap itself is allowed
    assert call(ns=many) == capi.PARAMETER_ERROR                            # beyond it
    assert call(var=-1) == capi.PARAMETER_ERROR and call(var=len(meteo.VARIABLES)) == capi.PARAMETER_ERROR
    assert call(method=-1) == capi.PARAMETER_ERROR and call(method=3) == capi.PARAMETER_ERROR
    assert call(st=None) == capi.PARAMETER_ERROR and call(xs=None) == capi.PARAMETER_ERROR
    assert call(st=meteo.settings_struct(dict(proxies=[{}] * (meteo.MAX_PROXIES + 1)))) == capi.PARAMETER_ERROR
    for option in meteo.UNSUPPORTED:                                        # what stays with the caller
        assert call(st=meteo.settings_struct({option: 1})) == capi.PARAMETER_ERROR, option
    assert len(meteo.UNSUPPORTED) == 7
    assert lib.sf3d_meteo_clean() == capi.OK
