"""Local detrending with every proxy, the parts that need no GPU: the ABI of include/sf3d_localproxies.h against the binding; the entry
points exported by the product library and absent from sf3d.h and the shim; the refusals that come before any device work; the pin's arm
list; the per-cell text of k_localdetrend_proxies compiled for the host (tests/localproxies_host.cpp) equal to the compiled-reference pin
tests/golden/localproxies.npz in every recorded quantity on both rasters, and once more as a stand-alone program under the address and
undefined-behaviour sanitizers; the same host text with no other proxy active equal to the pin of the height alone
(tests/golden/localdetrend.npz); the Python restatement equal to the pin on every cell of `tiny`; and off the pin
(localproxies_cases.OFF_PIN) the host build equal to the restatement in every cell and quantity, the sanitizer program on the same inputs,
and what the table is there for asserted on the references: every number of significant other proxies from 0 to 7 on lists above a wave,
gaps in the significant set, cells of one raster that differ in it, a list above 64 whose interpolated list is not."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, localdetrend as ld, localproxies as lp, meteo
from tests import localdetrend_cases as lc
from tests import localproxies_cases as pc
from tests.raster_helpers import build_host_program, declared_entry_points, exported_names, header_text, same

ROOT = Path(__file__).resolve().parent.parent
MUST = ("0 other proxies active", "1 other proxies active", "2 other proxies active", "4 other proxies active", "7 other proxies active", "the height not active",
        "the height not significant with others significant", "a proxy fails the first pass for count", "a proxy fails the first pass for deviation",
        "every proxy fails the first pass: the list untouched", "a station pruned for NODATA", "a station pruned from interpolation only: all significant values 0",
        "interpolated count < selected count", "a proxy fails only the second pass", "a proxy passes only the second pass",
        "a station erased by detrendingOtherProxies: NODATA entered the fit as a predictor", "too few fit points", "a proxy parameter clamped at its minimum",
        "a proxy parameter clamped at its maximum", "the proxies' fit ends on the iteration cap", "the proxies' fit ends on |diffSSE| <= epsilon",
        "the cell's proxy NODATA for a significant proxy: retrend 0", "the cell's proxy NODATA for a proxy that is not significant", "method idw", "method shepard",
        "method shepard_modified", "variable airT", "variable dewT")


@pytest.fixture(scope="module")
def pin():
    return pc.load_pin()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_program("localproxies", tmp_path_factory.mktemp("localproxies_host"))


@pytest.fixture(scope="module")
def host(pin, exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("localproxies_run")
    return {name: pc.run_host(exe, pin[name], d) for name in pc.RASTERS}


@pytest.fixture(scope="module")
def off_pin(exe, tmp_path_factory):
    """label -> (raster, case, the host build's outcome) of every case of pc.OFF_PIN"""
    d = tmp_path_factory.mktemp("localproxies_off_pin")
    out = {}
    for label, _ in pc.OFF_PIN:
        r, c = pc.off_pin(label)
        out[label] = (r, c, pc.run_host(exe, r, d, [c])[0])
    return out


@pytest.fixture(scope="module")
def off_pin_restated(off_pin):
    """label -> (the restatement's outcome, its arms) of the cases that are not in pc.HOST_ONLY, computed once"""
    out = {}
    for label, (r, c, _) in off_pin.items():
        if label not in pc.HOST_ONLY:
            arms = {}
            out[label] = (pc.restated(r, c, arms=arms), arms)
    return out


def test_header_and_binding_table_agree():
    text, declared = header_text("sf3d_localproxies.h"), declared_entry_points("sf3d_localproxies.h", "sf3d_localproxies_")
    assert declared == sorted(lp.SIGNATURES)
    assert re.search(rf"#define SF3D_LOCALPROXIES_MAX_OTHERS {lp.MAX_OTHERS}\b", text) and lp.MAX_OTHERS == meteo.MAX_PROXIES - 1 == 7
    device = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_device.h").read_text()
    assert re.search(rf"#define LOCALPROXIES_MAX_OTHERS {lp.MAX_OTHERS}\b", device)
    assert ctypes.sizeof(lp.OtherProxy) == 40 and ctypes.sizeof(lp.Others) == 40 * meteo.MAX_PROXIES
    assert (lp.MAX_ITERATIONS, lp.FIT_EPSILON, lp.RATIO_DELTA) == (100, 0.005, 1000)


def test_product_library_exports_the_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(lp.SIGNATURES) <= names
    assert "localproxies" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("localproxies" in n.lower() for n in capi.SIGNATURES) and not any("localproxies" in n.lower() for n in capi.REFERENCE_API)
    assert not any("localproxies" in n.lower() for n in exported_names(build.build_shim()))


def _fit(**change) -> dict:
    fit = ld.make_fit(ld.PIECEWISE_TWO, [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1], (3.0, 21.0), 8)
    fit.update(change)
    return fit


def test_refusals_come_before_any_device_work():
    sf = lp.bind(capi.load_product())
    lib = sf.lib
    many = meteo.MAX_STATIONS + 1
    x, v = np.zeros(many, np.float64), np.zeros(many, np.float32)
    rows = np.zeros((meteo.MAX_PROXIES + 1, many), np.float32)
    px, pv = x.ctypes.data_as(meteo.pf64), v.ctypes.data_as(meteo.pf32)
    height, other, off = dict(active=1, isHeight=1), dict(active=1, isHeight=0), dict(active=0, isHeight=0)

    def call(var=meteo.AIR_TEMPERATURE, method=0, ns=12, proxies=(height, other), settings=None, fit=None, others=None, xs=px, ys=px, vs=pv, values=rows, np_=None,
             st=True, ot=True):
        s = meteo.settings_struct(lp.local_settings(list(proxies), settings))
        ft = ld.fit_struct(fit if fit else _fit())
        o = lp.others_struct(others if others is not None else pc.default_others())
        n_proxies = len(proxies) if np_ is None else np_
        block = np.ascontiguousarray(values[:max(n_proxies, 1), :ns]) if values is not None else None
        return lib.sf3d_localproxies_interpolate(var, method, ns, xs, ys, vs, n_proxies, block.ctypes.data_as(meteo.pf32) if block is not None else None, 100.0,
                                                 ctypes.byref(s) if st else None, ctypes.byref(ft) if fit is not False else None, ctypes.byref(o) if ot else None, None)
    assert lib.sf3d_localproxies_bytes() == 0 and lib.sf3d_localproxies_kernel_ms() == 0.0
    # valid calls: no meteo raster
    assert call() == capi.MEMORY_ERROR and call(var=meteo.AIR_DEW_TEMPERATURE) == capi.MEMORY_ERROR
    assert call(proxies=[height]) == capi.MEMORY_ERROR                                         # no other proxy active
    assert call(proxies=[other, off, other]) == capi.MEMORY_ERROR                              # the height not in the list
    assert call(proxies=[dict(active=0, isHeight=1), other]) == capi.MEMORY_ERROR              # the height not active
    assert call(proxies=[height] + [other] * lp.MAX_OTHERS) == capi.MEMORY_ERROR               # the cap
    assert call(ns=meteo.MAX_STATIONS) == capi.MEMORY_ERROR and call(ns=0) == capi.MEMORY_ERROR
    gaps = rows.copy()
    gaps[1, 3] = ld.NODATA
    assert call(values=gaps) == capi.MEMORY_ERROR                                              # -9999 is a value
    # what sf3d_localdetrend_interpolate refuses, except its proxy rule
    for var in range(-1, len(meteo.VARIABLES) + 1):
        if var not in ld.LOCAL_VARIABLES:
            assert call(var=var) == capi.PARAMETER_ERROR, var
    assert call(method=-1) == capi.PARAMETER_ERROR and call(method=3) == capi.PARAMETER_ERROR
    for option in ld.REQUIRED:
        assert call(settings={option: 0}) == capi.PARAMETER_ERROR, option
    for option in ld.UNSUPPORTED:
        assert call(settings={option: 1}) == capi.PARAMETER_ERROR, option
    assert call(fit=_fit(function=3)) == capi.PARAMETER_ERROR and call(fit=_fit(nParameters=5)) == capi.PARAMETER_ERROR
    assert call(fit=_fit(first_guess=[])) == capi.PARAMETER_ERROR and call(fit=_fit(minPointsLocalDetrending=0)) == capi.PARAMETER_ERROR
    assert call(fit=_fit(max=[2500.0, np.nan, 0.007, -0.0015])) == capi.PARAMETER_ERROR
    assert call(fit=False) == capi.PARAMETER_ERROR and call(st=False) == capi.PARAMETER_ERROR and call(ot=False) == capi.PARAMETER_ERROR
    assert call(ns=many) == capi.PARAMETER_ERROR
    assert call(xs=None) == capi.PARAMETER_ERROR and call(ys=None) == capi.PARAMETER_ERROR and call(vs=None) == capi.PARAMETER_ERROR and call(values=None) == capi.PARAMETER_ERROR
    # the proxies: more others than the cap, two heights, a count that is not the settings'
    assert call(proxies=[other] * (lp.MAX_OTHERS + 1)) == capi.PARAMETER_ERROR
    assert call(proxies=[height, height]) == capi.PARAMETER_ERROR and call(proxies=[height, other, dict(active=0, isHeight=1)]) == capi.PARAMETER_ERROR
    assert call(proxies=[height] * (meteo.MAX_PROXIES + 1)) == capi.PARAMETER_ERROR
    assert call(np_=1) == capi.PARAMETER_ERROR and call(np_=3) == capi.PARAMETER_ERROR
    # the ranges: min > max, a non-finite value, a NaN threshold - of an active proxy only
    for bad in (dict(min=[1.0, -40.0], max=[0.5, 50.0]), dict(min=[-1.0, 60.0], max=[1.0, 50.0]), dict(min=[-1.0, -40.0], max=[np.inf, 50.0]),
                dict(min=[np.nan, -40.0], max=[1.0, 50.0]), dict(min=[-1.0, -40.0], max=[1.0, 50.0], stdDevThreshold=np.nan)):
        others = pc.default_others()
        others[1] = dict(dict(stdDevThreshold=ld.NODATA), **bad)
        assert call(others=others) == capi.PARAMETER_ERROR, bad
        others[1], others[2] = pc.default_others()[1], dict(dict(stdDevThreshold=ld.NODATA), **bad)
        assert call(others=others) == capi.MEMORY_ERROR, bad                                  # slot 2 is not in the call
    # the proxy values: non-finite other than -9999, of an active proxy only
    for value in (np.nan, np.inf, -np.inf):
        for slot in (0, 1):
            bad = rows.copy()
            bad[slot, 5] = value
            assert call(values=bad) == capi.PARAMETER_ERROR, (value, slot)
        bad = rows.copy()
        bad[1, 5] = value
        assert call(proxies=[height, off], values=bad) == capi.MEMORY_ERROR
        badx = np.zeros(12, np.float64)
        badx[5] = value
        assert call(xs=badx.ctypes.data_as(meteo.pf64)) == capi.PARAMETER_ERROR
    # the getters
    assert lib.sf3d_localproxies_get_interpolated(16, None) == capi.MEMORY_ERROR and lib.sf3d_localproxies_get_proxy_fit(16, None, None, None) == capi.MEMORY_ERROR
    # sf3d_localdetrend_interpolate still refuses a second active proxy
    st = meteo.settings_struct(ld.local_settings(dict(proxies=[height, other])))
    ft = ld.fit_struct(_fit())
    assert lib.sf3d_localdetrend_interpolate(0, 0, 12, px, px, pv, pv, 100.0, ctypes.byref(st), ctypes.byref(ft), None) == capi.PARAMETER_ERROR
    assert lib.sf3d_localproxies_clean() == capi.OK and lib.sf3d_meteo_clean() == capi.OK


def test_the_pin_holds_the_arms_the_issue_lists(pin):
    assert pc.PIN.stat().st_size < (1 << 18)
    for must in MUST:
        assert pin["arms"].get(must, 0) > 0, must
    assert any("undefined" in n for n in pin["notes"])
    relief, tiny = pin["relief"], pin["tiny"]
    assert relief["dem"].shape == (7, 37) and tiny["dem"].shape == (5, 9) and relief["maps"].shape == (pc.SLOTS, 7, 37)
    assert all(12 <= len(c["x"]) <= 16 for c in tiny["cases"]) and all(len(c["x"]) == 38 for c in relief["cases"])
    cases = relief["cases"] + tiny["cases"]
    assert {sum(c["active"][1:]) for c in cases} >= {0, 1, 2, 4, lp.MAX_OTHERS} and any(not c["active"][0] for c in cases)
    assert {c["method"] for c in cases} == {0, 1, 2} and {c["var"] for c in cases} == set(ld.LOCAL_VARIABLES)
    for r in (relief, tiny):
        assert (r["maps"][2] == pin["flag"]).any() and ((r["maps"][2] == 0) | (r["maps"][2] == pin["flag"]) | (r["maps"][2] > 0)).all()
        out = r["dem"] == pin["flag"]
        for c in r["cases"]:
            w = c["want"]
            assert (w["value"][out] == pin["flag"]).all() and (w["count"][out] == 0).all() and (w["count"][~out] > 0).all()
            assert (w["interpolated"] <= w["count"]).all() and not w["proxy_significant"][..., 0].any()
            assert not w["proxy_significant"][..., [k for k in range(pc.SLOTS) if not c["active"][k]]].any()
            assert ((w["slope"] == ld.NODATA) == ~w["proxy_significant"]).all()
    # std::sort inside shepardSearchNeighbour leaves equal keys open: no shepardIdw case sees two listed stations at one float distance
    for r in (relief, tiny):
        cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
        for c in r["cases"]:
            if c["method"] != meteo.SHEPARD:
                continue
            for row, col in np.argwhere(r["dem"] != pin["flag"]):
                sel, d, _, _ = ld.local_selection(cx[row, col], cy[row, col], c["x"], c["y"], c["fit"]["minPointsLocalDetrending"], c["area"])
                if d is None:
                    dx, dy = c["x"].astype(np.float32) - np.float32(cx[row, col]), c["y"].astype(np.float32) - np.float32(cy[row, col])
                    d = np.sqrt(dx * dx + dy * dy)
                assert len(set(np.asarray(d).tolist())) == len(d), (pc.case_name(c), row, col)


@pytest.mark.parametrize("name", pc.RASTERS)
def test_host_build_of_the_kernels_text_equals_the_pin_in_every_quantity(pin, host, name):
    r = pin[name]
    for k, (c, got) in enumerate(zip(r["cases"], host[name])):
        same(got, c["want"], f"{name} {k} {pc.case_name(c)}", pc.QUANTITIES)
    assert sum(int(c["want"]["proxy_significant"].sum()) for c in r["cases"]) > 100                 # not vacuous


def test_host_build_under_the_sanitizers_reports_nothing(pin, host, off_pin, tmp_path):
    """a stand-alone program with its own main: nothing is loaded into Python.  The pin, then the inputs of pc.OFF_PIN"""
    san = build_host_program("localproxies", tmp_path, sanitize=True)
    for name in pc.RASTERS:
        got = pc.run_host(san, pin[name], tmp_path)                     # asserts exit status 0 and an empty stderr
        for k, (a, b) in enumerate(zip(got, host[name])):
            same(a, b, f"{name} {k} under the sanitizers", pc.QUANTITIES)
    for label, (r, c, want) in off_pin.items():
        same(pc.run_host(san, r, tmp_path, [c])[0], want, f"{label} under the sanitizers", pc.QUANTITIES)


@pytest.mark.parametrize("name", lc.RASTERS)
def test_host_text_with_no_other_proxy_equals_the_pin_of_the_height_alone(exe, tmp_path, name):
    """the cases of tests/golden/localdetrend.npz through the new per-cell text: the two kernels are one text where they overlap"""
    r = dict(lc.load_pin()[name])
    r["maps"] = np.zeros((pc.SLOTS,) + r["dem"].shape, np.float32)
    cases = []
    for c in r["cases"]:
        pv = np.zeros((pc.SLOTS, len(c["x"])), np.float32)
        pv[0] = c["height"]
        cases.append(dict(c, proxy_values=pv, active=[1] + [0] * (pc.SLOTS - 1), others=pc.default_others()))
    for k, (c, got) in enumerate(zip(cases, pc.run_host(exe, r, tmp_path, cases))):
        same(got, c["want"], f"{name} {k} {lc.case_name(c)}", lc.QUANTITIES)
        assert (got["interpolated"] == got["count"]).all() and not got["proxy_significant"].any()


def test_restatement_equals_the_pin_on_every_cell_of_tiny(pin):
    r = pin["tiny"]
    arms = {}
    for k, c in enumerate(r["cases"]):
        same(pc.restated(r, c, arms=arms), c["want"], f"tiny {k} {pc.case_name(c)}", pc.QUANTITIES)
    for must in MUST:
        if must.startswith(("method", "variable", "interpolated count")):
            continue
        assert arms.get(must, 0) > 0, must


@pytest.mark.parametrize("label", [label for label, _ in pc.OFF_PIN if label not in pc.HOST_ONLY])
def test_host_build_equals_the_restatement_off_the_pin(off_pin, off_pin_restated, label):
    """every cell and every quantity of pc.QUANTITIES, bit for bit.  The two cases of pc.HOST_ONLY (a three-piece function under five other
    proxies: more than 5 s in the restatement) are held host build against device only (tests/test_gpu_localproxies.py)"""
    r, c, got = off_pin[label]
    same(got, off_pin_restated[label][0], label, pc.QUANTITIES)
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got["value"][out] == r["flag"]).all() and (got["count"][out] == 0).all() and (got["count"][~out] > 0).all()


def test_the_off_pin_table_reaches_what_it_claims(off_pin, off_pin_restated):
    """asserted on the two references, so that an edit of the table cannot hollow it out"""
    assert len(pc.OFF_PIN) == len(dict(pc.OFF_PIN)) == len(off_pin) and set(pc.HOST_ONLY) < set(off_pin)
    k_any, k_long, functions_long, gaps, across, differ = set(), set(), set(), 0, 0, 0
    for label, (r, c, got) in off_pin.items():
        inside = r["dem"] != r["flag"]
        k = got["proxy_significant"][inside].sum(axis=1)
        count, interpolated = got["count"][inside], got["interpolated"][inside]
        k_any |= set(k.tolist())
        k_long |= set(k[count > 64].tolist())
        if count.min() > 64 and k.min() >= 5:
            functions_long.add(c["fit"]["function"])
        across += int(((count > 64) & (interpolated <= 64)).sum())
        differ += len(set(k.tolist())) > 1 and count.min() > 64
        active = [p for p in range(1, pc.SLOTS) if c["active"][p]]
        for row in got["proxy_significant"][inside]:
            significant = [p for p in active if row[p]]
            gaps += significant != active[:len(significant)]
        assert c["method"] != meteo.SHEPARD, label                          # no shepardIdw case, so no order left open by std::sort
        assert not got["proxy_significant"][..., [p for p in range(pc.SLOTS) if p == 0 or not c["active"][p]]].any(), label
    assert k_any == set(range(lp.MAX_OTHERS + 1)) and k_long == set(range(lp.MAX_OTHERS + 1))         # 3, 5 and 6 (65 entries at 5) on lists above a wave
    assert functions_long == {0, 1, 2} and gaps > 0 and across > 0 and differ >= 1
    assert {len(c["fit"]["first_guess"]) for _, c, _ in off_pin.values()} >= {2, 3, 4}
    r, c, got = off_pin["noheight70-k3"]
    assert not c["active"][0] and not got["significant"].any() and (got["proxy_significant"][r["dem"] != r["flag"]].sum(axis=1) == 3).all()
    arms = {}
    for _, a in off_pin_restated.values():
        for name, n in a.items():
            arms[name] = arms.get(name, 0) + n
    for must in ("a proxy fails the first pass for count", "a proxy fails the first pass for deviation", "a proxy fails only the second pass",
                 "a proxy passes only the second pass", "every proxy fails the first pass: the list untouched", "the height not active", "a station pruned for NODATA"):
        assert arms.get(must, 0) > 0, must


def test_make_others_lays_the_configured_range_out_per_slot():
    others = lp.make_others([None, dict(range=[-1.0, -40.0, 1.0, 50.0]), dict(range=[0.0, 1.0, 2.0, 3.0], stdDevThreshold=0.25)])
    assert others[1] == dict(min=[-1.0, -40.0], max=[1.0, 50.0], stdDevThreshold=ld.NODATA) and others[2]["min"] == [0.0, 1.0] and others[2]["max"] == [2.0, 3.0]
    s = lp.others_struct(others)
    assert s.proxy[2].stdDevThreshold == 0.25 and list(s.proxy[2].max) == [2.0, 3.0] and s.proxy[0].stdDevThreshold == np.float32(ld.NODATA)
    with pytest.raises(ValueError):
        lp.make_others([dict(range=[0.0, 1.0])])
