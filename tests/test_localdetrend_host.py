"""Local detrending, the parts that need no GPU: the ABI of include/sf3d_localdetrend.h against the binding; the entry points exported by
the product library and absent from sf3d.h and the shim; the refusals that come before any device work (and sf3d_meteo_interpolate's
own, which stay); the pin's arm list and size; the per-cell text of k_localdetrend compiled for the host (tests/localdetrend_host.cpp)
equal to the compiled-reference pin tests/golden/localdetrend.npz in every recorded quantity, and once more as a stand-alone program under
the address and undefined-behaviour sanitizers; the Python restatement equal to the pin on every cell of `tiny`; the restated range
and first-guess list equal to what the pin recorded from the reference; and off the pin (localdetrend_cases.OFF_PIN) the host build equal to
the restatement in every cell and quantity, the sanitizer program on the same inputs, and the list lengths, functions, methods, guess
counts and arms that the table is there for, asserted on the two references."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, localdetrend as ld, meteo
from tests import localdetrend_cases as lc
from tests.raster_helpers import build_host_program, declared_entry_points, exported_names, header_text, same

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return lc.load_pin()


@pytest.fixture(scope="module")
def host(pin, tmp_path_factory):
    d = tmp_path_factory.mktemp("localdetrend_host")
    exe = build_host_program("localdetrend", d)
    return {name: lc.run_host(exe, pin[name], d) for name in lc.RASTERS}


@pytest.fixture(scope="module")
def off_pin(tmp_path_factory):
    """label -> (raster, case, the host build's outcome) of every case of lc.OFF_PIN"""
    d = tmp_path_factory.mktemp("localdetrend_off_pin")
    exe = build_host_program("localdetrend", d)
    out = {}
    for label, _ in lc.OFF_PIN:
        r, c = lc.off_pin(label)
        out[label] = (r, c, lc.run_host(exe, r, d, [c])[0])
    return out


@pytest.fixture(scope="module")
def off_pin_restated(off_pin):
    """label -> (the restatement's outcome, its arms) of the cases that are not in lc.HOST_ONLY, computed once"""
    out = {}
    for label, (r, c, _) in off_pin.items():
        if label not in lc.HOST_ONLY:
            arms = {}
            out[label] = (lc.restated(r, c, arms=arms), arms)
    return out


def test_header_and_binding_table_agree():
    text, declared = header_text("sf3d_localdetrend.h"), declared_entry_points("sf3d_localdetrend.h", "sf3d_localdetrend_")
    assert declared == sorted(ld.SIGNATURES)
    assert re.search(rf"#define SF3D_LOCALDETREND_MAX_PARAMETERS {ld.MAX_PARAMETERS}\b", text) and ld.MAX_PARAMETERS == 6
    assert re.search(rf"#define SF3D_LOCALDETREND_MAX_FIRST_GUESS {ld.MAX_FIRST_GUESS}\b", text) and ld.MAX_FIRST_GUESS == 31
    device = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_device.h").read_text()
    assert re.search(rf"#define LOCALDETREND_MAX_PARAMETERS {ld.MAX_PARAMETERS}\b", device) and re.search(rf"#define LOCALDETREND_MAX_FIRST_GUESS {ld.MAX_FIRST_GUESS}\b", device)
    for k, name in enumerate(("PIECEWISE_TWO", "PIECEWISE_THREE_FREE", "PIECEWISE_THREE")):
        assert re.search(rf"SF3D_LOCALDETREND_{name} = {k}\b", text) and getattr(ld, name) == k
    assert ld.PARAMETERS == (4, 6, 5) and ld.MAX_STATIONS == meteo.MAX_STATIONS == 1024
    assert ctypes.sizeof(ld.Fit) == 24 + (3 + ld.MAX_FIRST_GUESS) * ld.MAX_PARAMETERS * 8
    assert [meteo.VARIABLES[v] for v in ld.LOCAL_VARIABLES] == ["airT", "dewT"]
    assert set(ld.UNSUPPORTED) == set(meteo.UNSUPPORTED) - set(ld.REQUIRED) and len(ld.UNSUPPORTED) == 5


def test_product_library_exports_the_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(ld.SIGNATURES) <= names
    assert "localdetrend" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("localdetrend" in n.lower() for n in capi.SIGNATURES) and not any("localdetrend" in n.lower() for n in capi.REFERENCE_API)
    assert not any("localdetrend" in n.lower() for n in exported_names(build.build_shim()))


def _fit(**change) -> dict:
    fit = ld.make_fit(ld.PIECEWISE_TWO, [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1], (3.0, 21.0), 8)
    fit.update(change)
    return fit


def test_refusals_come_before_any_device_work():
    sf = ld.bind(capi.load_product())
    lib = sf.lib
    many = meteo.MAX_STATIONS + 1
    x, v = np.zeros(many, np.float64), np.zeros(many, np.float32)
    px, pv = x.ctypes.data_as(meteo.pf64), v.ctypes.data_as(meteo.pf32)
    ok = meteo.settings_struct(ld.local_settings())

    def call(var=meteo.AIR_TEMPERATURE, method=0, ns=12, st=ok, fit=None, xs=px, ys=px, hs=pv, vs=pv):
        ft = ld.fit_struct(fit if fit else _fit())
        return lib.sf3d_localdetrend_interpolate(var, method, ns, xs, ys, hs, vs, 100.0, ctypes.byref(st) if st is not None else None,
                                                 ctypes.byref(ft) if fit is not False else None, None)
    assert lib.sf3d_localdetrend_bytes() == 0 and lib.sf3d_localdetrend_kernel_ms() == 0.0
    # valid calls: no meteo raster
    assert call() == capi.MEMORY_ERROR and call(var=meteo.AIR_DEW_TEMPERATURE) == capi.MEMORY_ERROR
    assert call(ns=meteo.MAX_STATIONS) == capi.MEMORY_ERROR and call(ns=0) == capi.MEMORY_ERROR
    for function, n in zip(range(3), ld.PARAMETERS):
        rng = [0.0] * n + [1.0] * n
        assert call(fit=_fit(function=function, min=rng[:n], max=rng[n:], delta=ld.parameters_delta(rng), first_guess=[[0.5] * n] * ld.MAX_FIRST_GUESS)) == capi.MEMORY_ERROR
    # the variables: the two temperatures only
    for var in range(-1, len(meteo.VARIABLES) + 1):
        if var not in ld.LOCAL_VARIABLES:
            assert call(var=var) == capi.PARAMETER_ERROR, var
    assert call(method=-1) == capi.PARAMETER_ERROR and call(method=3) == capi.PARAMETER_ERROR
    # the block is for the pair of options only; the five others stay with the caller
    for off in ld.REQUIRED:
        assert call(st=meteo.settings_struct(ld.local_settings({off: 0}))) == capi.PARAMETER_ERROR, off
    for option in ld.UNSUPPORTED:
        assert call(st=meteo.settings_struct(ld.local_settings({option: 1}))) == capi.PARAMETER_ERROR, option
    # the proxies: exactly one active, and that one the height
    height, other = dict(active=1, isHeight=1), dict(active=1, isHeight=0)
    for proxies in ([], [dict(active=0, isHeight=1)], [other], [height, other], [height, height], [height] * (meteo.MAX_PROXIES + 1)):
        assert call(st=meteo.settings_struct(ld.local_settings(dict(proxies=proxies)))) == capi.PARAMETER_ERROR, proxies
    assert call(st=meteo.settings_struct(ld.local_settings(dict(proxies=[dict(active=0, isHeight=0), height])))) == capi.MEMORY_ERROR
    # the fit
    assert call(fit=_fit(function=3)) == capi.PARAMETER_ERROR and call(fit=_fit(function=-1)) == capi.PARAMETER_ERROR
    for n in (3, 5, 6):
        assert call(fit=_fit(nParameters=n)) == capi.PARAMETER_ERROR, n
    assert call(fit=_fit(function=ld.PIECEWISE_THREE)) == capi.PARAMETER_ERROR              # four parameters, the function takes five
    assert call(fit=_fit(first_guess=[[0.0] * 4] * (ld.MAX_FIRST_GUESS + 1))) == capi.PARAMETER_ERROR
    assert call(fit=_fit(first_guess=[])) == capi.PARAMETER_ERROR
    assert call(fit=_fit(minPointsLocalDetrending=0)) == capi.PARAMETER_ERROR and call(fit=_fit(minPointsLocalDetrending=-3)) == capi.PARAMETER_ERROR
    assert call(fit=_fit(max=[2500.0, np.nan, 0.007, -0.0015])) == capi.PARAMETER_ERROR
    assert call(fit=False) == capi.PARAMETER_ERROR and call(st=None) == capi.PARAMETER_ERROR
    # the stations
    assert call(ns=many) == capi.PARAMETER_ERROR
    assert call(xs=None) == capi.PARAMETER_ERROR and call(ys=None) == capi.PARAMETER_ERROR and call(hs=None) == capi.PARAMETER_ERROR and call(vs=None) == capi.PARAMETER_ERROR
    for value in (np.nan, np.inf, -np.inf):
        bad, badf = np.zeros(12, np.float64), np.zeros(12, np.float32)
        bad[5] = badf[5] = value
        assert call(xs=bad.ctypes.data_as(meteo.pf64)) == capi.PARAMETER_ERROR and call(ys=bad.ctypes.data_as(meteo.pf64)) == capi.PARAMETER_ERROR
        assert call(hs=badf.ctypes.data_as(meteo.pf32)) == capi.PARAMETER_ERROR
    # the getters
    assert lib.sf3d_localdetrend_get_fit(16, None, pv, None) == capi.MEMORY_ERROR and lib.sf3d_localdetrend_get_selection(16, None, pv) == capi.MEMORY_ERROR
    # sf3d_meteo_interpolate still refuses both options
    for option in ld.REQUIRED:
        st = meteo.settings_struct({option: 1})
        assert lib.sf3d_meteo_interpolate(0, 0, 12, px, px, pv, 100.0, ctypes.byref(st), None) == capi.PARAMETER_ERROR, option
    assert set(ld.REQUIRED) <= set(meteo.UNSUPPORTED)
    assert lib.sf3d_localdetrend_clean() == capi.OK and lib.sf3d_meteo_clean() == capi.OK


def test_the_pin_holds_what_the_issue_lists(pin):
    assert lc.PIN.stat().st_size < (1 << 18)
    relief, tiny = pin["relief"], pin["tiny"]
    assert relief["dem"].shape == (7, 37) and relief["cell_size"] == 500.0 and tiny["dem"].shape == (5, 9)
    assert (relief["dem"] == pin["flag"]).sum() >= 6 and relief["xll"] > 1e5 and relief["yll"] > 1e6
    valid = relief["dem"][relief["dem"] != pin["flag"]]
    assert valid.max() - valid.min() > 1000.0
    for must in ("all stations selected", "one ring suffices", "several 7 500 m rings", "the step drops to 1 000 m", "beyondLastPoint ends the loop short of minPoints",
                 "a station on the cell centre", "height not significant: standard deviation below the threshold",
                 "height not significant: fewer elevation points than minPointsLocalDetrending", "the fit ends on |diffSSE| <= epsilon", "the fit ends on the iteration cap",
                 "a parameter clamped to its range", "a later first guess replaces the best fit", "bestR2 < 0: the fit is repeated from the RMSE index",
                 "all station values equal: R2 is x / 0", "piecewiseThreeFree: par[2] raised to 10", "piecewiseThree: par[2] raised to 10"):
        assert pin["arms"][must] > 0, must
    cases = relief["cases"] + tiny["cases"]
    assert {c["fit"]["function"] for c in cases} == {0, 1, 2} and {c["method"] for c in cases} == {0, 1, 2}
    assert {c["var"] for c in cases} == set(ld.LOCAL_VARIABLES) and {c["fit"]["minPointsLocalDetrending"] for c in relief["cases"]} >= {5, 8, 20}
    assert all(np.isfinite(c["want"]["value"]).all() for c in cases)
    # equal station values: the map is finite although R2 is not
    equal = next(c for c in relief["cases"] if c["label"] == "equal")
    assert not np.isfinite(equal["want"]["r2"][relief["dem"] != pin["flag"]]).any()
    # every cell outside the DEM holds the flag, and no selection
    for r in (relief, tiny):
        for c in r["cases"]:
            out = r["dem"] == pin["flag"]
            assert (c["want"]["value"][out] == pin["flag"]).all() and (c["want"]["count"][out] == 0).all() and (c["want"]["count"][~out] > 0).all()
    # std::sort inside shepardSearchNeighbour leaves equal keys open: no shepardIdw case sees two selected stations at one float distance
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
                assert len(set(np.asarray(d).tolist())) == len(d), (lc.case_name(c), row, col)
    assert all(e["seconds"] >= 0 and e["cells"] > 0 for e in pin["cpu"])


@pytest.mark.parametrize("name", lc.RASTERS)
def test_host_build_of_the_kernels_text_equals_the_pin_in_every_quantity(pin, host, name):
    r = pin[name]
    for k, (c, got) in enumerate(zip(r["cases"], host[name])):
        same(got, c["want"], f"{name} {k} {lc.case_name(c)}", lc.QUANTITIES)
    assert sum(int(c["want"]["significant"].sum()) for c in r["cases"]) > 100                 # not vacuous


def test_host_build_under_the_sanitizers_reports_nothing(pin, host, off_pin, tmp_path):
    """a stand-alone program with its own main: nothing is loaded into Python.  The pin, then the inputs of lc.OFF_PIN"""
    exe = build_host_program("localdetrend", tmp_path, sanitize=True)
    for name in lc.RASTERS:
        got = lc.run_host(exe, pin[name], tmp_path)                    # asserts exit status 0 and an empty stderr
        for k, (a, b) in enumerate(zip(got, host[name])):
            same(a, b, f"{name} {k} under the sanitizers", lc.QUANTITIES)
    for label, (r, c, want) in off_pin.items():
        same(lc.run_host(exe, r, tmp_path, [c])[0], want, f"{label} under the sanitizers", lc.QUANTITIES)


def test_restatement_equals_the_pin_on_every_cell_of_tiny(pin):
    r = pin["tiny"]
    arms = {}
    for k, c in enumerate(r["cases"]):
        same(lc.restated(r, c, arms=arms), c["want"], f"tiny {k} {lc.case_name(c)}", lc.QUANTITIES)
    assert arms["the fit ends on the iteration cap"] > 0 and arms["max iterations"] == ld.MAX_ITERATIONS + 1


def test_restated_range_and_first_guesses_equal_the_reference(pin):
    assert len(pin["ranges"]) >= 6 and {c["function"] for c in pin["ranges"]} == {0, 1, 2}
    for c in pin["ranges"]:
        rng = ld.height_temperature_range(c["function"], c["configured"], c["points_range"])
        assert np.array_equal(np.array(rng).view(np.uint64), np.array(c["want_range"]).view(np.uint64)), c
        got = ld.first_guess_combinations(c["function"], rng, c["position"])
        assert np.array_equal(np.array(got).view(np.uint64), np.array(c["want_combinations"]).view(np.uint64)), c
        n = ld.PARAMETERS[c["function"]]
        assert ld.parameters_delta(rng) == [(rng[n + j] - rng[j]) / 800 for j in range(n)]
    assert max(len(c["want_combinations"]) for c in pin["ranges"]) == ld.MAX_FIRST_GUESS
    fit = ld.make_fit("piecewiseThree", pin["ranges"][0]["configured"] if pin["ranges"][0]["function"] == 2 else
                      [-350.0, 0.0, 300.0, 0.002, -0.01, 2500.0, 0.0, 1000.0, 0.007, -0.0015], [0, 1, 1, 1, 1], (3.0, 21.0), 8, 5.0)
    assert fit["function"] == ld.PIECEWISE_THREE and len(fit["min"]) == 5 and fit["min"][1] == 1.0 and fit["max"][1] == 27.0 and len(fit["first_guess"]) == 30


@pytest.mark.parametrize("label", [label for label, _ in lc.OFF_PIN if label not in lc.HOST_ONLY])
def test_host_build_equals_the_restatement_off_the_pin(off_pin, off_pin_restated, label):
    """every cell and every quantity of lc.QUANTITIES, bit for bit.  The cases of lc.HOST_ONLY - the full first-guess lists of the
    three-piece functions, 10 to 30 s a case in the restatement - are held host build against device only (tests/test_gpu_localdetrend.py);
    the long-ring case here is rings150-two-16"""
    r, c, got = off_pin[label]
    want = off_pin_restated[label][0]
    same(got, want, label, lc.QUANTITIES)
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got["value"][out] == r["flag"]).all() and (got["count"][out] == 0).all() and (got["count"][~out] > 0).all()


def test_the_off_pin_table_reaches_what_it_claims(pin, off_pin, off_pin_restated):
    """asserted on the two references, so that an edit of the table cannot hollow it out.  All four arms occur above 64 stations: the cap
    and the later guess through cap70 (a first guess below its range, as the pin's `cap`), bestR2 < 0 through equal70"""
    assert len(lc.OFF_PIN) == len(dict(lc.OFF_PIN)) == len(off_pin) and set(lc.HOST_ONLY) < set(off_pin) and "rings150-two-16" in off_pin_restated
    lengths, functions, methods, guesses, shapes = set(), set(), set(), set(), set()
    for label, (r, c, got) in off_pin.items():
        inside = r["dem"] != r["flag"]
        counts = set(got["count"][inside].tolist())
        lengths |= counts
        guesses.add(len(c["fit"]["first_guess"]))
        shapes.add((r["dem"].shape, bool(r["dem"][0, 0] == r["flag"])))
        if min(counts) > 64:
            functions.add(c["fit"]["function"])
            methods.add(c["method"])
        if c["method"] == meteo.SHEPARD:
            assert not lc.ties(r, c), label
            if label in off_pin_restated:
                assert not off_pin_restated[label][0]["ties"].any(), label
    assert {63, 64, 65, 128, 129} <= lengths and {1, 4, 5} <= lengths
    rings = off_pin["rings150-free-31"]
    assert len(rings[1]["x"]) == 150 > rings[2]["count"].max() > 128                         # a ring-selected list above 128
    assert functions == {0, 1, 2} and methods == {0, 1, 2} and ld.MAX_FIRST_GUESS in guesses and {16, 30} <= guesses
    assert shapes >= {((3, 11), False), ((1, 4), False), ((1, 5), True), ((2, 4), False)}
    # the positions of the 31-guess list are a configuration the pin recorded from the reference, with the synthetic range's configured values
    for function, position in lc.POSITION_31.items():
        assert any(e["function"] == function and e["position"] == position and len(e["want_combinations"]) == ld.MAX_FIRST_GUESS for e in pin["ranges"])
    for arm in ("the fit ends on the iteration cap", "a later first guess replaces the best fit", "bestR2 < 0: the fit is repeated from the RMSE index",
                "a parameter clamped to its range"):
        assert any(arms.get(arm, 0) > 0 and off_pin[label][2]["count"][off_pin[label][0]["dem"] != off_pin[label][0]["flag"]].min() > 64
                   for label, (_, arms) in off_pin_restated.items()), arm
    # the arms at more than 64 stations that the pin has below a wave only
    r, c, got = off_pin["dew70-undetrended"]
    assert c["var"] == meteo.AIR_DEW_TEMPERATURE and c["useDetrending"] == 0 and got["significant"][r["dem"] != r["flag"]].all()
    r, c, got = off_pin["equal70"]
    assert not np.isfinite(got["r2"][r["dem"] != r["flag"]]).any() and np.isfinite(got["value"]).all()
    r, c, got = off_pin["flat70"]
    assert not got["significant"].any() and (got["count"][r["dem"] != r["flag"]] == 70).all()
    assert off_pin_restated["flat70"][1]["height not significant: standard deviation below the threshold"] == 32
