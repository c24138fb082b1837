"""Multiple detrending without areas, the parts that need no GPU: the ABI of include/sf3d_multidetrend.h against the binding; the entry
points exported by the product library and absent from sf3d.h and the shim; the pin's arm list; the text of k_multidetrend_fit,
k_multidetrend_cells and k_multidetrend_points compiled for the host (tests/multidetrend_host.cpp) equal to the compiled-reference pin
tests/golden/multidetrend.npz in every map cell, every fit quantity and every point on both rasters, and once more as a stand-alone
program under the address and undefined-behaviour sanitizers; the Python restatement equal to the pin on `tiny` with no empty arm;
`proxy_values_xy` and `residuals`' arithmetic on hand-made input; every refusal of the three entry points through the HIP-free check
functions they share with the host program; and off the pin (multidetrend_cases.OFF_PIN, each row with its property) the host build
equal to the restatement, with two hours on one block.

The mutation these cases catch and the earlier tests do not: in md_fit (sf3d_multidetrend.inc) writing the kept stations' coordinates
as `v.keptX[i] = v.sx[i]` in the place of `v.sx[at]` - the list's position for the station's index.  Every test of the other blocks
passes (none reads keptX); here every case in which a station is erased before a kept one fails in the map and at the points
("urban", "gaps", "noheight" and "secondpass" of the pin, "erased-chunk" off it), and the cases without an erased station ("height") still pass."""
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, localdetrend as ld, meteo, multidetrend as md
from tests import multidetrend_cases as mc
from tests.raster_helpers import build_host_program, declared_entry_points, exported_names, header_text, same

ROOT = Path(__file__).resolve().parent.parent
MUST = ("the height not active", "the height not significant: fewer than five heights", "the height not significant: the standard deviation",
        "the height significant alone", "the height significant with 1 other proxies", "the height significant with 3 other proxies",
        "the height withdrawn by isVectorNodataOrZero", "no other proxy active", "every proxy fails the first pass: the list untouched",
        "a proxy fails only the second pass", "a proxy passes only the second pass",
        "a station erased by detrendingOtherProxies: NODATA entered the fit as a predictor", "a station pruned for NODATA",
        "a station pruned from interpolation only: all significant values 0", "an erased station absent from the map's neighbours",
        "a station with a NODATA height while the height is significant", "a place lacking a significant proxy: value kept, retrend 0",
        "a cell lacking only a non-significant active proxy", "a cell whose interpolate() gives NODATA", "useDetrending 0",
        "a point: a station at its own coordinates", "a point: an erased station still evaluated", "a point on a cell centre", "a point outside the raster",
        "a point with a NODATA value of a significant proxy", "method idw", "method shepard", "method shepard_modified", "variable airT", "variable dewT",
        "function piecewiseTwo", "function piecewiseThreeFree", "function piecewiseThree")
# the arms the restatement itself counts on `tiny` (the others are counted from the driver's outcome when the pin is made)
RESTATED = tuple(a for a in MUST if not a.startswith(("a point", "method", "variable", "function", "an erased station absent", "a cell whose interpolate")))


@pytest.fixture(scope="module")
def pin():
    return mc.load_pin()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_program("multidetrend", tmp_path_factory.mktemp("multidetrend_host"))


@pytest.fixture(scope="module")
def host(pin, exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("multidetrend_run")
    return {name: mc.run_host(exe, pin[name], d) for name in mc.RASTERS}


def test_header_and_binding_table_agree():
    assert declared_entry_points("sf3d_multidetrend.h", "sf3d_multidetrend_") == sorted(md.SIGNATURES)
    device = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_device.h").read_text()
    assert re.search(r"struct MultiDetrendRecord\b", device) and "sf3d_localproxies.h" in header_text("sf3d_multidetrend.h")
    assert f"#define SF3D_MULTIDETREND_MAX_POINTS (1u << 24)" in header_text("sf3d_multidetrend.h") and md.MAX_POINTS == 1 << 24
    text = (ROOT / "include" / "sf3d_multidetrend.h").read_text()
    for kept_out in ("lapse-rate codes", "topographic distance", "optimalDetrending", "meteo-grid variant", "station list and its quality control"):
        assert kept_out in text, kept_out


def test_product_library_exports_the_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(md.SIGNATURES) <= names
    assert "multidetrend" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("multidetrend" in n.lower() for n in capi.SIGNATURES) and not any("multidetrend" in n.lower() for n in capi.REFERENCE_API)
    assert not any("multidetrend" in n.lower() for n in exported_names(build.build_shim()))


def test_pin_reaches_every_arm_or_says_why_not(pin):
    explained = " ".join(pin["notes"])
    for arm in MUST:
        assert pin["arms"].get(arm, 0) > 0 or arm in explained, arm
    assert "isEqual(R2, NODATA)" in explained                                # why the one empty arm cannot be reached, from the reference's text
    assert mc.PIN.stat().st_size < (1 << 18)
    assert pin["tiny"]["dem"].shape == (5, 9) and pin["relief"]["dem"].shape == (7, 37)


@pytest.mark.parametrize("name", mc.RASTERS)
def test_host_build_equals_the_pin_in_every_cell_fit_quantity_and_point(pin, host, name):
    for c, g in zip(pin[name]["cases"], host[name]):
        assert g["status"] == 0 and g["points_status"] == 0, mc.case_name(c)
        same(g, c["want"], f"{name} {mc.case_name(c)}", mc.QUANTITIES)


def test_restatement_equals_the_pin_on_tiny_and_leaves_no_arm_empty(pin):
    r = pin["tiny"]
    arms = {}
    for c in r["cases"]:
        same(mc.restated(r, c, arms=arms), c["want"], f"tiny {mc.case_name(c)}", mc.QUANTITIES)
    explained = " ".join(pin["notes"])
    for arm in RESTATED:
        assert arms.get(arm, 0) > 0 or arm in explained, arm
        assert arms.get(arm, 0) == pin["arms"][arm], arm                     # the counts the pin was written with


def test_the_pin_s_cases_show_what_they_were_built_for(pin):
    """per label of `tiny`: the outcome the case is there for, read from the recorded reference"""
    want = {c["label"]: c["want"] for c in pin["tiny"]["cases"]}
    case = {c["label"]: c for c in pin["tiny"]["cases"]}
    inside = pin["tiny"]["dem"] != pin["flag"]
    assert want["height"]["significant"] and not want["height"]["proxy_significant"].any() and want["height"]["kept"] == 24
    assert want["three-others"]["significant"] and want["three-others"]["proxy_significant"].sum() == 3
    assert not want["noheight"]["significant"] and want["noheight"]["r2"] == mc.NODATA32 and want["noheight"]["proxy_significant"].any()
    for label in ("flatheight", "fewheights"):
        assert not want[label]["significant"] and (want[label]["parameters"] == ld.NODATA).all() and want[label]["r2"] == mc.NODATA32
    assert (case["fewheights"]["proxy_values"][0] != mc.NODATA32).sum() == 4
    # the stations without a height stay in the list, detrended by the function of -9999
    lost = case["noheightvalue"]["proxy_values"][0] == mc.NODATA32
    assert lost.sum() == 3 and want["noheightvalue"]["significant"] and want["noheightvalue"]["station_kept"][lost].all()
    assert want["allfail"]["kept"] == 24 and not want["allfail"]["proxy_significant"].any()
    # erased for a NODATA proxy, erased for all-zero proxies: absent from the kept list
    gaps = case["gaps"]
    assert not want["gaps"]["station_kept"][[2, 9, 15]].any()
    urban = case["urban"]["proxy_values"][2] == 0
    assert urban.any() and not want["urban"]["station_kept"][urban].any() and want["urban"]["station_kept"][~urban].all()
    # a proxy significant in the second pass only: the station whose NODATA entered the fit is erased by detrendingOtherProxies
    assert want["secondpass"]["proxy_significant"][[1, 7]].all() and not want["secondpass"]["proxy_significant"][5]
    assert not want["secondpass"]["station_kept"][[0, 1, 2, 8]].any() and want["secondpass"]["kept"] == 20
    # no station left: -9999 in every cell and at every point, and the call is no failure
    assert want["allzero"]["kept"] == 0 and (want["allzero"]["value"][inside] == mc.NODATA32).all() and (want["allzero"]["points"] == mc.NODATA32).all()
    # the erased stations are still evaluated as points
    assert (want["gaps"]["points"][:24] != mc.NODATA32).all() and len(gaps["points"]["x"]) == 27


def test_sanitized_host_program_runs_clean_on_the_pin_and_off_it(pin, host, tmp_path):
    san = build_host_program("multidetrend", tmp_path, sanitize=True)
    got = mc.run_host(san, pin["tiny"], tmp_path)                    # run_host_program asserts an empty stderr
    for c, g, h in zip(pin["tiny"]["cases"], got, host["tiny"]):
        same(g, h, mc.case_name(c), mc.QUANTITIES)
    for label in ("list4", "list65", "list1024", "no-height-third", "erased-chunk", "guesses31-free"):
        r, c = mc.off_pin(label)
        g = mc.run_host(san, r, tmp_path, [c])[0]
        assert g["status"] == 0 and g["points_status"] == 0, label
    r, hours = mc.two_hours()
    assert [g["status"] for g in mc.run_host(san, r, tmp_path, hours)] == [0, 0]


def test_proxy_values_xy_is_getproxyvaluesxy_for_points():
    dem = np.array([[10.0, 20.0, 30.0], [40.0, -9999.0, 60.0]], np.float32)
    sea = np.array([[1.0, 2.0, -9999.0], [4.0, 5.0, 6.0]], np.float32)
    proxies = [dict(active=1, isHeight=1), dict(active=1, isHeight=0), dict(active=0, isHeight=0)]
    x = np.array([105.0, 125.0, 115.0, 95.0, 129.99, 130.0], np.float32)
    y = np.array([215.0, 215.0, 205.0, 205.0, 200.0, 219.0], np.float32)
    got = md.proxy_values_xy(dem, 100.0, 200.0, 10.0, [None, sea, sea], proxies, x, y)
    n = np.float32(-9999.0)
    # the DEM's flag and the raster's are NODATA; x = 130 is outside; x = 95, half a cell west of the raster, reads column int(-0.5) = 0:
    # Crit3DRasterGrid::getValueFromXY takes int(), not floor - the reference's, kept
    assert got[0].tolist() == [10.0, 30.0, n, 40.0, 60.0, n]
    assert got[1].tolist() == [1.0, n, 5.0, 4.0, 6.0, n] and (got[2] == n).all()             # a proxy that is not active: NODATA
    assert md.cell_at(dem.shape, 100.0, 200.0, 10.0, 95.0, 205.0) == (1, 0) and md.cell_at(dem.shape, 100.0, 200.0, 10.0, 89.0, 205.0) is None


def test_cell_xy_is_the_single_precision_header_overload():
    x, y = md.cell_xy((2, 3), 100.0, 200.0, 10.0)
    assert x.dtype == np.float32 and x[0].tolist() == [100.5, 110.5, 120.5] and y[:, 0].tolist() == [219.5, 209.5]
    assert md.cell_at((2, 3), 100.0, 200.0, 10.0, x[1, 2], y[1, 2]) == (1, 2)


def test_residuals_are_computeresiduals_arithmetic():
    value = np.array([10.5, -9999.0, 3.0, 2.0], np.float32)
    got = np.array([9.25, 4.0, -9999.0, 2.0], np.float32)
    assert md.residual_of(value, got).tolist() == [1.25, -9999.0, -9999.0, 0.0] and md.residual_of(value, got).dtype == np.float32


def _valid():
    r, c = mc.synthetic(n_stations=20, method=meteo.IDW, n_others=1)
    r["name"] = "refusals"
    return r, c


def test_every_refusal_of_interpolate(exe, tmp_path):
    r, c = _valid()

    def status(**change) -> int:
        q = dict(c)
        for k, v in change.items():
            q[k] = v(c[k]) if callable(v) else v
        return mc.run_host(exe, r, tmp_path, [dict(q, points=None)])[0]["status"]

    def edited(a, at, value):
        a = np.array(a, copy=True)
        a[at] = value
        return a
    assert status() == 0
    assert status(options=dict(useLocalDetrending=1)) == 2 and status(options=dict(useMultipleDetrending=0)) == 2 and status(options=dict(nProxies=7)) == 2
    assert status(var=meteo.PRECIPITATION) == 2 and status(method=3) == 2 and status(method=-1) == 2
    assert status(x=lambda a: edited(a, 0, np.inf)) == 2 and status(y=lambda a: edited(a, 3, np.nan)) == 2
    assert status(proxy_values=lambda a: edited(a, (1, 0), np.nan)) == 2 and status(proxy_values=lambda a: edited(a, (0, 2), np.inf)) == 2
    assert status(proxy_values=lambda a: edited(a, (5, 0), np.nan)) == 0                      # a slot that is not active is not read
    assert status(fit=dict(c["fit"], first_guess=[])) == 2 and status(fit=dict(c["fit"], stdDevThreshold=float("nan"))) == 2
    assert status(fit=dict(c["fit"], min=list(c["fit"]["min"][:3]), max=list(c["fit"]["max"][:3]), delta=list(c["fit"]["delta"][:3]))) == 2
    assert status(fit=dict(c["fit"], minPointsLocalDetrending=-3)) == 0                       # not read
    others = [dict(o) for o in c["others"]]
    others[1]["min"] = [5.0, 0.0]
    assert status(others=others) == 2                                                         # min > max
    many = meteo.MAX_STATIONS + 1
    big = dict(x=np.zeros(many), y=np.zeros(many), value=np.zeros(many, np.float32), proxy_values=np.zeros((mc.SLOTS, many), np.float32))
    assert status(**big) == 2
    at_cap = mc.off_pin("list1024")
    assert mc.run_host(exe, at_cap[0], tmp_path, [at_cap[1]])[0]["status"] == 0


def test_every_refusal_of_points_and_of_the_getter(exe, tmp_path):
    r, c = _valid()
    only = lambda **o: dict(c, options=dict(pointsOnly=1, **o))

    def edited(key, at, value):
        q = {k: np.array(v, copy=True) for k, v in c["points"].items()}
        q[key][at] = value
        return q
    # before the first interpolate; after a good one; the fit stays the last accepted call's after a refused one
    first, good, after, refused, still = mc.run_host(exe, r, tmp_path, [only(), c, only(), dict(c, var=meteo.PRECIPITATION), only()])
    assert first["status"] == 3 and first["points_status"] == 2
    assert good["points_status"] == 0 and after["points_status"] == 0 and refused["status"] == 2 and still["points_status"] == 0
    assert np.array_equal(after["points"].view(np.uint32), good["points"].view(np.uint32))
    assert np.array_equal(still["points"].view(np.uint32), good["points"].view(np.uint32))
    bad = [only(nullArrays=1), only(nullArrays=2), only(nullArrays=4), only(nullArrays=8), dict(only(), points=edited("x", 0, np.inf)),
           dict(only(), points=edited("y", 1, np.nan)), dict(only(), points=edited("values", (3, 2), np.nan))]
    got = mc.run_host(exe, r, tmp_path, [c] + bad)
    assert [g["points_status"] for g in got] == [0] + [2] * len(bad)
    # no point: nothing to do, no refusal; -9999 and an infinite proxy value are values
    empty = dict(only(), points=dict(x=np.zeros(0, np.float32), y=np.zeros(0, np.float32), z=np.zeros(0, np.float32), values=np.zeros((mc.SLOTS, 0), np.float32)))
    assert mc.run_host(exe, r, tmp_path, [c, empty])[1]["points_status"] == 0


def test_the_entry_points_before_a_raster_are_the_library_s_refusal():
    sf = md.bind(capi.load_product())
    with pytest.raises(capi.SF3DError):                                     # no raster, no call: refused by the library, whatever the handle holds
        md.get_fit(sf)
    with pytest.raises(capi.SF3DError):
        md.points(sf, [0.0], [0.0], [0.0], np.zeros((0, 1), np.float32))
    assert md.bytes_held(sf) == 0 and md.kernel_ms(sf) == (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def off_pin(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("multidetrend_off_pin")
    out = {}
    for label in mc.OFF_PIN_LABELS:
        r, c = mc.off_pin(label)
        out[label] = (r, c, mc.run_host(exe, r, d, [c])[0])
    return out


@pytest.mark.parametrize("label", mc.OFF_PIN_LABELS)
def test_off_pin_host_build_equals_the_restatement_and_shows_the_row_s_property(off_pin, label):
    r, c, g = off_pin[label]
    mc.must_of(label)(r, c, g)
    assert g["points_status"] == 0 and len(g["points"]) == len(c["points"]["x"])
    mine = mc.restated(r, c)
    same(g, mine, label, mc.QUANTITIES)
    inside = r["dem"] != r["flag"]
    assert (g["value"][inside] != r["flag"]).all() and (g["value"][~inside] == r["flag"]).all()


def test_two_hours_on_one_block_the_sparse_one_reads_nothing_the_full_one_left(exe, tmp_path):
    r, hours = mc.two_hours()
    both = mc.run_host(exe, r, tmp_path, hours)
    alone = mc.run_host(exe, r, tmp_path, [hours[1]], name="sparse-alone")[0]
    assert both[0]["fitted"] == 129 and both[1]["fitted"] == 26 == alone["fitted"] and both[1]["kept"] < both[0]["kept"]
    same(both[1], alone, "the sparse hour behind the full one", mc.QUANTITIES)
    same(both[1], mc.restated(r, hours[1]), "the sparse hour against the restatement", mc.QUANTITIES)
