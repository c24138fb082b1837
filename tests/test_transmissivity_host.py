"""The station transmissivity block without a device: the header against the binding, what the entry points refuse before they need a
device, the Python restatement of criteria3d_amd/transmissivity.py against the compiled-reference pin (tests/golden/transmissivity.npz)
bit for bit on every case and station, the host build of the kernel's evaluation and summation text (tests/transmissivity_host.cpp)
against the pin - the int window widths and the float transmissivities, with no exclusions - the pin's arm table and cases, and the small
seeded sets of tests/transmissivity_cases.py against the arms of the pin.  The double sin / cos / tan of sf3d_trig.inc are not the C
library's, and here radPoint.global is summed as a double: equality of the host build with the pin is expected, not guaranteed by
construction; a (case, station) that differs would be listed in ONE_ULP below at one float ulp, at most three - none is."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, radiation as rad, transmissivity as tr
from tests import raster_helpers as rh
from tests import transmissivity_cases as tc

ROOT = Path(__file__).resolve().parent.parent
ONE_ULP = ()              # (case name, station) pairs whose float result differs from the pin by one ulp: none


@pytest.fixture(scope="module")
def pin():
    return tc.load_pin()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return rh.build_host_program("transmissivity", tmp_path_factory.mktemp("transmissivity_host"))


def test_header_and_binding_agree():
    text = (ROOT / "include" / "sf3d_transmissivity.h").read_text()
    declared = set(re.findall(r"\b(sf3d_transmissivity_\w+)\s*\(", text))
    assert declared == set(tr.SIGNATURES)
    assert ctypes.sizeof(tr.Point) == 40 and [f[0] for f in tr.Point._fields_] == ["x", "y", "z", "lat", "lon"]
    assert re.search(r"typedef struct \{\s*double x, y, z;\s*double lat, lon;\s*\} sf3d_transmissivity_point_t;", text)
    for name, value in (("MAX_WIDTH", tr.MAX_WIDTH), ("MAX_POINTS", tr.MAX_POINTS), ("WINDOW_SLOTS", tr.WINDOW_SLOTS)):
        assert re.search(rf"SF3D_TRANSMISSIVITY_{name} = {value}\b", text)
    assert tr.MAX_POINTS >= 1024 and tr.MAX_WIDTH == 63
    comments = re.findall(r"/\*((?:(?!\*/).)*)\*/\s*(?:sf3d_error_t|double) sf3d_transmissivity_\w+\(", text, re.S)
    assert len(comments) == len(tr.SIGNATURES) and all(re.search(r"\.cpp:\d+", c) for c in comments)      # every entry point cites file:line
    # sf3d_rad.h gains no entry point: its names are still the radiation binding's
    assert set(re.findall(r"\b(sf3d_rad_\w+)\s*\(", (ROOT / "include" / "sf3d_rad.h").read_text())) == set(rad.SIGNATURES)


def test_product_library_exports_the_entry_points_outside_the_drop_in_abi():
    functions = rh.exported_names(build.build_product(), "T")
    for name in tr.SIGNATURES:
        assert name in functions, name
    assert not any("transmissivity" in n for n in capi.SIGNATURES)


def test_refusals_without_a_device():
    sf = tr.bind(capi.load_product())
    lib = sf.lib
    assert rad.bind(sf).lib.sf3d_rad_clean() == capi.OK
    p = tr.point_array([[683800.0, 4928260.0, 130.0, 44.49, 11.31]] * 3)
    pp = p.ctypes.data_as(tr.ppoint)
    m = np.full((3, 13), 100.0, np.float32)
    pm = m.ctypes.data_as(capi.pf32)
    out = np.zeros(3, np.float32)
    po = out.ctypes.data_as(capi.pf32)
    nv = ctypes.c_uint32(7)
    steps = ctypes.c_int32(7)

    def points(when=(2021, 3, 20, 11, 30, 0), width=13, step=3600, n=3, pts=pp, meas=pm, res=po, valid=ctypes.byref(nv)):
        return lib.sf3d_transmissivity_points(*when, width, step, n, pts, meas, res, valid)

    def window(when=(2021, 3, 20, 11, 30, 0), step=3600, pt=pp, res=ctypes.byref(steps)):
        return lib.sf3d_transmissivity_window(*when, step, pt, res)
    # a valid call without an initialised radiation block
    assert points() == capi.MEMORY_ERROR and window() == capi.MEMORY_ERROR and points(n=0, pts=None, meas=None, res=None) == capi.MEMORY_ERROR
    # null pointers
    assert points(pts=None) == capi.PARAMETER_ERROR and points(meas=None) == capi.PARAMETER_ERROR and points(res=None) == capi.PARAMETER_ERROR
    assert points(valid=None) == capi.PARAMETER_ERROR and window(pt=None) == capi.PARAMETER_ERROR and window(res=None) == capi.PARAMETER_ERROR
    # an even or non-positive width, a width or a point count beyond the cap
    for w in (0, -1, 2, 12, 64, 65, 1001):
        assert points(width=w) == capi.PARAMETER_ERROR, w
    assert points(width=63) == capi.MEMORY_ERROR and points(width=1) == capi.MEMORY_ERROR
    assert points(n=tr.MAX_POINTS + 1) == capi.PARAMETER_ERROR
    # the time step
    for s in (0, -3600, 86401):
        assert points(step=s) == capi.PARAMETER_ERROR and window(step=s) == capi.PARAMETER_ERROR, s
    # a centre date or time that is none
    for when in ((2021, 0, 20, 11, 30, 0), (2021, 13, 1, 0, 0, 0), (2021, 2, 29, 0, 0, 0), (2021, 3, 0, 0, 0, 0), (2021, 3, 20, 24, 0, 0), (2021, 3, 20, -1, 0, 0),
                 (2021, 3, 20, 11, 60, 0), (2021, 3, 20, 11, 30, 60), (0, 3, 20, 11, 30, 0)):
        assert points(when=when) == capi.PARAMETER_ERROR and window(when=when) == capi.PARAMETER_ERROR, when
    assert points(when=(2020, 2, 29, 0, 0, 0)) == capi.MEMORY_ERROR
    assert (nv.value, steps.value) == (7, 7)                                 # nothing was written
    # the evaluations of a call that never ran
    w, e, g = np.zeros(39, np.uint8), np.zeros(39, np.float32), np.zeros(39)
    ev = lambda n=3, width=13, a=w.ctypes.data_as(tr.pu8), b=e.ctypes.data_as(capi.pf32), c=g.ctypes.data_as(capi.pd): lib.sf3d_transmissivity_get_evaluations(n, width, a, b, c)
    assert ev() == capi.MEMORY_ERROR and ev(a=None) == capi.PARAMETER_ERROR and ev(b=None) == capi.PARAMETER_ERROR and ev(c=None) == capi.PARAMETER_ERROR
    assert ev(width=0) == capi.PARAMETER_ERROR and ev(width=64) == capi.PARAMETER_ERROR
    assert lib.sf3d_transmissivity_kernel_ms() == 0.0


def test_samani_and_station_points(pin):
    assert tr.samani(-9999.0, 20.0, 0.17) == -9999.0 and tr.samani(5.0, -9999.0, 0.17) == -9999.0 and tr.samani(5.0, 20.0, -9999.0) == -9999.0
    assert tr.samani(21.0, 20.0, 0.17) == 0.0                                # `return false`
    assert tr.samani(4.0, 20.0, 0.17) == np.float32(np.float32(0.17) * np.float32(4.0)) and tr.samani(20.0, 20.0, 0.17) == 0.0
    # a NODATA height is the DEM's value at the point's cell, the flag on a flag cell and outside; column 0 one metre west of the raster
    k = next(k for k, c in enumerate(pin["cases"]) if c["raster"] == 1 and len(pin[f"xyz{k}"]) == 7)
    dem, flag, geo = tc.raster_of(pin, 1)
    xyz, st = pin[f"xyz{k}"], pin[f"stations{k}"]
    rows = dem.shape[0]
    cell = lambda p: ((rows - 1) - int((p[1] - geo[1]) / geo[2]), int((p[0] - geo[0]) / geo[2]))
    assert xyz[1][2] == -9999.0 and st[1][2] == dem[cell(xyz[1])] != flag
    assert xyz[2][2] == -9999.0 and st[2][2] == flag and dem[cell(xyz[2])] == flag
    assert xyz[3][0] < geo[0] and cell(xyz[3])[1] == 0 and st[3][2] == dem[cell(xyz[3])]
    assert st[4][2] > dem[dem != flag].max() and np.array_equal(st[:, :2], xyz[:, :2])
    r = pin["rasters"][1]
    again = tr.station_points(xyz[:, 0], xyz[:, 1], xyz[:, 2], dict(utmZone=r["utmZone"], startLatitude=r["startLatitude"]), dem,
                              dict(xllcorner=geo[0], yllcorner=geo[1], cellsize=geo[2]), flag)
    assert np.array_equal(again, st) and 44.4 < st[0][3] < 44.6 and 11.2 < st[0][4] < 11.4
    assert pin["stations" + str(next(k for k, c in enumerate(pin["cases"]) if c["raster"] == 2))][0][3] < -33.9        # the southern raster


def test_the_pin_reaches_every_arm_and_holds_the_cases_the_issue_lists(pin):
    assert list(pin["arm_names"]) == list(tr.ARMS) and (pin["arm_counts"] > 0).all()
    assert list(pin["model_arm_names"]) == list(rad.ARMS)
    model = dict(zip(pin["model_arm_names"], pin["model_arm_counts"]))
    for n in ("not illuminated", "illuminated", "shadow: hit", "shadow: miss (above the highest cell)", "shadow: ray left the grid", "real sky: total transmissivity",
              "real sky: Linke", "clear sky: total transmissivity", "clear sky: Linke", "air mass > 20", "A0 patch (A0 Trd < 0.0022)", "flat (slope == 0)",
              "false: S_solpos range check"):
        assert model[n] > 0, n
    assert (tc.GOLDEN / "transmissivity.npz").stat().st_size <= (tc.GOLDEN / "ravone_window.npz").stat().st_size
    cases = pin["cases"]
    names = " | ".join(c["name"] for c in cases)
    for piece in ("noon", "hour of sunrise", "hour of sunset", "wholly at night", "across midnight", "across the year's end", "isUTC off", "S_solpos refuses",
                  "NODATA is added", "2101", "total transmissivity, real sky", "clear sky", "no shadowing", "monthly Linke", "Linke map", "south", "window: "):
        assert piece in names, piece
    pts = [c for c in cases if c["mode"] == tc.POINTS]
    assert {(c["width"], c["step"]) for c in pts} >= {(w, s) for w in (1, 3, 13, 23) for s in (3600, 1800)}
    assert {len(c["arms"]) for c in pts} >= {1, 7, 40} and {c["raster"] for c in cases} == {0, 1, 2}
    assert pin["rasters"][2]["startLatitude"] < 0
    kinds = {k for c in pts for k in c["kinds"]}
    assert kinds == set(tc.KINDS)
    # the two counts either side of 0.66 * width, for each width above 1
    for w in (3, 13, 23):
        enough = int(np.ceil(0.66 * w))
        counts = set()
        for k, c in enumerate(cases):
            if c["mode"] == tc.POINTS and c["width"] == w:
                m = pin[f"measured{k}"]
                centre_there = m[:, (w - 1) // 2] != -9999.0
                counts |= set((m != -9999.0).sum(axis=1)[centre_there].tolist())
        assert {enough, enough - 1} <= counts, (w, counts)
    night = next(k for k, c in enumerate(cases) if "wholly at night" in c["name"])
    assert all(a & tr._A["sumClearSky <= 1e-6: Kt = 0"] for a in cases[night]["arms"] if a & tr._A["result computed"])
    assert (pin[f"result{night}"][[bool(a & tr._A["result computed"]) for a in cases[night]["arms"]]] == 0).all()
    windows = np.concatenate([pin[f"result{k}"] for k, c in enumerate(cases) if c["mode"] == tc.WINDOW])
    assert {1, 23} <= set(windows.tolist()) and len(set(windows.tolist()) - {1, 23}) >= 3 and (windows % 2 == 1).all()
    assert any(c["ret"] == 0 for c in pts) or all(c["ret"] == 1 for c in pts)
    clamp = np.float32(1.2 * 0.75)
    assert any((pin[f"result{k}"] == clamp).any() for k, c in enumerate(cases) if c["mode"] == tc.POINTS)


def test_restatement_equals_the_compiled_reference_in_every_case_and_station(pin):
    union = 0
    for k, c in enumerate(pin["cases"]):
        dem, flag, geo = tc.raster_of(pin, c["raster"])
        grid = tr.grid_of(dem, flag, *geo)
        st = pin[f"stations{k}"]
        if c["mode"] == tc.POINTS:
            got, n_valid, arms, model, _ = tr.restate_points(grid, c["settings"], c["when"], c["width"], c["step"], st, pin[f"measured{k}"])
            assert not rh.differing(got, pin[f"result{k}"]).any(), c["name"]
            assert (n_valid > 0) == bool(c["ret"]), c["name"]
        else:
            res = [tr.restate_window(grid, c["settings"], c["when"], p, c["step"]) for p in st]
            assert [v[0] for v in res] == pin[f"result{k}"].tolist(), c["name"]
            arms = [v[1] for v in res]
        assert [int(a) for a in arms] == c["arms"], c["name"]
        union |= int(np.bitwise_or.reduce(np.asarray(arms, np.int64)))
    assert union == (1 << len(tr.ARMS)) - 1


def test_host_build_of_the_kernels_text_equals_the_pin(pin, host, tmp_path):
    """the window widths with zero exclusions; the float transmissivities bit for bit but for the pairs of ONE_ULP (none)"""
    checked, differing = 0, []
    for r in range(len(pin["rasters"])):
        dem, flag, geo = tc.raster_of(pin, r)
        idx, calls = tc.pin_calls(pin, r)
        for k, got in zip(idx, tc.run_host(host, tmp_path, dem, flag, geo, calls, tag=f"pin{r}")):
            c = pin["cases"][k]
            assert (got["status"] == 0).all(), c["name"]
            if c["mode"] == tc.WINDOW:
                assert got["result"].tolist() == pin[f"result{k}"].tolist(), c["name"]
            else:
                same = ~rh.differing(got["result"], pin[f"result{k}"])
                differing += [(c["name"], int(s), float(got["result"][s]), float(pin[f"result{k}"][s])) for s in np.nonzero(~same)[0]]
            checked += 1
    assert checked == len(pin["cases"]) >= 40
    for name, s, mine, want in differing:
        print("differs:", name, s, mine, want)
    assert sorted((n, s) for n, s, _, _ in differing) == sorted(ONE_ULP) and len(ONE_ULP) <= 3
    for _, _, mine, want in differing:
        assert abs(int(np.float32(mine).view(np.int32)) - int(np.float32(want).view(np.int32))) == 1


def test_host_build_equals_the_restatement_off_the_pin_and_the_small_sets_reach_every_arm(pin, host, tmp_path):
    ref, windows = tc.small_reference()
    dem, flag, geo = tc.raster_of(pin, 1)
    calls = [(tc.SMALL[s][0], tc.SMALL[s][1], tc.POINTS, s[1], tc.SMALL[s][2], tc.small_set(s)[0], tc.small_set(s)[1]) for s in tc.SHAPES]
    st = tc.small_set((65, 23))[0]
    calls += [(settings, when, tc.WINDOW, tr.WINDOW_SLOTS, step, st[:count], None) for settings, when, step, count in tc.SMALL_WINDOWS]
    got = tc.run_host(host, tmp_path, dem, flag, geo, calls, tag="small")
    union = 0
    for shape, g in zip(tc.SHAPES, got):
        want, _, arms, evals = ref[shape]
        assert not rh.differing(g["result"], want).any(), shape
        for p, slots in enumerate(evals):                                   # the double global and the elevation of every evaluation
            for s, (written, elev, glob) in slots.items():
                assert g["written"][p, s] == written and not rh.differing(g["elev"][p, s], np.float32(elev)).any(), (shape, p, s)
                # the restatement's sin / cos / tan are the C library's, the kernel text's are faithful routines (within an ulp): the double
                # differs in its last places at most, through a handful of well-conditioned operations
                assert written == 0 or abs(g["glob"][p, s] - glob) <= 1e-12 * abs(glob), (shape, p, s, g["glob"][p, s], glob)
            assert int(g["written"][p].sum()) == sum(v[0] for v in slots.values())
        union |= int(np.bitwise_or.reduce(arms))
    for (steps, arms), g, (_, _, _, count) in zip(windows, got[len(tc.SHAPES):], tc.SMALL_WINDOWS):
        keep = [k for k, v in enumerate(steps) if v is not None]
        assert len(keep) >= 3 and [steps[k] for k in keep] == g["result"][keep].tolist()
        assert [k for k in range(count) if g["status"][k]] == [k for k in range(count) if steps[k] is None]
        union |= int(np.bitwise_or.reduce(np.asarray(arms, np.int64)))
    missing = [n for k, n in enumerate(tr.ARMS) if not union >> k & 1]
    assert not missing, missing


def test_host_build_runs_clean_under_asan_and_ubsan_as_a_stand_alone_program(pin, tmp_path):
    """the program has its own main and is not loaded into python; a sanitizer report ends it with a non-zero status"""
    exe = rh.build_host_program("transmissivity", tmp_path, sanitize=True)
    dem, flag, geo = tc.raster_of(pin, 1)
    idx, calls = tc.pin_calls(pin, 1)
    got = tc.run_host(exe, tmp_path, dem, flag, geo, calls, tag="san")
    k0 = idx[0]
    assert not rh.differing(got[0]["result"], pin[f"result{k0}"]).any()
