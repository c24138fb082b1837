"""Glocal detrending, the parts that need no GPU: the ABI of include/sf3d_glocal.h against the binding; the entry points exported by the
product library and absent from sf3d.h and the shim; the pin's arm list; the per-area and per-cell text of k_glocal_areas and
k_glocal_cells compiled for the host (tests/glocal_host.cpp) equal to the compiled-reference pin tests/golden/glocal.npz in every cell
and every area quantity on both rasters, and once more as a stand-alone program under the address and undefined-behaviour sanitizers;
the Python restatement equal to the pin on `tiny`; `areas_from_maps` against a hand-made three-area layout; every refusal of
sf3d_glocal_set_areas and sf3d_glocal_interpolate through the HIP-free check functions the entry points share with the host program;
and off the pin (glocal_cases.OFF_PIN, and OFF_PIN_EDGES with the property of every row) the host build equal to the restatement, with the
flag an interpolate() raises when it gives NODATA: IDW on the stations' own place, both Shepard methods over one station."""
import hashlib
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, glocal as gl, localdetrend as ld, meteo
from tests import glocal_cases as gc
from tests.raster_helpers import build_host_program, declared_entry_points, exported_names, header_text, same

ROOT = Path(__file__).resolve().parent.parent
MUST = ("a cell visited by its area number 1", "a cell visited by its area number 2", "a cell visited by its area number 3", "a DEM cell covered by no area",
        "an area without a weight map", "weights that do not add up to 1", "a cell set to NODATA by a later area",
        "a cell set to NODATA by an earlier area and then refilled", "the height not active", "the height not significant",
        "the height significant with others significant", "a first guess skipped for leaving its range", "the double-inversion rule refuses a better R2",
        "bestR2 < 0 with the refit", "the maximum clamp with lambda >= 1000 not clamping", "a station pruned in the fit of step 1 but present in the rebuilt subset",
        "a station erased by detrendingOtherProxies in step 2", "a proxy significant in one area and not in another", "method idw", "method shepard",
        "method shepard_modified", "variable airT", "variable dewT", "function piecewiseTwo", "function piecewiseThreeFree", "function piecewiseThree")


@pytest.fixture(scope="module")
def pin():
    return gc.load_pin()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_program("glocal", tmp_path_factory.mktemp("glocal_host"))


@pytest.fixture(scope="module")
def host(pin, exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("glocal_run")
    return {name: gc.run_host(exe, pin[name], d) for name in gc.RASTERS}


def test_header_and_binding_table_agree():
    assert declared_entry_points("sf3d_glocal.h", "sf3d_glocal_") == sorted(gl.SIGNATURES)
    device = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_device.h").read_text()
    assert re.search(r"struct GlocalAreaDev\b", device) and "sf3d_localproxies.h" in header_text("sf3d_glocal.h")
    assert gl.MAX_CELLS == 1 << 24 and int(np.float32(gl.MAX_CELLS - 1)) == gl.MAX_CELLS - 1 and int(np.float32(gl.MAX_CELLS + 1)) != gl.MAX_CELLS + 1


def test_product_library_exports_the_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(gl.SIGNATURES) <= names
    assert "glocal" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("glocal" in n.lower() for n in capi.SIGNATURES) and not any("glocal" in n.lower() for n in capi.REFERENCE_API)
    assert not any("glocal" in n.lower() for n in exported_names(build.build_shim()))


def test_pin_reaches_every_arm_or_says_why_not(pin):
    explained = " ".join(pin["notes"])
    for arm in MUST:
        assert pin["arms"].get(arm, 0) > 0 or arm in explained, arm
    assert any("index order" in n for n in pin["notes"])
    assert gc.PIN.stat().st_size < (1 << 18)
    for name in gc.RASTERS:
        assert 2 <= len(pin[name]["areas"]) <= 5


@pytest.mark.parametrize("name", gc.RASTERS)
def test_host_build_equals_the_pin_in_every_cell_and_every_area_quantity(pin, host, name):
    for c, g in zip(pin[name]["cases"], host[name]):
        assert g["status"] == 0, gc.case_name(c)
        same(g, c["want"], f"{name} {gc.case_name(c)}", gc.QUANTITIES)


def test_restatement_equals_the_pin_on_tiny(pin):
    r = pin["tiny"]
    for c in r["cases"]:
        mine = gc.restated(r, c)
        assert not mine["failed"]
        same(mine, c["want"], f"tiny {gc.case_name(c)}", gc.QUANTITIES)


def test_unit_weights_make_the_weighted_marquardt_the_unweighted_one(pin):
    """what the kernel stands on: the weighted restatement with every weight 1 walks the unweighted one's parameters to the bit"""
    c = pin["tiny"]["cases"][0]
    fit, h, v = c["fit"], [float(a) for a in c["proxy_values"][0]], [float(a) for a in c["value"]]
    for guess in fit["first_guess"][:4]:
        a, b = [float(g) for g in guess], [float(g) for g in guess]
        gl.marquardt_unweighted(fit["function"], a, fit["min"], fit["max"], fit["delta"], h, v)
        ld.marquardt_fit(fit["function"], b, fit["min"], fit["max"], fit["delta"], h, v, [1.0] * len(v))
        assert np.array_equal(np.array(a).view(np.uint64), np.array(b).view(np.uint64))


def test_sanitized_host_program_runs_clean_on_the_pin_and_off_it(pin, host, tmp_path):
    san = build_host_program("glocal", tmp_path, sanitize=True)
    got = gc.run_host(san, pin["tiny"], tmp_path)                    # run_host_program asserts an empty stderr
    for c, g, h in zip(pin["tiny"]["cases"], got, host["tiny"]):
        same(g, h, gc.case_name(c), gc.QUANTITIES)
    r, c = gc.off_pin("lists65-130")
    assert gc.run_host(san, r, tmp_path, [c])[0]["status"] == 0
    r, c = gc.failing_area()
    assert gc.run_host(san, r, tmp_path, [c])[0]["status"] == 1
    # entries without a point, a chunk without one, lists of METEO_MAX_STATIONS entries, an area with no point at all
    for label in ("holes-third", "holes-run64-idw", "lists-cap", "empty-area"):
        r, c = gc.off_pin(label)
        assert gc.run_host(san, r, tmp_path, [c])[0]["status"] == 0, label
    r, c = gc.failing_single_station(meteo.SHEPARD)
    assert gc.run_host(san, r, tmp_path, [c])[0]["status"] == 1


def test_areas_from_maps_on_a_hand_made_layout():
    hdr = dict(nrows=2, ncols=3, xllcorner=100.0, yllcorner=200.0, cellsize=10.0, nodata_value=-9999.0)
    first = np.array([[0.5, 0.0, -9999.0], [1.0, 0.25, 0.0]], np.float32)
    # a map on a header of its own, shifted one cell to the east: the DEM's column 0 lies outside it
    shifted = (np.array([[0.7, 0.2, 0.1], [0.0, 0.3, -9999.0]], np.float32), dict(hdr, xllcorner=110.0))
    areas = gl.areas_from_maps(hdr, [first, shifted, None], [["b", "a", "zz"], ["c"], ["a", "c"]], ["a", "b", "c", "a"])
    assert [a["stations"] for a in areas] == [[1, 0], [2], [0, 2]]           # the csv's order, the first point of an id, an unknown id skipped
    assert areas[0]["cells"].tolist() == [0.0, 3.0, 4.0] and areas[0]["weights"].tolist() == [0.5, 1.0, 0.25]
    assert areas[1]["cells"].tolist() == [1.0, 2.0, 5.0] and np.allclose(areas[1]["weights"], [0.7, 0.2, 0.3])
    assert len(areas[2]["cells"]) == 0 and areas[0]["cells"].dtype == np.float32
    assert gl.cell_row_col(np.float32(5.0), 3) == (1, 2)
    flat = gl.flat_areas(areas)
    assert flat["cell_offset"].tolist() == [0, 3, 6, 6] and flat["station_offset"].tolist() == [0, 2, 3, 5]


def test_read_areas_reads_the_glocal_folder_and_the_csv_as_the_application_does(tmp_path):
    """loadGlocalStationsCsv: the area number in the first field, the ids after it; lines out of order, a gap (area 2: no line), a line
    with one field (skipped), a number that does not parse (0, QString::toInt) overwriting what area 0 held, an id that is a number"""
    from criteria3d_amd import esri
    hdr = dict(ncols=3, nrows=2, xllcorner=100.0, yllcorner=200.0, cellsize=10.0, nodata_value=-9999.0, byteorder="LSBFIRST")
    esri.write_grid(tmp_path / "glocalWeight_1", np.array([[0.5, 0.0, -9999.0], [1.0, 0.25, 0.0]], np.float32), hdr)
    (tmp_path / "areas.csv").write_text("3,c,1\n0,zz\n1,b,a\n7\nc\nx,a,c\n")
    assert gl.read_stations_csv(tmp_path / "areas.csv") == [["a", "c"], ["b", "a"], [], ["c", "1"]]
    areas = gl.read_areas(tmp_path, tmp_path / "areas.csv", hdr, ["a", "b", "c", "1"])
    assert [a["stations"] for a in areas] == [[0, 2], [1, 0], [], [2, 3]]                     # "1" is a station id in a line, never an area's
    assert areas[1]["cells"].tolist() == [0.0, 3.0, 4.0] and [len(a["cells"]) for a in areas] == [0, 3, 0, 0]
    (tmp_path / "bad.csv").write_text("-1,a\n")
    with pytest.raises(ValueError):
        gl.read_stations_csv(tmp_path / "bad.csv")


def _valid():
    r, c = gc.synthetic(n_stations=20, lists=(20, 9), method=meteo.IDW, n_others=1)
    r["name"] = "refusals"
    return r, c


def test_every_refusal_of_set_areas(exe, tmp_path):
    r, c = _valid()
    assert gc.run_host(exe, r, tmp_path, [c])[0]["status"] == 0
    cols = r["dem"].shape[1]
    n = r["dem"].size

    def refused(change) -> bool:
        q = dict(r, areas=[dict(a) for a in r["areas"]])
        change(q["areas"])
        return gc.run_host(exe, q, tmp_path, [c]) is None

    def set_cell(areas, value):
        areas[0]["cells"] = areas[0]["cells"].copy()
        areas[0]["cells"][2] = value

    def set_weight(areas, value):
        areas[0]["weights"] = areas[0]["weights"].copy()
        areas[0]["weights"][2] = value
    assert not refused(lambda a: None)
    assert refused(lambda a: set_cell(a, n)) and refused(lambda a: set_cell(a, -1.0)) and refused(lambda a: set_cell(a, np.nan))
    assert not refused(lambda a: set_cell(a, n - 1) if np.float32(n - 1) not in a[0]["cells"] else None)
    for w in (0.0, -9999.0, np.inf, np.nan):
        assert refused(lambda a, w=w: set_weight(a, w)), w
    assert refused(lambda a: set_cell(a, a[0]["cells"][3]))                                   # one cell twice in one area
    assert refused(lambda a: a[1].update(stations=np.arange(meteo.MAX_STATIONS + 1, dtype=np.int32)))
    assert refused(lambda a: a.clear())                                                       # no area
    # a raster of more than 2^24 cells: the float cell number is no longer exact
    run = lambda rows, columns: subprocess.run([str(exe), "shape", str(rows), str(columns)]).returncode
    assert run(4096, 4096) == 0 and run(4097, 4096) == 1 and run(0, 5) == 1
    assert cols == 11


def test_every_refusal_of_interpolate(exe, tmp_path):
    r, c = _valid()

    def status(**change) -> int:
        q = dict(c)
        for k, v in change.items():
            q[k] = v(c[k]) if callable(v) else v
        return gc.run_host(exe, r, tmp_path, [q])[0]["status"]

    def edited(a, at, value):
        a = np.array(a, copy=True)
        a[at] = value
        return a
    assert status() == 0
    assert status(options=dict(useLocalDetrending=1)) == 2 and status(options=dict(useMultipleDetrending=0)) == 2 and status(options=dict(nProxies=7)) == 2
    assert status(var=meteo.PRECIPITATION) == 2 and status(method=3) == 2
    assert status(point_index=lambda a: edited(a, 1, a[0])) == 2                              # a repeated point index
    # area 1 has cells and none of its stations has a point this hour
    theirs = set(int(s) for s in r["areas"][1]["stations"])
    assert status(point_index=lambda a: np.array([i + 1000 if int(i) in theirs else i for i in a], np.int32)) == 2
    keep = np.array([int(i) not in theirs for i in c["point_index"]])
    fewer = dict(point_index=c["point_index"][keep], x=c["x"][keep], y=c["y"][keep], value=c["value"][keep], proxy_values=c["proxy_values"][:, keep])
    assert status(**fewer) == 2
    assert status(x=lambda a: edited(a, 0, np.inf)) == 2 and status(proxy_values=lambda a: edited(a, (1, 0), np.nan)) == 2
    assert status(fit=dict(c["fit"], first_guess=[])) == 2 and status(fit=dict(c["fit"], stdDevThreshold=float("nan"))) == 2
    assert status(fit=dict(c["fit"], minPointsLocalDetrending=-3)) == 0                       # not read
    others = [dict(o) for o in c["others"]]
    others[1]["min"] = [5.0, 0.0]
    assert status(others=others) == 2                                                         # min > max
    many = meteo.MAX_STATIONS + 1
    big = dict(point_index=np.arange(many, dtype=np.int32), x=np.zeros(many), y=np.zeros(many), value=np.zeros(many, np.float32),
               proxy_values=np.zeros((gc.SLOTS, many), np.float32))
    assert status(**big) == 2
    # a call before sf3d_glocal_set_areas
    assert gc.run_host(exe, dict(r, areas=None, name="unset"), tmp_path, [c])[0]["status"] == 2


def test_the_getter_before_the_areas_is_the_library_s_refusal():
    sf = gl.bind(capi.load_product())
    with pytest.raises(capi.SF3DError):                                     # no raster, no areas: refused by the library, whatever the handle holds
        gl.get_area_fit(sf)


@pytest.fixture(scope="module")
def off_pin(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("glocal_off_pin")
    out = {}
    for label, _ in gc.OFF_PIN:
        r, c = gc.off_pin(label)
        out[label] = (r, c, gc.run_host(exe, r, d, [c])[0])
    return out


@pytest.mark.parametrize("label", [label for label, _ in gc.OFF_PIN])
def test_off_pin_host_build_equals_the_restatement(off_pin, label):
    r, c, g = off_pin[label]
    arms = {}
    mine = gc.restated(r, c, arms=arms)
    assert g["status"] == 0 and not mine["failed"]
    same(g, mine, label, gc.QUANTITIES)
    inside = r["dem"] != r["flag"]
    assert (g["value"][inside] != r["flag"]).any()
    if label.startswith("lists"):
        assert sorted(g["fitted"].tolist()) == [12, 30, 64, 65, 130] and len(r["areas"]) == 5
    if label.startswith("guesses31"):
        assert len(c["fit"]["first_guess"]) == 31
    if label == "five-deep":
        assert arms.get("a cell visited by more than three areas", 0) > 0


def test_an_interpolate_that_gives_nodata_raises_the_flag(exe, tmp_path):
    r, c = gc.failing_area()
    g = gc.run_host(exe, r, tmp_path, [c])[0]
    assert g["status"] == 1 and g["kept"][1] == 6
    assert gc.restated(r, c)["failed"]


# sha256 of glocal_cases.input_parts of the five cases of OFF_PIN as they stood before `synthetic` took use_detrending, var, empty_areas and missing
OFF_PIN_INPUTS = {"lists65-130": "4063fcca8a6b5481d6a3e77c5450ce43c44fa52092c7776dffd372822af7df5b",
                  "lists-modified": "925b240b42fc5736b9b948946921adce7656c78e672d2f78cdebb9a9511414ae",
                  "guesses31-three": "1f65c2a61ca51cf9aedaa439e74a637d4d94805f4a5cddaf522e924d37234040",
                  "guesses31-free": "14ae3b9ce6027bcfc437858170efa6dec75ecd1f7ae848e9969724e28b0ddeb5",
                  "five-deep": "1bd36a9df686377e1ef6623473fd8ac2d8b0ceee73df3c6c159552327f9959f9"}


def test_the_new_arguments_of_synthetic_leave_the_five_off_pin_cases_as_they_were():
    assert [label for label, _ in gc.OFF_PIN] == list(OFF_PIN_INPUTS)
    for label, want in OFF_PIN_INPUTS.items():
        r, c = gc.off_pin(label)
        h = hashlib.sha256()
        for part in gc.input_parts(r, [c]):
            h.update(np.ascontiguousarray(part).tobytes())
        assert h.hexdigest() == want, label


def test_without_points_cuts_the_call_and_leaves_the_areas():
    r, c = gc.off_pin("lists65-130")
    keep = gc.missing_points(r, c, ("every", 3))
    q = gc.without_points(c, keep)
    assert len(q["point_index"]) == 140 - 47 and q["proxy_values"].shape == (gc.SLOTS, 93) and len(c["point_index"]) == 140
    for key in ("point_index", "x", "y", "value"):
        assert np.array_equal(q[key], c[key][keep]) and len(q[key]) == 93
    assert np.array_equal(q["proxy_values"], c["proxy_values"][:, keep]) and q["fit"] is c["fit"] and q["area"] == c["area"]
    keep = gc.missing_points(r, c, ("entries", 1, 0, 64))
    assert keep.sum() == 140 - 64 and not np.isin(r["areas"][1]["stations"][:64], c["point_index"][keep]).any()


@pytest.mark.parametrize("label", gc.EDGE_LABELS)
def test_edge_rows_host_build_equals_the_restatement_and_shows_the_row_s_property(exe, tmp_path, label):
    """glocal_cases.OFF_PIN_EDGES: every quantity of the host build equal to the restatement's, and the outcome shows what the row is
    there for (its third column)"""
    _, arguments, must = next(row for row in gc.OFF_PIN_EDGES if row[0] == label)
    r, c = gc.off_pin(label)
    g = gc.run_host(exe, r, tmp_path, [c])[0]

    def again(**changed):
        q, qc = gc.synthetic(**dict(arguments, **changed))
        q["name"], qc["label"] = f"{label}-again", label
        return gc.run_host(exe, q, tmp_path, [qc])[0]
    must(r, c, g, again)
    mine = gc.restated(r, c)
    assert g["status"] == 0 and not mine["failed"]
    same(g, mine, label, gc.QUANTITIES)
    inside = r["dem"] != r["flag"]
    assert (g["value"][inside] != r["flag"]).any()


def test_the_sparse_hour_on_the_cap_s_areas_is_legal_and_fits_the_last_chunk_alone(exe, tmp_path):
    """what tests/test_gpu_glocal.py calls between two full hours: of the list of 1024 only entries of the last chunk have a point"""
    r, c = gc.off_pin("lists-cap")
    q = gc.without_points(c, gc.missing_points(r, c, gc.CAP_TAIL))
    g = gc.run_host(exe, r, tmp_path, [q])[0]
    assert g["status"] == 0 and g["fitted"][0] == 64 and (g["fitted"][1:] > 0).all() and (g["fitted"] < np.array(gc.lengths(r)) // 4).all()
    kept = g["station_kept"][gc.entries(r, 0)]
    assert kept.any() and not kept[:meteo.MAX_STATIONS - 64].any()
    mine = gc.restated(r, q)
    assert not mine["failed"]
    same(g, mine, "cap-tail", gc.QUANTITIES)


@pytest.mark.parametrize("method", (meteo.SHEPARD, meteo.SHEPARD_MODIFIED))
def test_both_shepard_methods_give_nodata_for_an_area_of_one_station(exe, tmp_path, method):
    r, c = gc.failing_single_station(method)
    g = gc.run_host(exe, r, tmp_path, [c])[0]
    assert g["status"] == 1 and g["fitted"].tolist() == [1, 30] and g["kept"][0] == 1
    mine = gc.restated(r, c)
    assert mine["failed"]
    same(g, mine, r["name"], gc.QUANTITIES)
