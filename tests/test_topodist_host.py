"""Topographic distance, the parts that need no GPU: the ABI of include/sf3d_topodist.h against the binding; the entry points exported
by the product library and absent from sf3d.h and the shim; the refusals that come before any device work; the per-cell text of the three
kernels compiled for the host (tests/topodist_host.cpp) equal to the compiled-reference pin tests/golden/topodist.npz on every value, and
once more as a stand-alone program under the address and undefined-behaviour sanitizers; the Python restatements (the maps, the
interpolation, the station matrix, the Kh search) equal to the pin; and the application's file names."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, esri, meteo, topodist
from tests import topodist_cases as tc
from tests.raster_helpers import bits, build_host_program, declared_entry_points, exported_names, header_text

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return tc.load_pin()


@pytest.fixture(scope="module")
def host(pin, tmp_path_factory):
    d = tmp_path_factory.mktemp("topodist_host")
    exe = build_host_program("topodist", d)
    return {name: tc.run_host(exe, pin[name], pin, d) for name in tc.RASTERS}


def test_header_and_binding_table_agree():
    text, declared = header_text("sf3d_topodist.h"), declared_entry_points("sf3d_topodist.h", "sf3d_topodist_")
    assert declared == sorted(topodist.SIGNATURES)
    assert re.search(rf"#define SF3D_TOPODIST_MAX_STEPS {topodist.MAX_STEPS}\b", text) and topodist.MAX_STEPS == 65536
    assert topodist.MAX_STATIONS == meteo.MAX_STATIONS == 1024
    device = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_device.h").read_text()
    assert re.search(rf"#define TOPODIST_MAX_STEPS {topodist.MAX_STEPS}\b", device)
    # getUseTdVar among the block's variables: all but precipitation, global irradiance and transmissivity
    assert [meteo.VARIABLES[v] for v in topodist.TD_VARIABLES] == ["airT", "relHum", "windInt", "dewT"]
    assert set(topodist.UNSUPPORTED) == set(meteo.UNSUPPORTED) - {"useTopographicDistance"} and len(topodist.UNSUPPORTED) == 6


def test_product_library_exports_the_entry_points_and_the_drop_in_abi_does_not():
    names = exported_names(build.build_product())
    assert set(topodist.SIGNATURES) <= names
    assert "topodist" not in (ROOT / "include" / "sf3d.h").read_text()
    assert not any("topodist" in n.lower() for n in capi.SIGNATURES) and not any("topodist" in n.lower() for n in capi.REFERENCE_API)
    assert not any("topodist" in n.lower() for n in exported_names(build.build_shim()))


def test_refusals_come_before_any_device_work():
    sf = topodist.bind(capi.load_product())
    lib = sf.lib
    many = meteo.MAX_STATIONS + 1
    x, v = np.zeros(many, np.float64), np.zeros(many, np.float32)
    bad = np.zeros(4, np.float64)
    idx = np.zeros(many, np.int32)
    px, pv, pi = x.ctypes.data_as(meteo.pf64), v.ctypes.data_as(meteo.pf32), idx.ctypes.data_as(topodist.pi32)
    assert lib.sf3d_topodist_bytes() == 0 and lib.sf3d_topodist_kernel_ms(0) == 0.0
    # sf3d_topodist_compute
    assert lib.sf3d_topodist_compute(4, px, px, px) == capi.MEMORY_ERROR                   # a valid call, no meteo raster
    assert lib.sf3d_topodist_compute(0, None, None, None) == capi.MEMORY_ERROR
    assert lib.sf3d_topodist_compute(meteo.MAX_STATIONS, px, px, px) == capi.MEMORY_ERROR  # the cap itself is allowed
    assert lib.sf3d_topodist_compute(many, px, px, px) == capi.PARAMETER_ERROR
    assert lib.sf3d_topodist_compute(4, px, None, px) == capi.PARAMETER_ERROR and lib.sf3d_topodist_compute(4, px, px, None) == capi.PARAMETER_ERROR
    for value in (np.nan, np.inf, -np.inf):
        bad[:] = 0.0
        bad[2] = value
        pb = bad.ctypes.data_as(meteo.pf64)
        for args in ((pb, px, px), (px, pb, px), (px, px, pb)):
            assert lib.sf3d_topodist_compute(4, *args) == capi.PARAMETER_ERROR
            assert lib.sf3d_topodist_station_matrix(4, *args, None, pv) == capi.PARAMETER_ERROR
    # the maps
    assert lib.sf3d_topodist_get_map(0, 16, pv) == capi.MEMORY_ERROR and lib.sf3d_topodist_set_map(0, 16, pv) == capi.MEMORY_ERROR
    assert lib.sf3d_topodist_drop_map(0) == capi.MEMORY_ERROR
    # sf3d_topodist_station_matrix
    assert lib.sf3d_topodist_station_matrix(4, px, px, px, pi, pv) == capi.MEMORY_ERROR
    assert lib.sf3d_topodist_station_matrix(many, px, px, px, pi, pv) == capi.PARAMETER_ERROR
    assert lib.sf3d_topodist_station_matrix(4, px, px, px, pi, None) == capi.PARAMETER_ERROR
    # sf3d_topodist_interpolate
    ok = meteo.settings_struct(dict(useTopographicDistance=1, proxies=[dict(active=1, isHeight=1, slope=-0.006)]))
    call = lambda var=0, method=0, ns=4, st=ok, kh=3, xs=px, zs=px: lib.sf3d_topodist_interpolate(var, method, ns, xs, px, zs, pv, pi, 100.0,
                                                                                                  ctypes.byref(st) if st is not None else None, kh, None)
    assert call() == capi.MEMORY_ERROR                                                     # a valid call, no raster yet
    assert call(st=meteo.settings_struct({})) == capi.MEMORY_ERROR                         # useTopographicDistance may be 0
    assert call(kh=0) == capi.MEMORY_ERROR and call(ns=meteo.MAX_STATIONS) == capi.MEMORY_ERROR
    assert call(kh=-1) == capi.PARAMETER_ERROR
    assert call(ns=many) == capi.PARAMETER_ERROR
    assert call(var=-1) == capi.PARAMETER_ERROR and call(var=len(meteo.VARIABLES)) == capi.PARAMETER_ERROR
    assert call(method=-1) == capi.PARAMETER_ERROR and call(method=3) == capi.PARAMETER_ERROR
    assert call(st=None) == capi.PARAMETER_ERROR and call(xs=None) == capi.PARAMETER_ERROR and call(zs=None) == capi.PARAMETER_ERROR
    bad[:] = 0.0
    bad[1] = np.nan
    assert call(zs=bad.ctypes.data_as(meteo.pf64)) == capi.PARAMETER_ERROR
    for option in topodist.UNSUPPORTED:                                                    # the six other options stay with the caller
        assert call(st=meteo.settings_struct({option: 1, "useTopographicDistance": 1})) == capi.PARAMETER_ERROR, option
    assert lib.sf3d_topodist_clean() == capi.OK and lib.sf3d_meteo_clean() == capi.OK


def test_the_pin_holds_what_the_issue_lists(pin):
    assert tc.PIN.stat().st_size < (1 << 18)
    relief, tiny = pin["relief"], pin["tiny"]
    assert relief["dem"].shape == (7, 37) and tiny["cell_size"] < 1.0 and tiny["xll"] > 1e5 and tiny["yll"] > 1e6
    assert (relief["dem"] == pin["flag"]).sum() >= 6 and len(relief["x"]) >= 12
    for must in ("walk from the cell (the cell is the lower end)", "walk from the station (or a tie)", "distance below a cell size", "sample on a flag cell",
                 "sample outside the grid", "map hit", "map miss falling back to the walk", "Shepard list by input order", "Shepard list by insertion",
                 "look-up: the float centre of a DEM cell lies in another cell"):
        assert pin["arms"][must] > 0, must
    cases = relief["cases"]
    assert {(c["method"], c["mode"]) for c in cases} >= {(m, mode) for m in range(3) for mode in ("none", "all", "mixed", "hand")}
    assert {c["kh"] for c in cases} >= {0, 1, 7, 40} and {meteo.VARIABLES[c["var"]] for c in cases} == {"airT", "relHum", "windInt", "prec"}
    x, y = relief["x"], relief["y"]
    w, h = 37 * relief["cell_size"], 7 * relief["cell_size"]
    assert (x < relief["xll"]).any() and (x > relief["xll"] + w).any() and (y < relief["yll"]).any() and (y > relief["yll"] + h).any()
    valid = relief["dem"][relief["dem"] != pin["flag"]]
    assert (relief["z"] < valid.min()).any() and (relief["z"] > valid.max()).any() and np.isin(relief["z"].astype(np.float32), valid).any()
    # the hand-made map differs from the computed one and changes the result
    assert (relief["hand_map"] != relief["maps"][relief["hand"]]).any()
    assert len(pin["opt"]) >= 2 and len({len(o["sub"]) for o in pin["opt"]}) >= 2
    assert all(np.isfinite(c["want"]).all() for r in (relief, tiny) for c in r["cases"])


@pytest.mark.parametrize("name", tc.RASTERS)
def test_host_build_of_the_kernels_text_equals_the_pin_on_every_value(pin, host, name):
    r = pin[name]
    maps, case_maps, matrices = host[name]
    assert np.array_equal(bits(maps), bits(r["maps"]))
    for k, c in enumerate(r["cases"]):
        bad = bits(case_maps[k]) != bits(c["want"])
        assert not bad.any(), (k, tc.case_name(c), int(bad.sum()), case_maps[k][bad][:4], c["want"][bad][:4])
    assert np.array_equal(bits(matrices), bits(r["matrices"]))
    assert (maps[r["dem"][None].repeat(len(maps), 0) != pin["flag"]] > 0).sum() > 100         # not vacuous


def test_host_build_under_the_sanitizers_reports_nothing(pin, host, tmp_path):
    """a stand-alone program with its own main: nothing is loaded into Python"""
    exe = build_host_program("topodist", tmp_path, sanitize=True)
    for name in tc.RASTERS:
        got = tc.run_host(exe, pin[name], pin, tmp_path)              # asserts exit status 0 and an empty stderr
        for a, b in zip(got, host[name]):
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", tc.RASTERS)
def test_restated_maps_and_matrices_equal_the_pin(pin, name):
    r = pin[name]
    for i in range(len(r["x"])):
        got = topodist.restate_map(r["dem"], r["xll"], r["yll"], r["cell_size"], r["x"][i], r["y"][i], r["z"][i], float(r["flag"]))
        assert np.array_equal(bits(got), bits(r["maps"][i])), i
    for k, mode in enumerate(pin["modes"]):
        held, index = tc.mode_maps(r, mode)
        got = topodist.restate_station_matrix(r["dem"], r["xll"], r["yll"], r["cell_size"], float(r["flag"]), r["x"], r["y"], r["z"], held, index)
        assert np.array_equal(bits(got), bits(r["matrices"][k])), mode
    # on the tiny raster the look-up is not the cell's own index: reading the station's map at the cell itself gives other values
    if name == "tiny":
        cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
        _, row, col, ok = topodist._lookup([], [], r["dem"].shape, r["xll"], r["yll"], r["cell_size"], cx.ravel().astype(np.float32), cy.ravel().astype(np.float32))
        r0, c0 = np.mgrid[0:r["dem"].shape[0], 0:r["dem"].shape[1]]
        assert ((row != r0.ravel()) | (col != c0.ravel()))[ok & (r["dem"].ravel() != r["flag"])].any()


@pytest.mark.parametrize("name", tc.RASTERS)
def test_restated_interpolation_equals_the_pin_in_every_cell_of_every_case(pin, name):
    r = pin[name]
    for k, c in enumerate(r["cases"]):
        got = tc.restated(r, c)
        bad = bits(got) != bits(c["want"])
        assert not bad.any(), (k, tc.case_name(c), int(bad.sum()), got[bad][:4], c["want"][bad][:4])
    if name == "relief":                                             # Kh, the maps and the hand-made map change the result
        by = {tc.case_name(c): c["want"] for c in r["cases"]}
        assert (by["airT-idw-kh0-all"] != by["airT-idw-kh7-all"]).any() and (by["airT-idw-kh7-all"] != by["airT-idw-kh40-all"]).any()
        assert np.array_equal(by["airT-idw-kh0-all"], by["airT-idw-kh0-none"])
        assert (by["airT-idw-kh4-hand"] != tc.restated(r, dict(r["cases"][0], kh=4, mode="all", method=0))).any()


def test_kh_zero_and_precipitation_equal_the_plain_interpolation(pin):
    r = pin["relief"]
    seen = 0
    for c in r["cases"]:
        if tc.effective_kh(c) == 0:
            plain = meteo.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], [None], c["var"], c["method"], r["x"], r["y"], c["value"], c["area"],
                                              dict(c["settings"], useTopographicDistance=0), float(r["flag"]))
            assert np.array_equal(bits(plain), bits(c["want"])), tc.case_name(c)
            seen += 1
    assert seen >= 12


def test_kh_search_equals_the_reference(pin):
    r = pin["relief"]
    for o in pin["opt"]:
        s = o["sub"]
        held, index = tc.mode_maps(r, o["mode"])
        matrix = topodist.restate_station_matrix(r["dem"], r["xll"], r["yll"], r["cell_size"], float(r["flag"]), r["x"][s], r["y"][s], r["z"][s], held, index[s])
        inside = ~((r["x"][s] < r["xll"]) | (r["y"][s] < r["yll"]) | (r["x"][s] >= r["xll"] + 37 * r["cell_size"]) | (r["y"][s] >= r["yll"] + 7 * r["cell_size"]))
        settings = dict(allZero=0, rainfallThreshold=0.2, useDetrending=1,
                        proxies=[dict(active=o["heightActive"], isHeight=1, inversion=0, slope=o["slope"])])
        pv = [[float(np.float32(z))] for z in r["z"][s]] if o["heightActive"] else None
        kh, series = topodist.optimize_kh(o["var"], o["method"], r["x"][s], r["y"][s], r["z"][s], o["value"], o["observed"], matrix, np.float32(o["area"]), settings,
                                          pin["max_kh"], pv, inside)
        assert kh == o["kh"] and isinstance(kh, int)
        assert np.array_equal(bits([p[0] for p in series]), bits(o["series_kh"]))
        assert np.array_equal(bits([p[1] for p in series]), bits(o["series_error"]))
    assert len({o["kh"] for o in pin["opt"]}) >= 2


def test_maps_round_trip_through_the_applications_files(pin, tmp_path):
    r = pin["relief"]
    ids = ["5012", "A_07", "station 3"]
    hdr = dict(xllcorner=r["xll"], yllcorner=r["yll"], cellsize=r["cell_size"], nodata=float(r["flag"]))
    paths = topodist.save_maps(tmp_path / "TD", "DATA/DEM/DEM_Ravone.flt", ids, r["maps"][:3], hdr)
    assert [p.name for p in paths] == ["TD_DEM_Ravone_5012", "TD_DEM_Ravone_A_07", "TD_DEM_Ravone_station 3"]
    assert all(p.with_suffix(".flt").exists() and Path(str(p) + ".hdr").exists() for p in paths)
    back = topodist.load_maps(tmp_path / "TD", "DEM_Ravone", ids + ["missing"])
    assert back[3] is None
    for a, b in zip(back[:3], r["maps"][:3]):
        assert np.array_equal(bits(a), bits(b))
    got, h = esri.read_grid(paths[0])
    assert h["ncols"] == 37 and h["nrows"] == 7 and h["cellsize"] == r["cell_size"] and h["nodata"] == float(r["flag"])
