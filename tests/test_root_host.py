"""Root length, depth and density maps, the parts that need no GPU: the ABI of include/sf3d_root.h against the binding, the error codes
of the entry points, the Python restatement of computeRootLength3D / computeRootDensity3D equal to the compiled-reference pin
tests/golden/root_density.npz bit for bit, the pin's arms, the root and soil table readers on the Ravone fixtures, the host lunette
table against the values the pin recorded; and the host build of the kernels' text behind the entry point's table builder
(tests/root_host.cpp): equal to the pin and to the restatement bit for bit, clean under the address and undefined-behaviour sanitizers on
the edges of the tables."""
import ctypes
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from criteria3d_amd import build, capi, crop, project3d as p3, root
from tests import root_cases as rc
from tests.raster_helpers import bits, build_host_program, declared_entry_points, differing, exported_names, header_text

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return rc.load_pin()


def test_root_header_and_binding_table_agree():
    text, declared = header_text("sf3d_root.h"), declared_entry_points("sf3d_root.h", "sf3d_root_")
    assert declared == sorted(root.SIGNATURES)
    assert not set(declared) & set(capi.SIGNATURES) and not set(declared) & set(crop.SIGNATURES)          # sf3d.h and sf3d_crop.h are unchanged
    for name, value in (("SOILS", root.MAX_SOILS), ("HORIZONS", root.MAX_HORIZONS), ("LAYERS", root.MAX_LAYERS), ("ATOMS", root.MAX_ATOMS)):
        assert re.search(rf"#define SF3D_ROOT_MAX_{name} {value}\b", text), name
    for k, n in enumerate(("CYLINDRICAL", "CARDIOID", "GAMMA")):
        assert re.search(rf"SF3D_ROOT_{n}_DISTRIBUTION = {k}\b", text)
    assert (root.CYLINDER, root.CARDIOID, root.GAMMA) == (0, 1, 2)
    for k, n in enumerate(("LINEAR", "EXPONENTIAL", "LOGISTIC")):
        assert re.search(rf"SF3D_ROOT_{n} = {k}\b", text) and getattr(root, n) == k
    # sf3d_root_unit_t: four int32 then four doubles, in the header's order; sf3d_root_soil_t: a double, two int32, three arrays of doubles
    unit = re.search(r"typedef struct \{([^}]*)\} sf3d_root_unit_t;", text).group(1)
    assert re.findall(r"int32_t (\w+);", unit) == list(root.UNIT_INT_FIELDS)
    assert [n.strip() for n in re.search(r"double ([\w, ]+);", unit).group(1).split(",")] == list(root.UNIT_DOUBLE_FIELDS)
    assert ctypes.sizeof(root.Unit) == 48 and root.Unit.shapeDeformation.offset == 16
    soil = re.search(r"typedef struct \{([^}]*)\} sf3d_root_soil_t;", text).group(1)
    assert re.findall(r"(?:double|int32_t) (\w+)", soil)[:3] == ["totalDepth", "nrHorizons", "reserved"]
    assert re.findall(r"(\w+)\[SF3D_ROOT_MAX_HORIZONS\]", soil) == ["upperDepth", "lowerDepth", "soilFraction"]
    assert ctypes.sizeof(root.Soil) == 16 + 3 * 8 * root.MAX_HORIZONS and root.Soil.upperDepth.offset == 16
    assert ctypes.sizeof(crop.Unit) == 96                                  # the crop table is as it was


def test_product_library_exports_the_root_entry_points():
    names = exported_names(build.build_product())
    assert set(root.SIGNATURES) <= names


def test_error_codes_without_a_device(pin):
    sf = root.bind(capi.load_product())
    lib = sf.lib
    n = 16
    d = np.zeros(n * 4, np.float64).ctypes.data_as(root.pf64)
    f = np.zeros(n, np.float32)
    pf = f.ctypes.data_as(root.pf32)
    i = np.zeros(n, np.int32)
    pi = i.ctypes.data_as(root.pi32)
    assert lib.sf3d_root_compute(n, pf) == capi.MEMORY_ERROR                       # before initialise
    assert lib.sf3d_root_compute(n, None) == capi.MEMORY_ERROR
    assert lib.sf3d_root_get_length(n, d) == capi.MEMORY_ERROR
    assert lib.sf3d_root_get_depth(n, d) == capi.MEMORY_ERROR
    assert lib.sf3d_root_get_layers(n, pi, pi) == capi.MEMORY_ERROR
    assert lib.sf3d_root_get_density(-1, n, d) == capi.MEMORY_ERROR
    assert lib.sf3d_root_get_keys(n, pi) == capi.MEMORY_ERROR
    assert lib.sf3d_root_table_rows() == 0 and lib.sf3d_root_kernel_ms(0) == 0.0
    units, soils = root.unit_array(pin["unit_list"]), root.soil_array(pin["soil_list"])
    nu, ns = len(pin["unit_list"]), len(pin["soil_list"])
    ld = np.ascontiguousarray(pin["layer_depth"]).ctypes.data_as(root.pf64)
    lt = np.ascontiguousarray(pin["layer_thickness"]).ctypes.data_as(root.pf64)
    nl = len(pin["layer_depth"])
    init = lambda *a: lib.sf3d_root_initialize(*a)
    ok = [4, 4, pf, -9999.0, nl, ld, lt, pi, pi, nu, units, ns, soils]

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return init(*a)
    assert with_(a0=0) == capi.PARAMETER_ERROR and with_(a1=0) == capi.PARAMETER_ERROR                     # empty raster
    assert with_(a2=None) == capi.PARAMETER_ERROR and with_(a7=None) == capi.PARAMETER_ERROR and with_(a8=None) == capi.PARAMETER_ERROR
    assert with_(a4=0) == capi.PARAMETER_ERROR and with_(a4=root.MAX_LAYERS + 1) == capi.PARAMETER_ERROR   # the layer cap
    assert with_(a5=None) == capi.PARAMETER_ERROR and with_(a6=None) == capi.PARAMETER_ERROR
    assert with_(a9=root.MAX_UNITS + 1) == capi.PARAMETER_ERROR and with_(a10=None) == capi.PARAMETER_ERROR
    assert with_(a11=root.MAX_SOILS + 1) == capi.PARAMETER_ERROR and with_(a12=None) == capi.PARAMETER_ERROR
    assert with_(a9=0) == capi.PARAMETER_ERROR                                                             # crop index 0 >= nUnits 0
    assert with_(a11=0) == capi.PARAMETER_ERROR                                                            # soil index 0 >= nSoils 0
    many = root.soil_array([dict(pin["soil_list"][0], upperDepth=[0.0] * 17, lowerDepth=[1.5] * 17, soilFraction=[1.0] * 17)])
    assert with_(a11=1, a12=many) == capi.PARAMETER_ERROR                                                  # 17 horizons
    deep = root.soil_array([dict(totalDepth=10.3, upperDepth=[0.0], lowerDepth=[10.3], soilFraction=[1.0])])
    assert with_(a11=1, a12=deep) == capi.PARAMETER_ERROR                                                  # more atoms than the cap
    none = root.soil_array([dict(totalDepth=-9999.0, upperDepth=[], lowerDepth=[], soilFraction=[])])
    assert with_(a11=1, a12=none) == capi.PARAMETER_ERROR                                                  # a soil of the raster without depth
    assert lib.sf3d_root_get_length(n, d) == capi.MEMORY_ERROR                                             # a refused initialise leaves no raster
    assert lib.sf3d_root_clean() == capi.OK


def test_the_pin_reaches_every_arm(pin):
    dem, flag = pin["dem"], pin["flag"]
    assert dem.shape == (24, 32) and rc.PIN.stat().st_size <= (ROOT / "tests" / "golden" / "snow_brooks.npz").stat().st_size
    assert list(pin["window"]) == [8, 280, 24, 32]                      # the snow and crop pins' window
    assert [str(n) for n in pin["unit_fields"]] == list(root.UNIT_FIELDS)
    arms = dict(zip((str(n) for n in pin["arm_names"]), (int(c) for c in pin["arm_counts"])))
    assert len(arms) >= 25 and all(c > 0 for c in arms.values()), {k: c for k, c in arms.items() if c == 0}
    for must in ("length: static roots", "length: linear growth", "length: logistic growth", "density: cylinder", "density: cardioid",
                 "density: gamma unit (becomes a cardioid)", "density: shapeDeformation < 1", "density: shapeDeformation in [1, 2]", "density: shapeDeformation > 2",
                 "density: rootDepthMin zero", "density: rootDepthMin non-zero", "length: rootDepthMax beyond the soil depth",
                 "density: roots too short (0 rooted atoms)", "density: atom clamp (top + rooted > nrAtoms)", "density: renormalised (coarse fragments differ)",
                 "density: not renormalised", "density: a layer below the last horizon", "cell: no crop index", "cell: no soil index", "cell: degree days at the flag",
                 "length: degree days <= 0", "length: degree days in (0, 1]", "length: beyond degreeDaysRootGrowth"):
        assert arms[must] > 0, must
    for n in rc.OUTPUTS:
        assert np.isfinite(pin[n]).all(), n
    assert np.isfinite(pin["degree_days"]).all() and len(pin["degree_days"]) >= 4
    # the layer grid cuts the deepest soil
    assert pin["layer_depth"][-1] + pin["layer_thickness"][-1] / 2 < pin["soil_total_depth"].max()
    calls = json.loads(str(pin["library_calls"]))
    assert "exp" in calls["getRootLengthDD"] and {"exp", "atan2"} <= set(calls["cardioidDistribution"]) and "round" in calls["computeRootDensity3D"]
    assert not any("log" in c for v in calls.values() if v for c in v)          # log(9.) ... are folded constants in the pin build


def test_restatement_equals_the_compiled_reference_on_every_map(pin):
    computed = 0
    for k in range(len(pin["degree_days"])):
        got = rc.restated(pin, k)
        for n in rc.OUTPUTS:
            bad = bits(got[n]) != bits(pin[n][k])
            print(f"map {k} {n}: {int(bad.sum())} values differ")
            assert not bad.any(), (k, n, int(bad.sum()), got[n][bad][:4], pin[n][k][bad][:4])
        computed += int((got["length"] != float(pin["flag"])).sum())
    # not vacuous: densities present, early returns present, keys repeat
    assert computed > 3000 and (pin["density"] > 0).any() and (pin["first"] == -9999).any() and (pin["last"] > 5).any()
    dens = pin["density"][2].reshape(len(pin["layer_depth"]), -1).T
    assert len(np.unique(dens, axis=0)) < dens.shape[0] // 2


def test_restatement_by_hand(pin):
    u = dict(rootShape=root.CYLINDER, growth=root.LINEAR, isRootStatic=0, degreeDaysRootGrowth=1000, shapeDeformation=1.0, rootDepthMin=0.0, rootDepthMax=0.5,
             degreeDaysEmergence=0.0)
    assert root.restate_root_length(u, 0.0, 1.0) == (0.0, 0.0) and root.restate_root_length(u, 1.0, 1.0) == (0.0, 0.0)
    assert root.restate_root_length(u, 500.0, 1.0) == (0.25, 0.25) and root.restate_root_length(u, 1001.0, 1.0) == (0.5, 0.5)
    assert root.restate_root_length(u, 1001.0, 0.3) == (0.3, 0.3)                                      # the soil cuts rootDepthMax
    assert root.restate_root_length(dict(u, growth=root.EXPONENTIAL), 500.0, 1.0)[0] == -9999.0
    soil = dict(totalDepth=1.0, upperDepth=[0.0], lowerDepth=[1.0], soilFraction=[1.0])
    ld, lt = [0.0, 0.05, 0.15, 0.25, 0.35], [0.0, 0.1, 0.1, 0.1, 0.1]
    dens, first, last = root.restate_root_density(u, soil, ld, lt, 0.2)
    # 20 rooted atoms of 0.05 each: atom 0 (depth 0) lies in the surface layer, atoms 1-10 in layer 1, atoms 11-19 in layer 2
    assert (first, last) == (0, 2) and dens[0] == 0.05 and abs(dens[1] - 0.5) < 1e-12 and abs(dens[2] - 0.45) < 1e-12 and dens[3:] == [0.0, 0.0]
    assert root.restate_root_density(u, soil, ld, lt, 0.0) == ([0.0] * 5, -9999, -9999)
    assert root.restate_root_density(u, soil, ld, lt, 0.004) == ([0.0] * 5, -9999, -9999)             # too short: 0 rooted atoms
    assert root._round_int(0.5) == 1 and root._round_int(2.5) == 3 and root._round_int(-0.5) == -1 and root._round_int(28.499999) == 28


def test_lunette_table_against_the_recorded_values(pin):
    o = 0
    for m in pin["lunette_m"]:
        got = np.array(root.lunette(int(m)))
        assert np.array_equal(got.view(np.uint64), pin["lunette"][o:o + m].view(np.uint64)), int(m)
        o += int(m)
    assert o == len(pin["lunette"]) and abs(root.lunette(7)[-1] - 0.5) < 1e-12


def test_root_and_soil_table_readers():
    rows = json.loads((ROOT / "tests" / "golden" / "ravone_crops.json").read_text())
    inp = p3.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz")
    table = p3.root_table(rows["crop"], inp.land_units)
    assert [t["id_crop"] for t in table] == ["SHRUB", "BROADLEAF", "BARE"] and [t["isCrop"] for t in table] == [1, 1, 0]
    shrub, broad, bare = table
    assert (shrub["rootShape"], shrub["growth"], shrub["isRootStatic"]) == (root.CARDIOID, root.LOGISTIC, 1)          # root_shape 4, a tree
    assert (shrub["rootDepthMin"], shrub["rootDepthMax"], shrub["shapeDeformation"]) == (0.05, 1.4, 0.0)
    assert (broad["rootDepthMax"], broad["degreeDaysRootGrowth"], shrub["degreeDaysRootGrowth"]) == (2.0, 2500, 1000)  # '' -> degree_days_lai_increase
    assert set(root.UNIT_FIELDS) <= set(shrub) and bare["rootDepthMax"] == 0.0
    root.unit_array(table)
    assert [p3.root_distribution_type(v) for v in ("cylinder", "cardioid", "gamma function", "anything", 1, 4, 5, 7, "", None, "1")] == [0, 1, 2, 1, 0, 1, 2, 1, 1, 1, 0]
    assert [p3.root_growth_type(v) for v in ("linear", "exponential", "logistic", "", None, "LINEAR")] == [0, 1, 2, 2, 2, 0]
    annual = dict(rows["crop"][1], id_crop="WHEAT", type="herbaceous", root_shape="cylinder", root_growth="linear", degree_days_root_increase=900)
    t = p3.root_table([annual], [dict(id=1, id_crop="WHEAT")])[0]
    assert (t["rootShape"], t["growth"], t["isRootStatic"], t["degreeDaysRootGrowth"]) == (root.CYLINDER, root.LINEAR, 0, 900)
    with pytest.raises(ValueError):
        p3.root_table(rows["crop"], [dict(id=9, id_crop="NOSUCHCROP")])
    soils = p3.soil_root_table(inp.soils)
    assert len(soils) == len(inp.soils) <= root.MAX_SOILS
    assert max(len(s["upperDepth"]) for s in soils) <= root.MAX_HORIZONS // 1 and max(len(s["upperDepth"]) for s in soils) == 9
    assert max(int(s["totalDepth"] * 100) + 1 for s in soils) == 321 <= root.MAX_ATOMS // 2               # room to spare
    age1 = soils[2]
    assert age1["totalDepth"] == 1.5 and age1["soilFraction"] == [0.99, 1.0, 1.0, 1.0] and age1["lowerDepth"] == [0.5, 0.8, 1.2, 1.5]
    root.soil_array(soils)
    thick, _ = p3.soil_layers(0.95)
    assert len(thick) <= root.MAX_LAYERS


# ---- the host build of the text of k_root_table, k_root_cell and k_root_gather behind sf3d_root_initialize's table builder
# (tests/root_host.cpp): the text == the pin, the text == the restatement

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("root_host")
    return SimpleNamespace(dir=d, exe=build_host_program("root", d), san=build_host_program("root", d, sanitize=True))


def _pin_case(pin):
    return rc.case_of(pin, pin["dem"], pin["crop_index"], pin["soil_index"], pin["degree_days"])


def _random_cases(pin):
    for shape in rc.SHAPES:
        for seed in rc.SEEDS:
            for continuous in (False, True):
                yield f"{'continuous' if continuous else 'lists'}-{shape[0]}x{shape[1]}-{seed}", rc.random_case(pin, shape, seed, continuous)


def test_host_text_equals_the_pin_on_every_map(pin, host):
    """no libm escape: the text carries its own exp; atan2 of the lunette table is the C library's on both sides"""
    got = rc.run_host(host.exe, host.dir, "pin", _pin_case(pin))
    assert got["status"] == 0 and len(got["maps"]) == len(pin["degree_days"])
    for k, maps in enumerate(got["maps"]):
        for n in rc.OUTPUTS:
            bad = differing(maps[n], pin[n][k])
            print(f"host text, map {k} {n}: values differ: {int(bad.sum())}")
            assert not bad.any(), (k, n, int(bad.sum()), maps[n][bad][:4], pin[n][k][bad][:4])
    # the gathered layers from layer 3 on are the same maps
    part = rc.run_host(host.exe, host.dir, "pin-3", _pin_case(pin), layer0=3)
    for k, maps in enumerate(part["maps"]):
        assert not differing(maps["density"], pin["density"][k][3:]).any() and not differing(maps["key"], got["maps"][k]["key"]).any(), k


def _against_the_restatement(name, case, got, exact):
    differ = 0
    for k in range(len(case["degree_days"])):
        want = rc.restated_case(case, k)
        for n in rc.OUTPUTS:
            g, w = got["maps"][k][n], want[n]
            bad = differing(g, w.astype(g.dtype))
            differ += int(bad.sum())
            if exact or g.dtype.kind != "f":
                assert not bad.any(), (name, k, n, int(bad.sum()), g[bad][:4], w[bad][:4])
            else:           # another C library under the restatement's exp: the last places of a double
                assert np.allclose(g, w, rtol=1e-12, atol=1e-12), (name, k, n)
    print(f"{name}: values differ: {differ}")


def test_host_text_equals_the_restatement_on_random_cases(pin, host):
    from tests import tolerances
    exact, why = tolerances.libm_probe()
    print(why)
    for name, case in _random_cases(pin):
        got = rc.run_host(host.exe, host.dir, name, case)
        assert got["status"] == 0
        _against_the_restatement(name, case, got, exact)


def test_random_cases_are_not_vacuous(pin):
    """from the restatement: roots on ROOTED_SHARE of the cells, in every phase of the growth, with density in the layers"""
    flag = float(pin["flag"])
    no_growth = 0
    for name, case in _random_cases(pin):
        for k in range(2):
            m = rc.restated_case(case, k)
            rooted = (m["length"] > 0) & (m["first"] != int(flag))
            assert np.count_nonzero(rooted) > rc.ROOTED_SHARE * rooted.size, (name, k)
            assert np.count_nonzero(m["length"] == flag) > 0, (name, k)                                                 # no cell
            no_growth += np.count_nonzero(m["length"] == 0)
            assert np.count_nonzero(m["density"][1:][:, rooted] > 0) > np.count_nonzero(rooted), (name, k)              # more than one layer per rooted cell
            assert m["length"].flat[-1] > 0, (name, k)                                                                  # the last lane computes
    assert no_growth > 0                                                                                                # degree days <= 0 on a growing unit


def test_sanitized_host_build_reports_nothing(pin, host):
    """address and undefined-behaviour sanitizers on the pin, on every random case and on the edge cases of the tables (every table a heap
    block of its own): exit 0, nothing on stderr; and the edge cases reach what they are made for"""
    from tests import tolerances
    exact = tolerances.libm_probe()[0]
    rc.run_host(host.san, host.dir, "san-pin", _pin_case(pin))
    rc.run_host(host.san, host.dir, "san-pin-3", _pin_case(pin), layer0=3)
    runs = 2
    for name, case in _random_cases(pin):
        assert rc.run_host(host.san, host.dir, "san-" + name, case)["status"] == 0
        runs += 1
    sf = capi.load_product()
    seen = {}
    for name, case in rc.edge_cases(pin):
        assert rc.accepted(sf, case), name                             # (a case the API refused would be dropped here)
        got = rc.run_host(host.san, host.dir, "san-" + name, case)
        assert got["status"] == 0, name
        _against_the_restatement(name, case, got, exact)
        seen[name] = (case, got)
        runs += 1
    nl = len(pin["layer_depth"])
    case, got = seen["caps"]
    m = got["maps"][0]
    last_pair = (case["crop_index"] == root.MAX_UNITS - 1) & (case["soil_index"] == len(case["soil_list"]) - 1) & (m["key"] >= 0)
    assert last_pair.sum() >= 3 and np.count_nonzero(m["key"] == got["rows"] - 1) > 0            # unit 63, the soil of 16 horizons, the last table row
    assert len(case["soil_list"][-1]["upperDepth"]) == root.MAX_HORIZONS and np.count_nonzero(m["first"][last_pair] == 0) > 0      # firstRootLayer == 0
    full = got["table"][:, got["rows"] - 1]                            # m = lunetteMax = 100 rooted atoms from the surface down
    assert full.sum() > 0.9 and got["row_layers"][got["rows"] - 1][0] == 0
    case, got = seen["clamp"]
    tops = {k: round(u["rootDepthMin"] / 0.01) for k, u in enumerate(case["unit_list"])}
    atoms = {k: int(s["totalDepth"] * 100) + 1 for k, s in enumerate(case["soil_list"])}
    pairs = {(int(c), int(s)) for c, s, d in zip(case["crop_index"].flat, case["soil_index"].flat, case["dem"].flat) if d != np.float32(case["flag"])}
    assert any(tops[c] >= atoms[s] for c, s in pairs) and any(0 < atoms[s] - tops[c] < round(case["soil_list"][s]["totalDepth"] / 0.01) for c, s in pairs)
    case, got = seen["deep"]
    assert np.count_nonzero(got["maps"][0]["last"] == nl - 1) > 0                                # lastRootLayer == nrLayers - 1
    case, got = seen["one-layer"]
    assert got["table"].shape[0] == 1 and not got["table"].any() and np.all(got["maps"][0]["first"][got["maps"][0]["key"] >= 0] == int(pin["flag"]))
    assert seen["1x8"][0]["dem"].shape == (1, 8)
    print(f"root_host_san: {runs} runs, nothing reported")
