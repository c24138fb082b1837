"""Topographic distance on the device (include/sf3d_topodist.h) against the compiled-reference pin tests/golden/topodist.npz and the
restatements of criteria3d_amd/topodist.py: the maps of k_topodist_maps, every interpolation case of k_meteo_idw_td with the maps set,
unset and mixed, the station matrix, the meteo block's slot, the life of the maps, two ranks, and the 1 024-station cap."""
import numpy as np
import pytest

from criteria3d_amd import capi, hour, meteo, topodist
from tests import meteo_cases as mc
from tests import ranks as mr
from tests import topodist_cases as tc
from tests.raster_helpers import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return tc.load_pin()


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


@pytest.mark.parametrize("name", tc.RASTERS)
def test_every_map_case_and_matrix_equals_the_pin(product, pin, name):
    r = pin[name]
    tc.initialize(product, r)
    topodist.compute(product, r["x"], r["y"], r["z"])
    assert topodist.bytes_held(product) == len(r["x"]) * r["dem"].size * 4
    for i in range(len(r["x"])):
        _same(topodist.get_map(product, i), r["maps"][i], f"map {i}")
    flag = r["flag"]
    for mode in pin["modes"]:
        index = tc.hold(product, r, mode)
        _same(topodist.station_matrix(product, r["x"], r["y"], r["z"], index), r["matrices"][pin["modes"].index(mode)], f"matrix {mode}")
        for k, c in enumerate(r["cases"]):
            if c["mode"] != mode:
                continue
            got = tc.interpolate(product, r, c, index)
            _same(got, c["want"], f"case {k} {tc.case_name(c)}")
            _same(meteo.get_map(product, c["var"]), c["want"], f"case {k}: the meteo block's slot")
            if tc.effective_kh(c) == 0:                                   # kh = 0, precipitation, useTD off: the plain interpolation's map
                plain = meteo.interpolate(product, c["var"], c["method"], r["x"], r["y"], c["value"], c["area"], dict(c["settings"], useTopographicDistance=0))
                _same(got, plain, f"case {k} against sf3d_meteo_interpolate")
            assert (got[r["dem"] != flag] != flag).all()
    topodist.clean(product)
    meteo.clean(product)


def test_set_get_and_drop_map(product, pin):
    r = pin["relief"]
    tc.initialize(product, r)
    topodist.compute(product, r["x"], r["y"], r["z"])
    hand = r["hand"]
    case = next(c for c in r["cases"] if c["mode"] == "hand" and c["method"] == meteo.IDW)
    every = np.arange(len(r["x"]), dtype=np.int32)
    before = tc.interpolate(product, r, case, every)
    topodist.set_map(product, hand, r["hand_map"])
    _same(topodist.get_map(product, hand), r["hand_map"], "get_map after set_map")
    _same(topodist.get_map(product, hand + 1), r["maps"][hand + 1], "the neighbouring map is untouched")
    after = tc.interpolate(product, r, case, every)
    _same(after, case["want"], "the hand-made map")
    assert (bits(before) != bits(after)).any()
    # a dropped map: the station is map-less; naming it is refused, -1 in its place gives the walk
    topodist.drop_map(product, hand)
    with pytest.raises(capi.SF3DError):
        tc.interpolate(product, r, case, every)
    with pytest.raises(capi.SF3DError):
        topodist.get_map(product, hand)
    without = every.copy()
    without[hand] = -1
    held = [m for m in r["maps"]]
    want = topodist.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], [None], case["var"], case["method"], r["x"], r["y"], r["z"], case["value"],
                                        case["area"], case["settings"], case["kh"], held, without, float(r["flag"]))
    _same(tc.interpolate(product, r, case, without), want, "map-less after drop_map")
    _same(want, tc.restated(r, dict(case, mode="all")), "the walk equals the computed map on this raster")
    # refused before any launch: an index beyond what is held, kh < 0, a point whose walk would be too long
    beyond = every.copy()
    beyond[0] = len(r["x"])
    with pytest.raises(capi.SF3DError):
        tc.interpolate(product, r, case, beyond)
    with pytest.raises(capi.SF3DError):
        topodist.interpolate(product, case["var"], case["method"], r["x"], r["y"], r["z"], case["value"], without, case["area"], case["settings"], -1)
    far = r["x"].copy()
    far[0] += r["cell_size"] * (topodist.MAX_STEPS + 1)
    with pytest.raises(capi.SF3DError):
        topodist.compute(product, far, r["y"], r["z"])
    with pytest.raises(capi.SF3DError):
        topodist.station_matrix(product, far, r["y"], r["z"], None)
    topodist.compute(product, [], [], [])                                 # no points: no maps
    assert topodist.bytes_held(product) == 0
    meteo.clean(product)


def test_the_result_counts_as_produced_and_the_maps_go_with_the_raster(product, pin):
    r = pin["relief"]
    tc.initialize(product, r)
    index = tc.hold(product, r, "all")
    case = next(c for c in r["cases"] if c["mode"] == "all" and c["var"] == meteo.AIR_TEMPERATURE and c["kh"] == 7 and c["method"] == meteo.SHEPARD)
    hour.bind(product)
    with pytest.raises(capi.SF3DError):                                   # neither temperature map has been produced yet
        hour.relative_humidity(product)
    air = tc.interpolate(product, r, case, index, download=False)
    assert air is None
    dew = topodist.interpolate(product, "dewT", case["method"], r["x"], r["y"], r["z"], case["value"] - np.float32(4), index, case["area"], case["settings"], case["kh"])
    rh = hour.relative_humidity(product)                                  # reads both slots in place: accepted as produced
    _same(rh, hour.restate_relative_humidity(case["want"], dew, float(r["flag"])), "relative humidity from the two slots")
    # after sf3d_meteo_clean the maps are gone: refused, not launched on a freed pointer
    meteo.clean(product)
    assert topodist.bytes_held(product) == 0
    with pytest.raises(capi.SF3DError):
        topodist.get_map(product, 0)
    with pytest.raises(capi.SF3DError):
        tc.interpolate(product, r, case, index)
    # a second sf3d_meteo_initialize drops them too
    tc.initialize(product, r)
    tc.hold(product, r, "all")
    tc.initialize(product, r)
    assert topodist.bytes_held(product) == 0
    with pytest.raises(capi.SF3DError):
        tc.interpolate(product, r, case, index)
    with pytest.raises(capi.SF3DError):
        topodist.station_matrix(product, r["x"], r["y"], r["z"], index)
    _same(tc.interpolate(product, r, case, None), tc.restated(r, dict(case, mode="none")), "map-less on the new raster")
    meteo.clean(product)


@pytest.mark.parametrize("stations", [1, 2, 65])
@pytest.mark.parametrize("shape", mc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_of_small_rasters_against_the_restatement(product, shape, stations):
    """33 cells: less than a wave; one row of 300: a partial second block; 1, 2 and 65 stations in blockIdx.y"""
    r = tc.with_heights(mc.small_raster(dict(flag=np.float32(-9999.0)), shape), 65)
    x, y, z = r["x"][:stations], r["y"][:stations], r["z"][:stations]
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], float(r["flag"]))
    topodist.compute(product, x, y, z)
    positive = 0
    for i in range(stations):
        want = topodist.restate_map(r["dem"], r["xll"], r["yll"], r["cell_size"], x[i], y[i], z[i], float(r["flag"]))
        got = topodist.get_map(product, i)
        _same(got, want, f"{shape} map {i}")
        assert got.flat[0] == r["flag"] and got.flat[-1] != r["flag"]
        positive += int((got > 0).sum())
    assert positive > 0 or stations < 65                                  # one station high above a few cells may see no rise at all; 65 do
    meteo.clean(product)


def test_two_ranks_merge_to_the_single_rank_maps_and_map(product, pin, tmp_path):
    r = pin["relief"]
    which = next(k for k, c in enumerate(r["cases"]) if c["mode"] == "mixed" and c["var"] == meteo.AIR_TEMPERATURE and c["kh"] == 7 and c["method"] == meteo.SHEPARD)
    ranks = mr.run("scripts/multirank_topodist_worker.py", 2, tc.PORT, [which], tmp_path)
    rows, cols = r["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(r["flag"])
    for k, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {k} getter")
    merged = mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map")
    _same(merged, r["cases"][which]["want"], "merged ranks")
    for i in range(len(r["x"])):
        _same(mr.merge([res["maps"][i] for res in ranks], cell_owner, flag, others=flag, what=f"map {i}"), r["maps"][i], f"merged map {i}")


@pytest.mark.parametrize("method", meteo.METHODS)
def test_1024_stations_on_257_x_3_cells_against_the_restatement(product, method):
    """the cap, the LDS staging loop (four passes a thread) and the tail block; every third station map-less"""
    r = tc.with_heights(mc.cap_raster(dict(flag=np.float32(-9999.0))), 1024)
    assert len(r["x"]) == meteo.MAX_STATIONS and r["dem"].size % 256 == 3
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], float(r["flag"]))
    topodist.compute(product, r["x"], r["y"], r["z"])
    maps = [topodist.get_map(product, i) if r["index"][i] >= 0 else None for i in range(len(r["x"]))]
    for i in (0, 511, 1023):
        _same(maps[i] if maps[i] is not None else topodist.get_map(product, i),
              topodist.restate_map(r["dem"], r["xll"], r["yll"], r["cell_size"], r["x"][i], r["y"][i], r["z"][i], float(r["flag"])), f"map {i}")
    got = topodist.interpolate(product, "airT", method, r["x"], r["y"], r["z"], r["value"], r["index"], r["area"], r["settings"], 3)
    want = topodist.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], "airT", method, r["x"], r["y"], r["z"], r["value"], r["area"],
                                        r["settings"], 3, maps, r["index"], float(r["flag"]))
    _same(got, want, f"1024 stations, {method}")
    assert got.flat[0] == r["flag"] and got.flat[-1] != r["flag"] and np.count_nonzero(got != r["flag"]) == r["dem"].size - 2
    plain = meteo.interpolate(product, "airT", method, r["x"], r["y"], r["value"], r["area"], dict(r["settings"], useTopographicDistance=0))
    assert (bits(plain) != bits(got)).any()                         # the topographic distance changes the map
    with pytest.raises(capi.SF3DError):                                   # one point beyond the cap
        topodist.compute(product, np.append(r["x"], 0.0), np.append(r["y"], 0.0), np.append(r["z"], 0.0))
    meteo.clean(product)
