"""Glocal detrending on the device (include/sf3d_glocal.h) against the compiled-reference pin tests/golden/glocal.npz: every case of the
pin in every cell and every area quantity on both rasters, the meteo block's slot, the same bits twice, the slot counted as produced and
read on the device by the hour block (its humidity pass and its ET0 hour), the life of the block, two ranks, and off the pin
(glocal_cases.OFF_PIN: area lists of 65 and 130 stations, five areas, 31 first guesses, cells under five areas; OFF_PIN_EDGES: list
entries without a point this hour, lists of 2 to 1024 stations, one to ten areas, an area with no point, no retrend) the device against
the host build of its own text, a sparse hour between two full ones on one set of areas, and the error an interpolate() that gives
NODATA must bring back."""
import numpy as np
import pytest

from criteria3d_amd import capi, crop, glocal as gl, hour, localdetrend as ld, meteo, radiation as rad
from tests import glocal_cases as gc
from tests import hour_cases as hc
from tests import ranks as mr
from tests import sink_cases as sc
from tests.raster_helpers import bits, build_host_program, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return gc.load_pin()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host build of the two kernels' text (tests/glocal_host.cpp), built once"""
    d = tmp_path_factory.mktemp("glocal_host")
    return build_host_program("glocal", d), d


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


@pytest.mark.parametrize("name", gc.RASTERS)
def test_every_case_equals_the_pin_in_every_cell_and_every_area_quantity(product, pin, name):
    r = pin[name]
    gc.initialize(product, r)
    flag = r["flag"]
    for k, c in enumerate(r["cases"]):
        what = f"{name} {k} {gc.case_name(c)}"
        got = gc.interpolate(product, c)
        same(gc.outcome(product, got), c["want"], what, gc.QUANTITIES)
        _same(meteo.get_map(product, c["var"]), c["want"]["value"], f"{what}: the meteo block's slot")
        assert (got[r["dem"] == flag] == flag).all()
    assert gl.bytes_held(product) > 0
    gl.clean(product)
    assert gl.bytes_held(product) == 0
    with pytest.raises(capi.SF3DError):                                     # the areas went with the block
        gc.interpolate(product, r["cases"][0])
    meteo.clean(product)


def test_two_calls_give_the_same_bits(product, pin):
    r = pin["relief"]
    gc.initialize(product, r)
    c = next(c for c in r["cases"] if c["label"] == "all")
    first = gc.outcome(product, gc.interpolate(product, c))
    other = next(c for c in r["cases"] if c["label"] == "two")
    gc.interpolate(product, other)                                          # another call in between leaves nothing behind
    second = gc.outcome(product, gc.interpolate(product, c))
    same(second, first, "the second call", gc.QUANTITIES)
    meteo.clean(product)


def test_the_map_counts_as_produced_and_the_block_goes_with_the_raster(product, pin):
    r = pin["tiny"]
    gc.initialize(product, r)
    hour.bind(product)
    with pytest.raises(capi.SF3DError):                                     # neither temperature map has been produced yet
        hour.relative_humidity(product)
    with pytest.raises(capi.SF3DError):                                     # no call yet: nothing to get
        gl.get_area_fit(product)
    air_case = next(c for c in r["cases"] if c["label"] == "gaps")
    dew_case = next(c for c in r["cases"] if c["label"] == "one")
    assert gc.interpolate(product, air_case, download=False) is None
    dew = gc.interpolate(product, dew_case)
    _same(meteo.get_map(product, "airT"), air_case["want"]["value"], "the air temperature stayed in its slot")
    rh = hour.relative_humidity(product)                                    # reads both slots in place: accepted as produced
    _same(rh, hour.restate_relative_humidity(air_case["want"]["value"], dew, float(r["flag"])), "relative humidity from the two slots")
    # after sf3d_meteo_clean the getter and the call are refused, not launched on a freed pointer
    meteo.clean(product)
    assert gl.bytes_held(product) == 0
    for refused in (lambda: gl.get_area_fit(product), lambda: gc.interpolate(product, air_case), lambda: gl.set_areas(product, r["areas"])):
        with pytest.raises(capi.SF3DError):
            refused()
    # a second sf3d_meteo_initialize drops the areas too
    gc.initialize(product, r)
    gc.interpolate(product, air_case)
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], gc.maps_of(r), float(r["flag"]))
    with pytest.raises(capi.SF3DError):
        gc.interpolate(product, air_case)
    gl.set_areas(product, r["areas"])
    same(gc.outcome(product, gc.interpolate(product, air_case)), air_case["want"], "on the new raster", gc.QUANTITIES)
    meteo.clean(product)


def test_the_et0_hour_reads_the_glocal_map_on_the_device(product):
    """an hour whose air temperature comes from sf3d_glocal_interpolate and stays on the device: the ET0 hour of include/sf3d_hour.h gives
    the bits of the same hour with every map handed over through the host-pointer entry point"""
    case = hc.world(sc.load_pin(), (3, 11))
    dem, flag, cell = case["dem"], float(case["flag"]), float(case["cell_size"])
    st = case["stations"][0]
    x, y, air, area = st["airT"]
    rng = np.random.default_rng(5)
    height = np.round(rng.uniform(float(dem[dem != np.float32(flag)].min()), float(dem.max()) + 200.0, len(x)), 1).astype(np.float32)
    fit = ld.make_fit(ld.PIECEWISE_TWO, [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1], (float(air.min()), float(air.max())), 0)
    fit["first_guess"] = fit["first_guess"][:3]
    index = np.arange(len(x), dtype=np.int32) + 40
    areas = gc.strip_areas(dem.shape, 2, len(x), (len(x), 8), rng)
    for a in areas:
        a["stations"] = index[a["stations"]]
    proxies, others = [dict(active=1, isHeight=1)], gc.pc.default_others()[:1]

    def blocks():
        meteo.initialize(product, dem, hc.GEO[0], hc.GEO[1], cell, [None], flag)
        gl.set_areas(product, areas)
        rad.initialize(product, dem, hc.GEO[0], hc.GEO[1], cell, case["lat"], case["lon"], case["slope"], case["aspect"], flag=flag)
        crop.initialize(product, dem, case["crop_index"], case["crop_units"], 44.5, flag)
        crop.set_degree_days(product, case["sink_degree_days"][0], 120)
        hour.bind(product)

    def meteo_maps(download):
        out = dict(airT=gl.interpolate(product, "airT", meteo.IDW, index, x, y, air, height[None, :], area, fit, proxies, others, download=download))
        for name in ("prec", "relHum", "windInt", "transmissivity"):
            out[name] = hc._interpolate(product, st, name, download)
        return out

    blocks()
    assert product.lib.sf3d_hour_et0(dem.size, 0.75) == capi.PARAMETER_ERROR      # nothing produced yet
    meteo_maps(False)
    rad.compute_hour(product, hc.HOURS[0], None)
    hour.et0_hour(product, 0.75)
    in_place = crop.get_et0(product)
    blocks()
    met = meteo_maps(True)
    rad.compute_hour(product, hc.HOURS[0], met["transmissivity"])
    met.update(globalRad=rad.get_map(product, "global"), beamRad=rad.get_map(product, "beam"), clearSkyTransmissivity=0.75)
    crop.compute_hour(product, met, 0.75)
    _same(in_place, crop.get_et0(product), "ET0 from the glocal map in its slot")
    valid = dem != np.float32(flag)
    assert (met["airT"][valid] != np.float32(flag)).all() and (in_place[valid] > 0).any()
    for clean in (crop.clean, rad.clean, meteo.clean):
        clean(product)


def test_two_ranks_merge_to_the_single_rank_map(product, pin, tmp_path):
    r = pin["relief"]
    which = next(k for k, c in enumerate(r["cases"]) if c["label"] == "four")
    ranks = mr.run("scripts/multirank_glocal_worker.py", 2, gc.PORT, [which], tmp_path)
    rows, cols = r["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                        # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(r["flag"])
    want = r["cases"][which]["want"]
    for k, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {k} getter")
        other = (cell_owner != k) & (cell_owner >= 0)
        assert (res["map"][other] == flag).all(), f"rank {k}: another rank's cells hold the flag"
        assert (res["kept"] == want["kept"]).all(), f"rank {k}: every rank fits every area"
    _same(mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map"), want["value"], "merged ranks")


@pytest.mark.parametrize("label", [label for label, _ in gc.OFF_PIN] + list(gc.EDGE_LABELS))
def test_off_the_pin_the_device_equals_the_host_build_of_its_text(product, host, label):
    """gc.OFF_PIN: an area list of 65 and one of 130 stations (one and two wave widths crossed) among five areas (the second block has
    one wave idle), 31 first guesses of both three-piece functions (lanes 0 to 30 busy), every cell under five areas; gc.OFF_PIN_EDGES:
    list entries without a point this hour (a ballot with gaps, a chunk whose ballot is 0, a list whose first two chunks are empty),
    lists of 63 to 129 and of 255 to 1024 stations, lists of 2 to 11, one, eight, nine and ten areas, an area with no point, no retrend,
    the dew point - every cell and area quantity bit for bit, NaN as "both NaN".  The host build is held to the restatement, and every
    row of OFF_PIN_EDGES to its property, in tests/test_glocal_host.py"""
    r, c = gc.off_pin(label)
    want = gc.run_host(host[0], r, host[1], [c])[0]
    assert want["status"] == 0
    gc.initialize(product, r)
    got = gc.interpolate(product, c)
    same(gc.outcome(product, got), want, label, gc.QUANTITIES)
    _same(meteo.get_map(product, c["var"]), want["value"], f"{label}: the meteo block's slot")
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got[out] == r["flag"]).all()
    meteo.clean(product)


def test_an_hour_with_fewer_stations_reads_nothing_the_fuller_hour_left(product, host):
    """the areas of `lists-cap` set once, then four hours: every list whole (1024, 1023, 257, 256, 255 fitted), every fifth point gone, of
    the list of 1024 only entries of the last chunk with a point (64 fitted, fifteen chunks whose ballot is 0), every list whole again.
    What an hour leaves in keptPoint, keptValue, detrended and keptBit beyond its own counts is the fuller hour's: each call equals the
    host build of that call alone, and the last the first"""
    r, c = gc.off_pin("lists-cap")
    hours = [c, gc.without_points(c, gc.missing_points(r, c, ("every", 5))), gc.without_points(c, gc.missing_points(r, c, gc.CAP_TAIL)), c]
    want = gc.run_host(host[0], r, host[1], hours)
    assert [w["status"] for w in want] == [0] * 4 and [int(w["fitted"][0]) for w in want] == [1024, 819, 64, 1024]
    gc.initialize(product, r)
    got = [gc.outcome(product, gc.interpolate(product, q)) for q in hours]
    for k in range(4):
        same(got[k], want[k], f"hour {k}", gc.QUANTITIES)
    same(got[3], got[0], "the full hour again", gc.QUANTITIES)
    meteo.clean(product)


def test_an_interpolate_that_gives_nodata_brings_the_error_back(product, host):
    """glocal_cases.failing_area: every station of an area on the centre of its one cell (IDW); failing_single_station: an area of one
    station that covers cells alone (both Shepard methods).  The host build raises its flag; the device returns SF3D_MISSING_DATA_ERROR,
    the variable's slot does not count as produced, the areas' records are there, and the next good call works.  (No input erases a
    whole rebuilt subset: tests/glocal_cases.py says why.)"""
    for which in (meteo.IDW, meteo.SHEPARD, meteo.SHEPARD_MODIFIED):
        r, c = gc.failing_area() if which == meteo.IDW else gc.failing_single_station(which)
        want = gc.run_host(host[0], r, host[1], [c])[0]
        assert want["status"] == 1
        gc.initialize(product, r)
        hour.bind(product)
        # the same stations off the centre; the same stations by IDW, which one station is enough for
        good = dict(c, x=c["x"] + 37.0) if which == meteo.IDW else dict(c, method=meteo.IDW)
        meteo.set_map(product, "dewT", np.where(r["dem"] != r["flag"], np.float32(2.0), r["flag"]).astype(np.float32))
        gc.interpolate(product, good)
        hour.relative_humidity(product)                                     # produced
        with pytest.raises(capi.SF3DError) as failure:
            gc.interpolate(product, c)
        assert capi.ERROR_NAMES[capi.MISSING_DATA_ERROR] in str(failure.value), r["name"]
        same(gl.get_area_fit(product), want, f"{r['name']}: the areas of the failed call", gc.AREA_QUANTITIES)
        with pytest.raises(capi.SF3DError):                                 # the overwritten slot no longer counts as produced
            hour.relative_humidity(product)
        gc.interpolate(product, good)
        hour.relative_humidity(product)
        meteo.clean(product)
