"""Multiple detrending without areas on the device (include/sf3d_multidetrend.h) against the compiled-reference pin
tests/golden/multidetrend.npz: every case of the pin through sf3d_multidetrend_interpolate, _get_fit and _points in every cell, every fit
quantity and every point on both rasters (`relief` has 259 cells: a last block of three threads), the meteo block's slot, the same bits
twice, the slot counted as produced and read on the device by the hour block (its humidity pass and its ET0 hour), the life of the block,
two ranks, the sibling blocks' pins in the same process behind a call of this one, and off the pin (multidetrend_cases.OFF_PIN: lists of
4 to 1 024 stations, stations without a height, a first chunk the prunings erase, 31 first guesses, a raster of exactly 256 cells, kept
lists of 255, 256 and 257 stations around the 256 a block stages in one pass) the device against the host build of its own text, lists
of 1, 255, 256 and 257 points, and two hours on one block."""
import numpy as np
import pytest

from criteria3d_amd import capi, crop, glocal as gl, hour, localdetrend as ld, meteo, multidetrend as md, radiation as rad
from tests import glocal_cases as gc
from tests import hour_cases as hc
from tests import localproxies_cases as pc
from tests import multidetrend_cases as mc
from tests import ranks as mr
from tests import sink_cases as sc
from tests.raster_helpers import bits, build_host_program, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return mc.load_pin()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host build of the three kernels' text (tests/multidetrend_host.cpp), built once"""
    d = tmp_path_factory.mktemp("multidetrend_host")
    return build_host_program("multidetrend", d), d


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


@pytest.mark.parametrize("name", mc.RASTERS)
def test_every_case_equals_the_pin_in_every_cell_fit_quantity_and_point(product, pin, name):
    r = pin[name]
    mc.initialize(product, r)
    flag = r["flag"]
    assert r["dem"].size == (259 if name == "relief" else 45)
    for k, c in enumerate(r["cases"]):
        what = f"{name} {k} {mc.case_name(c)}"
        got = mc.interpolate(product, c)
        same(mc.outcome(product, got, c), c["want"], what, mc.QUANTITIES)
        _same(meteo.get_map(product, c["var"]), c["want"]["value"], f"{what}: the meteo block's slot")
        assert (got[r["dem"] == flag] == flag).all()
        m = len(c["x"])
        q = c["points"]
        _same(md.residuals(product, q["x"][:m], q["y"][:m], q["z"][:m], c["value"], q["values"][:, :m]), md.residual_of(c["value"], c["want"]["points"][:m]),
              f"{what}: computeResiduals")
    assert md.bytes_held(product) > 0
    md.clean(product)
    assert md.bytes_held(product) == 0
    with pytest.raises(capi.SF3DError):                                     # the fit went with the block
        mc.points(product, r["cases"][0])
    with pytest.raises(capi.SF3DError):
        md.get_fit(product)
    same(mc.outcome(product, mc.interpolate(product, r["cases"][0]), r["cases"][0]), r["cases"][0]["want"], "after sf3d_multidetrend_clean", mc.QUANTITIES)
    meteo.clean(product)


def test_two_calls_give_the_same_bits_and_the_points_keep_their_fit(product, pin):
    r = pin["relief"]
    mc.initialize(product, r)
    c = next(c for c in r["cases"] if c["label"] == "all")
    first = mc.outcome(product, mc.interpolate(product, c), c)
    other = next(c for c in r["cases"] if c["label"] == "two")
    mc.interpolate(product, other)                                          # another call in between leaves nothing behind
    second = mc.outcome(product, mc.interpolate(product, c), c)
    same(second, first, "the second call", mc.QUANTITIES)
    # an interpolation of another variable through the meteo block writes its stations over the call's table: the points are evaluated
    # with what the fit kept, not with the table
    st = dict(x=other["x"][:9] + 11.0, y=other["y"][:9] - 7.0, v=np.linspace(40.0, 90.0, 9).astype(np.float32))
    meteo.interpolate(product, "relHum", meteo.IDW, st["x"], st["y"], st["v"], other["area"])
    _same(mc.points(product, c), first["points"], "the points behind another variable's interpolation")
    meteo.clean(product)


def test_the_map_counts_as_produced_and_the_block_goes_with_the_raster(product, pin):
    r = pin["tiny"]
    mc.initialize(product, r)
    hour.bind(product)
    with pytest.raises(capi.SF3DError):                                     # neither temperature map has been produced yet
        hour.relative_humidity(product)
    with pytest.raises(capi.SF3DError):                                     # no call yet: nothing to get, no fit to evaluate
        md.get_fit(product)
    air_case = next(c for c in r["cases"] if c["label"] == "gaps")
    dew_case = next(c for c in r["cases"] if c["label"] == "one")
    with pytest.raises(capi.SF3DError):
        mc.points(product, air_case)
    assert mc.interpolate(product, air_case, download=False) is None
    dew = mc.interpolate(product, dew_case)
    _same(meteo.get_map(product, "airT"), air_case["want"]["value"], "the air temperature stayed in its slot")
    rh = hour.relative_humidity(product)                                    # reads both slots in place: accepted as produced
    _same(rh, hour.restate_relative_humidity(air_case["want"]["value"], dew, float(r["flag"])), "relative humidity from the two slots")
    # after sf3d_meteo_clean the getter and both calls are refused, not launched on a freed pointer
    meteo.clean(product)
    assert md.bytes_held(product) == 0
    for refused in (lambda: md.get_fit(product), lambda: mc.interpolate(product, air_case), lambda: mc.points(product, air_case)):
        with pytest.raises(capi.SF3DError):
            refused()
    # a second sf3d_meteo_initialize drops the fit too; the next call works
    mc.initialize(product, r)
    mc.interpolate(product, air_case)
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], mc.maps_of(r), float(r["flag"]))
    for refused in (lambda: md.get_fit(product), lambda: mc.points(product, air_case)):
        with pytest.raises(capi.SF3DError):
            refused()
    same(mc.outcome(product, mc.interpolate(product, air_case), air_case), air_case["want"], "on the new raster", mc.QUANTITIES)
    meteo.clean(product)


def test_the_et0_hour_reads_the_map_on_the_device(product):
    """an hour whose air temperature comes from sf3d_multidetrend_interpolate and stays on the device: the ET0 hour of
    include/sf3d_hour.h gives the bits of the same hour with every map handed over through the host-pointer entry point"""
    case = hc.world(sc.load_pin(), (3, 11))
    dem, flag, cell = case["dem"], float(case["flag"]), float(case["cell_size"])
    st = case["stations"][0]
    x, y, air, area = st["airT"]
    rng = np.random.default_rng(5)
    height = np.round(rng.uniform(float(dem[dem != np.float32(flag)].min()), float(dem.max()) + 200.0, len(x)), 1).astype(np.float32)
    fit = ld.make_fit(ld.PIECEWISE_TWO, [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1], (float(air.min()), float(air.max())), 0)
    fit["first_guess"] = fit["first_guess"][:3]
    proxies, others = [dict(active=1, isHeight=1)], pc.default_others()[:1]

    def blocks():
        meteo.initialize(product, dem, hc.GEO[0], hc.GEO[1], cell, [None], flag)
        rad.initialize(product, dem, hc.GEO[0], hc.GEO[1], cell, case["lat"], case["lon"], case["slope"], case["aspect"], flag=flag)
        crop.initialize(product, dem, case["crop_index"], case["crop_units"], 44.5, flag)
        crop.set_degree_days(product, case["sink_degree_days"][0], 120)
        hour.bind(product)

    def meteo_maps(download):
        out = dict(airT=md.interpolate(product, "airT", meteo.IDW, x, y, air, height[None, :], area, fit, proxies, others, download=download))
        for name in ("prec", "relHum", "windInt", "transmissivity"):
            out[name] = hc._interpolate(product, st, name, download)
        return out

    blocks()
    assert product.lib.sf3d_hour_et0(dem.size, 0.75) == capi.PARAMETER_ERROR      # nothing produced yet
    meteo_maps(False)
    assert md.get_fit(product)["significant"]
    rad.compute_hour(product, hc.HOURS[0], None)
    hour.et0_hour(product, 0.75)
    in_place = crop.get_et0(product)
    blocks()
    met = meteo_maps(True)
    rad.compute_hour(product, hc.HOURS[0], met["transmissivity"])
    met.update(globalRad=rad.get_map(product, "global"), beamRad=rad.get_map(product, "beam"), clearSkyTransmissivity=0.75)
    crop.compute_hour(product, met, 0.75)
    _same(in_place, crop.get_et0(product), "ET0 from the map in its slot")
    valid = dem != np.float32(flag)
    assert (met["airT"][valid] != np.float32(flag)).all() and (in_place[valid] > 0).any()
    for clean in (crop.clean, rad.clean, meteo.clean):
        clean(product)


def test_two_ranks_merge_to_the_single_rank_map(product, pin, tmp_path):
    r = pin["relief"]
    which = next(k for k, c in enumerate(r["cases"]) if c["label"] == "four")
    ranks = mr.run("scripts/multirank_multidetrend_worker.py", 2, mc.PORT, [which], tmp_path)
    rows, cols = r["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                        # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(r["flag"])
    want = r["cases"][which]["want"]
    for k, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {k} getter")
        other = (cell_owner != k) & (cell_owner >= 0)
        assert (res["map"][other] == flag).all(), f"rank {k}: another rank's cells hold the flag"
        assert int(res["kept"]) == want["kept"], f"rank {k}: every rank runs the one fit"
        _same(res["points"], want["points"], f"rank {k}: every rank evaluates every point")
    _same(mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map"), want["value"], "merged ranks")


def test_the_sibling_blocks_give_their_pins_bits_behind_a_call_of_this_one(product, pin):
    """sf3d_glocal_interpolate and sf3d_localproxies_interpolate in the same process, after and between calls of this block: they share
    the station table and the functions this block calls"""
    gpin, ppin = gc.load_pin(), pc.load_pin()
    r = pin["tiny"]
    mc.initialize(product, r)
    c = next(c for c in r["cases"] if c["label"] == "secondpass")
    first = mc.outcome(product, mc.interpolate(product, c), c)
    same(first, c["want"], "this block first", mc.QUANTITIES)
    meteo.clean(product)
    g = gpin["tiny"]
    gc.initialize(product, g)
    for k in (0, 4):
        same(gc.outcome(product, gc.interpolate(product, g["cases"][k])), g["cases"][k]["want"], f"glocal {k}", gc.QUANTITIES)
    meteo.clean(product)
    p = ppin["tiny"]
    pc.initialize(product, p)
    lp_case = p["cases"][3]
    same(pc.outcome(product, pc.interpolate(product, lp_case)), lp_case["want"], "localproxies", pc.QUANTITIES)
    # on one raster, this block in between: its stations, fit table and proxy rows take the place of the sibling's and go again
    mc.interpolate(product, c)
    mc.points(product, c)
    same(pc.outcome(product, pc.interpolate(product, lp_case)), lp_case["want"], "localproxies again", pc.QUANTITIES)
    meteo.clean(product)


@pytest.mark.parametrize("label", mc.OFF_PIN_LABELS)
def test_off_the_pin_the_device_equals_the_host_build_of_its_text(product, host, label):
    """every cell, fit quantity and point bit for bit, NaN as "both NaN".  The host build is held to the restatement, and every row to
    its property, in tests/test_multidetrend_host.py"""
    r, c = mc.off_pin(label)
    want = mc.run_host(host[0], r, host[1], [c])[0]
    assert want["status"] == 0 and want["points_status"] == 0
    mc.must_of(label)(r, c, want)
    mc.initialize(product, r)
    got = mc.interpolate(product, c)
    same(mc.outcome(product, got, c), want, label, mc.QUANTITIES)
    _same(meteo.get_map(product, c["var"]), want["value"], f"{label}: the meteo block's slot")
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got[out] == r["flag"]).all()
    meteo.clean(product)


@pytest.mark.parametrize("n_points", (1, 255, 256, 257))
def test_lists_of_points_at_the_block_s_edges(product, host, n_points):
    r, c = mc.off_pin("list65")
    q = mc.cut_points(c, n_points)
    want = mc.run_host(host[0], r, host[1], [q])[0]
    assert want["points_status"] == 0 and len(want["points"]) == n_points
    mc.initialize(product, r)
    mc.interpolate(product, q, download=False)
    _same(mc.points(product, q), want["points"], f"{n_points} points")
    assert len(md.points(product, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((mc.SLOTS, 0), np.float32))) == 0      # no point: no launch, no refusal
    meteo.clean(product)


def test_an_hour_with_fewer_stations_reads_nothing_the_fuller_hour_left(product, host):
    """129 stations, then every fifth of them, then all again on one block: each call equals the host build of that call alone"""
    r, hours = mc.two_hours()
    hours = hours + [hours[0]]
    alone = [mc.run_host(host[0], r, host[1], [q], name=f"hour{k}")[0] for k, q in enumerate(hours)]
    assert [w["fitted"] for w in alone] == [129, 26, 129]
    mc.initialize(product, r)
    got = [mc.outcome(product, mc.interpolate(product, q), q) for q in hours]
    for k in range(3):
        same(got[k], alone[k], f"hour {k}", mc.QUANTITIES)
    same(got[2], got[0], "the full hour again", mc.QUANTITIES)
    meteo.clean(product)
