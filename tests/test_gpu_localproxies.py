"""Local detrending with every proxy on the device (include/sf3d_localproxies.h) against the compiled-reference pin
tests/golden/localproxies.npz and the restatement of criteria3d_amd/localproxies.py: every case of the pin in every cell and every
recorded quantity, the cases of the pin of the height alone through the new entry point, the meteo block's slot, the same bits twice, the
life of the per-cell outcome, two ranks, lists longer than a wave, and the cases of localproxies_cases.OFF_PIN (every number of
significant other proxies from 0 to 7 on lists above and below a wave) and of localdetrend_cases.OFF_PIN (the height alone) against the
host builds of the kernels' own text."""
import numpy as np
import pytest

from criteria3d_amd import capi, hour, localdetrend as ld, localproxies as lp, meteo
from tests import localdetrend_cases as lc
from tests import localproxies_cases as pc
from tests import ranks as mr
from tests.raster_helpers import bits, build_host_program, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return pc.load_pin()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host builds of the two kernels' per-cell text (tests/localproxies_host.cpp, tests/localdetrend_host.cpp), built once"""
    d = tmp_path_factory.mktemp("localproxies_host")
    return build_host_program("localproxies", d), build_host_program("localdetrend", d), d


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


@pytest.mark.parametrize("name", pc.RASTERS)
def test_every_case_equals_the_pin_in_every_cell_and_quantity(product, pin, name):
    r = pin[name]
    pc.initialize(product, r)
    flag = r["flag"]
    for k, c in enumerate(r["cases"]):
        what = f"{name} {k} {pc.case_name(c)}"
        got = pc.interpolate(product, c)
        same(pc.outcome(product, got), c["want"], what, pc.QUANTITIES)
        _same(meteo.get_map(product, c["var"]), c["want"]["value"], f"{what}: the meteo block's slot")
        assert (got[r["dem"] == flag] == flag).all()
    assert lp.bytes_held(product) > r["dem"].size * (meteo.MAX_PROXIES * 17 + 4)
    lp.clean(product)
    assert lp.bytes_held(product) == 0
    meteo.clean(product)


@pytest.mark.parametrize("name", lc.RASTERS)
def test_the_pin_of_the_height_alone_through_the_new_entry_point(product, name):
    """the cases of tests/golden/localdetrend.npz with no other proxy active: k_localdetrend_proxies gives the bits k_localdetrend is held to"""
    r = lc.load_pin()[name]
    lc.initialize(product, r)
    for k, c in enumerate(r["cases"]):
        got = lp.interpolate(product, c["var"], c["method"], c["x"], c["y"], c["value"], c["height"][None, :], c["area"], c["fit"], [dict(active=1, isHeight=1)],
                             pc.default_others()[:1], dict(useDetrending=c["useDetrending"]))
        same(dict(value=got, **ld.get_selection(product), **ld.get_fit(product)), c["want"], f"{name} {k} {lc.case_name(c)}", lc.QUANTITIES)
        assert (lp.get_interpolated(product) == c["want"]["count"]).all() and not lp.get_proxy_fit(product)["proxy_significant"].any()
    meteo.clean(product)


def test_two_calls_give_the_same_bits(product, pin):
    r = pin["relief"]
    pc.initialize(product, r)
    c = next(c for c in r["cases"] if c["label"] == "cap")
    first = pc.outcome(product, pc.interpolate(product, c))
    other = next(c for c in r["cases"] if c["label"] == "two")
    pc.interpolate(product, other)                                          # another call in between leaves nothing behind
    second = pc.outcome(product, pc.interpolate(product, c))
    same(second, first, "the second call", pc.QUANTITIES)
    meteo.clean(product)


def test_the_map_counts_as_produced_and_the_outcome_goes_with_the_raster(product, pin):
    r = pin["tiny"]                                                         # its maps are temperatures the humidity formula takes
    pc.initialize(product, r)
    hour.bind(product)
    with pytest.raises(capi.SF3DError):                                     # neither temperature map has been produced yet
        hour.relative_humidity(product)
    with pytest.raises(capi.SF3DError):                                     # no call yet: nothing to get
        lp.get_proxy_fit(product)
    air_case = next(c for c in r["cases"] if c["label"] == "four")
    dew_case = next(c for c in r["cases"] if c["label"] == "one")
    assert pc.interpolate(product, air_case, download=False) is None
    dew = pc.interpolate(product, dew_case)
    _same(meteo.get_map(product, "airT"), air_case["want"]["value"], "the air temperature stayed in its slot")
    rh = hour.relative_humidity(product)                                    # reads both slots in place: accepted as produced
    _same(rh, hour.restate_relative_humidity(air_case["want"]["value"], dew, float(r["flag"])), "relative humidity from the two slots")
    # a call of the height alone overwrites the elevation's outcome: the proxies' getters are refused until the next call of this block
    ld.interpolate(product, "airT", air_case["method"], air_case["x"], air_case["y"], air_case["proxy_values"][0], air_case["value"], air_case["area"], air_case["fit"])
    with pytest.raises(capi.SF3DError):
        lp.get_interpolated(product)
    # an active proxy without a raster is refused
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], [None, None] + pc.maps_of(r)[2:], float(r["flag"]))
    with pytest.raises(capi.SF3DError):
        pc.interpolate(product, next(c for c in r["cases"] if c["label"] == "one"))
    # after sf3d_meteo_clean the getters and the call are refused, not launched on a freed pointer
    pc.initialize(product, r)
    pc.interpolate(product, air_case)
    meteo.clean(product)
    assert lp.bytes_held(product) == 0
    for refused in (lambda: lp.get_proxy_fit(product), lambda: lp.get_interpolated(product), lambda: ld.get_fit(product), lambda: pc.interpolate(product, air_case)):
        with pytest.raises(capi.SF3DError):
            refused()
    # a second sf3d_meteo_initialize drops the outcome too
    pc.initialize(product, r)
    pc.interpolate(product, air_case)
    pc.initialize(product, r)
    with pytest.raises(capi.SF3DError):
        lp.get_interpolated(product)
    same(pc.outcome(product, pc.interpolate(product, air_case)), air_case["want"], "on the new raster", pc.QUANTITIES)
    meteo.clean(product)


def test_two_ranks_merge_to_the_single_rank_map(product, pin, tmp_path):
    r = pin["relief"]
    which = next(k for k, c in enumerate(r["cases"]) if c["label"] == "four")
    ranks = mr.run("scripts/multirank_localproxies_worker.py", 2, pc.PORT, [which], tmp_path)
    rows, cols = r["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                        # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(r["flag"])
    want = r["cases"][which]["want"]
    for k, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {k} getter")
        other = (cell_owner != k) & (cell_owner >= 0)
        assert (res["map"][other] == flag).all() and (res["interpolated"][other] == 0).all() and (res["slope"][other] == ld.NODATA).all(), \
            f"rank {k}: another rank's cells hold the flag"
    _same(mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map"), want["value"], "merged ranks")
    merged = mr.merge([res["interpolated"].astype(np.float32) for res in ranks], cell_owner, np.float32(0), others=np.float32(0), what="interpolated")
    assert (merged == want["interpolated"]).all()


@pytest.mark.parametrize("others", [2, lp.MAX_OTHERS], ids=lambda v: f"others{v}")
@pytest.mark.parametrize("stations,min_points_local", [(70, 60), (150, 60)], ids=lambda v: str(v))
def test_lists_longer_than_a_wave_against_the_restatement(product, stations, min_points_local, others):
    """70 stations, all selected: lists of 70, the prunings' compaction over two ballots; 150: rings that select more than 64 stations.  Two
    other proxies: five matrix entries and two gradients, a lane each; the cap: 119 entries, two a lane.  33 cells: a last block of one wave"""
    r, c = pc.synthetic(stations, min_points_local, meteo.SHEPARD_MODIFIED, others)
    pc.initialize(product, r)
    got = pc.outcome(product, pc.interpolate(product, c))
    want = pc.restated(r, c)
    same(got, want, f"{stations} stations, {others} other proxies", pc.QUANTITIES)
    inside = r["dem"] != r["flag"]
    assert want["count"][inside].min() > 64 and want["proxy_significant"][inside].sum() >= others * inside.sum() // 2
    assert (want["interpolated"][inside] < want["count"][inside]).all() and want["interpolated"][inside].min() > 32
    meteo.clean(product)


@pytest.mark.parametrize("label", [label for label, _ in pc.OFF_PIN])
def test_off_the_pin_the_device_equals_the_host_build_of_its_text(product, host, label):
    """pc.OFF_PIN: 1 to 7 significant other proxies (5, 14, 27, 44, 65, 90, 119 entries of matrix and gradient) on lists within a wave and
    on lists of 70 whose interpolated list ends at 63 or 66, the three-piece functions and an inactive height under them, and thresholds
    and spoilt slots that leave gaps in the significant set and 2 to 5 significant proxies within one raster on lists of 122 to 131 -
    every cell and quantity bit for bit, NaN as "both NaN".  The host build is held to the restatement in tests/test_localproxies_host.py,
    except the cases of pc.HOST_ONLY"""
    r, c = pc.off_pin(label)
    want = pc.run_host(host[0], r, host[2], [c])[0]
    pc.initialize(product, r)
    got = pc.interpolate(product, c)
    same(pc.outcome(product, got), want, label, pc.QUANTITIES)
    _same(meteo.get_map(product, c["var"]), want["value"], f"{label}: the meteo block's slot")
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got[out] == r["flag"]).all() and (ld.get_selection(product)["count"][out] == 0).all() and (lp.get_interpolated(product)[out] == 0).all()
    meteo.clean(product)


@pytest.mark.parametrize("label", [label for label, _ in lc.OFF_PIN])
def test_the_height_alone_off_the_pin_through_the_new_entry_point(product, host, label):
    """lc.OFF_PIN with no other proxy active: k_localdetrend_proxies gives the bits k_localdetrend is held to, those of the host build of
    k_localdetrend's text"""
    r, c = lc.off_pin(label)
    want = lc.run_host(host[1], r, host[2], [c])[0]
    lc.initialize(product, r)
    got = lp.interpolate(product, c["var"], c["method"], c["x"], c["y"], c["value"], c["height"][None, :], c["area"], c["fit"], [dict(active=1, isHeight=1)],
                         pc.default_others()[:1], dict(useDetrending=c["useDetrending"]))
    same(dict(value=got, **ld.get_selection(product), **ld.get_fit(product)), want, label, lc.QUANTITIES)
    _same(meteo.get_map(product, c["var"]), want["value"], f"{label}: the meteo block's slot")
    assert (lp.get_interpolated(product) == want["count"]).all() and not lp.get_proxy_fit(product)["proxy_significant"].any()
    meteo.clean(product)
