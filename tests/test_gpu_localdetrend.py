"""Air and dew-point temperature with local detrending on the device (include/sf3d_localdetrend.h) against the compiled-reference pin
tests/golden/localdetrend.npz and the restatement of criteria3d_amd/localdetrend.py: every case of the pin in every cell and every
recorded quantity, the meteo block's slot, the same bits twice, the life of the per-cell outcome, two ranks, selected lists longer
than a wave up to the 1 024-station cap, and the cases of localdetrend_cases.OFF_PIN - list lengths at the wave's edges, full first-guess
lists, every function and method above 64 stations, small block shapes - against the host build of the kernel's own text."""
import numpy as np
import pytest

from criteria3d_amd import capi, hour, localdetrend as ld, meteo
from tests import localdetrend_cases as lc
from tests import ranks as mr
from tests.raster_helpers import bits, build_host_program, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return lc.load_pin()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host build of the kernel's per-cell text (tests/localdetrend_host.cpp), built once in a temporary directory"""
    d = tmp_path_factory.mktemp("localdetrend_host")
    return build_host_program("localdetrend", d), d


def _same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


@pytest.mark.parametrize("name", lc.RASTERS)
def test_every_case_equals_the_pin_in_every_cell_and_quantity(product, pin, name):
    r = pin[name]
    lc.initialize(product, r)
    flag = r["flag"]
    for k, c in enumerate(r["cases"]):
        what = f"{name} {k} {lc.case_name(c)}"
        got = lc.interpolate(product, c)
        same(lc.outcome(product, got), c["want"], what, lc.QUANTITIES)
        _same(meteo.get_map(product, c["var"]), c["want"]["value"], f"{what}: the meteo block's slot")
        assert (got[r["dem"] != flag] != flag).all() and (got[r["dem"] == flag] == flag).all()
    assert ld.bytes_held(product) > r["dem"].size * (ld.MAX_PARAMETERS * 8 + 13)
    ld.clean(product)
    assert ld.bytes_held(product) == 0
    meteo.clean(product)


def test_two_calls_give_the_same_bits(product, pin):
    r = pin["relief"]
    lc.initialize(product, r)
    c = next(c for c in r["cases"] if c["label"] == "rings")
    first = lc.outcome(product, lc.interpolate(product, c))
    other = next(c for c in r["cases"] if c["label"] == "vee")
    lc.interpolate(product, other)                                          # another call in between leaves nothing behind
    second = lc.outcome(product, lc.interpolate(product, c))
    same(second, first, "the second call", lc.QUANTITIES)
    meteo.clean(product)


def test_the_map_counts_as_produced_and_the_outcome_goes_with_the_raster(product, pin):
    r = pin["relief"]
    lc.initialize(product, r)
    hour.bind(product)
    with pytest.raises(capi.SF3DError):                                     # neither temperature map has been produced yet
        hour.relative_humidity(product)
    with pytest.raises(capi.SF3DError):                                     # no call yet: nothing to get
        ld.get_fit(product)
    air_case = next(c for c in r["cases"] if c["label"] == "plain")
    dew_case = next(c for c in r["cases"] if c["label"] == "rings")
    assert lc.interpolate(product, air_case, download=False) is None
    dew = lc.interpolate(product, dew_case)
    _same(meteo.get_map(product, "airT"), air_case["want"]["value"], "the air temperature stayed in its slot")
    rh = hour.relative_humidity(product)                                    # reads both slots in place: accepted as produced
    _same(rh, hour.restate_relative_humidity(air_case["want"]["value"], dew, float(r["flag"])), "relative humidity from the two slots")
    # the plain interpolation still refuses the two options on this raster
    with pytest.raises(capi.SF3DError):
        meteo.interpolate(product, "airT", meteo.IDW, air_case["x"], air_case["y"], air_case["value"], air_case["area"], lc.settings_of(air_case))
    # after sf3d_meteo_clean the getters and the call are refused, not launched on a freed pointer
    meteo.clean(product)
    assert ld.bytes_held(product) == 0
    for refused in (lambda: ld.get_fit(product), lambda: ld.get_selection(product), lambda: lc.interpolate(product, air_case)):
        with pytest.raises(capi.SF3DError):
            refused()
    # a second sf3d_meteo_initialize drops the outcome too
    lc.initialize(product, r)
    lc.interpolate(product, air_case)
    lc.initialize(product, r)
    with pytest.raises(capi.SF3DError):
        ld.get_selection(product)
    same(lc.outcome(product, lc.interpolate(product, air_case)), air_case["want"], "on the new raster", lc.QUANTITIES)
    meteo.clean(product)


def test_two_ranks_merge_to_the_single_rank_map(product, pin, tmp_path):
    r = pin["relief"]
    which = next(k for k, c in enumerate(r["cases"]) if c["label"] == "rings")
    ranks = mr.run("scripts/multirank_localdetrend_worker.py", 2, lc.PORT, [which], tmp_path)
    rows, cols = r["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                        # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(r["flag"])
    want = r["cases"][which]["want"]
    for k, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {k} getter")
        other = (cell_owner != k) & (cell_owner >= 0)
        assert (res["map"][other] == flag).all() and (res["count"][other] == 0).all(), f"rank {k}: another rank's cells hold the flag"
    _same(mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map"), want["value"], "merged ranks")
    _same(mr.merge([res["radius"] for res in ranks], cell_owner, np.float32(ld.NODATA), others=np.float32(ld.NODATA), what="radius"), want["radius"], "merged radius")


@pytest.mark.parametrize("stations,min_points_local,method", [(70, 60, meteo.SHEPARD_MODIFIED), (150, 60, meteo.SHEPARD_MODIFIED), (150, 60, meteo.SHEPARD),
                                                              (1024, 20, meteo.IDW)], ids=lambda v: str(v))
def test_lists_longer_than_a_wave_against_the_restatement(product, stations, min_points_local, method):
    """70 stations, all selected: a list of 70 from one pass of two ballots; 150: rings that select more than 64 stations, a third, partial
    ballot a ring, the direction terms with two rows a lane; 1 024: the cap, sixteen ballots a ring.  33 cells: a last block of one wave"""
    r, c = lc.synthetic(stations, min_points_local, method)
    lc.initialize(product, r)
    got = lc.outcome(product, lc.interpolate(product, c))
    want = lc.restated(r, c)
    same(got, want, f"{stations} stations, {meteo.METHODS[method]}", lc.QUANTITIES)
    inside = r["dem"] != r["flag"]
    assert want["count"][inside].min() >= min(stations, ld.min_points(min_points_local)) > 20 and want["significant"][inside].all()
    if stations != 1024:
        assert want["count"][inside].min() > 64
    if method == meteo.SHEPARD:
        assert not want["ties"].any()
    if stations == 1024:
        with pytest.raises(capi.SF3DError):                                 # one station beyond the cap
            ld.interpolate(product, "airT", method, np.append(c["x"], 0.0), np.append(c["y"], 0.0), np.append(c["height"], 0.0), np.append(c["value"], 0.0),
                           c["area"], c["fit"])
    meteo.clean(product)


@pytest.mark.parametrize("label", [label for label, _ in lc.OFF_PIN])
def test_off_the_pin_the_device_equals_the_host_build_of_its_text(product, host, label):
    """lc.OFF_PIN: lists of 1, 4, 5, 63, 64, 65, 128 and 129 entries with every method, ring-selected lists of 122 to 131 with 16, 30 and 31
    first guesses, the dew point without retrend, equal values, a height that is not significant, the iteration cap, and rasters of one
    block, a block and a wave (the flag in the first cell) and two blocks - every cell and quantity bit for bit, R2 NaN as "both NaN".
    The host build is held to the restatement in tests/test_localdetrend_host.py, except the cases of lc.HOST_ONLY"""
    r, c = lc.off_pin(label)
    want = lc.run_host(host[0], r, host[1], [c])[0]
    lc.initialize(product, r)
    got = lc.interpolate(product, c)
    same(lc.outcome(product, got), want, label, lc.QUANTITIES)
    _same(meteo.get_map(product, c["var"]), want["value"], f"{label}: the meteo block's slot")
    out = r["dem"] == r["flag"]
    assert out.sum() == 1 and (got[out] == r["flag"]).all() and (ld.get_selection(product)["count"][out] == 0).all() and (want["count"][~out] > 0).all()
    meteo.clean(product)
