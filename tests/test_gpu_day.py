"""A day of device-to-device hours (hour.run_day) against the chained restatements (tests/day_cases.py RestatedDay): two dates, five hours
across midnight - 22:00 and 23:00 of 2021-03-20 without a daily update, then 00:00, 06:00 and 12:00 of 2021-03-21 behind the crop maps'
daily update and the day's ponds - on a raster of less than a wave and one of a block plus three lanes, with snow, the humidity from the
dew point and IDW, and without snow, the humidity from stations and Shepard.  The restated day carries its own radiation maps, snow
state, crop maps and pond map from hour to hour; the only thing it takes from the device is the solver's node state an hour starts from
(the water contents) and the node ponds before the day's pond update.  Every map of every hour, the station transmissivities, the crop
maps and the ponds after each date's start: bit for bit.  The three totals: within the bound of two orders of summation.  The balance of
every hour: the identities of test_gpu_hour.py::test_run_hour_closes_its_balance_and_steps_as_the_per_block_calls.

The observation point is run_day's `stations_of` callback: it runs after the date's start and between two hours, before the next hour's
first launch.  The pond map of a date's start stays on the device (run_day does not download it): the callback reads the node ponds that
start has set, then repeats hour.update_ponds with a download - the same kernel on the same LAI map.  run_hour keeps the station
transmissivities to itself as well: they are computed once more after the hour, by the call run_hour makes on the stations it was given."""
import numpy as np
import pytest

from criteria3d_amd import crop, hour, transmissivity as tr
from tests import day_cases as dc
from tests import hour_cases as hc
from tests import sink_cases as sc
from tests.raster_helpers import bits as _bits, need_glibc_set as _need_glibc_set

pytestmark = pytest.mark.gpu
IDS = ("snow-dew-idw", "rain-stations-shepard")


@pytest.fixture(scope="module")
def pin():
    return sc.load_pin()


def _node_ponds(product, m):
    return np.array([product.lib.sf3d_get_node_pond(i) for i in range(m.ns)])


def _set_up(product, case, processes):
    m = hc.build_model(product, case)
    hc.initialize_blocks(product, case, processes["computeSnow"])
    mp, lm, ic = hc.pond_tables(case)
    hour.set_ponds(product, case["slope"], case["crop_index"], mp, lm, ic, True, float(case["flag"]))
    return m


def _clean(product):
    hc.clean_blocks(product)
    product.lib.sf3d_clean()


def _run(product, case, processes):
    """the calendar through hour.run_day with the restated day walking beside it -> per date (got, want) of the start, per hour (got, want)
    of the maps, and per hour the balance with the solver's getters read right after it"""
    m = _set_up(product, case, processes)
    lib = product.lib
    p = dict(processes, surfaceArea=float(case["cell_size"]) ** 2 * int(np.count_nonzero(case["columns"][0] >= 0)))
    day = dc.RestatedDay(case, processes)
    starts, hours, pending = [], [], []

    def observe_hour():
        """what the hour that has just ended left: its maps, the station transmissivities it computed, the solver's getters"""
        want = pending.pop()
        got = dc.device_maps(product, case, m, processes)
        t = want["stations"]["transmissivity"]
        got["station_transmissivity"] = tr.points(product, want["when"], t["width"], t["time_step_second"], t["points"], t["measured"])[0]
        got["totals"] = hour.totals(product)
        getters = dict(current=lib.sf3d_get_total_water_content(), runoff=lib.sf3d_get_total_boundary_water_flow(hour.BND_RUNOFF),
                       drainage=lib.sf3d_get_total_boundary_water_flow(hour.BND_FREE_DRAINAGE) + lib.sf3d_get_total_boundary_water_flow(hour.BND_FREE_LATERAL_DRAINAGE))
        hours.append((got, want, getters))

    for d, (date, hs) in enumerate(case["calendar"]):
        before = _node_ponds(product, m)
        want_start = day.start_date(date, dc.PREVIOUS_HOUR[d])
        want_start["pond_after"] = day.node_ponds(before)

        def stations_of(h, date=date, hs=hs, want_start=want_start):
            if h == hs[0]:
                got = {n: crop.get_state(product, n) for n in crop.STATE}
                got["pond_after"] = _node_ponds(product, m)                   # what run_day's own pond update has set
                got["pond_map"] = hour.update_ponds(product)                  # the same kernel again, downloaded
                got["pond_again"] = _node_ponds(product, m)
                starts.append((got, want_start))
            else:
                observe_hour()
            when = tuple(date) + (int(h), 0, 0)
            st = case["day_stations"][(tuple(date), h)]
            want = day.hour(when, st, product.water_content(0, m.n))          # the node state this hour starts from
            want.update(when=when, stations=st)
            pending.append(want)
            return st
        balances = hour.run_day(product, date, hs, stations_of, p, previous_hour=dc.PREVIOUS_HOUR[d], date_doy=dc.doy_of(date))
        observe_hour()
        for k, res in enumerate(balances):
            hours[len(hours) - len(balances) + k][2]["balance"] = res
    _clean(product)
    return p, starts, hours


def _same(got, want, names, what):
    for name in names:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        bad = _bits(a) != _bits(b)
        print(f"{what} {name}: {int(bad.sum())} of {bad.size} values differ")
        assert not bad.any(), (what, name, int(bad.sum()), a[bad][:4], b[bad][:4])


@pytest.mark.parametrize("processes", dc.PROCESS_SETS, ids=IDS)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_hour_of_two_dates_equals_the_restated_day(product, pin, shape, processes):
    _need_glibc_set(product)
    case = dc.day_world(pin, shape)
    n = case["dem"].size
    flag = np.float32(case["flag"])
    valid = case["dem"] != flag
    assert not valid.flat[0] and valid.flat[-1]                               # the first cell is a flag cell, the last lane computes
    p, starts, hours = _run(product, case, processes)
    assert len(starts) == 2 and [w["when"][3] for _, w, _ in hours] == [22, 23, 0, 6, 12]
    # each date's start: the four crop maps, the pond map, the ponds of the surface nodes
    for d, (got, want) in enumerate(starts):
        _same(got, want, crop.STATE + ("pond_map", "pond_after"), f"start of date {d}")
        assert np.array_equal(_bits(got["pond_again"]), _bits(got["pond_after"]))
    moved = _bits(starts[1][0]["degreeDays"]) != _bits(hours[1][0]["degreeDays"])
    assert np.count_nonzero(moved) > dc.crop_cells(case).sum() / 4            # the second date's daily update did change the device's maps
    names = dc.compared_names(processes)
    assert len(names) == 5 + 5 + 5 + 5 + 3 + (1 if processes["useDewPoint"] else 0) + (13 if processes["computeSnow"] else 0)
    for got, want, getters in hours:
        h = want["when"][3]
        what = f"{shape} {processes['method']} {h:02d}:00"
        _same(got, want, names + ("station_transmissivity",), what)
        # flag cells hold the flag, the first cell is one, the last lane computes
        for name in ("airT", "prec", "relHum", "windInt", "transmissivity", "rad_global", "rad_beam", "et0", "evaporation", "transpiration", "root_length") + \
                (("swe", "liquid") if processes["computeSnow"] else ()):
            a = got[name]
            assert np.all(a[~valid] == flag) and a.flat[0] == flag and a.flat[-1] != flag, (what, name)
        assert not got["sinks"][np.arange(len(case["layer_depth"])) * n].any(), what          # the flag cell's column holds no sink
        # the three totals against the restated sequential sum
        res = getters["balance"]
        device = np.array([res["totalPrecipitation"], res["totalEvaporation"], res["totalTranspiration"]])
        seq, absolute = want["totals"], want["totals_absolute"]
        bound = n * hc.TWO_POW_MINUS_53 * absolute
        print(f"{what}: totals {device}, sequential {seq}, difference {device - seq}, bound {bound}; steps {res['steps']}")
        assert np.array_equal(_bits(device), _bits(got["totals"]))
        assert np.all(np.abs(device - seq) <= bound), (what, device, seq, bound)
        assert seq[1] > 0 and (processes["computeSnow"] or (seq[0] > 0) == (h in dc.RAIN_HOURS)), what      # (with snow, melt water is liquid water too)
        # the balance closes: the identities of test_run_hour_closes_its_balance_and_steps_as_the_per_block_calls
        current, runoff, drainage = getters["current"], getters["runoff"], getters["drainage"]
        assert res["currentWaterContent"] == current and res["runoff"] == runoff and res["freeDrainage"] + res["lateralDrainage"] == drainage, what
        again = current - (res["previousTotalWaterContent"] + runoff + drainage + seq[0] - seq[1] - seq[2])
        bound = n * hc.TWO_POW_MINUS_53 * absolute.sum() + 8 * hc.TWO_POW_MINUS_53 * max(abs(current), abs(res["previousTotalWaterContent"]))
        assert abs(res["massBalanceError"] - again) <= bound, (what, res["massBalanceError"], again, bound)
        assert res["massBalanceError_mm"] == res["massBalanceError"] / p["surfaceArea"] * 1000 and res["steps"] >= 1, what
    # an hour starts from the water content the hour before left
    for (_, _, before), (_, _, after) in zip(hours, hours[1:]):
        assert after["balance"]["previousTotalWaterContent"] == before["balance"]["currentWaterContent"]
    # the day was not one regime on the device either
    by_hour = {w["when"][3]: g for g, w, _ in hours}
    assert np.all(by_hour[0]["rad_global"][valid] == 0) and np.all(by_hour[0]["et0"][valid] > 0) and np.all(by_hour[12]["rad_global"][valid] > 0)
    assert np.all(by_hour[6]["station_transmissivity"] == dc.CAP) and np.all((by_hour[12]["station_transmissivity"] > 0) & (by_hour[12]["station_transmissivity"] < dc.CAP))
    assert np.count_nonzero((by_hour[12]["transpiration"] != flag) & (by_hour[12]["transpiration"] > 0)) > 0
    if processes["computeSnow"]:
        assert np.count_nonzero(by_hour[23]["snowFall"][valid] > 0) > 0 and np.count_nonzero(by_hour[12]["snowMelt"][valid] > 0) > 0


def test_without_compute_crop_the_last_hour_of_a_day_leaves_the_crop_maps(product, pin):
    """computeCrop off on the second date with previous_hour = 23: the four crop maps keep their bits over the date's start - maps on which
    the daily update would have changed more than a quarter of the crop cells (the mild hour 22:00 has set the daily extremes)."""
    _need_glibc_set(product)
    case = dc.day_world(pin, (3, 11))
    processes = dc.PROCESS_SETS[0]
    _set_up(product, case, processes)
    (first, _), (second, _) = case["calendar"]
    hour.run_day(product, first, (22,), lambda h: case["day_stations"][(tuple(first), h)], processes, previous_hour=21, date_doy=dc.doy_of(first))
    before = {n: crop.get_state(product, n) for n in crop.STATE}
    seen = {}

    def stations_of(h):
        seen.update({n: crop.get_state(product, n) for n in crop.STATE})
        return case["day_stations"][(tuple(second), h)]
    hour.run_day(product, second, (0,), stations_of, dict(processes, computeCrop=False), previous_hour=23, date_doy=dc.doy_of(second))
    _clean(product)
    assert set(seen) == set(crop.STATE)
    for name in crop.STATE:
        assert np.array_equal(_bits(seen[name]), _bits(before[name])), name
    updated = crop.restate_crop_day(before, case["dem"], case["crop_index"], case["crop_units"], dc.LATITUDE, dc.doy_of(second), flag=float(case["flag"]))
    changed = _bits(updated["degreeDays"]) != _bits(before["degreeDays"])
    assert np.count_nonzero(changed) > dc.crop_cells(case).sum() / 4 and np.count_nonzero(before["dailyTmin"] != np.float32(case["flag"])) > 0
