"""The restated day without a GPU (tests/day_cases.py): the restatements of every raster block chained over two dates and five hours that
cross midnight, on both rasters and both process sets tests/test_gpu_day.py runs.  What is held here are conditions on the inputs: the
chain composes and stays finite, and the day is not one regime - night and day, the transmissivity cap and the measured ratio, snowfall,
melt and bare ground, rain and none, a daily crop update that changes the maps, daily extremes reset by the day, a pond update that
changes some nodes and leaves others.  Every arm is counted and printed.  The node state is the CPU oracle's van Genuchten curve on the
case's potentials, kept for every hour: here it only steers the sink arms."""
import numpy as np
import pytest

from tests import day_cases as dc
from tests import sink_cases as sc
from tests.raster_helpers import bits as _bits


@pytest.fixture(scope="module")
def pin():
    return sc.load_pin()


def test_day_world_leaves_the_hour_world_as_it_was(pin):
    from tests import hour_cases as hc
    for shape in dc.SHAPES:
        base, case = hc.world(pin, shape), dc.day_world(pin, shape)
        assert set(base) | {"calendar", "day_stations"} == set(case)
        for name, want in base.items():
            if isinstance(want, np.ndarray):
                assert case[name].dtype == want.dtype and np.array_equal(_bits(want), _bits(case[name])), name
        for k, st in enumerate(base["stations"]):
            for name, values in st.items():
                assert all(np.array_equal(a, b) for a, b in zip(values, case["stations"][k][name])), (k, name)
        # the calendar's stations: quantised, no NaN, the irradiance of the night 0
        for (date, h), st in case["day_stations"].items():
            for name in ("airT", "prec", "dewT", "relHum", "windInt"):
                v = st[name][2]
                assert v.dtype == np.float32 and np.isfinite(v).all() and np.array_equal(v * 16, np.round(v * 16)), (h, name)
            m = st["transmissivity"]["measured"]
            assert np.isfinite(m).all() and (not m.any() if h in dc.NIGHT else (m > 0).all()), h
            assert (st["prec"][2] > 0).all() if h in dc.RAIN_HOURS else not st["prec"][2].any(), h
        assert np.count_nonzero(case["day_stations"][((2021, 3, 20), 23)]["airT"][2] < 0) > 0 and np.count_nonzero(case["day_stations"][((2021, 3, 21), 0)]["airT"][2] < 0) > 0


@pytest.mark.parametrize("processes", dc.PROCESS_SETS, ids=("snow-dew-idw", "rain-stations-shepard"))
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_restated_day_composes_and_is_not_one_regime(pin, oracle, shape, processes):
    case = dc.day_world(pin, shape)
    flag = np.float32(case["flag"])
    valid = case["dem"] != flag
    day, starts, hours = dc.restated_day_on(dc.host_state(oracle, case), case, processes)
    by_hour = {h: res for (_, _, h), res in zip(dc.hours_of(), hours)}
    assert list(by_hour) == [22, 23, 0, 6, 12]
    assert all(dc.finite(res) for res in hours) and all(dc.finite(s) for s in starts)
    arms = {}
    # night: no global radiation anywhere, ET0 still computed (the aerodynamic term)
    for h in dc.NIGHT:
        res = by_hour[h]
        assert np.all(res["rad_global"][valid] == 0) and np.all(res["station_transmissivity"] == 0), h
        arms[f"night {h}: cells with ET0 > 0"] = int(np.count_nonzero(res["et0"][valid] > 0))
        assert np.all(res["et0"][valid] != flag)
    for h in dc.SUNRISE + dc.NOON:
        arms[f"day {h}: cells with global radiation > 0"] = int(np.count_nonzero(by_hour[h]["rad_global"][valid] > 0))
    # the transmissivity cap and the measured ratio
    arms["stations at the cap at 06:00"] = int(np.count_nonzero(by_hour[6]["station_transmissivity"] == dc.CAP))
    t = by_hour[12]["station_transmissivity"]
    arms["stations with the measured ratio at 12:00"] = int(np.count_nonzero((t > 0) & (t < dc.CAP)))
    # rain and none
    for h, res in by_hour.items():
        wet = int(np.count_nonzero(res["prec"][valid] > 0))
        assert (wet == valid.sum()) if h in dc.RAIN_HOURS else wet == 0, h
    arms["hours with rain"], arms["hours without rain"] = len(dc.RAIN_HOURS), len(by_hour) - len(dc.RAIN_HOURS)
    if processes["computeSnow"]:
        front = by_hour[23]
        arms["23:00: cells with snowfall"] = int(np.count_nonzero(front["snowFall"][valid] > 0))
        arms["12:00: cells with rain and no snowfall"] = int(np.count_nonzero((by_hour[12]["snowFall"][valid] == 0) & (by_hour[12]["prec"][valid] > 0)))
        arms["cells that melt in some hour"] = int(np.count_nonzero(np.any([res["snowMelt"][valid] > 0 for res in hours], axis=0)))
        arms["cells with snow that do not melt at 00:00"] = int(np.count_nonzero((by_hour[0]["swe"][valid] > 0) & (by_hour[0]["snowMelt"][valid] == 0)))
        arms["cells without snow at 12:00"] = int(np.count_nonzero(by_hour[12]["swe"][valid] == 0))
    # the day's start: no crop update on the first date, one on the second; the extremes are reset by it
    crop_cells = dc.crop_cells(case)
    before, after = by_hour[23], starts[1]
    changed = (_bits(before["degreeDays"]) != _bits(after["degreeDays"])) | (_bits(before["lai"]) != _bits(after["lai"]))
    arms["crop cells the daily update changes"] = int(np.count_nonzero(changed & crop_cells))
    assert arms["crop cells the daily update changes"] > crop_cells.sum() / 4
    assert np.all(after["dailyTmin"] == flag) and np.count_nonzero(before["dailyTmin"] != flag) > 0
    arms["cells whose daily extremes differ after 00:00"] = int(np.count_nonzero((by_hour[0]["dailyTmin"] != before["dailyTmin"]) | (by_hour[0]["dailyTmax"] != before["dailyTmax"])))
    # the ponds
    surface = int(np.count_nonzero(case["columns"][0] >= 0))
    moved = starts[0]["pond_after"] != starts[0]["pond_before"]
    arms["surface nodes the first pond update changes"], arms["... and leaves"] = int(moved.sum()), int((~moved).sum())
    assert moved.sum() > surface / 4
    arms["surface nodes the second pond update changes"] = int(np.count_nonzero(starts[1]["pond_after"] != starts[1]["pond_before"]))
    # the sinks
    noon = by_hour[12]
    arms["cells that transpire at 12:00"] = int(np.count_nonzero((noon["transpiration"] != flag) & (noon["transpiration"] > 0)))
    arms["cells that evaporate at 00:00"] = int(np.count_nonzero((by_hour[0]["evaporation"] != flag) & (by_hour[0]["evaporation"] > 0)))
    for name, count in arms.items():
        print(f"{shape} {processes['method']}: {name}: {count}")
    empty = [name for name, count in arms.items() if count <= 0]
    assert not empty, empty
    # a flag cell holds the flag, the last lane computes
    for res in hours:
        assert res["et0"].flat[0] == flag and res["et0"].flat[-1] != flag and res["evaporation"].flat[0] == flag and res["evaporation"].flat[-1] != flag
        assert np.all(res["totals"] >= 0) and res["totals"][1] > 0
