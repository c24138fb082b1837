"""What tests/test_day_host.py and tests/test_gpu_day.py share (no tests here): the small world of tests/hour_cases.py with a calendar of
two dates whose five hours cross midnight - frost and rain at night, sunrise, noon - and `RestatedDay`, the day of hour.run_day on plain
numpy: the restatements of every block chained in run_hour's order, with the radiation maps of the hour before, the snow state, the four
crop maps and the pond map carried from hour to hour and from date to date.  Nothing of it is re-seeded from a device: the only thing a
caller hands in is the solver's node state at the start of an hour (water contents) and the node ponds before the day's pond update."""
import datetime

import numpy as np

from criteria3d_amd import crop, hour, meteo, radiation as rad, root, sinks, snow, transmissivity as tr
from tests import hour_cases as hc
from tests import sink_cases as sc

SHAPES = ((3, 11), (7, 37))                    # 33 cells: less than a wave; 259: a block plus three lanes
CALENDAR = (((2021, 3, 20), (22, 23)), ((2021, 3, 21), (0, 6, 12)))
PREVIOUS_HOUR = (21, 23)                       # of the hour before each date's first: no daily update on the first date, one on the second
NIGHT, SUNRISE, NOON = (22, 23, 0), (6,), (12,)
RAIN_HOURS = (23, 12)
PROCESS_SETS = (dict(computeSnow=True, useDewPoint=True, method="idw"), dict(computeSnow=False, useDewPoint=False, method="shepard"))
LATITUDE, START_DOY = 44.5, 120                # what hour_cases.initialize_blocks gives the crop block
RADIATION_STATIONS, WIDTH = 6, 3
CAP = np.float32(1.2 * 0.75)                   # computePointTransmissivity clamps Kt to 1.2 (transmissivity.restate_point)


def doy_of(date):
    return datetime.date(*map(int, date)).timetuple().tm_yday


def hours_of():
    """(date index, date, hour) of the calendar, in order"""
    return [(d, date, h) for d, (date, hours) in enumerate(CALENDAR) for h in hours]


def day_world(pin, shape):
    """hour_cases.world(pin, shape), untouched, with case["calendar"] and case["day_stations"][(date, hour)]: the stations of that hour
    as hour.run_hour takes them (hour_cases.hour_stations on this hour's values).  The values are quantised as `world` quantises them:
      22:00 mild and dry; 23:00 a cold front: below 0 degC at most stations, with precipitation (snow on the cold cells, rain on the
      others); 00:00 frost, dry; 06:00 near 0 degC, dry, the first light: a measured irradiance far above the clear-sky one (Kt is
      clamped); 12:00 mild with rain and a measured irradiance below the clear-sky one.  The measured irradiance of the night hours is 0."""
    case = hc.world(pin, shape)
    rows, cols = shape
    rng = np.random.default_rng(7000 * rows + cols)
    sx, sy, _, area = case["stations"][0]["airT"]
    ns = len(sx)
    q = lambda v, step: (np.round(np.asarray(v) / step) * step).astype(np.float32)
    air_range = {22: (9.0, 16.0), 23: (-4.0, 4.5), 0: (-7.0, -1.0), 6: (-2.0, 3.0), 12: (7.0, 15.0)}
    case["calendar"] = CALENDAR
    case["day_stations"] = {}
    for _, date, h in hours_of():
        air = q(rng.uniform(*air_range[h], ns), 1 / 16)
        prec = q(rng.uniform(0.5, 3.0, ns), 1 / 8) if h in RAIN_HOURS else np.zeros(ns, np.float32)
        values = dict(airT=(sx, sy, air, area), prec=(sx, sy, prec, area), relHum=(sx, sy, q(rng.uniform(35.0, 95.0, ns), 1), area),
                      dewT=(sx, sy, q(air - rng.uniform(0.5, 12.0, ns), 1 / 16), area), windInt=(sx, sy, q(rng.uniform(0.0, 6.0, ns), 1 / 4), area))
        st = hc.hour_stations(dict(case, stations=[values]), 0)
        if h in NIGHT:
            measured = np.zeros((RADIATION_STATIONS, WIDTH), np.float32)
        elif h in SUNRISE:
            measured = np.round(rng.uniform(150.0, 400.0, (RADIATION_STATIONS, WIDTH))).astype(np.float32)
        else:
            measured = np.round(rng.uniform(150.0, 600.0, (RADIATION_STATIONS, WIDTH))).astype(np.float32)
        st["transmissivity"] = dict(st["transmissivity"], measured=measured)
        case["day_stations"][(tuple(date), h)] = st
    return case


def crop_cells(case):
    return crop._crop_cells(case["dem"], case["crop_index"], case["crop_units"], float(np.float32(case["flag"])))


class RestatedDay:
    """The day on plain numpy.  start_date() and hour() are called in the order hour.run_day makes its calls."""

    def __init__(self, case, processes=None, pond_compute_crop=True):
        p = dict(hour.DEFAULT_PROCESSES)
        p.update(processes or {})
        self.case, self.p, self.pond_compute_crop = case, p, pond_compute_crop
        self.flag = float(case["flag"])
        self.cell = float(case["cell_size"])
        self.grid = tr.grid_of(case["dem"], self.flag, hc.GEO[0], hc.GEO[1], self.cell)
        self.radiation = None                                                 # the five maps of the hour before
        self.snow = snow.restate_reset(case["swe"], self.flag) if p["computeSnow"] else None
        self.crop = crop.restate_degree_days(case["dem"], case["crop_index"], case["crop_units"], LATITUDE, case["sink_degree_days"][0], START_DOY, self.flag)
        self.pond = None
        self.arms = {}                                                        # of the sink hours

    def start_date(self, date, previous_hour, compute_crop=None):
        """dailyUpdateCropMaps when the hour before was the day's last (and computeCrop), then dailyUpdatePond -> the four crop maps and
        the pond map"""
        case = self.case
        compute_crop = self.p["computeCrop"] if compute_crop is None else compute_crop
        if compute_crop and previous_hour == 23:
            self.crop = crop.restate_crop_day(self.crop, case["dem"], case["crop_index"], case["crop_units"], LATITUDE, doy_of(date), flag=self.flag)
        mp, lm, ic = hc.pond_tables(case)
        self.pond = hour.restate_pond(case["slope"], case["crop_index"], mp, lm, ic, self.pond_compute_crop, self.crop["lai"], self.flag, self.flag,
                                      surface_index=case["columns"][0])
        return dict({n: v.copy() for n, v in self.crop.items()}, pond_map=self.pond.copy())

    def node_ponds(self, before):
        """the ponds of the surface nodes after dailyUpdatePond, given those before: the pond map's value where it holds one"""
        after = np.array(before, np.float64)
        col = self.case["columns"][0]
        has = (col >= 0) & (self.pond != np.float32(hour.NODATA))
        after[col[has]] = self.pond[has].astype(np.float64)
        return after

    def _interpolate(self, st, name):
        case = self.case
        x, y, v, area, settings = st[name]
        return meteo.restate_interpolate(case["dem"], hc.GEO[0], hc.GEO[1], self.cell, [None], name, self.p["method"], x, y, v, area, settings, self.flag)

    def hour(self, when, stations, vwc):
        """runModelHour at `when` on the water contents `vwc` of the nodes -> every map by name"""
        case, p, flag = self.case, self.p, self.flag
        dem = case["dem"]
        clear = float(p["clearSkyTransmissivity"])
        out = {}
        # 1. the five interpolations; 2. the humidity
        air, prec = self._interpolate(stations, "airT"), self._interpolate(stations, "prec")
        if p["useDewPoint"]:
            out["dewT"] = self._interpolate(stations, "dewT")
            humidity = hour.restate_relative_humidity(air, out["dewT"], flag)
        else:
            humidity = self._interpolate(stations, "relHum")
        wind = self._interpolate(stations, "windInt")
        t = stations["transmissivity"]
        points = tr.point_array(t["points"])
        values = tr.restate_points(self.grid, None, when, t["width"], t["time_step_second"], points, t["measured"])[0]
        has = np.abs(values.astype(np.float64) - hour.NODATA) >= hour.EPSILON
        trans = meteo.restate_interpolate(dem, hc.GEO[0], hc.GEO[1], self.cell, [None], "transmissivity", p["method"], points[has, 0], points[has, 1], values[has],
                                          t["area"], t.get("settings", p["settings"]), flag)
        out.update(airT=air, prec=prec, relHum=humidity, windInt=wind, transmissivity=trans, station_transmissivity=values)
        # 3. the radiation hour on the maps of the hour before
        maps, _ = rad.restate_radiation_hour(dem, flag, hc.GEO[0], hc.GEO[1], self.cell, case["lat"], case["lon"], case["slope"], case["aspect"], when, trans,
                                             previous=self.radiation)
        assert maps is not None, when
        self.radiation = maps
        out.update({"rad_" + n: maps[k].copy() for k, n in enumerate(rad.MAPS)})
        met = dict(airT=air, prec=prec, relHum=humidity, windInt=wind, globalRad=out["rad_global"], beamRad=out["rad_beam"], transmissivity=trans,
                   clearSkyTransmissivity=clear, surfaceWater=p["surfaceWater"])
        # 4. snow, or rain alone
        if p["computeSnow"]:
            self.snow = snow.restate_snow_hour(self.snow, met, dem, flag)
            out.update({n: v.copy() for n, v in self.snow.items()})
            liquid = self.snow["liquid"]
        else:
            liquid = prec
        # 5. ET0 and the daily extremes
        et0 = crop.restate_et0_hour(dem, met, flag, clear)
        tmin, tmax = crop.restate_daily_temperatures(self.crop["dailyTmin"], self.crop["dailyTmax"], air, flag)
        self.crop = dict(self.crop, dailyTmin=tmin, dailyTmax=tmax)
        out.update({n: v.copy() for n, v in self.crop.items()}, et0=et0)
        # 6. the root maps of the restated degree days
        roots = root.restate_root_maps(dem, case["crop_index"], case["soil_index"], case["unit_list"], case["soil_list"], case["layer_depth"],
                                       case["layer_thickness"], self.crop["degreeDays"], flag)
        out.update({"root_" + n: roots[n] for n in ("length", "depth", "first", "last", "density")})
        # 7. the sink hour
        sunk = sinks.restate_sink_hour(dem, flag, self.cell, case["columns"], vwc, case["crop_index"], case["soil_index"], case["sink_units"], case["sink_soils"],
                                       case["layer_depth"], case["layer_thickness"], float(case["computation_depth"]), et0, self.crop["lai"], self.crop["degreeDays"],
                                       liquid, dict(length=roots["length"], first=roots["first"], last=roots["last"], density=roots["density"]),
                                       case["columns"].size, self.arms)
        out.update(sinks=sunk["sinks"], evaporation=sunk["evaporation"], transpiration=sunk["transpiration"], liquid_read=liquid)
        # 8. the sequential totals
        out["totals"], out["totals_absolute"] = hc.totals_restated(case, liquid, sunk["evaporation"], sunk["transpiration"])
        return out


MAP_NAMES = ("airT", "prec", "relHum", "windInt", "transmissivity") + tuple("rad_" + n for n in rad.MAPS) + crop.MAPS + \
    ("root_length", "root_depth", "root_first", "root_last", "root_density", "sinks", "evaporation", "transpiration")


def compared_names(processes):
    """the maps of an hour that the device and the restated day both hold"""
    names = MAP_NAMES + (("dewT",) if processes["useDewPoint"] else ())
    return names + ((snow.STATE + snow.OUTPUT) if processes["computeSnow"] else ())


def device_maps(sf, case, m, processes):
    """every map the last hour left on the device, under RestatedDay's names"""
    res = hc.all_maps(sf, case, m, processes["computeSnow"])
    res.update({n: meteo.get_map(sf, n) for n in ("airT", "prec", "relHum", "windInt", "transmissivity") + (("dewT",) if processes["useDewPoint"] else ())})
    res.update({"rad_" + n: v for n, v in rad.all_maps(sf).items()})
    return res


def finite(maps):
    """no NaN or infinity in any float map of a dict"""
    return all(np.isfinite(v).all() for v in maps.values() if isinstance(v, np.ndarray) and v.dtype.kind == "f")


def host_state(checker, case):
    """(the water contents of the case's potentials, the ponds of the surface nodes) from a checker library (the CPU oracle): the node
    model and the setter the device test uses.  The host test keeps this state for every hour: there it only steers the arms."""
    from criteria3d_amd import catchment as cm
    m = sc.node_model(case)
    checker.check(checker.lib.sf3d_reset_solver_state(), "reset")
    cm.build(checker, m, threads=1)
    checker.set_matric_potential_bulk(0, case["psi"])
    vwc = checker.water_content(0, m.n)
    ponds = np.array([checker.lib.sf3d_get_node_pond(i) for i in range(m.ns)])
    checker.lib.sf3d_clean()
    return vwc, ponds


def restated_day_on(state, case, processes):
    """the whole calendar on one node state (host_state) -> (RestatedDay, [the maps of each date's start], [the maps of each hour])"""
    vwc, ponds = state
    day = RestatedDay(case, processes)
    starts, hours = [], []
    for d, (date, hs) in enumerate(case["calendar"]):
        start = day.start_date(date, PREVIOUS_HOUR[d])
        start["pond_before"], start["pond_after"] = ponds, day.node_ponds(ponds)
        ponds = start["pond_after"]
        starts.append(start)
        for h in hs:
            hours.append(day.hour(tuple(date) + (h, 0, 0), case["day_stations"][(tuple(date), h)], vwc))
    return day, starts, hours
