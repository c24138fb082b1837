"""The radiation block without a device: the header against the binding, the Python restatement of criteria3d_amd/radiation.py (point
model through `math`, which is the C library, and the library's acosf / powf) against the compiled-reference pin
(tests/golden/rad_rsun.npz) bit for bit in every cell, map and case, latlon_maps against the lat / lon maps the reference computed, the
small rasters of tests/rad_cases.py against the arms of the pin, and what the entry points refuse before they need a device.  The same
against the places pin (tests/golden/rad_rsun_places.npz: five other places, edited cells at the poles and on the date line, leap years and
centuries): every cell, the table of the sun-position arms (rad.SUN_ARMS), and the small rasters at other places against that table."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import build, capi, radiation as rad
from tests import rad_cases
from tests.raster_helpers import differing, exported_names

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pin():
    return rad_cases.load_pin()


def test_rad_header_and_binding_agree():
    text = (ROOT / "include" / "sf3d_rad.h").read_text()
    declared = set(re.findall(r"\b(sf3d_rad_\w+)\s*\(", text))
    assert declared == set(rad.SIGNATURES)
    for name, value in dict(REALSKY_TOTALTRANSMISSIVITY=0, REALSKY_LINKE=1, MODE_FIXED=0, MODE_MAP=1, MODE_MONTHLY=2, TILT_FIXED=1, TILT_DEM=2).items():
        assert re.search(rf"SF3D_RAD_{name} = {value}\b", text) and getattr(rad, name) == value
    for k, name in enumerate(("SUN_ELEVATION", "GLOBAL", "BEAM", "DIFFUSE", "REFLECTED")):
        assert re.search(rf"SF3D_RAD_{name} = {k}\b", text) and getattr(rad, name) == k
    fields = re.search(r"typedef struct \{(.*?)\} sf3d_rad_settings_t;", text, re.S).group(1)
    names = [n for line in re.findall(r"^\s*(?:int32_t|float)\s+([^;]+);", fields, re.M) for n in re.split(r",\s*", line)]
    assert [n.split("[")[0] for n in names] == [f[0] for f in rad.Settings._fields_]
    assert ctypes.sizeof(rad.Settings) == 8 * 4 + 17 * 4
    assert all(re.search(r"\.(cpp|h):\d+", c) for c in re.findall(r"/\*(.*?)\*/\s*sf3d_error_t sf3d_rad_\w+\(", text, re.S))      # every entry point cites file:line


def test_product_library_exports_the_rad_entry_points_outside_the_drop_in_abi():
    functions = exported_names(build.build_product(), "T")
    for name in rad.SIGNATURES:
        assert name in functions, name
    assert not any("rad" in n.lower().split("_") for n in capi.SIGNATURES)


def test_the_pin_reaches_every_arm_and_holds_the_cases_the_issue_lists(pin):
    assert list(pin["arm_names"]) == list(rad.ARMS) and (pin["arm_counts"] > 0).all()
    assert (GOLDEN_SIZE := (rad_cases.GOLDEN / "rad_rsun.npz").stat().st_size) <= (rad_cases.GOLDEN / "ravone_window.npz").stat().st_size, GOLDEN_SIZE
    names = " | ".join(c["name"] for c in pin["cases"])
    for piece in ("night", "hour of sunrise", "hour of sunset", "noon", "just above zero", "June solstice", "December solstice", "equinox",
                  "total transmissivity, real sky", "clear sky", "no shadowing", "fixed tilt", "monthly Linke", "Linke map", "albedo map",
                  "isUTC off", "day before", "day after", "second hour on the same maps"):
        assert piece in names, piece
    assert pin["dem"].shape == (2, 24, 32) and (pin["dem"] == pin["flag"]).any()
    for r in (0, 1):
        assert (pin["slope_reference"][r] == 0).sum() >= 9                       # the flat patch
    low = [rad_cases.pin_maps(pin, c)[0] for c in pin["cases"] if "just above zero" in c["name"]]
    assert all(((m > 0) & (m <= 1e-3)).any() for m in low)
    rise = [rad_cases.pin_maps(pin, c) for c in pin["cases"] if "hour of sunrise" in c["name"]]
    assert all(((m[0] > 0) & (m[0] < 3) & (m[1] > 0)).any() for m in rise)       # a lit cell below 3 degrees


def test_latlon_maps_equal_the_reference_bit_for_bit(pin):
    rows, cols = pin["dem"].shape[1:]
    header = dict(nrows=rows, ncols=cols, xllcorner=pin["geo"][0], yllcorner=pin["geo"][1], cellsize=pin["geo"][2])
    for r in (0, 1):
        lat, lon = rad.latlon_maps(header, dem=pin["dem"][r], flag=pin["flag"])
        assert not differing(lat, pin["lat"][r]).any() and not differing(lon, pin["lon"][r]).any()
    assert 44.4 < float(pin["lat"][0].max()) < 44.6 and 11.2 < float(pin["lon"][0].max()) < 11.4


def test_restatement_equals_the_compiled_reference_in_every_cell_map_and_case(pin):
    geo, flag = pin["geo"], pin["flag"]
    for raster, chain in rad_cases.pin_chains(pin):
        prev = None
        for case in chain:
            got, _ = rad.restate_radiation_hour(pin["dem"][raster], flag, geo[0], geo[1], geo[2], pin["lat"][raster], pin["lon"][raster], pin["slope"][raster],
                                                pin["aspect"][raster], case["when"], pin["transmissivity"][case["transmissivity"]], case["settings"], previous=prev)
            want = rad_cases.pin_maps(pin, case)
            if got is None:                                                      # a date S_solpos refuses: nothing is written
                got = np.full_like(want, flag)
            same = ~differing(got, want)
            assert same.all(), (case["name"], int((~same).sum()))
            prev = got


@pytest.fixture(scope="module")
def places():
    return rad_cases.load_places_pin()


def test_the_places_pin_reaches_the_sun_arms_and_holds_the_places_cells_and_dates_the_issue_lists(places):
    pin = places
    assert list(pin["sun_arm_names"]) == list(rad.SUN_ARMS) and list(pin["arm_names"]) == list(rad.ARMS)
    never = {n for n, k in zip(pin["sun_arm_names"], pin["sun_arm_counts"]) if k == 0}
    # only what rounding alone reaches may be missing (each with its failed search in the generator's docstring) and the one arm no valid cell can take
    assert never <= set(rad.SUN_ARMS_BY_ROUNDING + rad.SUN_ARMS_UNREACHABLE), never
    assert never == {"|cz| > 1", "elevref < -9"}                              # what the generator's docstring records
    # the table is the union of what the cases record, and the hemisphere, wrap and leap arms are among the reached
    union = 0
    for c in pin["cases"]:
        union |= c["sun_arms"]
    assert {n for k, n in enumerate(rad.SUN_ARMS) if union >> k & 1} == set(rad.SUN_ARMS) - never
    assert (rad_cases.GOLDEN / "rad_rsun_places.npz").stat().st_size < (rad_cases.GOLDEN / "rad_rsun.npz").stat().st_size
    assert pin["dem"].shape == (6, 16, 24) and (pin["dem"][0] == pin["flag"]).any() and len(pin["cases"]) >= 36
    old = rad_cases.load_pin()
    r0, c0, rows, cols = pin["cut"]
    assert np.array_equal(pin["dem"][0], old["dem"][1][r0:r0 + rows, c0:c0 + cols])          # cut from raster 1 of the first pin
    assert (pin["slope"] == 0).reshape(6, -1).sum(axis=1).min() >= 9 and (pin["slope"] == -9999.0).reshape(6, -1).sum(axis=1).min() >= 1
    want = [(33, 69.67, (420000.0, 7730000.0, 4.0), 1), (32, 0.23, (520000.0, 25000.0, 10.0), 1), (34, -33.93, (262000.0, 6243000.0, 2.5), 2),
            (10, 37.77, (551000.0, 4180000.0, 4.0), -8), (1, -17.2, (300000.0, 8100000.0, 10.0), -12)]
    for r, (zone, lat, geo, tz) in enumerate(want):
        p = pin["places"][r]
        assert (p["utmZone"], p["startLatitude"], rad_cases.pin_geo(pin, r), p["timeZone"]) == (zone, lat, geo, tz)
        assert abs(float(pin["lat"][r][8, 12]) - lat) < 0.05                   # (the places are named to a tenth of a degree)
        assert all(c["settings"]["timeZone"] == tz for c in pin["cases"] if c["raster"] == r)
    assert pin["places"][5]["utmZone"] == 32 and rad_cases.pin_geo(pin, 5) == (old["geo"][0] + c0 * 4.0, old["geo"][1] + (24 - r0 - rows) * 4.0, 4.0)
    assert np.array_equal(pin["lon"][5][8], old["lon"][1][r0 + 8, c0:c0 + cols])
    valid = pin["dem"][0] != pin["flag"]
    for name, values in (("lat", (90.0, -90.0, 89.97, 90.5)), ("lon", (180.0, -180.0, 179.99, 180.5)), ("aspect", (361.0,))):
        for v in values:
            assert ((pin[name][5] == np.float32(v)) & valid).sum() == 1, (name, v)
    whens = [(tuple(c["when"]), c["settings"]["timeZone"]) for c in pin["cases"]]
    for w in (((2024, 2, 29, 9, 30, 0), -8), ((2024, 3, 1, 0, 30, 0), -8), ((2000, 2, 29, 11, 30, 0), 1), ((1999, 12, 31, 23, 30, 0), 1),
              ((1950, 1, 1, 0, 30, 0), -12)):
        assert w in whens, w
    for day in ((2024, 12, 31), (2100, 3, 1), (2100, 12, 31), (1951, 1, 1)):
        assert any(w[:3] == day for w, _ in whens), day
    names = " | ".join(c["name"] for c in pin["cases"])
    for piece in ("polar: 21 June 2021, midnight", "polar: 21 June 2021, noon", "polar night) on the maps of the hour before", "polar: equinox noon",
                  "equator: equinox noon", "elevetr > 85 in most cells", "nearest the zenith", "south: 21 December 2021, noon", "south: 21 June 2021, morning",
                  "west: 21 June 2021, an hour by day", "west: 21 June 2021, an hour by night", "west: local time", "date line: 21 December 2021, an hour by day",
                  "date line: 21 June 2021, an hour by night", "date line: local time", "edited: equinox noon", "edited: June midnight", "refuses"):
        assert piece in names, piece
    # a value hangs on each tstfix wrap and on ssha = 0 under cssha > 1: the sun is up over the cell (and its transmissivity is there), yet
    # isIlluminated says no - without the wrap, or with any other ssha, the cell would be lit
    for piece, arm, where in (("tstfix < -720 wrap", "tstfix < -720", pin["lon"][5] == -180.0), ("tstfix > 720 wrap", "tstfix > 720", pin["lon"][5] == 180.0),
                              ("edited: December noon", "ssha: cssha > 1 (polar night)", np.abs(pin["lat"][5] - 66.566) < 1e-3)):
        case = next(c for c in pin["cases"] if piece in c["name"])
        maps, t = rad_cases.pin_maps(pin, case), pin["transmissivity"][case["transmissivity"]]
        assert case["sun_arms"] & rad._SUN[arm] and (where & valid).sum() == 1
        assert maps[0][where & valid][0] > 0.4 and maps[1][where & valid][0] == 0 and t[where & valid][0] > 0, piece
    # the sun in the north at the southern place: lit cells whose rays leave the grid, none of them by the south
    south = next(c for c in pin["cases"] if c["name"].startswith("south: 21 December 2021, noon"))
    assert south["arms"] & rad._ARM["shadow: ray left the grid"] and south["arms"] & rad._ARM["shadow: miss (above the highest cell)"]
    h = rad.hour_setup(south["when"], 2, True)
    sun = rad.sun_position(h, rad.cell_setup(100.0, float(pin["lat"][2][8, 12]), float(pin["lon"][2][8, 12]), 10.0, 0.0))
    assert (sun["azimuth"] < 90 or sun["azimuth"] > 270) and sun["elevationRefr"] > 60
    # what the issue measured on the restatement at 69.67 N and 0.23 N
    day = next(c for c in pin["cases"] if "polar day" in c["name"])
    night = next(c for c in pin["cases"] if c["name"].startswith("polar: 21 December 2021, an hour"))
    cell = rad.cell_setup(100.0, float(pin["lat"][0][8, 12]), float(pin["lon"][0][8, 12]), 10.0, 0.0)
    s_day, s_night = (rad.sun_position(rad.hour_setup(c["when"], 1, True), cell) for c in (day, night))
    assert (s_day["rise"], s_day["set"]) == (-179940.0, 179940.0) and (s_night["rise"], s_night["set"]) == (179940.0, -179940.0)
    assert s_night["relOptAirMassCorr"] == -1.0
    noon = rad_cases.pin_maps(pin, next(c for c in pin["cases"] if c["name"] == "equator: equinox noon"))[0]
    assert 89.7 < noon[valid].max() < 89.8


def test_latlon_maps_equal_the_reference_at_the_other_places(places):
    pin = places
    rows, cols = pin["dem"].shape[1:]
    edited = np.zeros((rows, cols), bool)
    for e in pin["edits"]:
        edited[e["row"], e["col"]] = True
    for r, p in enumerate(pin["places"]):
        geo = rad_cases.pin_geo(pin, r)
        lat, lon = rad.latlon_maps(dict(nrows=rows, ncols=cols, xllcorner=geo[0], yllcorner=geo[1], cellsize=geo[2]),
                                   dict(utmZone=p["utmZone"], startLatitude=p["startLatitude"]), dem=pin["dem"][r], flag=pin["flag"])
        keep = ~edited if r == 5 else np.ones_like(edited)
        assert not differing(lat, pin["lat"][r])[keep].any() and not differing(lon, pin["lon"][r])[keep].any(), p["name"]
    assert float(pin["lat"][2].max()) < -33.9 and float(pin["lon"][3].max()) < -122.4 and float(pin["lon"][4].min()) < -178.8


def test_restatement_equals_the_compiled_reference_at_the_other_places_in_every_cell_map_and_case(places):
    pin, flag = places, places["flag"]
    for raster, chain in rad_cases.pin_chains(pin):
        geo = rad_cases.pin_geo(pin, raster)
        prev = None
        for case in chain:
            sun_arms = np.zeros(pin["dem"][raster].shape, np.int64)
            got, arms = rad.restate_radiation_hour(pin["dem"][raster], flag, geo[0], geo[1], geo[2], pin["lat"][raster], pin["lon"][raster], pin["slope"][raster],
                                                   pin["aspect"][raster], case["when"], pin["transmissivity"][case["transmissivity"]], case["settings"],
                                                   previous=prev, sun_arms=sun_arms)
            want = rad_cases.pin_maps(pin, case)
            assert (got is None) == ("refuses" in case["name"])
            if got is None:                                                      # a date S_solpos refuses: the maps of the hour before stay
                got, arms = (prev if prev is not None else np.full_like(want, flag)), np.zeros(1, np.int64)
            same = ~differing(got, want)
            assert same.all(), (case["name"], int((~same).sum()))
            assert int(np.bitwise_or.reduce(arms, axis=None)) == case["arms"] and int(np.bitwise_or.reduce(sun_arms, axis=None)) == case["sun_arms"], case["name"]
            prev = got
    refused = [c for c in pin["cases"] if "refuses" in c["name"]]
    assert len(refused) == 1 and refused[0]["keep"] == 1 and (rad_cases.pin_maps(pin, refused[0])[1] > 0).any()      # it keeps the day hour's maps


def test_small_rasters_at_other_places_reach_every_sun_arm_the_places_pin_reaches(places):
    ref, reached = rad_cases.small_reference_places()
    want = {n for n, k in zip(places["sun_arm_names"], places["sun_arm_counts"]) if k > 0}
    assert {n for k, n in enumerate(rad.SUN_ARMS) if reached >> k & 1} == want
    assert set(rad_cases.PLACES) == {place for _, place, _, _ in rad_cases.small_chains_places()}
    cells = sorted({rad_cases.PLACES[p][2] for p in rad_cases.PLACES})
    assert cells == [2.5, 10.0] and {rad_cases.PLACES[p][1] for p in rad_cases.PLACES} == {-179.9, 179.9}
    g = rad_cases.small_raster((3, 11), "pole row")
    assert (g["lat"][0] == 90).sum() == 5 and (g["lat"][0] == -90).sum() == 6
    for piece in ("tstfix < -720 wrap", "tstfix > 720 wrap"):                 # the sun is up and every cell is dark: the wrap decides
        maps, arms = next(hours for (shape, name), hours in ref.items() if shape == (7, 37) and piece in name)[0]
        done = (arms & rad._ARM["not illuminated"]) != 0                        # (every cell but the one S_solpos refuses)
        assert done.sum() > 200 and (maps[0][done] > 1).all() and (maps[1][done] == 0).all() and not (arms & rad._ARM["illuminated"]).any(), piece
    # shadows fall both ways at both cell sizes: the march runs with invCellSize 0.1 and 0.4
    for place in ("80 N", "80 S"):
        hits = [arms for (shape, name), hours in ref.items() if name.startswith(place) for _, arms in hours if arms is not None]
        union = int(np.bitwise_or.reduce([np.bitwise_or.reduce(a, axis=None) for a in hits]))
        assert union & rad._ARM["shadow: hit"] and union & rad._ARM["shadow: ray left the grid"], place


def test_the_maps_are_state_across_hours(pin):
    """a cell whose transmissivity is NODATA in the second hour keeps the first hour's value in the reference's maps"""
    seen = 0
    for raster, chain in rad_cases.pin_chains(pin):
        for first, second in zip(chain, chain[1:]):
            a, b = rad_cases.pin_maps(pin, first), rad_cases.pin_maps(pin, second)
            t = pin["transmissivity"][second["transmissivity"]]
            kept = (t == -9999.0) & (pin["dem"][raster] != pin["flag"]) & (b[0] > 0) & (a[1] != pin["flag"])
            if kept.any() and (b[1][kept] == a[1][kept]).all() and (b[0][kept] == a[0][kept]).all():
                seen += int(kept.sum())
    assert seen > 0


def test_small_rasters_reach_the_arms_of_the_pin_and_every_edge():
    ref = rad_cases.small_reference()
    reached = 0
    for (shape, name), hours in ref.items():
        for maps, arms in hours:
            reached |= int(np.bitwise_or.reduce(arms, axis=None))
    missing = [n for k, n in enumerate(rad.ARMS) if not reached >> k & 1]
    assert not missing, missing
    # the sun stands in all four quadrants while rays leave the grid: north / east, south / east, south / west, north / west edges
    quadrants = set()
    g = rad_cases.small_raster((7, 37))
    cell = rad.cell_setup(float(g["dem"][1, 1]), float(g["lat"][1, 1]), float(g["lon"][1, 1]), 10.0, 180.0)
    for name, settings, hours in rad_cases.small_chains():
        s = rad.settings_dict(settings)
        for k, (when, _) in enumerate(hours):
            arms = ref[((7, 37), name)][k][1]
            if (arms & rad._ARM["shadow: ray left the grid"]).any():
                sun = rad.sun_position(rad.hour_setup(when, s["timeZone"], bool(s["isUTC"])), cell)
                quadrants.add(int(sun["azimuth"] // 90))
    assert quadrants == {0, 1, 2, 3}, quadrants
    for n, k in (("night, then the sun low in the east, then mid-morning", 1), ("noon, the sun low in the west, after sunset", 1)):
        maps, arms = ref[((7, 37), n)][k]
        lit = (arms & rad._ARM["illuminated"]) != 0
        written = lit & (maps[1] != rad_cases.FLAG) & (maps[0] > 0)          # (a lit cell without transmissivity keeps the hour before)
        assert written.sum() > 180 and (maps[0][written] < 8).mean() > 0.8, n          # the sun low in the east / in the west


def test_refusals_without_a_device(pin):
    sf = rad.bind(capi.load_product())
    lib = sf.lib
    n = 12
    buf = np.zeros(n, np.float32)
    pf = buf.ctypes.data_as(capi.pf32)
    assert lib.sf3d_rad_clean() == capi.OK
    assert lib.sf3d_rad_get_map(0, n, pf) == capi.MEMORY_ERROR              # before initialise
    assert lib.sf3d_rad_kernel_ms() == 0.0
    assert lib.sf3d_rad_default_parameters(None) == capi.PARAMETER_ERROR
    st = rad.Settings()
    assert lib.sf3d_rad_default_parameters(ctypes.byref(st)) == capi.OK
    d = rad.DEFAULT_SETTINGS
    assert [getattr(st, k) for k in ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")] == \
        [d[k] for k in ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")]
    assert (st.linke, st.albedo, st.tilt, st.aspect, st.clearSky) == (4.0, np.float32(0.2), 0.0, 0.0, 0.75) and list(st.linkeMonthly) == [-9999.0] * 12

    def init(rows=3, cols=4, dem=pf, cell=4.0, lat=pf, lon=pf, slope=pf, aspect=pf, linke=None, albedo=None, settings=None):
        s = ctypes.byref(rad.settings_struct(settings)) if settings is not None else None
        return lib.sf3d_rad_initialize(rows, cols, dem, -9999.0, 0.0, 0.0, cell, lat, lon, slope, aspect, linke, albedo, s)
    # shape mismatches and NULL static maps
    assert init(rows=0) == capi.PARAMETER_ERROR and init(cols=0) == capi.PARAMETER_ERROR and init(dem=None) == capi.PARAMETER_ERROR
    assert init(cell=0.0) == capi.PARAMETER_ERROR and init(cell=-4.0) == capi.PARAMETER_ERROR
    assert init(lat=None) == capi.PARAMETER_ERROR and init(lon=None) == capi.PARAMETER_ERROR
    assert init(slope=None) == capi.PARAMETER_ERROR and init(aspect=None) == capi.PARAMETER_ERROR          # DEM tilt needs both
    # map mode without a map, modes out of range, a time zone S_solpos refuses
    assert init(settings=dict(linkeMode=rad.MODE_MAP)) == capi.PARAMETER_ERROR
    assert init(settings=dict(albedoMode=rad.MODE_MAP)) == capi.PARAMETER_ERROR
    assert init(settings=dict(albedoMode=rad.MODE_MONTHLY)) == capi.PARAMETER_ERROR
    assert init(settings=dict(linkeMode=3)) == capi.PARAMETER_ERROR and init(settings=dict(tiltMode=0)) == capi.PARAMETER_ERROR
    assert init(settings=dict(realSkyAlgorithm=2)) == capi.PARAMETER_ERROR
    assert init(settings=dict(timeZone=13)) == capi.PARAMETER_ERROR and init(settings=dict(timeZone=-13)) == capi.PARAMETER_ERROR
    # whatever is acceptable needs a device from here on (SF3D_SOLVER_ERROR without one)
    assert init(slope=None, aspect=None, settings=dict(tiltMode=rad.TILT_FIXED)) in (capi.OK, capi.SOLVER_ERROR)
    assert lib.sf3d_rad_clean() == capi.OK

    hour = lambda y=2021, mo=3, d=20, h=11, mi=30, s=0, cells=n, t=pf: lib.sf3d_rad_compute_hour(y, mo, d, h, mi, s, cells, t)
    assert hour() == capi.MEMORY_ERROR                                      # a valid call, no raster yet
    # a date outside 1950-2050 that S_solpos refuses (its bound is 2100, solPos.cpp:301), dates and times that are none
    assert hour(y=1949) == capi.PARAMETER_ERROR and hour(y=2101) == capi.PARAMETER_ERROR and hour(y=1900) == capi.PARAMETER_ERROR
    assert hour(y=1950, mo=1, d=1, h=0, mi=0) == capi.MEMORY_ERROR and hour(y=2100, mo=12, d=31, h=12) == capi.MEMORY_ERROR
    assert hour(y=1950, mo=1, d=1, h=0, mi=30, t=pf) == capi.MEMORY_ERROR
    assert hour(y=2100, mo=12, d=31, h=23, mi=30) == capi.PARAMETER_ERROR   # UTC + 1: the local date is in 2101
    assert hour(mo=0) == capi.PARAMETER_ERROR and hour(mo=13) == capi.PARAMETER_ERROR and hour(d=0) == capi.PARAMETER_ERROR
    assert hour(mo=2, d=29) == capi.PARAMETER_ERROR and hour(y=2020, mo=2, d=29) == capi.MEMORY_ERROR
    assert hour(h=24) == capi.PARAMETER_ERROR and hour(h=-1) == capi.PARAMETER_ERROR and hour(mi=60) == capi.PARAMETER_ERROR and hour(s=60) == capi.PARAMETER_ERROR
    # NULL transmissivity without a meteo hour
    assert hour(t=None) == capi.PARAMETER_ERROR
    assert lib.sf3d_rad_clean() == capi.OK
