"""The hourly r.sun radiation maps with DEM shadows on the device (include/sf3d_rad.h, criteria3d_amd/csrc/sf3d_rad.inc): what
`Project::interpolateDemRadiation` (agrolib/project/project.cpp:3387-3465) runs at the half hour after it interpolates the
transmissivity map - `radiation::computeRadiationDEM` (agrolib/solarRadiation/solarRadiation.cpp:1045-1069): the NREL sun position
(solPos.cpp), the shadow ray across the DEM (computeShadow) and the r.sun clear-sky / real-sky model (computeRadiationRsun).

Three parts:
  * the binding (`bind`, `initialize`, `compute_hour`, `get_map`, `all_maps`, `clean`): the five maps live on the device, k_rad_hour
    writes them once per hour; a missing kernel or library is an error;
  * `latlon_maps`: gis::computeLatLonMaps (gis.cpp:1081-1110) over utmToLatLon (:1005-1063), the way `project3d.slope_aspect` gives
    slope and aspect;
  * `restate_radiation_hour`: the point model cell by cell through python's `math` (the C library's sin / cos / tan / exp / pow) and
    the C library's acosf / powf (the float overloads the compiled reference calls) with the reference's types and operation order -
    the checker of the CPU tests against the compiled-reference pins (tests/golden/rad_rsun.npz, rad_rsun_places.npz), of the GPU tests
    off the pins, and the source of their arm tables (ARMS: the radiation model; SUN_ARMS: the sun position and its date).  A checker,
    never a fallback."""
from __future__ import annotations

import ctypes as C
import ctypes.util
import math
from functools import partial

import numpy as np

from . import capi, raster
from .capi import pf32

NODATA = -9999.0
EPSILON = 0.00001                               # commonConstants.h:252
RADDEG = 0.0174532925                           # solPos.cpp:122
DEGRAD = 57.295779513                           # solPos.cpp:121
DEG_TO_RAD = 0.01745329252                      # commonConstants.h:255
RAD_TO_DEG = 57.295779513
PI = 3.1415926535898                            # commonConstants.h:249
TEMPERATURE_DEFAULT = 10.0                      # radiationDefinitions.h:22

MAPS = ("sunElevation", "global", "beam", "diffuse", "reflected")
(SUN_ELEVATION, GLOBAL, BEAM, DIFFUSE, REFLECTED) = range(5)
REALSKY_TOTALTRANSMISSIVITY, REALSKY_LINKE = 0, 1
MODE_FIXED, MODE_MAP, MODE_MONTHLY = 0, 1, 2
TILT_FIXED, TILT_DEM = 1, 2

# Crit3DRadiationSettings::initialize (radiationSettings.cpp:41-72) and Crit3DGisSettings (gis.cpp:47-54)
DEFAULT_SETTINGS = dict(realSky=1, realSkyAlgorithm=REALSKY_LINKE, shadowing=1, linkeMode=MODE_FIXED, albedoMode=MODE_FIXED, tiltMode=TILT_DEM,
                        timeZone=1, isUTC=1, linke=4.0, linkeMonthly=(NODATA,) * 12, albedo=0.2, tilt=0.0, aspect=0.0, clearSky=0.75)
DEFAULT_GIS = dict(utmZone=32, startLatitude=44.501)


class Settings(C.Structure):
    """sf3d_rad_settings_t"""
    _fields_ = [(n, C.c_int32) for n in ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")] + \
               [("linke", C.c_float), ("linkeMonthly", C.c_float * 12), ("albedo", C.c_float), ("tilt", C.c_float), ("aspect", C.c_float),
                ("clearSky", C.c_float)]


psettings = C.POINTER(Settings)
# name -> (restype, argtypes): every symbol include/sf3d_rad.h declares
SIGNATURES = {
    "sf3d_rad_default_parameters": (capi.u8, [psettings]),
    "sf3d_rad_initialize": (capi.u8, [capi.u32, capi.u32, pf32, capi.f32, capi.f64, capi.f64, capi.f64, pf32, pf32, pf32, pf32, pf32, pf32, psettings]),
    "sf3d_rad_compute_hour": (capi.u8, [capi.i32, capi.i32, capi.i32, capi.i32, capi.i32, capi.i32, capi.u32, pf32]),
    "sf3d_rad_get_map": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_rad_device_trig": (capi.u8, [capi.i32, capi.u32, capi.pd, capi.pd, capi.pd]),
    "sf3d_rad_kernel_ms": (capi.f64, []),
    "sf3d_rad_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_rad.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

_f32 = partial(raster.f32, what="radiation")
_index = raster.index


def settings_dict(settings: dict | None) -> dict:
    s = dict(DEFAULT_SETTINGS)
    s.update(settings or {})
    return s


def settings_struct(settings: dict | None) -> Settings:
    s = settings_dict(settings)
    return Settings(int(s["realSky"]), int(s["realSkyAlgorithm"]), int(s["shadowing"]), int(s["linkeMode"]), int(s["albedoMode"]), int(s["tiltMode"]),
                    int(s["timeZone"]), int(s["isUTC"]), float(s["linke"]), (C.c_float * 12)(*map(float, s["linkeMonthly"])), float(s["albedo"]),
                    float(s["tilt"]), float(s["aspect"]), float(s["clearSky"]))


def _opt(a, shape):
    return None if a is None else _f32(a, shape)


def _ptr(a):
    return a.ctypes.data_as(pf32) if a is not None else pf32()


def initialize(sf: capi.SF3D, dem, xll: float, yll: float, cell_size: float, lat, lon, slope=None, aspect=None, linke_map=None, albedo_map=None,
               settings: dict | None = None, flag: float = NODATA) -> None:
    """Crit3DRadiationMaps(dem, gisSettings): the five maps at `flag`, the static maps of the cell on the device"""
    bind(sf)
    dem = _f32(dem)
    maps = [_f32(lat, dem.shape), _f32(lon, dem.shape), _opt(slope, dem.shape), _opt(aspect, dem.shape), _opt(linke_map, dem.shape), _opt(albedo_map, dem.shape)]
    sf._rad_shape = dem.shape
    sf.check(sf.lib.sf3d_rad_initialize(dem.shape[0], dem.shape[1], dem.ctypes.data_as(pf32), float(flag), float(xll), float(yll), float(cell_size),
                                        *map(_ptr, maps), C.byref(settings_struct(settings))), "rad_initialize")


def compute_hour(sf: capi.SF3D, when, transmissivity=None) -> None:
    """computeRadiationDEM at `when` = (year, month, day, hour, minute, second); transmissivity None: the meteo block's map on the device"""
    t = _opt(transmissivity, sf._rad_shape)
    n = int(np.prod(sf._rad_shape))
    sf.check(sf.lib.sf3d_rad_compute_hour(*map(int, when), n, _ptr(t)), "rad_compute_hour")


def get_map(sf: capi.SF3D, which) -> np.ndarray:
    out = np.empty(sf._rad_shape, np.float32)
    sf.check(sf.lib.sf3d_rad_get_map(_index(which, MAPS), out.size, out.ctypes.data_as(pf32)), f"rad_get_map({which})")
    return out


def all_maps(sf: capi.SF3D) -> dict:
    """the five maps, by name"""
    return {n: get_map(sf, n) for n in MAPS}


def device_trig(sf: capi.SF3D, which: int, x, y=None) -> np.ndarray:
    """test hook: the device build of sf3d_trig.inc (0 sin, 1 cos, 2 tan, 3 acos, 4 acosf, 5 powf(x, y)) on the doubles `x`"""
    bind(sf)
    x = np.ascontiguousarray(x, np.float64)
    y = None if y is None else np.ascontiguousarray(y, np.float64)
    out = np.empty_like(x)
    sf.check(sf.lib.sf3d_rad_device_trig(int(which), x.size, x.ctypes.data_as(capi.pd), y.ctypes.data_as(capi.pd) if y is not None else capi.pd(),
                                         out.ctypes.data_as(capi.pd)), "rad_device_trig")
    return out


def kernel_ms(sf: capi.SF3D) -> float:
    return float(sf.lib.sf3d_rad_kernel_ms())


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_rad_clean(), "rad_clean")


# ------------------------------------------------------------------------------------------------ lat / lon

def utm_to_latlon(zone: int, reference_lat: float, easting: float, northing: float):
    """gis::utmToLatLon, gis.cpp:1005-1063 (WGS84: Crit3DEllipsoid, gis.cpp:41-45)"""
    ae, ecc = 6378137.0, 6.69438000426083E-03
    k0 = 0.9996
    e1 = (1. - math.sqrt(1. - ecc)) / (1. + math.sqrt(1. - ecc))
    x = easting - 500000.0
    y = northing
    if reference_lat < 0:
        y -= 10000000.
    ecc_prime = ecc / (1. - ecc)
    m = y / k0
    mu = m / (ae * (1. - ecc / 4. - 3. * ecc * ecc / 64. - 5. * ecc * ecc * ecc / 256.))
    phi1 = mu + (3.0 * e1 / 2.0 - 27.0 * e1 * e1 * e1 / 32.0) * math.sin(2.0 * mu) \
        + (21.0 * e1 * e1 / 16.0 - 55.0 * e1 * e1 * e1 * e1 / 32.0) * math.sin(4.0 * mu) \
        + (151.0 * e1 * e1 * e1 / 96.0) * math.sin(6.0 * mu)
    n1 = ae / math.sqrt(1.0 - ecc * math.sin(phi1) * math.sin(phi1))
    t1 = math.tan(phi1) * math.tan(phi1)
    c1 = ecc_prime * math.cos(phi1) * math.cos(phi1)
    r1 = ae * (1.0 - ecc) / math.pow(1.0 - ecc * (math.sin(phi1) * math.sin(phi1)), 1.5)
    d = x / (n1 * k0)
    lat = phi1 - (n1 * math.tan(phi1) / r1) * (d * d / 2.0
                                                 - (5.0 + 3.0 * t1 + 10 * c1 - 4.0 * c1 * c1 - 9.0 * ecc_prime) * d * d * d * d / 24.0
                                                 + (61.0 + 90.0 * t1 + 298 * c1 + 45.0 * t1 * t1 - 252.0 * ecc_prime - 3.0 * c1 * c1) * d * d * d * d * d * d / 720.0)
    lat *= RAD_TO_DEG
    lon = (d - (1.0 + 2.0 * t1 + c1) * d * d * d / 6.0
           + (5.0 - 2.0 * c1 + 28 * t1 - 3.0 * c1 * c1 + 8.0 * ecc_prime + 24.0 * t1 * t1) * d * d * d * d * d / 120.0) / math.cos(phi1)
    long_origin = float(zone - 1.) * 6. - 180. + 3.
    lon *= RAD_TO_DEG
    lon += long_origin
    return lat, lon


def latlon_maps(header: dict, gis_settings: dict | None = None, dem=None, flag: float = NODATA):
    """gis::computeLatLonMaps (gis.cpp:1081-1110): float latitude and longitude of every cell centre of the raster `header` describes
    (nrows, ncols, xllcorner, yllcorner, cellsize); `flag` where `dem` holds it (all cells without a dem)"""
    g = dict(DEFAULT_GIS)
    g.update(gis_settings or {})
    nrows, ncols = int(header["nrows"]), int(header["ncols"])
    xll, yll, cs = float(header["xllcorner"]), float(header["yllcorner"]), float(header["cellsize"])
    lat = np.full((nrows, ncols), flag, np.float32)
    lon = np.full((nrows, ncols), flag, np.float32)
    for row in range(nrows):
        y = yll + cs * (float(nrows - row) - 0.5)
        for col in range(ncols):
            if dem is not None and abs(float(dem[row, col]) - float(flag)) < EPSILON:
                continue
            x = xll + cs * (float(col) + 0.5)
            la, lo = utm_to_latlon(g["utmZone"], g["startLatitude"], x, y)
            lat[row, col] = la
            lon[row, col] = lo
    return lat, lon


# ------------------------------------------------------------------------------------------------ restatement (checker)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = C.c_float
_libm.acosf.argtypes = [C.c_float]
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]
_acosf = _libm.acosf
_powf = _libm.powf
_cf = C.c_float


def f32(x: float) -> float:
    """round to float, as an assignment to a float does (inf when out of range)"""
    return _cf(x).value


def _int(x: float) -> int:
    return int(x)          # truncation, as (int) of a double in range


def _pow(x: float, y: float) -> float:
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.nan


def _exp(x: float) -> float:
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _div(a: float, b: float) -> float:
    """IEEE division"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _max(a, b):
    return b if a < b else a           # std::max


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if hi < v else v)          # std::clamp


def _leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def _month_days(y: int, m: int) -> int:
    return 29 if (m == 2 and _leap(y)) else (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


# arms of the sun position (S_solpos) and of its date and time, as bits: what a place other than 44 N 11 E and a year other than 2021
# reach (the table of tests/golden/rad_rsun_places.npz).  hour_setup reports its bits as h["sunArms"] (hour_sun_arms: also for a date
# S_solpos refuses), cell_setup as c["sunArms"], sun_position as sun["sunArms"]; restate_radiation_hour gives their union per cell.
SUN_ARMS = ("lmst < 0", "hrang < -180", "hrang > 180", "hrang > 0", "|cz| > 1", "zenetr > 99",
            "ssha: pole (|cd cl| < 0.001), the hemisphere of the declination", "ssha: pole (|cd cl| < 0.001), the other hemisphere",
            "ssha: cssha < -1 (polar day)", "ssha: cssha > 1 (polar night)", "srss: ssha <= 1", "srss: ssha >= 179",
            "tstfix > 720", "tstfix < -720", "sazm: default 180 at a pole (|cl| < 0.001)", "sazm: default 180 off the poles (|ce cl| < 0.001)",
            "sazm: ca > 1", "sazm: ca < -1", "refrac: elevetr > 85", "refrac: elevetr >= 5", "refrac: -0.575 <= elevetr < 5", "refrac: elevetr < -0.575",
            "elevref < -9", "zenref > 93", "coszen <= 0",
            "validate: |latitude| > 90", "validate: |longitude| > 180", "validate: |aspect| > 360", "validate: |slope| > 180",
            "leap year", "leap year: daynum += 1", "29 February", "day 366", "400-year rule", "100-year rule", "validate: year < 1950",
            "local date steps back over 1 January", "local date steps back over 1 March", "ectime < 0", "mnlong < 0", "mnanom < 0")
_SUN = {n: 1 << k for k, n in enumerate(SUN_ARMS)}
# the arms that only some place or second reaches by the rounding of floats: a pin may miss them, with the failed search written down
SUN_ARMS_BY_ROUNDING = ("|cz| > 1", "sazm: ca > 1", "sazm: ca < -1", "sazm: default 180 off the poles (|ce cl| < 0.001)")
# no cell that validate() accepts reaches this one: zenetr <= 99 bounds elevetr at -9, and below -0.575 degrees the correction is
# -20.774 / tan(elevetr) times a pressure term that validate() keeps in [0, 2000] hPa - never negative, so elevref >= elevetr >= -9
SUN_ARMS_UNREACHABLE = ("elevref < -9",)


def hour_setup(when, time_zone: int, is_utc: bool):
    """the date-and-time part of computeRadiationRsun and S_solpos (solarRadiation.cpp:714-726; solPos.cpp:293-331, 373-382, 426-555):
    None when S_solpos refuses the date"""
    return _hour(when, time_zone, is_utc)[0]


def hour_sun_arms(when, time_zone: int, is_utc: bool) -> int:
    """the SUN_ARMS bits of the date and time, also of a date S_solpos refuses"""
    return _hour(when, time_zone, is_utc)[1]


def _hour(when, time_zone: int, is_utc: bool):
    """hour_setup -> (h or None, SUN_ARMS bits)"""
    bits = 0
    year, month, day, hour, minute, second = map(int, when)
    t = hour * 3600 + minute * 60 + second
    if is_utc:
        t += time_zone * 3600
    while not (0 <= t < 86400):
        if t >= 86400:
            t -= 86400
            day += 1
            if day > _month_days(year, month):
                day = 1
                month += 1
                if month > 12:
                    month, year = 1, year + 1
        else:
            t += 86400
            day -= 1
            if day < 1:
                month -= 1
                if month < 1:
                    month, year = 12, year - 1
                    bits |= _SUN["local date steps back over 1 January"]
                elif month == 2:
                    bits |= _SUN["local date steps back over 1 March"]
                day = _month_days(year, month)
    h = dict(hour=t // 3600)
    h["minute"] = (t - h["hour"] * 3600) // 60
    h["second"] = t - h["hour"] * 3600 - h["minute"] * 60
    h["localTime"] = f32(float(t))
    h["timezone"] = f32(float(time_zone))
    if year < 1950:
        bits |= _SUN["validate: year < 1950"]
    if year < 1950 or year > 2100 or abs(time_zone) > 12:
        return None, bits
    daynum = day + (0, 0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334)[month]
    if year % 400 == 0:
        bits |= _SUN["400-year rule"]
    elif year % 100 == 0:
        bits |= _SUN["100-year rule"]
    if _leap(year):
        bits |= _SUN["leap year"]
        if month == 2 and day == 29:
            bits |= _SUN["29 February"]
    if _leap(year) and month > 2:
        daynum += 1
        bits |= _SUN["leap year: daynum += 1"]
    if daynum == 366:
        bits |= _SUN["day 366"]
    dayang = f32(360.0 * (daynum - 1) / 365.0)
    sd = math.sin(RADDEG * dayang)
    cd = math.cos(RADDEG * dayang)
    d2 = 2.0 * dayang
    c2 = math.cos(RADDEG * d2)
    s2 = math.sin(RADDEG * d2)
    erv = f32(1.000110 + 0.034221 * cd + 0.001280 * sd)
    erv = f32(erv + f32(0.000719 * c2 + 0.000077 * s2))
    utime = f32(h["hour"] * 3600.0 + h["minute"] * 60.0 + h["second"] - 0 / 2.0)
    utime = f32(utime / 3600.0 - h["timezone"])
    delta = f32(float(year - 1949))
    leap = _int(delta / 4.0)
    julday = f32(32916.5 + delta * 365.0 + leap + daynum + utime / 24.0)
    ectime = f32(julday - 51545.0)
    if ectime < 0.0:
        bits |= _SUN["ectime < 0"]

    def wrap(v, period, arm=None):
        nonlocal bits
        v = f32(v - f32(period * _int(v / period)))
        if v < 0.0 and arm:
            bits |= _SUN[arm]
        return f32(v + period) if v < 0.0 else v
    mnlong = wrap(f32(280.460 + 0.9856474 * ectime), 360.0, "mnlong < 0")
    mnanom = wrap(f32(357.528 + 0.9856003 * ectime), 360.0, "mnanom < 0")
    eclong = wrap(f32(mnlong + 1.915 * math.sin(mnanom * RADDEG) + 0.020 * math.sin(2.0 * mnanom * RADDEG)), 360.0)
    ecobli = f32(23.439 - 4.0e-07 * ectime)
    h["declin"] = f32(DEGRAD * math.asin(math.sin(ecobli * RADDEG) * math.sin(eclong * RADDEG)))
    top = math.cos(RADDEG * ecobli) * math.sin(RADDEG * eclong)
    bottom = math.cos(RADDEG * eclong)
    rascen = f32(DEGRAD * math.atan2(top, bottom))
    if rascen < 0.0:
        rascen = f32(rascen + 360.0)
    h["rascen"] = rascen
    gmst = f32(f32(f32(6.697375) + f32(f32(0.0657098242) * ectime)) + utime)
    h["gmst"] = wrap(gmst, 24.0)
    h["erv"] = erv
    h["cd"] = f32(math.cos(RADDEG * h["declin"]))
    h["sd"] = f32(math.sin(RADDEG * h["declin"]))
    h["etrn"] = f32(1367.0 * erv)
    h["sunArms"] = bits
    return h, bits


def cell_setup(height: float, lat: float, lon: float, slope: float, aspect: float) -> dict:
    """the cell's part (solarRadiation.cpp:734, 479-496, 534; solPos.cpp:327-344, 886-890, 912-917); arguments are float32 values"""
    c = dict(height=height, lat=lat, lon=lon, slope=slope, aspect=aspect)
    c["cl"] = f32(math.cos(RADDEG * lat))
    c["sl"] = f32(math.sin(RADDEG * lat))
    c["press"] = f32(101325. * _pow(1 + height * 0.0065 / 293.16, -9.80665 / (0.0065 * 287.058)) * 0.01)
    c["cp"], c["ct"] = math.cos(RADDEG * aspect), math.cos(RADDEG * slope)
    c["sp"], c["st"] = math.sin(RADDEG * aspect), math.sin(RADDEG * slope)
    slope_rad = slope * DEG_TO_RAD
    c["sinSlope"], c["cosSlope"] = math.sin(slope_rad), math.cos(slope_rad)
    half = math.sin(slope * 0.5 * DEG_TO_RAD)
    c["Fg"] = c["sinSlope"] - slope_rad * c["cosSlope"] - PI * (half * half)
    c["reflGeom"] = 1. - math.cos(slope * DEG_TO_RAD)
    c["ok"] = not (abs(lon) > 180. or abs(lat) > 90. or c["press"] < 0.0 or c["press"] > 2000.0 or abs(slope) > 180.0 or abs(aspect) > 360.0)
    c["sunArms"] = (_SUN["validate: |latitude| > 90"] if abs(lat) > 90. else 0) | (_SUN["validate: |longitude| > 180"] if abs(lon) > 180. else 0) \
        | (_SUN["validate: |aspect| > 360"] if abs(aspect) > 360.0 else 0) | (_SUN["validate: |slope| > 180"] if abs(slope) > 180.0 else 0)
    return c


def sun_position(h: dict, c: dict):
    """RSUN_compute_solar_position + computeSunPosition for one cell; None: S_solpos refuses the cell"""
    if not c["ok"]:
        return None
    sin, cos, tan = math.sin, math.cos, math.tan
    bits = 0
    lmst = f32(f32(h["gmst"] * 15.) + c["lon"])
    lmst = f32(lmst - f32(360.0 * _int(lmst / 360.0)))
    if lmst < 0.:
        lmst = f32(lmst + 360.0)
        bits |= _SUN["lmst < 0"]
    hrang = f32(lmst - h["rascen"])
    if hrang < -180.0:
        hrang = f32(hrang + 360.0)
        bits |= _SUN["hrang < -180"]
    elif hrang > 180.0:
        hrang = f32(hrang - 360.0)
        bits |= _SUN["hrang > 180"]
    ch = f32(cos(RADDEG * hrang))
    cz = f32(f32(h["sd"] * c["sl"]) + f32(f32(h["cd"] * c["cl"]) * ch))
    if abs(cz) > 1.0:
        cz = 1.0 if cz >= 0.0 else -1.0
        bits |= _SUN["|cz| > 1"]
    zenetr = f32(_acosf(cz) * DEGRAD)
    if zenetr > 99.0:
        zenetr = 99.0
        bits |= _SUN["zenetr > 99"]
    elevetr = f32(90. - zenetr)
    cdcl = f32(h["cd"] * c["cl"])
    if abs(cdcl) >= 0.001:
        cssha = f32(f32(-c["sl"] * h["sd"]) / cdcl)
        if cssha < -1.0:
            ssha = 180.0
            bits |= _SUN["ssha: cssha < -1 (polar day)"]
        elif cssha > 1.0:
            ssha = 0.0
            bits |= _SUN["ssha: cssha > 1 (polar night)"]
        else:
            ssha = f32(DEGRAD * _acosf(cssha))
    elif (h["declin"] >= 0.0 and c["lat"] > 0.0) or (h["declin"] < 0.0 and c["lat"] < 0.0):
        ssha = 180.0
        bits |= _SUN["ssha: pole (|cd cl| < 0.001), the hemisphere of the declination"]
    else:
        ssha = 0.0
        bits |= _SUN["ssha: pole (|cd cl| < 0.001), the other hemisphere"]
    tst = f32(f32(180. + hrang) * 4.)
    tstfix = f32(f32(f32(f32(tst - f32(h["hour"] * 60.)) - float(h["minute"])) - f32(h["second"] / 60.)) + 0.0)
    while tstfix > 720.0:
        tstfix = f32(tstfix - 1440.0)
        bits |= _SUN["tstfix > 720"]
    while tstfix < -720.0:
        tstfix = f32(tstfix + 1440.0)
        bits |= _SUN["tstfix < -720"]
    if ssha <= 1.0:
        sretr, ssetr = 2999.0, -2999.0
        bits |= _SUN["srss: ssha <= 1"]
    elif ssha >= 179.0:
        sretr, ssetr = -2999.0, 2999.0
        bits |= _SUN["srss: ssha >= 179"]
    else:
        sretr = f32(720.0 - 4.0 * ssha - tstfix)
        ssetr = f32(720.0 + 4.0 * ssha - tstfix)
    ce = f32(cos(RADDEG * elevetr))
    se = f32(sin(RADDEG * elevetr))
    azim = 180.0
    cecl = f32(ce * c["cl"])
    if abs(cecl) >= 0.001:
        ca = f32(f32(f32(se * c["sl"]) - h["sd"]) / cecl)
        if ca > 1.0:
            ca = 1.0
            bits |= _SUN["sazm: ca > 1"]
        elif ca < -1.0:
            ca = -1.0
            bits |= _SUN["sazm: ca < -1"]
        azim = f32(180. - f32(_acosf(ca) * DEGRAD))
        if hrang > 0:
            azim = f32(360. - azim)
            bits |= _SUN["hrang > 0"]
    else:
        bits |= _SUN["sazm: default 180 at a pole (|cl| < 0.001)" if abs(c["cl"]) < 0.001 else "sazm: default 180 off the poles (|ce cl| < 0.001)"]
    if elevetr > 85.0:
        refcor = 0.0
        bits |= _SUN["refrac: elevetr > 85"]
    else:
        tanelev = tan(RADDEG * elevetr)
        if elevetr >= 5.0:
            refcor = _div(58.1, tanelev) - _div(0.07, _pow(tanelev, 3)) + _div(0.000086, _pow(tanelev, 5))
            bits |= _SUN["refrac: elevetr >= 5"]
        elif elevetr >= -0.575:
            refcor = 1735.0 + elevetr * (-518.2 + elevetr * (103.4 + elevetr * (-12.79 + elevetr * 0.711)))
            bits |= _SUN["refrac: -0.575 <= elevetr < 5"]
        else:
            refcor = _div(-20.774, tanelev)
            bits |= _SUN["refrac: elevetr < -0.575"]
        prestemp = (c["press"] * 283.0) / (1013.0 * (273.0 + TEMPERATURE_DEFAULT))
        refcor *= f32(prestemp / 3600.0)
    elevref = f32(elevetr + refcor)
    if elevref < -9.0:
        elevref = -9.0
        bits |= _SUN["elevref < -9"]
    zenref = f32(90.0 - elevref)
    cos_zenref = cos(RADDEG * zenref)
    coszen = f32(cos_zenref)
    if zenref > 93.0:
        ampress = -1.0
        bits |= _SUN["zenref > 93"]
    else:
        amass = f32(_div(1.0, f32(cos_zenref + f32(f32(0.50572) * _powf(f32(f32(96.07995) - zenref), f32(-1.6364))))))
        ampress = f32(f32(amass * c["press"]) / 1013.0)
    if coszen > 0.0:
        etrn = h["etrn"]
        etr = f32(etrn * coszen)
    else:
        etrn = etr = 0.0
        bits |= _SUN["coszen <= 0"]
    ca_ = cos(RADDEG * azim)
    sa_ = sin(RADDEG * azim)
    sz = sin(RADDEG * zenref)
    cosinc = f32(coszen * c["ct"] + sz * c["st"] * (ca_ * c["cp"] + sa_ * c["sp"]))
    return dict(relOptAirMassCorr=ampress, azimuth=azim, elevationRefr=elevref, extraIrradianceHorizontal=etr, extraIrradianceNormal=etrn,
                incidence=f32(_max(0., RAD_TO_DEG * ((PI / 2.0) - _acosf(cosinc)))), rise=f32(sretr * 60.), set=f32(ssetr * 60.), sunArms=bits)


# arms of the point model, as bits (the arm table of tests/golden/rad_rsun.npz)
ARMS = ("not illuminated", "illuminated", "shadow: hit", "shadow: miss (above the highest cell)", "shadow: ray left the grid", "shadow: step > 1",
        "shadow: flag cell on the ray", "real sky: total transmissivity", "real sky: Linke", "clear sky: total transmissivity", "clear sky: Linke",
        "Erbs: Kt <= 0.22", "Erbs: 0.22 < Kt <= 0.80", "Erbs: Kt > 0.80", "Muneer: shaded or incidence <= 0.1", "Muneer: sun at 3 deg or higher",
        "Muneer: low sun (fmod)", "air mass <= 20", "air mass > 20", "A0 patch (A0 Trd < 0.0022)", "flat (slope == 0)", "no direct beam (shaded or incidence <= 0)",
        "false: transmissivity NODATA by day", "false: S_solpos range check")
_ARM = {n: 1 << k for k, n in enumerate(ARMS)}


def shadow(grid: dict, x0: float, y0: float, z0: float, sun: dict):
    """computeShadow, solarRadiation.cpp:547-617 -> (shaded, arm bits)"""
    dem, flag = grid["dem"], float(grid["flag"])
    nrows, ncols = dem.shape
    cs, inv = grid["cellsize"], 1.0 / grid["cellsize"]
    xll, yll = grid["xll"], grid["yll"]
    sin_az, cos_az = math.sin(sun["azimuth"] * DEG_TO_RAD), math.cos(sun["azimuth"] * DEG_TO_RAD)
    sin_el, cos_el = math.sin(sun["elevationRefr"] * DEG_TO_RAD), math.cos(sun["elevationRefr"] * DEG_TO_RAD)
    tg = sin_el / _max(cos_el, 1e-6)
    step_x, step_y, step_z = 1.0 * sin_az * cs, 1.0 * cos_az * cs, 1.0 * cs * tg
    max_dh = cs * 1.0 * 2.0
    max_count = (grid["demMax"] - z0) / EPSILON if abs(step_z) < 1e-6 else (grid["demMax"] - z0) / step_z
    count, step, arms = 0.0, 1.0, 0
    while count < max_count:
        count += step
        x, y, z = x0 + step_x * count, y0 + step_y * count, z0 + step_z * count
        row = (nrows - 1) - _int((y - yll) * inv)
        col = _int((x - xll) * inv)
        if not (0 <= row < nrows and 0 <= col < ncols):
            return False, arms | _ARM["shadow: ray left the grid"]
        z_dem = float(dem[row, col])
        if z_dem != flag:
            if (z_dem - z) > 0.5:
                return True, arms | _ARM["shadow: hit"]
            step = (z - z_dem) / max_dh
            if step < 1.0:
                step = 1.0
            else:
                arms |= _ARM["shadow: step > 1"]
        else:
            arms |= _ARM["shadow: flag cell on the ray"]
    return False, arms | _ARM["shadow: miss (above the highest cell)"]


def _separate(clear_sky, transmissivity, elev_deg, sin_elev_deg):
    """separateTransmissivity_Erbs_Reindl -> (td, Tt, arm bits)"""
    tt = _clamp(transmissivity, 1e-6, clear_sky)
    if clear_sky <= 1e-6:
        return 0.0, tt, 0
    kt = _clamp(tt / clear_sky, 0.0, 1.2)
    sin_elev = _max(sin_elev_deg, 1e-4)
    if kt <= 0.22:
        kd, arm = 1.0 - 0.09 * kt, _ARM["Erbs: Kt <= 0.22"]
    elif kt <= 0.80:
        kd, arm = 0.9511 - 0.1604 * kt + 4.388 * kt * kt - 16.638 * kt * kt * kt + 12.336 * kt * kt * kt * kt, _ARM["Erbs: 0.22 < Kt <= 0.80"]
    else:
        kd, arm = 0.165, _ARM["Erbs: Kt > 0.80"]
    kd_r = kd
    if elev_deg > 0.0:
        kd_r = kd + (0.10 + 0.12 * elev_deg / 90.0) * (1.0 - _exp(-1.0 / sin_elev))
    kd_r = _clamp(kd_r, 0.0, 1.0)
    return tt * kd_r, tt, arm


def rad_point(grid: dict, h: dict, c: dict, row: int, col: int, transmissivity: float, sun_arms: list | None = None):
    """computeRadiationDemPoint + computeRadiationRsun -> (the five values or None when nothing is written, arm bits); sun_arms: a list that
    receives the SUN_ARMS bits of the cell's sun position"""
    nrows = grid["dem"].shape[0]
    x0 = grid["xll"] + grid["cellsize"] * (float(col) + 0.5)
    y0 = grid["yll"] + grid["cellsize"] * (float(nrows - row) - 0.5)
    v, arms = rad_eval(grid, h, c, x0, y0, float(c["height"]), True, transmissivity, sun_arms)
    return (None if v is None else (v[0],) + tuple(f32(x) for x in v[1:])), arms


def rad_eval(grid: dict, h: dict, c: dict, x0: float, y0: float, z0: float, march: bool, transmissivity: float, sun_arms: list | None = None,
             sun_out: list | None = None):
    """computeRadiationRsun for a point at (x0, y0, z0) -> ((elevationRefr, global, beam, diffuse, reflected) with the four radiations as
    the doubles of TradPoint, or None when nothing is written, arm bits).  march: the shadow ray runs (the point is inside the DEM);
    sun_out: a list that receives the sun position where it was computed (also when the evaluation then fails)"""
    sun = sun_position(h, c)
    if sun is None:
        return None, _ARM["false: S_solpos range check"]
    if sun_arms is not None:
        sun_arms.append(sun["sunArms"])
    if sun_out is not None:
        sun_out.append(sun)
    lit = False
    if sun["rise"] != NODATA and sun["set"] != NODATA and sun["elevationRefr"] != NODATA:
        lit = h["localTime"] >= sun["rise"] and h["localTime"] <= sun["set"] and sun["elevationRefr"] > 0
    arms = _ARM["illuminated"] if lit else _ARM["not illuminated"]
    shaded = True           # TsunPosition::shadow is never set with shadowing off and reads non-zero in the pin build (sf3d_rad.inc)
    if h["shadowing"]:
        shaded = not lit
        if lit and march:
            shaded, a = shadow(grid, x0, y0, z0, sun)
            arms |= a
    if not lit:
        return (sun["elevationRefr"], 0.0, 0.0, 0.0, 0.0), arms
    if h["realSky"] and transmissivity == NODATA:
        return None, arms | _ARM["false: transmissivity NODATA by day"]
    linke, clear_sky = h["linke"], h["clearSky"]
    elev = sun["elevationRefr"]
    sin_elev_refr = math.sin(elev * DEG_TO_RAD)
    if h["realSkyAlgorithm"] == REALSKY_TOTALTRANSMISSIVITY:
        arms |= _ARM["real sky: total transmissivity"] if h["realSky"] else _ARM["clear sky: total transmissivity"]
        if not h["realSky"]:
            transmissivity = clear_sky
        td, tt, a = _separate(clear_sky, transmissivity, elev, sin_elev_refr)
        arms |= a
        gh = sun["extraIrradianceHorizontal"] * transmissivity
        dh = sun["extraIrradianceHorizontal"] * td
    else:
        air = sun["relOptAirMassCorr"]
        if air <= 20:
            arms |= _ARM["air mass <= 20"]
            rayleigh = _div(1., 6.6296 + 1.7513 * air - 0.1202 * air * air + 0.0065 * _pow(air, 3) - 0.00013 * _pow(air, 4))
        else:
            arms |= _ARM["air mass > 20"]
            rayleigh = _div(1., 10.4 + 0.718 * air)
        bhc = sun["extraIrradianceNormal"] * sin_elev_refr * _exp(-0.8662 * linke * air * rayleigh)
        dhc = 0.0
        if not (elev <= 1e-3):
            trd = _max(-0.015843 + linke * (0.030543 + 0.0003797 * linke), 1e-6)
            sin_elev = _max(sin_elev_refr, 1e-5)
            a0 = 0.26463 + linke * (-0.061581 + 0.0031408 * linke)
            if (a0 * trd) < 0.0022:
                a0 = 0.002 / trd
                arms |= _ARM["A0 patch (A0 Trd < 0.0022)"]
            a1 = 2.0402 + linke * (0.018945 - 0.011161 * linke)
            a2 = -1.3025 + linke * (0.039231 + 0.0085079 * linke)
            fd = a0 + a1 * sin_elev + a2 * sin_elev * sin_elev
            dhc = sun["extraIrradianceNormal"] * fd * trd
        ghc = dhc + bhc
        if h["realSky"]:
            arms |= _ARM["real sky: Linke"]
            gh = _div(ghc * transmissivity, clear_sky)
            td, tt, a = _separate(clear_sky, transmissivity, elev, sin_elev_refr)
            arms |= a
            dh = _div(td, tt) * gh
        else:
            arms |= _ARM["clear sky: Linke"]
            gh, dh = ghc, dhc
    direct = (not shaded) and sun["incidence"] > 0.
    if direct:
        bh = gh - dh
    else:
        arms |= _ARM["no direct beam (shaded or incidence <= 0)"]
        bh, gh = 0.0, dh
    if c["slope"] == 0:
        arms |= _ARM["flat (slope == 0)"]
        beam, diffuse, reflected, glob = bh, dh, 0.0, gh
    else:
        sin_inc = math.sin(sun["incidence"] * DEG_TO_RAD)
        beam = bh * _div(_max(sin_inc, 0.0), _max(sin_elev_refr, 1e-6)) if direct else 0.0
        if elev < 1e-6:
            diffuse = 0.0
        else:
            aspect_rad = c["aspect"] * DEG_TO_RAD
            elev_rad = elev * DEG_TO_RAD
            sin_elev = _max(sin_elev_refr, 1e-6)
            kb = _clamp(_div(bh, sun["extraIrradianceNormal"] * sin_elev), 0.0, 1.2)
            r_sky = (1.0 + c["cosSlope"]) / 2.0
            fg = c["Fg"]
            if shaded or sun["incidence"] <= 0.1:
                arms |= _ARM["Muneer: shaded or incidence <= 0.1"]
                fx = r_sky + fg * 0.252271
            else:
                n = 0.00263 - kb * (0.712 + 0.6883 * kb)
                term = sin_inc / sin_elev
                if not (elev < 3.0):
                    arms |= _ARM["Muneer: sun at 3 deg or higher"]
                    fx = (n * fg + r_sky) * (1.0 - kb) + kb * term
                else:
                    arms |= _ARM["Muneer: low sun (fmod)"]
                    diff = math.fmod(sun["azimuth"] * DEG_TO_RAD - aspect_rad + 2 * PI, 2 * PI)
                    denom2 = _max(0.05, 0.1 - 0.008 * elev_rad)
                    fx = (n * fg + r_sky) * (1.0 - kb) + kb * c["sinSlope"] * math.cos(diff) / denom2
            diffuse = dh * fx
        if c["slope"] < 1e-6:
            reflected = 0.
        else:
            reflected = _clamp(h["albedo"], 0.0, 1.0) * (bh + dh) * c["reflGeom"] / 2.
        glob = beam + diffuse + reflected
    return (elev, glob, beam, diffuse, reflected), arms


def restate_radiation_hour(dem, flag, xll, yll, cell_size, lat, lon, slope, aspect, when, transmissivity, settings: dict | None = None, previous=None,
                           mine=None, sun_arms=None):
    """computeRadiationDEM on the host -> (the five maps [5, rows, cols] float32, arm bits [rows, cols] int64), or (None, None) when S_solpos
    refuses the date.  previous: the maps of the hour before (the flag everywhere without); mine: bool mask of the cells to compute;
    sun_arms: an int64 array [rows, cols] that receives the SUN_ARMS bits of every computed cell (also when the date is refused)"""
    s = settings_dict(settings)
    dem = np.ascontiguousarray(dem, np.float32)
    h, hour_bits = _hour(when, int(s["timeZone"]), bool(s["isUTC"]))
    if h is None:
        if sun_arms is not None:
            sun_arms[...] = np.where((np.abs(dem.astype(np.float64) - float(flag)) >= EPSILON) & (True if mine is None else mine), hour_bits, 0)
        return None, None
    month = int(when[1])
    if s["linkeMode"] == MODE_MONTHLY:
        h["linke"] = f32(s["linkeMonthly"][month - 1])
    else:
        h["linke"] = f32(s["linke"]) if s["linkeMode"] == MODE_FIXED else NODATA
    h["albedo"] = f32(s["albedo"]) if s["albedoMode"] == MODE_FIXED else NODATA
    h["clearSky"] = f32(s["clearSky"])
    h["realSky"], h["realSkyAlgorithm"], h["shadowing"] = bool(s["realSky"]), int(s["realSkyAlgorithm"]), bool(s["shadowing"])
    valid = np.abs(dem.astype(np.float64) - float(flag)) >= EPSILON
    real = valid & (np.abs(dem.astype(np.float64) - NODATA) >= EPSILON)
    grid = dict(dem=dem, flag=np.float32(flag), xll=float(xll), yll=float(yll), cellsize=float(cell_size),
                demMax=float(dem[real].max()) if real.any() else NODATA)
    out = np.full((5,) + dem.shape, np.float32(flag), np.float32) if previous is None else np.array(previous, np.float32)
    arms = np.zeros(dem.shape, np.int64)
    fixed = s["tiltMode"] == TILT_FIXED
    trans = np.ascontiguousarray(transmissivity, np.float32)
    for row in range(dem.shape[0]):
        for col in range(dem.shape[1]):
            if not valid[row, col] or (mine is not None and not mine[row, col]):
                continue
            c = cell_setup(float(dem[row, col]), float(lat[row, col]), float(lon[row, col]),
                           f32(s["tilt"]) if fixed else float(slope[row, col]), f32(s["aspect"]) if fixed else float(aspect[row, col]))
            position = []
            v, a = rad_point(grid, h, c, row, col, float(trans[row, col]), position)
            arms[row, col] = a
            if sun_arms is not None:
                sun_arms[row, col] = hour_bits | c["sunArms"] | sum(position)
            if v is not None:
                out[:, row, col] = v
    return out, arms
