"""The hourly snow model of the application on the device (include/sf3d_snow.h, criteria3d_amd/csrc/sf3d_snow.inc): what
`Crit3DProject::computeSnowModel` (bin/CRITERIA3D/criteria3DProject.cpp:1815-1878) computes before the hour's water is handed to the
solver - `Crit3DSnow::computeSnowBrooksModel` (src/snow/snow.cpp:142-525, the Brooks energy balance) on seven float state maps - and the
liquid water `assignPrecipitation` (:914-968) then feeds the solver: prec - snowFall + snowMelt.

Three parts:
  * the binding (`bind`, `initialize`, `compute_hour`, `get_state` ...): the maps live on the device, k_snow_hour advances them by one
    hour; a missing kernel or library is an error;
  * host plumbing: `surface_sources` (liquid-water map -> per-node source of assignPrecipitation, without soil cracking) and the
    application's `snow/` state folder (`save_snow_state` / `load_snow_state`, ESRI float grids);
  * `restate_snow_hour`: the point model cell by cell in python's `math` (the C library's exp / log / pow) with the reference's
    operation order - the checker of the CPU tests against the compiled-reference pin (tests/golden/snow_brooks.npz) and the host
    figure of scripts/snow_timing.py.  A checker, never a fallback."""
from __future__ import annotations

import ctypes as C
import math
from functools import partial
from pathlib import Path

import numpy as np

from . import capi, raster
from .capi import pf32

NODATA = -9999.0
EPSILON = 0.00001                               # commonConstants.h:252

# state maps (Crit3DSnowMaps) and hourly outputs, in the order of include/sf3d_snow.h
STATE = ("swe", "ice", "lwc", "internalEnergy", "surfaceEnergy", "surfaceTemp", "age")
OUTPUT = ("snowFall", "snowMelt", "deltaSWE", "sensibleHeat", "latentHeat", "liquid")
(SWE, ICE_CONTENT, LW_CONTENT, INTERNAL_ENERGY, SURFACE_ENERGY, SURFACE_TEMP, AGE_OF_SNOW) = range(7)
(SNOW_FALL, SNOW_MELT, DELTA_SWE, SENSIBLE_HEAT, LATENT_HEAT, LIQUID_WATER) = range(6)
INPUT = ("airT", "prec", "relHum", "windInt", "globalRad", "beamRad", "transmissivity", "surfaceWater")
# file names of saveSnowState / loadSnowState (criteria3DProject.cpp:2310-2380)
STATE_FILES = {"swe": "SWE", "age": "AgeOfSnow", "surfaceTemp": "SnowSurfaceTemp", "ice": "IceContent", "lwc": "LWContent",
               "internalEnergy": "InternalEnergy", "surfaceEnergy": "SurfaceInternalEnergy"}

PARAMETER_NAMES = ("skinThickness", "soilAlbedo", "snowVegetationHeight", "snowWaterHoldingCapacity", "tempMaxWithSnow", "tempMinWithRain",
                   "snowSurfaceDampingDepth")
DEFAULT_PARAMETERS = dict(skinThickness=0.02, soilAlbedo=0.2, snowVegetationHeight=1.0, snowWaterHoldingCapacity=0.05, tempMaxWithSnow=2.0,
                          tempMinWithRain=-0.5, snowSurfaceDampingDepth=0.05)      # initializeSnowParameters, snow.cpp:39-50


class Parameters(C.Structure):
    """sf3d_snow_parameters_t"""
    _fields_ = [(n, C.c_double) for n in PARAMETER_NAMES]


pparams = C.POINTER(Parameters)
# name -> (restype, argtypes): every symbol include/sf3d_snow.h declares
SIGNATURES = {
    "sf3d_snow_default_parameters": (capi.u8, [pparams]),
    "sf3d_snow_initialize": (capi.u8, [capi.u32, capi.u32, pf32, capi.f32, pparams]),
    "sf3d_snow_set_parameters": (capi.u8, [pparams]),
    "sf3d_snow_reset": (capi.u8, []),
    "sf3d_snow_set_state": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_snow_get_state": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_snow_get_output": (capi.u8, [capi.i32, capi.u32, pf32]),
    "sf3d_snow_compute_hour": (capi.u8, [capi.u32, pf32, pf32, pf32, pf32, pf32, pf32, pf32, pf32, capi.f64]),
    "sf3d_snow_kernel_ms": (capi.f64, []),
    "sf3d_snow_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_snow.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

_f32 = partial(raster.f32, what="snow")
_index = raster.index


def _params(parameters) -> Parameters:
    p = dict(DEFAULT_PARAMETERS)
    p.update(parameters or {})
    return Parameters(*(float(p[n]) for n in PARAMETER_NAMES))


def initialize(sf: capi.SF3D, dem, flag: float = NODATA, parameters: dict | None = None) -> None:
    """initializeSnowMaps + resetSnowModel on the cells of `dem` [rows, cols] that do not hold `flag`: SWE 0, surface 5.0 degC, pack
    3.4 degC"""
    bind(sf)
    dem = _f32(dem)
    sf._snow_shape = dem.shape
    sf.check(sf.lib.sf3d_snow_initialize(dem.shape[0], dem.shape[1], dem.ctypes.data_as(pf32), float(flag), C.byref(_params(parameters))),
             "snow_initialize")


def set_parameters(sf: capi.SF3D, parameters: dict) -> None:
    sf.check(sf.lib.sf3d_snow_set_parameters(C.byref(_params(parameters))), "snow_set_parameters")


def reset(sf: capi.SF3D) -> None:
    """resetSnowModel on the SWE map the device holds (after a hand-edited SWE map)"""
    sf.check(sf.lib.sf3d_snow_reset(), "snow_reset")


def set_state(sf: capi.SF3D, which, values) -> None:
    v = _f32(values, sf._snow_shape)
    sf.check(sf.lib.sf3d_snow_set_state(_index(which, STATE), v.size, v.ctypes.data_as(pf32)), f"snow_set_state({which})")


def get_state(sf: capi.SF3D, which) -> np.ndarray:
    out = np.empty(sf._snow_shape, np.float32)
    sf.check(sf.lib.sf3d_snow_get_state(_index(which, STATE), out.size, out.ctypes.data_as(pf32)), f"snow_get_state({which})")
    return out


def get_output(sf: capi.SF3D, which) -> np.ndarray:
    out = np.empty(sf._snow_shape, np.float32)
    sf.check(sf.lib.sf3d_snow_get_output(_index(which, OUTPUT), out.size, out.ctypes.data_as(pf32)), f"snow_get_output({which})")
    return out


def all_maps(sf: capi.SF3D) -> dict:
    """the seven state maps and the six outputs, by name"""
    d = {n: get_state(sf, n) for n in STATE}
    d.update({n: get_output(sf, n) for n in OUTPUT})
    return d


def compute_hour(sf: capi.SF3D, meteo: dict) -> None:
    """one hour of the snow model on the device.  meteo: the float maps "airT", "prec", "relHum", "windInt", "globalRad", "beamRad",
    "transmissivity", optionally "surfaceWater" [mm] (the application passes 0), and the scalar "clearSkyTransmissivity"."""
    maps = [_f32(meteo[n], sf._snow_shape) for n in INPUT[:7]]
    water = _f32(meteo["surfaceWater"], sf._snow_shape) if meteo.get("surfaceWater") is not None else None
    ptrs = [m.ctypes.data_as(pf32) for m in maps] + [water.ctypes.data_as(pf32) if water is not None else pf32()]
    sf.check(sf.lib.sf3d_snow_compute_hour(maps[0].size, *ptrs, float(meteo["clearSkyTransmissivity"])), "snow_compute_hour")


def clean(sf: capi.SF3D) -> None:
    sf.check(sf.lib.sf3d_snow_clean(), "snow_clean")


# ------------------------------------------------------------------------------------------------ host plumbing

def surface_sources(model, liquid_mm, flag: float = NODATA) -> np.ndarray:
    """the per-node source [m3 s-1] of assignPrecipitation (criteria3DProject.cpp:954-964) for a liquid-water map [mm], WITHOUT soil
    cracking (computeSoilCracking stays with the caller: precSurfaceWater = liquidWater): on the surface node of every cell whose
    liquid water is > 0, area * (mm / 1000.) / 3600. - the float map value divided by the double 1000., as there; 0 elsewhere (flag
    cells, cells without a node).  Ready for set_nodes_water_sink_source / set_sink_source_bulk."""
    idx = np.asarray(model.meta["index"])[0]
    liquid = np.asarray(liquid_mm, dtype=np.float32)
    if liquid.shape != idx.shape:
        raise ValueError(f"liquid-water map of shape {liquid.shape}, the index map is {idx.shape}")
    cell = float(model.meta["cell"])
    area = cell * cell                                          # DEM.header->cellSize squared
    q = np.zeros(model.n, np.float64)
    ok = (idx >= 0) & ~(np.abs(liquid.astype(np.float64) - float(np.float32(flag))) < EPSILON) & (liquid > 0)
    flow = area * (liquid[ok].astype(np.float64) / 1000.0)
    rate = flow / 3600.0
    nodes = idx[ok]
    pos = rate > 0.0
    q[nodes[pos]] = rate[pos]
    return q


def save_snow_state(sf: capi.SF3D, directory, header: dict) -> Path:
    """saveSnowState: <directory>/snow/{SWE, AgeOfSnow, SnowSurfaceTemp, IceContent, LWContent, InternalEnergy, SurfaceInternalEnergy}.flt/.hdr"""
    return raster.save_state(directory, "snow", STATE_FILES, partial(get_state, sf), header)


def load_snow_state(sf: capi.SF3D, directory) -> None:
    """loadSnowState: the seven maps of <directory>/snow onto the device (the raster must be initialised with the same DEM)"""
    raster.load_state(directory, "snow", STATE_FILES, partial(set_state, sf))


# ------------------------------------------------------------------------------------------------ restatement (checker)

# snow.h / commonConstants.h
SNOW_EMISSIVITY, SOIL_EMISSIVITY = 0.97, 0.92
THERMO_WATER_VAPOR = 0.4615
LATENT_HEAT_FUSION_KJ, LATENT_HEAT_VAPORIZATION_KJ = 335.0, 2500.0
SNOW_SPECIFIC_HEAT, SOIL_SPECIFIC_HEAT = 2.1, 1.4
DEFAULT_BULK_DENSITY = 1350
SOIL_DAMPING_DEPTH = 0.3
SNOW_MINIMUM_HEIGHT = 1.0
WATER_DENSITY = 1000.0
ZEROCELSIUS = 273.15
STEFAN_BOLTZMANN = 5.670373E-8
VON_KARMAN_CONST = 0.41
HEAT_CAPACITY_WATER, HEAT_CAPACITY_AIR, HEAT_CAPACITY_SNOW = 4182000.0, 1290.0, 2100000.0
# snow.cpp:482 reads `snowWaterEquivalent` without the underscore: not the state but the meteoVariable enumerator of that name
# (agrolib/meteo/meteo.h:103), 56 in the compiled reference (recorded in the pin).  Kept: it is part of the result.
SNOW_WATER_EQUIVALENT_ENUM = 56
INIT_SOIL_PACK_TEMP, INIT_SNOW_SURFACE_TEMP = 3.4, 5.0        # snowMaps.cpp:98-99


def _eq(a: float, b: float) -> bool:
    return abs(a - b) < EPSILON                                 # isEqual, basicMath.h:25-29


def _cmin(a, b):
    return b if b < a else a                                    # std::min


def _cmax(a, b):
    return b if a < b else a                                    # std::max


def _pow(x: float, y: float) -> float:
    if x == 0.0 and y < 0.0:
        return math.inf                                         # C's pow(0, negative); python raises instead
    return math.pow(x, y)


def t_dew_from_rel_hum(rh: float, t: float) -> float:
    """tDewFromRelHum(double, double), agrolib/meteo/meteo.cpp:288-298"""
    if _eq(rh, NODATA) or _eq(t, NODATA) or rh == 0:
        return NODATA
    rh = 100 if 100 < rh else rh
    sat = math.exp((16.78 * t - 116.9) / (t + 237.3))
    actual = rh / 100.0 * sat
    return (math.log(actual) * 237.3 + 116.9) / (16.78 - math.log(actual))


def aerodynamic_resistance(is_snow: bool, z_ref_wind: float, wind: float, veg_height: float) -> float:
    """aerodynamicResistanceCampbell77, snow.cpp:527-557"""
    z_ref_temp = 2.0
    wind = _cmax(wind, 0.05)
    wind = _cmin(wind, 10.0)
    veg_height = _cmax(veg_height, 0.01)
    if is_snow:
        zero_plane, roughness = 0.0, 0.001
    else:
        zero_plane, roughness = 0.64 * veg_height, 0.13 * veg_height
    a = z_ref_wind - zero_plane
    log1 = math.log(((a if a > 1.0 else 1.0) + roughness) / roughness)
    heat = 0.2 * roughness
    b = z_ref_temp - zero_plane
    log2 = math.log(((b if b > 1.0 else 1.0) + heat) / heat)
    return log1 * log2 / (VON_KARMAN_CONST * VON_KARMAN_CONST * wind)


def surface_energy_snow(t, skin):
    return t * WATER_DENSITY * SNOW_SPECIFIC_HEAT * skin


def surface_energy_soil(t, skin):
    return t * DEFAULT_BULK_DENSITY * SOIL_SPECIFIC_HEAT * skin


def internal_energy(t, bulk_density, swe):
    return t * (WATER_DENSITY * SNOW_SPECIFIC_HEAT * swe * 0.001 + bulk_density * SOIL_SPECIFIC_HEAT * SOIL_DAMPING_DEPTH)


def restate_reset(swe, flag: float = NODATA, parameters: dict | None = None) -> dict:
    """resetSnowModel (snowMaps.cpp:177-218) on a float SWE map -> the twelve maps of the application (flag cells untouched: flag)"""
    p = dict(DEFAULT_PARAMETERS); p.update(parameters or {})
    swe = np.asarray(swe, np.float32)
    f32 = np.float32
    m = {n: np.full(swe.shape, f32(flag), np.float32) for n in STATE + OUTPUT[:5]}
    m["swe"] = swe.copy()
    for c in np.ndindex(swe.shape):
        s = swe[c]
        if _eq(float(s), float(f32(flag))):
            continue
        m["ice"][c] = s
        m["lwc"][c] = 0
        m["age"][c] = NODATA
        m["surfaceTemp"][c] = f32(INIT_SNOW_SURFACE_TEMP)
        m["surfaceEnergy"][c] = f32(surface_energy_snow(INIT_SNOW_SURFACE_TEMP, p["skinThickness"]) if s > 0
                                    else surface_energy_soil(INIT_SNOW_SURFACE_TEMP, p["skinThickness"]))
        m["internalEnergy"][c] = f32(internal_energy(INIT_SOIL_PACK_TEMP, DEFAULT_BULK_DENSITY, float(s) / 1000.))
        for n in OUTPUT[:5]:
            m[n][c] = 0
    return m


def snow_point(state, inp, clear_sky: float, p: dict):
    """computeSnowPoint for one cell: state = the seven floats of the maps (widened), inp = the eight float inputs (widened) ->
    (seven state doubles, five output doubles as the getters return them).  snow.cpp:92-516."""
    swe, ice, lwc, ie, se, ts, age = state
    air_t, prec, rh, wind, glob, beam, trans, water = inp
    water = _cmax(water, 0.0)
    invalid = (_eq(air_t, NODATA) or _eq(prec, NODATA) or _eq(glob, NODATA) or _eq(beam, NODATA) or _eq(swe, NODATA) or _eq(ts, NODATA))
    if water > 100.0 or invalid:
        # the internal energy keeps its value; getSnowMelt is MAXVALUE(_snowMelt, 0): 0, not NODATA
        return (NODATA, NODATA, NODATA, ie, NODATA, NODATA, NODATA), (NODATA, 0.0, NODATA, NODATA, NODATA)

    # computeSnowFall
    liquid = prec
    if liquid > 0:
        if air_t <= p["tempMinWithRain"]:
            liquid = 0
        elif air_t < p["tempMaxWithSnow"]:
            liquid *= (air_t - p["tempMinWithRain"]) / (p["tempMaxWithSnow"] - p["tempMinWithRain"])
    d = prec - liquid
    prec_snow = d if d > 0 else 0.0
    prec_rain = liquid

    dew = t_dew_from_rel_hum(rh, air_t)
    if not _eq(trans, NODATA):
        cloud = 1 - _cmin(trans / clear_sky, 1.0)
    else:
        cloud = 0.1

    max_snow_height = swe * 10 / 1000
    height_veg = p["snowVegetationHeight"] - max_snow_height
    shadow = _cmax(_cmin(height_veg / 4, 1.0), 0.0)
    solar = glob - beam * shadow

    prev_swe, prev_ie, prev_se, prev_ts, prev_ice, prev_lw = swe, ie, se, ts, ice, lwc
    whc = p["snowWaterHoldingCapacity"]
    if prev_swe > 0:
        if prev_ice <= 0 and prev_lw <= 0:
            prev_ice = prev_swe
            prev_lw = prev_swe * whc / (1 - whc)
            prev_ie = -prev_swe * 0.001 * LATENT_HEAT_FUSION_KJ * WATER_DENSITY
            prev_ts = _cmin(prev_ts, 0.0)
            prev_se = surface_energy_snow(prev_ts, _cmin(prev_swe, p["skinThickness"]))
            age = 1
        ratio = prev_swe / (prev_ice + prev_lw)
        if not _eq(ratio, 1):
            prev_ice = prev_ice * ratio
            prev_lw = prev_lw * ratio
    else:
        prev_ice = 0
        prev_lw = 0
        age = NODATA

    if prev_swe < EPSILON:
        est = prev_ts * DEFAULT_BULK_DENSITY * SOIL_SPECIFIC_HEAT * SOIL_DAMPING_DEPTH
        if abs(est - prev_ie) > 1000:
            if _eq(est, 0):
                est = EPSILON
            r = prev_ie / est
            if r < 0.5 or r > 2:
                prev_ie = (prev_ie + est) * 0.5

    resistance = aerodynamic_resistance(prev_swe > SNOW_MINIMUM_HEIGHT, 10, wind, p["snowVegetationHeight"])

    air_vap = math.exp((16.78 * dew - 116.9) / (dew + 237.3)) / ((ZEROCELSIUS + dew) * THERMO_WATER_VAPOR)
    water_vap = math.exp((16.78 * prev_ts - 116.9) / (prev_ts + 237.3)) / ((ZEROCELSIUS + prev_ts) * THERMO_WATER_VAPOR)

    emissivity_atm = (0.72 + 0.005 * air_t) * (1.0 - 0.84 * cloud) + 0.84 * cloud

    if not _eq(age, NODATA):
        albedo = _cmin(0.9, 0.74 * _pow(age, -0.191))
    else:
        albedo = p["soilAlbedo"]

    q_prec_w = (HEAT_CAPACITY_WATER / 1000.) * (prec_rain / 1000.) * (_cmax(0., air_t) - prev_ts)
    q_prec_s = (HEAT_CAPACITY_SNOW / 1000.) * (prec_snow / 1000.) * (_cmin(0., air_t) - prev_ts)
    q_prec = q_prec_w + q_prec_s
    q_water_heat = (HEAT_CAPACITY_WATER / 1000.) * (water / 1000.) * (_cmax(1., (prev_ts + air_t) / 2.) - prev_ts)
    q_water_kinetic = 0
    q_solar = (1. - albedo) * (solar * 3600.) / 1000.
    emissivity = SNOW_EMISSIVITY if prev_swe > SNOW_MINIMUM_HEIGHT else SOIL_EMISSIVITY
    # both pow(x, 4.0) are calls of the library's pow in the compiled reference (gcc -O2 folds pow(x, 2) only)
    q_long = STEFAN_BOLTZMANN * 3.6 * (emissivity_atm * _pow(air_t + ZEROCELSIUS, 4.0) - emissivity * _pow(prev_ts + ZEROCELSIUS, 4.0))
    q_temp = 3600. * (HEAT_CAPACITY_AIR / 1000.) * (air_t - prev_ts) / resistance
    q_vap = 3600. * (LATENT_HEAT_VAPORIZATION_KJ + LATENT_HEAT_FUSION_KJ) * (air_vap - water_vap) / resistance
    if prev_swe < EPSILON:
        q_vap *= 0.4
    q_total = q_solar + q_prec + q_long + q_temp + q_vap + q_water_heat + q_water_kinetic
    sensible, latent = q_temp, q_vap

    sublimation = 0
    if prev_swe > EPSILON:
        sublimation = q_vap / (LATENT_HEAT_FUSION_KJ + LATENT_HEAT_VAPORIZATION_KJ)
        if sublimation < 0:
            sublimation = -_cmin(abs(sublimation), prev_swe + prec_snow)

    freeze_melt = 0
    w = (prev_ie + q_total) / (LATENT_HEAT_FUSION_KJ * WATER_DENSITY)
    if w < 0:
        if prev_ts <= 0:
            freeze_melt = _cmin(prev_lw + prec_rain, -w * 1000.)
    elif w > 0:
        freeze_melt = -_cmin(prev_ice + prec_snow + sublimation, w * 1000.)
    snow_melt = -freeze_melt
    qr = (freeze_melt / 1000.) * LATENT_HEAT_FUSION_KJ * WATER_DENSITY
    ie = prev_ie + q_total + qr

    if ie > EPSILON:
        ice = 0
    else:
        ice = prev_ice + prec_snow + sublimation + freeze_melt
        ice = _cmax(ice, 0.)
    holding = whc / (1 - whc)
    if ie > EPSILON:
        lwc = 0
    else:
        lwc = prev_lw + prec_rain + water - freeze_melt
        lwc = _cmax(lwc, 0.)
        lwc = _cmin(lwc, ice * holding)
    swe = ice + lwc
    delta = swe - prev_swe

    skin = p["skinThickness"]
    if swe > 0 and abs(ie) < EPSILON:
        se_snow = 0.
    else:
        snow_ratio = _cmin(SNOW_WATER_EQUIVALENT_ENUM * 0.001, skin) / p["snowSurfaceDampingDepth"]
        se_snow = _cmin(0., prev_se + (q_total + qr) * snow_ratio)
    ts_snow = se_snow / (WATER_DENSITY * SNOW_SPECIFIC_HEAT * skin)
    se_soil = prev_se + (q_total + qr) * (skin / SOIL_DAMPING_DEPTH)
    ts_soil = se_soil / (DEFAULT_BULK_DENSITY * SOIL_SPECIFIC_HEAT * skin)
    fraction = _cmin(swe * 4. / 1000., skin) / skin
    se = (se_snow * fraction) + se_soil * (1 - fraction)
    ts = (ts_snow * fraction) + ts_soil * (1 - fraction)

    if swe > EPSILON:
        if age == NODATA or prec_snow > 0.1:
            age = 0
        else:
            age += 1. / 24.
    else:
        age = NODATA
    return (swe, ice, lwc, ie, se, ts, age), (prec_snow, snow_melt if snow_melt > 0 else 0.0, delta, sensible, latent)


def restate_snow_hour(state: dict, meteo: dict, dem, flag: float = NODATA, parameters: dict | None = None) -> dict:
    """one hour of computeSnowModel + the liquid-water map of assignPrecipitation on float maps: state = the seven maps by name (the other
    keys are ignored), meteo as for compute_hour -> all thirteen maps (new arrays).  State is rounded to float every hour, as the
    application's maps do."""
    p = dict(DEFAULT_PARAMETERS); p.update(parameters or {})
    dem = np.asarray(dem, np.float32)
    f32 = np.float32
    fl = float(f32(flag))
    st = [np.asarray(state[n], np.float32).astype(np.float64) for n in STATE]
    water = meteo.get("surfaceWater")
    inp = [np.asarray(meteo[n], np.float32).astype(np.float64) for n in INPUT[:7]] + \
          [np.asarray(water, np.float32).astype(np.float64) if water is not None else np.zeros(dem.shape)]
    clear = float(meteo["clearSkyTransmissivity"])
    out = {n: np.empty(dem.shape, np.float32) for n in STATE + OUTPUT}
    names = STATE + OUTPUT[:5]
    prec32 = np.asarray(meteo["prec"], np.float32)
    for c in np.ndindex(dem.shape):
        if _eq(float(dem[c]), fl):
            for n in STATE + OUTPUT:
                out[n][c] = fl
            continue
        s, o = snow_point([float(a[c]) for a in st], [float(a[c]) for a in inp], clear, p)
        with np.errstate(over="ignore"):
            for n, v in zip(names, s + o):
                out[n][c] = f32(v)
        pr = prec32[c]
        if _eq(float(pr), fl):
            out["liquid"][c] = fl
        else:
            fall, melt = out["snowFall"][c], out["snowMelt"][c]
            liquid = pr
            if not _eq(float(fall), fl) and not _eq(float(melt), fl):
                liquid = f32(f32(pr - fall) + melt)
            out["liquid"][c] = liquid
    return out
