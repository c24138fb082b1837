"""The hourly water sinks on the device (include/sf3d_sink.h, criteria3d_amd/csrc/sf3d_sink.inc): the cell loop of
`Crit3DProject::assignETreal` (bin/CRITERIA3D/criteria3DProject.cpp:796-911) around `Project3D::assignEvaporation`
(src/project3D/project3D.cpp:2377-2451) and `Project3D::assignTranspiration` (:2461-2610), and the rain term of `assignPrecipitation`
(criteria3DProject.cpp:939-964), with `Crit3DProject::computeSoilCracking` (:978-1123) as an option (`set_cracking`).

Three parts:
  * the binding (`bind`, `initialize`, `compute_hour`, `get_node_sinks`, `get_actual`, `apply` ...): k_sink_hour reads ET0, LAI and degree
    days from the crop block, the liquid water from the snow block, the roots from the root block and the water content from the solver's
    accepted state, all on the device; a missing kernel or library is an error;
  * `sink_hour`: root compute -> sink compute -> apply, the hour's hand-over to the solver;
  * `restate_sink_hour` (and `evaporation_coefficients`, `horizon_table`): both functions and the rain term in plain Python doubles with
    the reference's operation order, the C library's exp (python's `math`) and layerTranspiration rounded to float - the checker of the
    CPU tests against the compiled-reference pin (tests/golden/water_sinks.npz).  A checker, never a fallback;
  * `crack_tables` and `restate_soil_cracking`: the host part and the per-cell part of computeSoilCracking restated, the checker of
    tests/golden/soil_cracking.npz; `restate_sink_hour(..., cracking=...)` calls the second in the rain term."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi, maps, raster, root
from .capi import pf32, pf64, pi32

NODATA = -9999
EPSILON = 0.00001                               # commonConstants.h:252
DBL_EPSILON = 2.220446049250313e-16
MAX_EVAPORATION_DEPTH = 0.25                    # commonConstants.h:116
MAX_UNITS = root.MAX_UNITS
MAX_SOILS = root.MAX_SOILS
MAX_HORIZONS = root.MAX_HORIZONS
MAX_LAYERS = root.MAX_LAYERS
HORIZON_FIELDS = ("upperDepth", "lowerDepth", "waterContentHH", "waterContentFC", "waterContentWP", "waterContentSAT", "soilFraction")


class Unit(C.Structure):
    """sf3d_sink_unit_t"""
    _fields_ = [("kcMax", C.c_double), ("fRAW", C.c_double), ("isWaterSurplusResistant", C.c_int32), ("reserved", C.c_int32)]


class Soil(C.Structure):
    """sf3d_sink_soil_t"""
    _fields_ = [("nrHorizons", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_double * MAX_HORIZONS) for n in HORIZON_FIELDS]


CRACK_FIELDS = ("clay", "silt", "coarseFragments", "organicMatter")
MAX_CRACKING_DEPTH = 0.6                        # criteria3DProject.cpp:980-985
MIN_FINE_LAYER_DEPTH = 0.2
MIN_VOID_VOLUME = 0.15
MAX_VOID_VOLUME = 0.20
MIN_FINE_FRACTION = 0.5
MAX_STORAGE = 0.05


class CrackSoil(C.Structure):
    """sf3d_sink_crack_soil_t"""
    _fields_ = [("nrHorizons", C.c_int32), ("reserved", C.c_int32), ("totalDepth", C.c_double)] + [(n, C.c_double * MAX_HORIZONS) for n in CRACK_FIELDS]


punit = C.POINTER(Unit)
psoil = C.POINTER(Soil)
pcrack = C.POINTER(CrackSoil)
# name -> (restype, argtypes): every symbol include/sf3d_sink.h declares
SIGNATURES = {
    "sf3d_sink_initialize": (capi.u8, [capi.u32, capi.u32, pf32, capi.f32, capi.f64, capi.u32, pf64, pf64, capi.f64, pi32, pi32, capi.u32, punit, capi.u32, psoil]),
    "sf3d_sink_get_tables": (capi.u8, [pf64, pf64, pi32, pi32]),
    "sf3d_sink_compute_hour": (capi.u8, [capi.u32, pf32, pf32, pf32, pf32]),
    "sf3d_sink_get_node_sinks": (capi.u8, [capi.u32, pf64]),
    "sf3d_sink_get_actual": (capi.u8, [capi.u32, pf64, pf64]),
    "sf3d_sink_apply": (capi.u8, []),
    "sf3d_sink_set_cracking": (capi.u8, [capi.u32, pcrack]),
    "sf3d_sink_get_crack_tables": (capi.u8, [pf64, pi32]),
    "sf3d_sink_get_crack": (capi.u8, [capi.u32, pf32, pf64]),
    "sf3d_sink_kernel_ms": (capi.f64, []),
    "sf3d_sink_clean": (capi.u8, []),
}


def bind(sf: capi.SF3D) -> capi.SF3D:
    """attach the signatures of include/sf3d_sink.h to a loaded product library (AttributeError if a symbol is missing)"""
    return capi.bind_signatures(sf, SIGNATURES)


# ------------------------------------------------------------------------------------------------ binding

def unit_array(units):
    """list of dicts (kcMax, fRAW, isWaterSurplusResistant) -> ctypes array of sf3d_sink_unit_t"""
    arr = (Unit * max(len(units), 1))()
    for k, u in enumerate(units):
        arr[k].kcMax, arr[k].fRAW, arr[k].isWaterSurplusResistant = float(u["kcMax"]), float(u["fRAW"]), int(bool(u["isWaterSurplusResistant"]))
    return arr


def soil_array(soils):
    """list of dicts (HORIZON_FIELDS: one list per field) -> ctypes array of sf3d_sink_soil_t"""
    arr = (Soil * max(len(soils), 1))()
    for k, s in enumerate(soils):
        nh = len(s["upperDepth"])
        if nh > MAX_HORIZONS:
            raise ValueError(f"soil {k}: {nh} horizons, the cap is {MAX_HORIZONS}")
        arr[k].nrHorizons = nh
        for name in HORIZON_FIELDS:
            for h in range(nh):
                getattr(arr[k], name)[h] = float(s[name][h])
    return arr


def initialize(sf: capi.SF3D, dem, cell_size, crop_index, soil_index, units, soils, layer_depth, layer_thickness, computation_depth, flag: float = -9999.0):
    """sf3d_sink_initialize: needs no device (the first hour uploads the tables); keeps the raster's shape on `sf`"""
    bind(sf)
    dem = np.ascontiguousarray(dem, np.float32)
    ci, si = raster.i32(crop_index, dem.shape, "sink"), raster.i32(soil_index, dem.shape, "sink")
    ld, lt = np.ascontiguousarray(layer_depth, np.float64), np.ascontiguousarray(layer_thickness, np.float64)
    ua, sa = unit_array(units), soil_array(soils)
    sf.check(sf.lib.sf3d_sink_initialize(dem.shape[0], dem.shape[1], dem.ctypes.data_as(pf32), float(flag), float(cell_size), len(ld), ld.ctypes.data_as(pf64),
                                         lt.ctypes.data_as(pf64), float(computation_depth), ci.ctypes.data_as(pi32), si.ctypes.data_as(pi32), len(units), ua,
                                         len(soils), sa), "sink_initialize")
    sf._sink_shape, sf._sink_layers, sf._sink_soils = dem.shape, len(ld), len(soils)


def set_columns(sf: capi.SF3D, columns, layer_thickness):
    """sf3d_set_output_columns (the column table the sink call reads): columns[layer][row][col] = node, -1 where there is none"""
    maps.set_columns(sf, columns, layer_thickness)


def get_tables(sf: capi.SF3D):
    """what the host evaluated: evapCoeff, layerEvapCoeff, lastEvapLayer and the [soil][layer] horizon table (-9999: none)"""
    nl, ns = sf._sink_layers, sf._sink_soils
    ec, lec, hz = np.zeros(nl), np.zeros(nl), np.zeros((ns, nl), np.int32)
    last = C.c_int32(0)
    sf.check(sf.lib.sf3d_sink_get_tables(ec.ctypes.data_as(pf64), lec.ctypes.data_as(pf64), C.byref(last), hz.ctypes.data_as(pi32)), "sink_get_tables")
    return dict(evap_coeff=ec, layer_evap_coeff=lec, last_evap_layer=int(last.value), horizon=hz)


def compute_hour(sf: capi.SF3D, et0=None, lai=None, degree_days=None, liquid_water=None):
    """sf3d_sink_compute_hour: a map left None is read from the crop block (ET0, LAI, degree days) / the snow block (liquid water)"""
    shape = sf._sink_shape
    given = [None if m is None else raster.f32(m, shape, "sink") for m in (et0, lai, degree_days, liquid_water)]
    sf.check(sf.lib.sf3d_sink_compute_hour(shape[0] * shape[1], *[None if m is None else m.ctypes.data_as(pf32) for m in given]), "sink_compute_hour")


def get_node_sinks(sf: capi.SF3D, n_nodes: int) -> np.ndarray:
    out = np.empty(n_nodes, np.float64)
    sf.check(sf.lib.sf3d_sink_get_node_sinks(n_nodes, out.ctypes.data_as(pf64)), "sink_get_node_sinks")
    return out


def get_actual(sf: capi.SF3D):
    """(actual evaporation, actual transpiration) [mm], the flag where the cell was not computed"""
    shape = sf._sink_shape
    e, t = np.empty(shape, np.float64), np.empty(shape, np.float64)
    sf.check(sf.lib.sf3d_sink_get_actual(e.size, e.ctypes.data_as(pf64), t.ctypes.data_as(pf64)), "sink_get_actual")
    return e, t


def apply(sf: capi.SF3D):
    sf.check(sf.lib.sf3d_sink_apply(), "sink_apply")


def crack_soil_array(crack_soils):
    """list of dicts (totalDepth; CRACK_FIELDS: one list per field) -> ctypes array of sf3d_sink_crack_soil_t (no check of the cap: the
    library refuses more horizons than it holds)"""
    arr = (CrackSoil * max(len(crack_soils), 1))()
    for k, s in enumerate(crack_soils):
        nh = len(s["clay"])
        arr[k].nrHorizons, arr[k].totalDepth = nh, float(s["totalDepth"])
        for name in CRACK_FIELDS:
            for h in range(min(nh, MAX_HORIZONS)):
                getattr(arr[k], name)[h] = float(s[name][h])
    return arr


def set_cracking(sf: capi.SF3D, crack_soils=None):
    """sf3d_sink_set_cracking: soil cracking (computeSoilCracking) for the hours that follow; None or an empty list turns it off"""
    bind(sf)
    if not crack_soils:
        sf.check(sf.lib.sf3d_sink_set_cracking(0, None), "sink_set_cracking")
        return
    sf.check(sf.lib.sf3d_sink_set_cracking(len(crack_soils), crack_soil_array(crack_soils)), "sink_set_cracking")


def get_crack_tables(sf: capi.SF3D):
    """what the host evaluated per soil: (maxDepth [m], lastLayer), -9999 where the soil never cracks"""
    ns = sf._sink_soils
    md, ll = np.zeros(ns), np.zeros(ns, np.int32)
    sf.check(sf.lib.sf3d_sink_get_crack_tables(md.ctypes.data_as(pf64), ll.ctypes.data_as(pi32)), "sink_get_crack_tables")
    return md, ll


def get_crack(sf: capi.SF3D):
    """(precSurfaceWater [mm] float32: what computeSoilCracking returned, crackWater [mm]: what went into the crack's nodes), the flag where
    the cell was not computed"""
    shape = sf._sink_shape
    p, w = np.empty(shape, np.float32), np.empty(shape, np.float64)
    sf.check(sf.lib.sf3d_sink_get_crack(p.size, p.ctypes.data_as(pf32), w.ctypes.data_as(pf64)), "sink_get_crack")
    return p, w


def kernel_ms(sf: capi.SF3D) -> float:
    return float(sf.lib.sf3d_sink_kernel_ms())


def clean(sf: capi.SF3D):
    bind(sf)
    sf.check(sf.lib.sf3d_sink_clean(), "sink_clean")


def sink_hour(sf: capi.SF3D, degree_days=None, et0=None, lai=None, liquid_water=None):
    """the hour's hand-over: the roots of the hour, the sinks from them, and the sinks into the solver's staging model (the next
    computeStep uploads them).  Maps left None are the crop / snow block's."""
    root.compute(sf, degree_days)
    compute_hour(sf, et0, lai, degree_days, liquid_water)
    apply(sf)


# ------------------------------------------------------------------------------------------------ restatement (a checker)

def _f32(x) -> float:
    return float(np.float32(x))


def evaporation_coefficients(layer_depth, layer_thickness, computation_depth):
    """initializeEvaporationCoefficient (project3D.cpp:2331-2368): (evapCoeff, layerEvapCoeff, lastEvapLayer), the vectors as long as the
    layer grid and 0 beyond lastEvapLayer; None when the reference returns false"""
    nl = len(layer_depth)

    def layer_index(depth):                      # getSoilLayerIndex :1764-1776
        if nl == 0 or depth < 0:
            return NODATA
        for layer in range(nl):
            if depth <= layer_depth[layer] + layer_thickness[layer] * 0.5:
                return layer
        return NODATA
    last = layer_index(MAX_EVAPORATION_DEPTH)
    if computation_depth < MAX_EVAPORATION_DEPTH:
        last = layer_index(computation_depth)
    if last == NODATA:
        return None
    ec, lec = [0.0] * nl, [0.0] * nl
    coeff_sum = 0.0
    for layer in range(1, last + 1):
        depth_coeff = max((layer_depth[layer] - layer_depth[1]) / (MAX_EVAPORATION_DEPTH - layer_depth[1]), 0.0)
        ec[layer] = math.exp(-2 * depth_coeff)
        lec[layer] = ec[layer] * (layer_thickness[layer] / 0.04)
        coeff_sum += lec[layer]
    if last >= 1:
        inv = 1.0 / coeff_sum
        for layer in range(1, last + 1):
            lec[layer] *= inv
    return np.array(ec), np.array(lec), last


def horizon_table(soils, layer_depth):
    """[soil][layer]: Crit3DSoil::getHorizonIndex(layerDepth[layer]) (soil.cpp:192-201), -9999 where there is none"""
    t = np.full((len(soils), len(layer_depth)), NODATA, np.int32)
    for s, so in enumerate(soils):
        for layer, d in enumerate(layer_depth):
            for h in range(len(so["upperDepth"])):
                if d >= so["upperDepth"][h] and d <= so["lowerDepth"][h] + EPSILON:
                    t[s, layer] = h
                    break
    return t


def crack_tables(soils, crack_soils, layer_depth, layer_thickness, computation_depth, reasons=None):
    """The part of computeSoilCracking that depends on the soil and the layer grid only (criteria3DProject.cpp:1003-1035, :1078; the layer
    index by getSoilLayerIndex, project3D.cpp:1764-1776): (maxDepth, lastLayer) per soil, -9999 where the soil never cracks.  `soils`: the
    sink soils (upperDepth, lowerDepth); `reasons`: a list that receives one arm name per soil."""
    nl = len(layer_depth)
    max_depth_of, last_layer_of = np.full(len(soils), float(NODATA)), np.full(len(soils), NODATA, np.int32)
    for s, (so, cs) in enumerate(zip(soils, crack_soils)):
        def never(why):
            if reasons is not None:
                reasons.append(why)
        soil_depth = min(computation_depth, cs["totalDepth"])
        if soil_depth <= MIN_FINE_LAYER_DEPTH:
            never("crack: soilDepth <= 0.2 by " + ("computationSoilDepth" if computation_depth <= MIN_FINE_LAYER_DEPTH else "totalDepth"))
            continue
        last_fine = NODATA
        max_depth = min(soil_depth, MAX_CRACKING_DEPTH)
        h = 0
        while h < len(cs["clay"]) and so["upperDepth"][h] < max_depth:
            fine = (cs["clay"][h] + cs["silt"][h] * 0.5) / 100 * (1 - cs["coarseFragments"][h]) * (1 - cs["organicMatter"][h])
            if fine < MIN_FINE_FRACTION:
                break
            last_fine = h
            h += 1
        ended_by_horizon = h < len(cs["clay"]) and so["upperDepth"][h] < max_depth
        if last_fine == NODATA:
            never("crack: first horizon not fine")
            continue
        max_depth = min(so["lowerDepth"][last_fine], MAX_CRACKING_DEPTH)
        max_depth = min(max_depth, computation_depth)
        if max_depth < MIN_FINE_LAYER_DEPTH:
            never("crack: fine horizon too thin")
            continue
        last_layer = NODATA
        if nl > 0 and max_depth >= 0:
            for layer in range(nl):
                if max_depth <= layer_depth[layer] + layer_thickness[layer] * 0.5:
                    last_layer = layer
                    break
        if last_layer == NODATA:
            never("crack: lastLayer NODATA")
            continue
        max_depth_of[s], last_layer_of[s] = max_depth, last_layer
        if reasons is not None:
            reasons.append("crack: fine down to MAX_CRACKING_DEPTH" if max_depth == MAX_CRACKING_DEPTH else
                           "crack: a second horizon ends the fine range" if ended_by_horizon and last_fine >= 0 else "crack: the soil ends the fine range")
    return max_depth_of, last_layer_of


def restate_soil_cracking(r, c, columns, water, max_water, minimum_pond, si, tables, soils, hz_of, layer_depth, layer_thickness, area, precipitation,
                          additions, hit, reasons=None):
    """The per-cell part of computeSoilCracking (criteria3DProject.cpp:988-1000, :1037-1122) behind crack_tables: `precipitation` a float32,
    `water` / `max_water`: getCriteria3DVar(volumetricWaterContent / maxVolumetricWaterContent) of a node, `minimum_pond`:
    getCriteria3DVar(surfacePond) of the surface node [mm].  Writes each filled node's flow rate into `additions`; returns (the function's
    float32, the water that went into the crack [mm])."""
    p = float(precipitation)
    nl = len(layer_depth)
    if si < 0:
        hit("crack: no soil index")
        return precipitation, 0.0
    if p <= minimum_pond:
        hit("crack: precipitation <= minimumPond")
        return precipitation, 0.0
    max_depth, last_layer = float(tables[0][si]), int(tables[1][si])
    if last_layer == NODATA:
        hit(reasons[si] if reasons else "crack: the soil never cracks")
        return precipitation, 0.0
    if reasons:
        hit(reasons[si])
    so = soils[si]

    def void_volume(layer):
        n = int(columns[layer][r][c])
        fraction = so["soilFraction"][int(hz_of[si, layer])]
        return max(0.0, max_water(n) - water(n)) * fraction
    crack_depth, voids_sum = 0.0, 0.0
    layer = 1
    while layer < nl and layer_depth[layer] <= max_depth:
        if int(columns[layer][r][c]) < 0:
            hit("crack: hole at layer 1" if layer == 1 else "crack: a hole inside the range")
            break
        if int(hz_of[si, layer]) == NODATA:
            hit("crack: horizon NODATA inside the range")
            break
        voids_sum += void_volume(layer) * layer_thickness[layer]
        crack_depth += layer_thickness[layer]
        layer += 1
    reached = layer
    if crack_depth == 0.0:
        hit("crack: crackDepth == 0")
        return precipitation, 0.0
    avg_void = voids_sum / crack_depth
    if avg_void <= MIN_VOID_VOLUME:
        hit("crack: avgVoidVolume <= 0.15")
        return precipitation, 0.0
    ratio = (avg_void - MIN_VOID_VOLUME) / (MAX_VOID_VOLUME - MIN_VOID_VOLUME)
    crack_ratio = 0.0 if ratio < 0.0 else (1.0 if 1.0 < ratio else ratio)
    hit("crack: crackRatio clamped to 1" if 1.0 < ratio else "crack: crackRatio inside (0, 1)" if 0.0 < ratio < 1.0 else "crack: crackRatio at a bound")
    max_infiltration = p * crack_ratio
    surface_water = max(p - max_infiltration, minimum_pond)
    if p - max_infiltration < minimum_pond:
        hit("crack: surfaceWater raised to minimumPond")
    potential = max(0.0, p - surface_water)
    residual = potential
    crack_water = 0.0
    capped = below = False
    broke = False
    for l in range(last_layer, 0, -1):
        if residual <= 0:
            broke = True
            break
        n = int(columns[l][r][c])
        if n < 0:
            continue
        void = void_volume(l) if l < reached else 0.0       # voidVolumeList is 0 where the first loop did not come
        storage = min(void, MAX_STORAGE)
        layer_water = min(layer_thickness[l] * 1000 * storage, residual)
        flow_rate = area * (layer_water / 1000.) / 3600.
        if flow_rate > 0.0:
            additions[n] = flow_rate
            residual -= layer_water
            crack_water += layer_water
            capped = capped or void > MAX_STORAGE
            below = below or void < MAX_STORAGE
    if capped and below:
        hit("crack: storage capped in one layer and below the cap in another")
    if broke:
        hit("crack: rain used up before layer 1")
    elif residual > 0:
        hit("crack: residual left after layer 1")
    return np.float32(surface_water + residual), crack_water


def _covered_surface_fraction(lai):
    return 0.0 if lai < EPSILON else 1 - math.exp(-0.6 * lai)


def restate_sink_hour(dem, flag, cell_size, columns, vwc, crop_index, soil_index, units, soils, layer_depth, layer_thickness, computation_depth,
                      et0, lai, degree_days, liquid_water, roots, n_nodes, arms=None, cracking=None):
    """One hour on plain doubles.  columns[layer][row][col]: the node, -1 where none; vwc[node]: getCriteria3DVar(volumetricWaterContent);
    roots: dict(length, first, last, density[layer]) of the hour (root.restate_root_maps or the root pin).  Returns dict(sinks_et: the
    node sinks after evaporation and transpiration, sinks: with the rain term, evaporation, transpiration).  `arms`: a dict that counts
    the (cell, hour) pairs per arm, for the tests.  `cracking`: None, or dict(crack_soils, max_vwc[node], pond[node]: getCriteria3DVar(
    maxVolumetricWaterContent / surfacePond [mm])) - then the rain term goes through restate_soil_cracking and the result also holds
    prec_surface_water (float32) and crack_water, the flag where the cell is not computed."""
    dem = np.asarray(dem, np.float32)
    rows, cols = dem.shape
    nl = len(layer_depth)
    fl = _f32(flag)
    area = float(cell_size) * float(cell_size)
    coeffs = evaporation_coefficients(layer_depth, layer_thickness, computation_depth)
    if coeffs is None:
        raise ValueError("initializeEvaporationCoefficient fails on this layer grid")
    evap_coeff, layer_evap_coeff, last_evap = coeffs
    hz_of = horizon_table(soils, layer_depth)
    sink = np.zeros(n_nodes, np.float64)
    rain = np.zeros(n_nodes, np.float64)
    evaporation = np.full(dem.shape, float(fl), np.float64)
    transpiration = np.full(dem.shape, float(fl), np.float64)

    def hit(name):
        if arms is not None:
            arms[name] = arms.get(name, 0) + 1

    def water(n):
        return float(NODATA) if n < 0 else float(vwc[n])

    if cracking is not None:
        reasons = []
        tables = crack_tables(soils, cracking["crack_soils"], layer_depth, layer_thickness, computation_depth, reasons)
        prec_surface = np.full(dem.shape, fl, np.float32)
        crack_water = np.full(dem.shape, float(fl), np.float64)

        def max_water(n):
            return float(NODATA) if n < 0 else float(cracking["max_vwc"][n])

    for r in range(rows):
        for c in range(cols):
            s0 = int(columns[0][r][c])
            if abs(float(dem[r, c]) - fl) < EPSILON or s0 < 0:
                continue
            si = int(soil_index[r][c])
            si = si if 0 <= si < len(soils) else -1
            e0 = float(np.float32(et0[r][c]))
            lai_map = np.float32(lai[r][c])
            current_lai = np.float32(0) if abs(float(lai_map) - fl) < EPSILON else lai_map
            la = float(current_lai)
            cov = _covered_surface_fraction(la)
            # ---- assignEvaporation
            evap_sum = 0.0
            max_evap = e0 * (1.0 - cov)
            if max_evap < EPSILON:
                hit("evaporation: maxEvaporation < EPSILON")
            else:
                surface_water = water(s0) * 1000
                surface_evap = min(max_evap, surface_water)
                surface_flow = area * (surface_evap / 1000.) / 3600.
                if surface_flow <= DBL_EPSILON:
                    surface_evap = 0.
                    hit("evaporation: surface flow <= DBL_EPSILON")
                else:
                    sink[s0] -= surface_flow
                    evap_sum += surface_evap
                    hit("evaporation: surface flow > DBL_EPSILON")
                residual = max_evap - surface_evap
                if residual < EPSILON:
                    hit("evaporation: residual < EPSILON")
                elif si < 0:
                    hit("evaporation: no soil")
                else:
                    it = 0
                    while residual > EPSILON and it < 3:
                        iteration_sum = 0.0
                        for layer in range(1, last_evap + 1):
                            n = int(columns[layer][r][c])
                            h = int(hz_of[si, layer])
                            if h == NODATA:
                                hit("evaporation: horizon NODATA")
                                continue
                            so = soils[si]
                            hh, fc = so["waterContentHH"][h], so["waterContentFC"][h]
                            threshold = hh + (1 - evap_coeff[layer]) * (fc - hh) * 0.5
                            layer_wc = water(n) * so["soilFraction"][h]
                            above = max(layer_wc - threshold, 0.0)
                            available = above * layer_thickness[layer] * 1000.
                            layer_evap = min(available, residual * layer_evap_coeff[layer])
                            if layer_evap > EPSILON:
                                flow = area * (layer_evap / 1000.) / 3600.
                                sink[n] -= flow
                                evap_sum += layer_evap
                                iteration_sum += layer_evap
                                hit("evaporation: layerEvaporation > EPSILON")
                            else:
                                hit("evaporation: layerEvaporation <= EPSILON")
                        residual -= iteration_sum
                        it += 1
                    hit(f"evaporation: loop ends after {it} iteration{'s' if it > 1 else ''}")
            evaporation[r, c] = evap_sum
            # ---- assignTranspiration behind the conditions of assignETreal
            transpiration[r, c] = _restate_transpiration(r, c, columns, water, int(crop_index[r][c]), si, units, soils, hz_of, nl, e0, current_lai, cov,
                                                         float(np.float32(degree_days[r][c])), roots, area, sink, hit)
            # ---- the rain term
            lw = np.float32(liquid_water[r][c])
            prec = lw
            if cracking is not None:
                prec_surface[r, c], crack_water[r, c] = lw, 0.0
            if not abs(float(lw) - fl) < EPSILON and lw > 0:
                if cracking is not None:
                    wet = [int(columns[layer][r][c]) for layer in range(1, nl) if int(columns[layer][r][c]) >= 0 and sink[int(columns[layer][r][c])] != 0]
                    prec, crack_water[r, c] = restate_soil_cracking(r, c, columns, water, max_water, float(cracking["pond"][s0]), si, tables, soils, hz_of,
                                                                    layer_depth, layer_thickness, area, lw, rain, hit, reasons)
                    prec_surface[r, c] = prec
                    if any(rain[n] > 0 for n in wet):
                        hit("crack: a filled layer already carries a subtraction")
                surface_flow = area * (float(prec) / 1000.)
                if surface_flow / 3600. > 0.:
                    rain[s0] = surface_flow / 3600.
            elif cracking is not None:
                hit("crack: liquidWater at the flag" if abs(float(lw) - fl) < EPSILON else "crack: liquidWater <= 0")
    total = sink.copy()
    total[rain > 0] = sink[rain > 0] + rain[rain > 0]
    out = dict(sinks_et=sink, sinks=total, evaporation=evaporation, transpiration=transpiration)
    if cracking is not None:
        out.update(prec_surface_water=prec_surface, crack_water=crack_water)
    return out


def _restate_transpiration(r, c, columns, water, ci, si, units, soils, hz_of, nl, et0, current_lai, cov, dd, roots, area, sink, hit):
    if not (0 <= ci < len(units)) or not current_lai > 0:
        hit("transpiration: no crop or LAI not positive (assignETreal)")
        return 0.0
    lai = float(current_lai)
    if lai < EPSILON or abs(dd - NODATA) < EPSILON:
        hit("transpiration: LAI < EPSILON or degree days NODATA")
        return 0.0
    if nl <= 1:
        hit("transpiration: only the surface layer")
        return 0.0
    if si < 0:
        hit("transpiration: no soil")
        return 0.0
    u = units[ci]
    kc_factor = 1 + (u["kcMax"] - 1) * cov
    max_t = et0 * cov * kc_factor
    if max_t < EPSILON:
        hit("transpiration: maxTranspiration < EPSILON")
        return 0.0
    if not float(roots["length"][r][c]) > 0:
        hit("transpiration: root length <= 0")
        return 0.0
    first, last = int(roots["first"][r][c]), int(roots["last"][r][c])
    density = [float(roots["density"][layer][r][c]) for layer in range(nl)]
    if first == NODATA or last == NODATA:
        hit("transpiration: empty density row" if not any(d > 0 for d in density) else "transpiration: root layers NODATA")
        return 0.0
    surplus_fraction = 0.0 if u["isWaterSurplusResistant"] else 0.5
    stressed = [False] * nl
    layer_t = [0.0] * nl                          # float values
    without_stress = 0.0
    subset_max = 0.0
    actual = 0.0
    so = soils[si]
    for layer in range(first, last + 1):
        n = int(columns[layer][r][c])
        if n < 0:
            hit("transpiration: a missing node inside the root range")
            continue
        h = int(hz_of[si, layer])
        if h == NODATA:
            hit("transpiration: horizon NODATA")
            continue
        fc, wp, sat = so["waterContentFC"][h], so["waterContentWP"][h], so["waterContentSAT"][h]
        w = water(n)
        surplus = sat - surplus_fraction * (sat - fc)
        scarcity = fc - u["fRAW"] * (fc - wp)
        if w <= wp:
            ratio = 0.0
            stressed[layer] = True
            hit("transpiration: no available water")
        elif w < scarcity:
            ratio = (w - wp) / (scarcity - wp)
            stressed[layer] = True
            hit("transpiration: water scarcity")
        elif (w - surplus) > EPSILON:
            ratio = (sat - w) / (sat - surplus)
            stressed[layer] = True
            hit("transpiration: water surplus")
        else:
            ratio = 1.0
            without_stress += density[layer]
            hit("transpiration: normal condition")
        layer_t[layer] = _f32(max_t * density[layer] * ratio)
        subset_max += max_t * density[layer]
        actual += layer_t[layer]
    stress = 1 - (actual / subset_max) if subset_max != 0 else float("nan")      # 1 - 0 / 0 in the reference
    if stress > EPSILON and without_stress > EPSILON:
        hit("transpiration: redistribution limited by waterStress" if stress < without_stress else "transpiration: redistribution limited by rootDensityWithoutStress")
        redistribution = subset_max * min(stress, without_stress)
        for layer in range(first, last + 1):
            if not stressed[layer] and layer_t[layer] > 0:
                layer_t[layer] = _f32(layer_t[layer] + redistribution * (density[layer] / without_stress))
    else:
        hit("transpiration: redistribution off")
    actual = 0.0
    for layer in range(first, last + 1):
        flow = area * (layer_t[layer] / 1000.) / 3600.
        if flow > DBL_EPSILON:
            n = int(columns[layer][r][c])
            if n >= 0:
                sink[n] -= flow
                actual += layer_t[layer]
        else:
            hit("transpiration: flow <= DBL_EPSILON")
    return actual
