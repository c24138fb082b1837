"""ctypes binding of the flat C ABI in include/sf3d.h.

The `SF3D` class drives any shared library that exports the ABI; this package only ever loads the HIP product
(`libsf3d_hip.so`, `load_product()`, which raises if it is missing - there is no CPU fallback).  The loaders of the
checkers (the CPU restatement and the wrapped reference under oracle/) live in tests/checkers.py: test infrastructure.
This module is plumbing only: it holds no numerical code.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PRODUCT_LIB = Path(os.environ.get("SF3D_PRODUCT_LIB", ROOT / "criteria3d_amd" / "csrc" / "libsf3d_hip.so"))

# --- enums (include/sf3d.h) ---------------------------------------------------------------
OK, INDEX_ERROR, MEMORY_ERROR, TOPOGRAPHY_ERROR, BOUNDARY_ERROR, MISSING_DATA_ERROR, \
    PARAMETER_ERROR, SOLVER_ERROR, FILE_ERROR = range(9)
BND_NONE, BND_RUNOFF, BND_FREE_DRAINAGE, BND_FREE_LATERAL_DRAINAGE, BND_PRESCRIBED, BND_URBAN, \
    BND_ROAD, BND_CULVERT, BND_HEAT_SURFACE, BND_SOLUTE_FLUX = range(10)
LINK_NONE, LINK_UP, LINK_DOWN, LINK_LATERAL = range(4)
WRC_VG, WRC_MODIFIED_VG, WRC_CAMPBELL = range(3)
MEAN_ARITHMETIC, MEAN_GEOMETRIC, MEAN_LOGARITHMIC = range(3)

ERROR_NAMES = ["ok", "index error", "memory error", "topography error", "boundary error",
               "missing data error", "parameter error", "solver error", "file error"]

u8, u16, u32, u64 = C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64
f64, f32, i32 = C.c_double, C.c_float, C.c_int
pd = C.POINTER(C.c_double)
pf32, pf64, pi32 = C.POINTER(C.c_float), pd, C.POINTER(C.c_int32)     # the raster bindings' names (maps.py, snow.py, crop.py, root.py, meteo.py, sinks.py)
p8, p16, p32, p64 = C.POINTER(u8), C.POINTER(u16), C.POINTER(u32), C.POINTER(u64)
cstr, vp = C.c_char_p, C.c_void_p

# name -> (restype, argtypes): every symbol include/sf3d.h declares
SIGNATURES = {
    "sf3d_initialize": (u8, [u32, u32, u8, i32, i32, i32, u8]),
    "sf3d_initialize_balance": (u8, []),
    "sf3d_initialize_log": (u8, [cstr, cstr]),
    "sf3d_clean": (u8, []),
    "sf3d_close_log": (u8, []),
    "sf3d_initialize_heat_flag": (u8, [u8, i32, i32]),
    "sf3d_set_threads_number": (u32, [u32]),
    "sf3d_set_use_lineal": (None, [i32]),
    "sf3d_set_lineal_method": (None, [i32]),
    "sf3d_set_soil_properties": (u8, [u16, u8] + [f64] * 10),
    "sf3d_set_surface_properties": (u8, [u16, f64]),
    "sf3d_set_numerical_parameters": (u8, [f64, f64, u16, u16, u8, u8]),
    "sf3d_set_hydraulic_properties": (u8, [u8, u8, f32]),
    "sf3d_set_culvert": (u8, [u32, f64, f64, f64, f64]),
    "sf3d_set_node": (u8, [u32, f64, f64, f64, f64, i32, u8, f64, f64]),
    "sf3d_set_node_link": (u8, [u32, u32, u8, f64]),
    "sf3d_set_node_boundary": (u8, [u32, u8, f64, f64]),
    "sf3d_set_node_soil": (u8, [u32, u16, u16]),
    "sf3d_set_node_surface": (u8, [u32, u16]),
    "sf3d_set_node_pond": (u8, [u32, f64]),
    "sf3d_set_node_water_content": (u8, [u32, f64]),
    "sf3d_set_node_degree_of_saturation": (u8, [u32, f64]),
    "sf3d_set_node_matric_potential": (u8, [u32, f64]),
    "sf3d_set_node_total_potential": (u8, [u32, f64]),
    "sf3d_set_node_water_sink_source": (u8, [u32, f64]),
    "sf3d_set_node_prescribed_total_potential": (u8, [u32, f64]),
    "sf3d_get_node_water_content": (f64, [u32]),
    "sf3d_get_node_maximum_water_content": (f64, [u32]),
    "sf3d_get_node_minimum_water_content": (f64, [u32]),
    "sf3d_get_node_available_water_content": (f64, [u32]),
    "sf3d_get_node_water_deficit": (f64, [u32, f64]),
    "sf3d_get_node_degree_of_saturation": (f64, [u32]),
    "sf3d_get_node_water_conductivity": (f64, [u32]),
    "sf3d_get_node_matric_potential": (f64, [u32]),
    "sf3d_get_node_total_potential": (f64, [u32]),
    "sf3d_get_node_pond": (f64, [u32]),
    "sf3d_get_node_max_water_flow": (f64, [u32, u8]),
    "sf3d_get_node_sum_lateral_water_flow": (f64, [u32]),
    "sf3d_get_node_sum_lateral_water_flow_in": (f64, [u32]),
    "sf3d_get_node_sum_lateral_water_flow_out": (f64, [u32]),
    "sf3d_get_node_boundary_water_flow": (f64, [u32]),
    "sf3d_get_total_boundary_water_flow": (f64, [u8]),
    "sf3d_get_total_water_content": (f64, []),
    "sf3d_get_water_storage": (f64, []),
    "sf3d_get_water_mbr": (f64, []),
    "sf3d_set_node_heat_sink_source": (u8, [u32, f64]),
    "sf3d_set_node_temperature": (u8, [u32, f64]),
    "sf3d_set_node_boundary_fixed_temperature": (u8, [u32, f64, f64]),
    "sf3d_set_node_boundary_height_wind": (u8, [u32, f64]),
    "sf3d_set_node_boundary_height_temperature": (u8, [u32, f64]),
    "sf3d_set_node_boundary_net_irradiance": (u8, [u32, f64]),
    "sf3d_set_node_boundary_temperature": (u8, [u32, f64]),
    "sf3d_set_node_boundary_relative_humidity": (u8, [u32, f64]),
    "sf3d_set_node_boundary_roughness": (u8, [u32, f64]),
    "sf3d_set_node_boundary_wind_speed": (u8, [u32, f64]),
    "sf3d_get_node_temperature": (f64, [u32]),
    "sf3d_get_node_heat_conductivity": (f64, [u32]),
    "sf3d_get_node_vapor": (f64, [u32]),
    "sf3d_get_node_heat_storage": (f64, [u32, f64]),
    "sf3d_get_node_heat_max_flux": (f64, [u32, u8, u8]),
    "sf3d_get_node_boundary_advective_flux": (f64, [u32]),
    "sf3d_get_node_boundary_latent_flux": (f64, [u32]),
    "sf3d_get_node_boundary_radiative_flux": (f64, [u32]),
    "sf3d_get_node_boundary_sensible_flux": (f64, [u32]),
    "sf3d_get_node_boundary_aerodynamic_conductance": (f64, [u32]),
    "sf3d_get_node_boundary_soil_conductance": (f64, [u32]),
    "sf3d_get_heat_mbr": (f64, []),
    "sf3d_get_heat_mbe": (f64, []),
    "sf3d_compute_period": (None, [f64]),
    "sf3d_compute_step": (f64, [f64]),
    # extensions
    "sf3d_backend_name": (cstr, []),
    "sf3d_set_nodes": (u8, [u32, u32, pd, pd, pd, pd, p8, p8, pd, pd]),
    "sf3d_set_node_links": (u8, [u64, p32, p32, p8, pd]),
    "sf3d_set_nodes_soil": (u8, [u32, u32, p16, p16]),
    "sf3d_set_nodes_surface": (u8, [u32, u32, p16]),
    "sf3d_set_nodes_pond": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_matric_potential": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_total_potential": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_water_sink_source": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_total_potential": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_degree_of_saturation": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_water_content": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_water_conductivity": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_boundary_water_flow": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_temperature": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_heat_sink_source": (u8, [u32, u32, pd]),
    "sf3d_get_nodes_temperature": (u8, [u32, u32, pd]),
    "sf3d_set_nodes_boundary_heat": (u8, [i32, u32, p32, pd]),
    "sf3d_get_counters": (u8, [p64]),
    "sf3d_get_linear_residual": (f64, []),
    "sf3d_get_time_step": (f64, []),
    "sf3d_set_time_step": (u8, [f64]),
    "sf3d_reset_solver_state": (u8, []),
    "sf3d_set_surface_nodes_number": (u8, [u32]),
    "sf3d_set_device": (u8, [i32]),
    "sf3d_synchronize": (u8, []),
    "sf3d_kernel_timing": (u8, [i32]),
    "sf3d_kernel_count": (i32, []),
    "sf3d_kernel_name": (cstr, [i32]),
    "sf3d_kernel_stats": (u8, [i32, p64, pd, p64]),
    "sf3d_libm_set": (i32, []),
    "sf3d_device_log": (u8, [u32, pd, pd]),
    "sf3d_device_exp": (u8, [u32, pd, pd]),
    "sf3d_device_cbrt": (u8, [u32, pd, pd]),
    "sf3d_device_norm_sum": (u8, [u32, pd, u32, i32, pd]),
    "sf3d_get_sweep_launches": (u8, [p64, p64]),
    "sf3d_get_resident_launches": (u8, [p64]),
    "sf3d_get_heat_counters": (u8, [p64]),
    "sf3d_device_pow": (u8, [u32, pd, pd, pd]),
    "sf3d_device_bytes": (u64, []),
    "sf3d_host_bytes": (u64, []),
    "sf3d_dist_blob_bytes": (i32, []),
    "sf3d_dist_prepare": (u8, [i32, i32]),
    "sf3d_dist_export": (u8, [vp]),
    "sf3d_dist_connect": (u8, [vp]),
    "sf3d_dist_status": (i32, []),
    "sf3d_dist_finalize": (u8, [i32]),
    "sf3d_dist_transport": (i32, []),
    "sf3d_dist_stats": (u8, [pd, i32]),
    "sf3d_get_regular_grid": (u8, [p32, p32, p32, C.POINTER(C.c_int8), C.POINTER(C.c_int8)]),
    "sf3d_dist_owner": (u8, [i32, u32, u32, C.POINTER(C.c_int32)]),
    "sf3d_dist_bounds": (u8, [u32, i32, p32]),
    "sf3d_dist_halo": (u8, [i32, i32, i32, i32, u32, p32, p32]),
}

# the 70 entry points that stand in for soilFluxes3D.h:9-104 (everything before "extensions")
REFERENCE_API = [k for k in SIGNATURES if k != "sf3d_backend_name"][:70]

COUNTER_NAMES = ["attempts", "accepted", "approximations", "sweeps", "courant_rejections",
                 "linear_failures", "restores", "early_courant_rejections"]


BOUNDARY_HEAT_FIELDS = ("height_wind", "height_temperature", "roughness", "temperature", "relative_humidity",
                        "wind_speed", "net_irradiance")


class SF3DError(RuntimeError):
    pass


def bind_signatures(sf, signatures: dict):
    """attach a name -> (restype, argtypes) table to a loaded library (AttributeError = symbol missing: fail loudly)"""
    for name, (res, args) in signatures.items():
        fn = getattr(sf.lib, name)
        fn.restype = res
        fn.argtypes = args
    return sf


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


class SF3D:
    """One loaded implementation of the sf3d C ABI (process-global model inside the library)."""

    def __init__(self, path: os.PathLike):
        path = Path(path)
        if not path.exists():
            raise SF3DError(f"shared library not found: {path}")
        self.path = path
        self.lib = C.CDLL(str(path), mode=C.RTLD_LOCAL)
        bind_signatures(self, SIGNATURES)
        self.backend = self.lib.sf3d_backend_name().decode()

    # -- helpers -------------------------------------------------------------------------
    def check(self, code: int, what: str = ""):
        if code != OK:
            raise SF3DError(f"{self.backend}: {what}: {ERROR_NAMES[code] if code < 9 else code}")

    def __getattr__(self, name):
        # raw access: obj.set_node(...) -> lib.sf3d_set_node(...)
        try:
            return getattr(self.__dict__["lib"], "sf3d_" + name)
        except (KeyError, AttributeError):
            raise AttributeError(name)

    # -- bulk helpers over numpy arrays ----------------------------------------------------
    def set_nodes_bulk(self, first, x, y, z, size, is_surface, btype, slope, barea):
        n = len(x)
        x, y, z, size = (_arr(a, np.float64) for a in (x, y, z, size))
        is_surface, btype = _arr(is_surface, np.uint8), _arr(btype, np.uint8)
        slope, barea = _arr(slope, np.float64), _arr(barea, np.float64)
        self.check(self.lib.sf3d_set_nodes(first, n, _ptr(x, f64), _ptr(y, f64), _ptr(z, f64),
                                           _ptr(size, f64), _ptr(is_surface, u8), _ptr(btype, u8),
                                           _ptr(slope, f64), _ptr(barea, f64)), "set_nodes")

    def set_links_bulk(self, node, linked, direction, area):
        node, linked = _arr(node, np.uint32), _arr(linked, np.uint32)
        direction, area = _arr(direction, np.uint8), _arr(area, np.float64)
        self.check(self.lib.sf3d_set_node_links(len(node), _ptr(node, u32), _ptr(linked, u32),
                                                _ptr(direction, u8), _ptr(area, f64)), "set_node_links")

    def set_soil_bulk(self, first, soil, horizon):
        soil, horizon = _arr(soil, np.uint16), _arr(horizon, np.uint16)
        self.check(self.lib.sf3d_set_nodes_soil(first, len(soil), _ptr(soil, u16), _ptr(horizon, u16)), "set_nodes_soil")

    def set_surface_bulk(self, first, surf):
        surf = _arr(surf, np.uint16)
        self.check(self.lib.sf3d_set_nodes_surface(first, len(surf), _ptr(surf, u16)), "set_nodes_surface")

    def _set_f64(self, fn, first, v, what):
        v = _arr(v, np.float64)
        self.check(fn(first, len(v), _ptr(v, f64)), what)

    def set_pond_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_pond, first, v, "set_nodes_pond")

    def set_matric_potential_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_matric_potential, first, v, "set_nodes_matric_potential")

    def set_total_potential_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_total_potential, first, v, "set_nodes_total_potential")

    def set_sink_source_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_water_sink_source, first, v, "set_nodes_water_sink_source")

    def _get_f64(self, fn, first, count, what):
        out = np.empty(count, dtype=np.float64)
        self.check(fn(first, count, _ptr(out, f64)), what)
        return out

    def total_potential(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_total_potential, first, count, "get_nodes_total_potential")

    def degree_of_saturation(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_degree_of_saturation, first, count, "get_nodes_degree_of_saturation")

    def water_content(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_water_content, first, count, "get_nodes_water_content")

    def water_conductivity(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_water_conductivity, first, count, "get_nodes_water_conductivity")

    def boundary_water_flow(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_boundary_water_flow, first, count, "get_nodes_boundary_water_flow")

    def set_temperature_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_temperature, first, v, "set_nodes_temperature")

    def set_heat_sink_source_bulk(self, first, v):
        self._set_f64(self.lib.sf3d_set_nodes_heat_sink_source, first, v, "set_nodes_heat_sink_source")

    def temperature(self, first, count):
        return self._get_f64(self.lib.sf3d_get_nodes_temperature, first, count, "get_nodes_temperature")

    def set_boundary_heat_bulk(self, field, nodes, values):
        """field: one of BOUNDARY_HEAT_FIELDS (name or index)"""
        f = BOUNDARY_HEAT_FIELDS.index(field) if isinstance(field, str) else int(field)
        nodes = _arr(nodes, np.uint32)
        values = _arr(np.broadcast_to(np.asarray(values, np.float64), nodes.shape), np.float64)
        self.check(self.lib.sf3d_set_nodes_boundary_heat(f, len(nodes), _ptr(nodes, u32), _ptr(values, f64)),
                   f"set_nodes_boundary_heat[{field}]")

    def counters(self):
        out = (u64 * 8)()
        code = self.lib.sf3d_get_counters(out)
        if code != OK:
            return None
        return dict(zip(COUNTER_NAMES, [int(v) for v in out]))

    def heat_counters(self):
        """heat steps accepted / halved, boundary Courant reductions of dtHeat, linear-solver sweeps since sf3d_initialize"""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.sf3d_get_heat_counters(out), "get_heat_counters")
        return dict(zip(("accepted", "halved", "boundary_reductions", "sweeps"), [int(v) for v in out]))

    def sweep_launches(self):
        """(single sweeps, paired passes) the product launched since sf3d_initialize"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.check(self.lib.sf3d_get_sweep_launches(C.byref(a), C.byref(b)), "get_sweep_launches")
        return int(a.value), int(b.value)

    def resident_launches(self):
        """resident sweep loops (all Jacobi iterations of an approximation in one launch) since sf3d_initialize"""
        a = C.c_uint64(0)
        self.check(self.lib.sf3d_get_resident_launches(C.byref(a)), "get_resident_launches")
        return int(a.value)

    # -- multi-GPU bootstrap -----------------------------------------------------------------
    def dist_connect(self, rank, world, allgather):
        """export this rank's window descriptor, all-gather the blobs with the launcher's control
        plane, connect to the peers' windows"""
        nbytes = self.lib.sf3d_dist_blob_bytes()
        blob = C.create_string_buffer(nbytes)
        self.check(self.lib.sf3d_dist_export(blob), "dist_export")
        blobs = allgather(blob.raw)
        assert len(blobs) == world and all(len(b) == nbytes for b in blobs)
        joined = C.create_string_buffer(b"".join(blobs), nbytes * world)
        self.check(self.lib.sf3d_dist_connect(joined), "dist_connect")
        if getattr(self, "legacy_connect", False):      # a launcher without the status / finalize round (tests): windows if they work
            return
        # which exchange: every rank reports whether its windows passed the self-check; one rank that needs RCCL moves all of them
        # the ranks' common decision: the device windows when every rank's passed their self-check; otherwise the same exchange through
        # host-memory windows (POSIX shared memory over PCIe: slower, same protocol) - or RCCL, only when SF3D_EXCHANGE=rccl asks for it
        status = allgather(bytes([self.lib.sf3d_dist_status() & 1]))
        failed = any(b[0] for b in status)
        mode = 0 if not failed else (1 if os.environ.get("SF3D_EXCHANGE") == "rccl" else 2)
        self.check(self.lib.sf3d_dist_finalize(mode), "dist_finalize")

    def dist_stats(self, world):
        """{"epochs": n, "peers": {p: {"hop_us", "mean_wait_us", "max_wait_us"}}} of a connected multi-rank model"""
        out = np.zeros(1 + 3 * world)
        self.check(self.lib.sf3d_dist_stats(out.ctypes.data_as(pd), out.size), "dist_stats")
        return {"epochs": int(out[0]), "peers": {p: {"hop_us": float(out[1 + 3 * p]), "mean_wait_us": float(out[2 + 3 * p]), "max_wait_us": float(out[3 + 3 * p])}
                                                 for p in range(world)}}

    def dist_bounds(self, ns, world):
        """surface-index bounds of the row strips of `world` ranks (world + 1 entries): rank r owns the columns of the surface nodes
        [bounds[r], bounds[r + 1]) - needs no model"""
        out = np.zeros(world + 1, dtype=np.uint32)
        self.check(self.lib.sf3d_dist_bounds(ns, world, _ptr(out, u32)), "dist_bounds")
        return out

    def owner_map(self, world, n):
        out = np.empty(n, dtype=np.int32)
        self.check(self.lib.sf3d_dist_owner(world, 0, n, out.ctypes.data_as(C.POINTER(C.c_int32))), "dist_owner")
        return out

    def halo_list(self, rank, world, peer, direction):
        cnt = u32(0)
        self.check(self.lib.sf3d_dist_halo(rank, world, peer, direction, 0, None, C.byref(cnt)), "dist_halo")
        out = np.empty(cnt.value, dtype=np.uint32)
        if cnt.value:
            self.check(self.lib.sf3d_dist_halo(rank, world, peer, direction, cnt.value, _ptr(out, u32), C.byref(cnt)), "dist_halo")
        return out

    def kernel_stats(self):
        """{kernel name: (launches, total_ms, nodes_per_launch)} from the HIP-event pool."""
        res = {}
        for k in range(self.lib.sf3d_kernel_count()):
            n, ms, npl = u64(0), f64(0.0), u64(0)
            self.check(self.lib.sf3d_kernel_stats(k, C.byref(n), C.byref(ms), C.byref(npl)), "kernel_stats")
            res[self.lib.sf3d_kernel_name(k).decode()] = (int(n.value), float(ms.value), int(npl.value))
        return res


def load_product() -> SF3D:
    """The HIP/gfx950 product library.  Raises (never falls back) if it has not been built."""
    if not PRODUCT_LIB.exists():
        raise SF3DError(f"{PRODUCT_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`; "
                        "there is no CPU fallback for the product path")
    return SF3D(PRODUCT_LIB)
