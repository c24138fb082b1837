#!/usr/bin/env python3
"""Time the output maps (include/sf3d_maps.h, k_output_map) on the whole Ravone project (BASELINE config 5, 5.85 M nodes) after a stretch
of hour 0, against the host path the caller had before: bulk getters of include/sf3d.h plus the numpy restatement of the reference's
loops (criteria3d_amd/maps.py).  Prints one JSON line (and writes it to --out).

  * kernel: event-timed us of k_output_map (sf3d_kernel_timing), for factorOfSafety over all layers and for volumetricWaterContent over
    all layers; WARM = right after a computeStep (the state was just written, the Infinity Cache holds what fits of it);
  * call: wall time of sf3d_compute_output_map, D2H copy of the maps included;
  * host: wall time of the bulk getters + the restated loops producing the same maps (checked equal here).

usage: python scripts/output_maps_timing.py --workload C5 [--steps 20] [--reps 5] [--out profiles/<name>.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                        # noqa: E402

from criteria3d_amd import build, capi, catchment as cm, maps             # noqa: E402


def csrc_fingerprint():
    """the rule of bench.py / scripts/profile_summary.py"""
    h = hashlib.sha256()
    for f in sorted((ROOT / "criteria3d_amd" / "csrc").iterdir()):
        if f.suffix in (".inc", ".h", ".hip", ".cpp"):
            h.update(f.name.encode()); h.update(f.read_bytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C5", choices=["C5"])
    ap.add_argument("--steps", type=int, default=20, help="computeSteps of hour 0 (25 mm) before the maps")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tests.scenarios import ravone_project_model
    build.build_product()
    sf = capi.load_product()
    t0 = time.time()
    m = ravone_project_model(None)
    t_model = time.time() - t0
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=16)
    cm.run_hour(sf, m, 25.0, max_steps=a.steps)
    maps.set_output(sf, m)
    index = np.asarray(m.meta["index"])
    nz, ny, nx = index.shape
    thick = [0.0] + list(m.meta["layers"])
    res = dict(workload=a.workload, nodes=int(m.n), cells=int(ny * nx), layers=int(nz), steps_before=a.steps, fingerprint=csrc_fingerprint(),
               model_build_s=round(t_model, 1), reps=a.reps, cache_state="warm: right after a computeStep")
    for name, var in (("factor_of_safety_all_layers", maps.FACTOR_OF_SAFETY), ("volumetric_water_content_all_layers", maps.VOLUMETRIC_WATER_CONTENT)):
        kern, call = [], []
        for _ in range(a.reps):
            cm.run_hour(sf, m, 25.0, max_steps=1)                        # warm: the state was just written by a step
            sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
            b = sf.kernel_stats()["k_output_map"]
            t = time.perf_counter()
            dev = maps.output_maps(sf, m, var)
            call.append(time.perf_counter() - t)
            e = sf.kernel_stats()["k_output_map"]
            sf.lib.sf3d_kernel_timing(0)
            kern.append((e[1] - b[1]) / max(1, e[0] - b[0]))
        # host path: bulk getters + the restated loops (the last state above)
        t = time.perf_counter()
        wc = sf.water_content(0, m.n)
        if var == maps.FACTOR_OF_SAFETY:
            dos = sf.degree_of_saturation(0, m.n)
            mpot = sf.total_potential(0, m.n) - m.z                      # getNodeMatricPotential = H - z
            tan_a, sin2 = maps.slope_terms(m.meta["slope"], False)
            geo = maps.node_geotechnics(m)
            host = np.stack([maps.restate_fos_map(index, thick, l, tan_a, sin2, geo, wc, dos, mpot) for l in range(nz)])
        else:
            host = np.stack([maps.restate_layer_map(index, var, l, wc) for l in range(nz)])
        t_host = time.perf_counter() - t
        res[name] = dict(kernel_us_median=round(1000 * float(np.median(kern)), 1), kernel_us_min=round(1000 * float(np.min(kern)), 1),
                         call_ms_median=round(1000 * float(np.median(call)), 2), host_path_ms=round(1000 * t_host, 1),
                         map_bytes=int(dev.nbytes), equal_to_host_path=bool(np.array_equal(dev.view(np.uint32), host.astype(np.float32).view(np.uint32))))
    # byte model: per soil node read H, Se, z (8 B each), class (2 B) + table entries; per cell-layer one float written + the column table
    res["byte_model_mb"] = round((m.n * (3 * 8 + 2 + 8) + nz * ny * nx * (4 + 4)) / 1e6, 1)
    sf.lib.sf3d_clean()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
