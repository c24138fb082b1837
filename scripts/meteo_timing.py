"""Time the hourly meteo maps on the Ravone DEM (519 x 1208 cells): k_meteo_idw alone (HIP events around the launch) for 10, 40 and 200
stations and each of the three methods, air temperature with the height proxy, 20 launches after 3 warm-ups; the call with its station
upload and its download on the host clock.  The station table lives in LDS, so the kernel is compute-bound: the figures are reported
against the operation count (N distance evaluations per cell and pass - one pass for idw, two for the Shepard methods - and up to 90
direction terms per cell for the Shepard methods), next to the byte model (the DEM read and one float written per cell).
usage: python scripts/meteo_timing.py [--launches 20] [--warmup 3] [--out profiles/meteo_C5_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, meteo                       # noqa: E402

BYTES_PER_CELL = 4 + 4                                       # the DEM read, one float written (the height proxy is the DEM)


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "meteo_C5_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    cs, xll, yll = float(z["cellsize"]), float(z["xllcorner"]), float(z["yllcorner"])
    valid = int((dem != np.float32(flag)).sum())
    sf = capi.load_product()
    meteo.initialize(sf, dem, xll, yll, cs, [None], flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    settings = dict(rainfallThreshold=0.2, proxies=[dict(active=1, isHeight=1, inversion=0, slope=-0.0065)])
    rng = np.random.default_rng(5)
    runs = []
    for n in (10, 40, 200):
        x = np.round(xll + rng.uniform(-0.2, 1.2, n) * dem.shape[1] * cs, 3)
        y = np.round(yll + rng.uniform(-0.2, 1.2, n) * dem.shape[0] * cs, 3)
        v = np.round(rng.uniform(4.0, 26.0, n), 2).astype(np.float32)
        area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
        for method in meteo.METHODS:
            kernel_us, call_ms = [], []
            for h in range(a.warmup + a.launches):
                t0 = time.perf_counter()
                out = meteo.interpolate(sf, "airT", method, x, y, v, area, settings)
                t1 = time.perf_counter()
                if h >= a.warmup:
                    kernel_us.append(meteo.kernel_ms(sf) * 1e3)
                    call_ms.append((t1 - t0) * 1e3)
            passes = 1 if method == "idw" else 2
            distances = valid * n * passes
            med = float(np.median(kernel_us)) * 1e-6
            runs.append(dict(stations=n, method=method, computed_cells=int((out != np.float32(flag)).sum()), **stats(kernel_us, "kernel_us"),
                             **stats(call_ms, "call_with_upload_and_d2h_ms"), distance_evaluations=int(distances),
                             direction_terms_at_most=int(0 if method == "idw" else valid * 90),
                             distance_evaluations_per_s=float(distances / med), model_bytes=int(dem.size * BYTES_PER_CELL)))
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_meteo_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=valid, launches=a.launches, warmup=a.warmup,
               measured_on_gpu=runs, measured_on_host="not measured", fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
