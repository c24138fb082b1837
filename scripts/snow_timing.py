"""Time the hourly snow model on the Ravone DEM (519 x 1208 cells): k_snow_hour alone (HIP events around the launch), the whole
sf3d_snow_compute_hour call with its seven H2D copies (host clock), and - for scale only - criteria3d_amd.snow.restate_snow_hour on the
host for the same grid: a python restatement of the point model, NOT the reference's OpenMP loop.
usage: python scripts/snow_timing.py [--launches 20] [--warmup 3] [--host-rows 40] [--out profiles/snow_C5_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, snow                        # noqa: E402

BYTES_PER_CELL = 27 * 4                                      # 7 state x 2 + 7 inputs + 6 outputs
HBM_BYTES_PER_S = 8e12


def forcing(dem, flag, hour, rng):
    valid = dem != np.float32(flag)
    cold = hour < 12
    f = lambda v: np.where(valid, v, flag).astype(np.float32)
    shape = dem.shape
    return dict(airT=f((-3.0 if cold else 6.0) + rng.uniform(-2, 2, shape)), prec=f(rng.uniform(0, 3, shape)), relHum=f(rng.uniform(40, 100, shape)),
                windInt=f(rng.uniform(0, 8, shape)), globalRad=f(rng.uniform(0, 500, shape)), beamRad=f(rng.uniform(0, 300, shape)),
                transmissivity=f(rng.uniform(0.1, 0.75, shape)), clearSkyTransmissivity=0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=40, help="rows of the grid the host restatement is timed on (scaled to the whole grid)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "snow_C5_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    rng = np.random.default_rng(5)
    sf = capi.load_product()
    snow.initialize(sf, dem, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    kernel_us, call_ms = [], []
    for h in range(a.warmup + a.launches):
        met = forcing(dem, flag, h, rng)
        t0 = time.perf_counter()
        snow.compute_hour(sf, met)
        t1 = time.perf_counter()
        if h >= a.warmup:
            kernel_us.append(sf.lib.sf3d_snow_kernel_ms() * 1e3)
            call_ms.append((t1 - t0) * 1e3)
    sf.lib.sf3d_kernel_timing(0)
    swe = snow.get_state(sf, "swe")
    state = {n: snow.get_state(sf, n) for n in snow.STATE}
    # host figure: the python restatement on a strip of rows, scaled by cells
    r0 = dem.shape[0] // 2
    rows = slice(r0, r0 + a.host_rows)
    met = forcing(dem, flag, a.warmup + a.launches, rng)
    t0 = time.perf_counter()
    snow.restate_snow_hour({n: v[rows] for n, v in state.items()}, {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in met.items()}, dem[rows], flag)
    host_s = (time.perf_counter() - t0) * dem.shape[0] / a.host_rows
    snow.clean(sf)
    cells = dem.size
    med = float(np.median(kernel_us))
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_snow.inc", "sf3d_snow_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(cells), valid_cells=int((dem != np.float32(flag)).sum()),
               launches=a.launches, warmup=a.warmup, measured_on_gpu=dict(
                   kernel_us_min=float(min(kernel_us)), kernel_us_median=med, kernel_us_max=float(max(kernel_us)),
                   call_ms_min=float(min(call_ms)), call_ms_median=float(np.median(call_ms)), call_ms_max=float(max(call_ms)),
                   model_bytes=int(cells * BYTES_PER_CELL), fraction_of_8TBps=float(cells * BYTES_PER_CELL / (med * 1e-6) / HBM_BYTES_PER_S),
                   cells_with_snow_at_the_end=int((swe > 0).sum())),
               measured_on_host=dict(what="criteria3d_amd.snow.restate_snow_hour (python restatement of the point model, one thread; not the reference's OpenMP loop)",
                                     rows_timed=a.host_rows, seconds_per_hour_scaled_to_the_grid=float(host_s)),
               fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
