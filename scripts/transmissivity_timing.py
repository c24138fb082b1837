"""Time the station transmissivity call on the Ravone DEM (519 x 1208 cells): k_transmissivity_points alone (HIP events around the launch),
20 launches after 3 warm-ups, with 40, 200 and 1 024 stations at window widths 13 and 23 (hourly steps around 08:00 UTC on the equinox, so
that the window holds night, low sun with long shadow rays, and day); the call with its uploads on the host clock; and beside it the
host build of the same text (tests/transmissivity_host.cpp) on one CPU of the same machine.  One wave evaluates one station: 40 stations
fill 40 waves of a device that holds thousands, so the small sets measure the launch and the longest ray, not throughput.
usage: python scripts/transmissivity_timing.py [--launches 20] [--warmup 3] [--out profiles/transmissivity_timing.json]"""
import argparse
import hashlib
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                          # noqa: E402
from criteria3d_amd import capi, radiation as rad, transmissivity as tr    # noqa: E402
from tests import transmissivity_cases as tc                               # noqa: E402
from tests.raster_helpers import build_host_program                          # noqa: E402

WHEN, STEP = (2021, 3, 20, 8, 0, 0), 3600
SETS, WIDTHS = (40, 200, 1024), (13, 23)


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "transmissivity_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    cs, xll, yll = float(z["cellsize"]), float(z["xllcorner"]), float(z["yllcorner"])
    rows, cols = dem.shape
    header = dict(nrows=rows, ncols=cols, xllcorner=xll, yllcorner=yll, cellsize=cs)
    # the station calls read neither the latitude / longitude maps nor slope and aspect: the corner's values stand for all cells
    la, lo = rad.utm_to_latlon(rad.DEFAULT_GIS["utmZone"], rad.DEFAULT_GIS["startLatitude"], xll, yll)
    lat, lon = np.full(dem.shape, la, np.float32), np.full(dem.shape, lo, np.float32)
    zeros = np.zeros_like(dem)
    sf = capi.load_product()
    rad.initialize(sf, dem, xll, yll, cs, lat, lon, zeros, zeros, flag=flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    rng = np.random.default_rng(20261019)
    runs, calls = [], []
    for n in SETS:
        x = xll + cs * cols * rng.uniform(0.02, 0.98, 4 * n)
        y = yll + cs * rows * rng.uniform(0.02, 0.98, 4 * n)
        st = tr.station_points(x, y, np.full(4 * n, -9999.0), None, dem, header, flag)
        st = st[np.abs(st[:, 2] - flag) > 1e-5][:n]                         # the first n on a cell with an elevation (on a flag cell S_solpos refuses the height)
        assert len(st) == n
        for width in WIDTHS:
            measured = np.round(rng.uniform(50, 700, (len(st), width))).astype(np.float32)
            kernel_us, call_ms = [], []
            for h in range(a.warmup + a.launches):
                t0 = time.perf_counter()
                out, n_valid = tr.points(sf, WHEN, width, STEP, st, measured)
                t1 = time.perf_counter()
                if h >= a.warmup:
                    kernel_us.append(tr.kernel_ms(sf) * 1e3)
                    call_ms.append((t1 - t0) * 1e3)
            w, _, g = tr.evaluations(sf, len(st), width)
            runs.append(dict(stations=len(st), width=width, evaluations=int(w.sum()), evaluations_by_day=int((g > 0).sum()), n_valid=n_valid,
                             result_min_max=[float(out.min()), float(out.max())], **stats(kernel_us, "kernel_us"), **stats(call_ms, "call_with_uploads_ms")))
            calls.append((None, WHEN, tc.POINTS, width, STEP, st, measured))
    sf.lib.sf3d_kernel_timing(0)
    rad.clean(sf)
    # the host build of the same text on one CPU: every call `repeat` times, the seconds without reading and writing
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host_program("transmissivity", tmp)
        for run, call in zip(runs, calls):
            tc.write_host_input(Path(tmp) / "in.bin", dem, flag, (xll, yll, cs), [call])
            repeat = 5
            out = subprocess.run([str(exe), str(Path(tmp) / "in.bin"), str(Path(tmp) / "out.bin"), str(repeat)], check=True, capture_output=True, text=True).stdout
            run["host_one_cpu_ms"] = float(out.split()[0]) / repeat * 1e3
            run["host_over_kernel"] = run["host_one_cpu_ms"] * 1e3 / run["kernel_us_median"]
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_transmissivity.inc", "sf3d_transmissivity_api.inc", "sf3d_rad.inc",
                                                                                "sf3d_rad_setup.inc", "sf3d_trig.inc"))
    res = dict(workload="Ravone DEM, station transmissivity", rows=rows, cols=cols, when=list(WHEN), step=STEP, launches=a.launches, warmup=a.warmup,
               measured_on_gpu=runs, fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
