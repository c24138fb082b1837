"""Time the local detrending block on the Ravone DEM (519 x 1208 cells), HIP events around each launch of k_localdetrend, medians of 20
launches after 3 warm-ups: synthetic stations (40, 200, 1 000) placed up to 20 km around the raster, each method, lapseRatePiecewise_two
and _three_free with setChosenElevationFunction's default ranges and the full first-guess list, minPointsLocalDetrending 8.  With every
row the mean and the largest number of selected stations per cell and the share of cells whose height proxy was significant.
usage: python scripts/localdetrend_timing.py [--launches 20] [--warmup 3] [--stations 40 200 1000] [--out profiles/localdetrend_timing.json]"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, localdetrend as ld, meteo  # noqa: E402

RANGES = {"piecewiseTwo": ([0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1]),
          "piecewiseThreeFree": ([-350.0, 0.0, 300.0, 0.002, -0.01, -0.01, 2500.0, 0.0, 1000.0, 0.007, -0.0015, -0.0015], [0, 1, 1, 1, 1, 1])}


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stations", type=int, nargs="+", default=[40, 200, 1000])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "localdetrend_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    cs, xll, yll = float(z["cellsize"]), float(z["xllcorner"]), float(z["yllcorner"])
    inside = dem != np.float32(flag)
    sf = capi.load_product()
    meteo.initialize(sf, dem, xll, yll, cs, [None], flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    rng = np.random.default_rng(24)
    runs = []
    for n in a.stations:
        x = np.round(xll + rng.uniform(-20000.0, dem.shape[1] * cs + 20000.0, n), 2)
        y = np.round(yll + rng.uniform(-20000.0, dem.shape[0] * cs + 20000.0, n), 2)
        h = np.round(rng.uniform(20.0, 1500.0, n), 1).astype(np.float32)
        t = np.round(np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0)) + rng.normal(0.0, 0.6, n), 1).astype(np.float32)
        area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
        for function, (configured, position) in RANGES.items():
            fit = ld.make_fit(function, configured, position, (float(t.min()), float(t.max())), 8)
            for method in meteo.METHODS:
                ms = []
                for k in range(a.warmup + a.launches):
                    ld.interpolate(sf, "airT", method, x, y, h, t, area, fit, download=False)
                    if k >= a.warmup:
                        ms.append(ld.kernel_ms(sf))
                count, sig = ld.get_selection(sf)["count"][inside], ld.get_fit(sf)["significant"][inside]
                runs.append(dict(stations=n, function=function, method=method, first_guesses=len(fit["first_guess"]), **stats(ms, "kernel_ms"),
                                 cells_per_s=float(inside.sum() / (np.median(ms) * 1e-3)), selected_mean=float(count.mean()), selected_max=int(count.max()),
                                 significant_share=float(sig.mean())))
                print(json.dumps(runs[-1]), flush=True)
    held = ld.bytes_held(sf)
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_localdetrend.inc", "sf3d_localdetrend_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=int(inside.sum()), cell_size=cs,
               launches=a.launches, warmup=a.warmup, minPointsLocalDetrending=8, k_localdetrend=runs, bytes_held=held, fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
