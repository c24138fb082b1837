"""Time local detrending with every proxy on the Ravone DEM (519 x 1208 cells), HIP events around each launch, medians of 20 launches after
3 warm-ups: the seeded stations of scripts/localdetrend_timing.py (the same generator, drawn in the same order: 40, 200, 1 000; the 200 are
timed by default), lapseRatePiecewise_two with the default range and the full first-guess list, minPointsLocalDetrending 8, idw; 0, 1, 4
and the cap of other proxies active on synthetic proxy rasters, and k_localdetrend on the same inputs beside the 0 row.  With every row the
mean selected and interpolated count and the share of cells per significant proxy count.
usage: python scripts/localproxies_timing.py [--launches 20] [--warmup 3] [--stations 200] [--out profiles/localproxies_timing.json]"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                           # noqa: E402
from criteria3d_amd import capi, localdetrend as ld, localproxies as lp, meteo  # noqa: E402

CONFIGURED, POSITION = [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1]
SLOTS = meteo.MAX_PROXIES


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stations", type=int, nargs="+", default=[200])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "localproxies_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    cs, xll, yll = float(z["cellsize"]), float(z["xllcorner"]), float(z["yllcorner"])
    inside = dem != np.float32(flag)
    rows, cols = dem.shape
    r_, c_ = np.mgrid[0:rows, 0:cols]
    prng = np.random.default_rng(25)
    maps = [None]
    for k in range(1, SLOTS):
        if k % 3 == 1:
            m = 2.0 + 0.01 * k * c_ + 0.004 * r_                                # a plane
        elif k % 3 == 2:
            m = np.where(prng.uniform(size=dem.shape) < 0.4, prng.uniform(0.05, 1.0, dem.shape), 0.0)      # a patchy 0 / fraction map
        else:
            m = np.sin(0.01 * k * c_) * np.cos(0.013 * r_)                      # a bounded index
        maps.append(np.round(m, 3).astype(np.float32))
    sf = capi.load_product()
    lp.bind(sf)
    meteo.initialize(sf, dem, xll, yll, cs, maps, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    rng = np.random.default_rng(24)
    others = lp.make_others([None] + [dict(range=[-1.0, -40.0, 1.0, 50.0])] * (SLOTS - 1))
    runs = []
    for n in (40, 200, 1000):
        x = np.round(xll + rng.uniform(-20000.0, dem.shape[1] * cs + 20000.0, n), 2)
        y = np.round(yll + rng.uniform(-20000.0, dem.shape[0] * cs + 20000.0, n), 2)
        h = np.round(rng.uniform(20.0, 1500.0, n), 1).astype(np.float32)
        t = np.round(np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0)) + rng.normal(0.0, 0.6, n), 1).astype(np.float32)
        if n not in a.stations:
            continue
        area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
        pv = np.zeros((SLOTS, n), np.float32)
        pv[0] = h
        for k in range(1, SLOTS):
            pv[k] = np.round(np.where(prng.uniform(size=n) < 0.4, prng.uniform(0.05, 1.0, n), 0.0) if k % 3 == 2 else prng.uniform(0.0, 10.0, n), 2)
        fit = ld.make_fit("piecewiseTwo", CONFIGURED, POSITION, (float(t.min()), float(t.max())), 8)

        def timed(call, read_ms):
            ms = []
            for k in range(a.warmup + a.launches):
                call()
                if k >= a.warmup:
                    ms.append(read_ms(sf))
            return ms
        ms = timed(lambda: ld.interpolate(sf, "airT", "idw", x, y, h, t, area, fit, download=False), ld.kernel_ms)
        runs.append(dict(kernel=ld.KERNEL, stations=n, others=0, **stats(ms, "kernel_ms"), selected_mean=float(ld.get_selection(sf)["count"][inside].mean())))
        print(json.dumps(runs[-1]), flush=True)
        for k_others in (0, 1, 4, lp.MAX_OTHERS):
            proxies = [dict(active=1, isHeight=1)] + [dict(active=int(k <= k_others), isHeight=0) for k in range(1, SLOTS)]
            ms = timed(lambda: lp.interpolate(sf, "airT", "idw", x, y, t, pv, area, fit, proxies, others, download=False), lp.kernel_ms)
            count, kept = ld.get_selection(sf)["count"][inside], lp.get_interpolated(sf)[inside]
            sig = lp.get_proxy_fit(sf)["proxy_significant"][inside].sum(axis=1)
            runs.append(dict(kernel=lp.KERNEL, stations=n, others=k_others, **stats(ms, "kernel_ms"), cells_per_s=float(inside.sum() / (np.median(ms) * 1e-3)),
                             selected_mean=float(count.mean()), interpolated_mean=float(kept.mean()), significant_proxies_mean=float(sig.mean())))
            print(json.dumps(runs[-1]), flush=True)
    held = lp.bytes_held(sf)
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_localdetrend.inc", "sf3d_localproxies.inc",
                                                                                 "sf3d_localproxies_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=int(inside.sum()), cell_size=cs,
               launches=a.launches, warmup=a.warmup, minPointsLocalDetrending=8, function="piecewiseTwo", method="idw", first_guesses=len(fit["first_guess"]), runs=runs,
               bytes_held=held, fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
