"""Time multiple detrending without areas on the Ravone DEM (519 x 1208 cells), HIP events around each launch, medians of 20 launches
after 3 warm-ups: the set-up of scripts/glocal_timing.py - its 200 seeded stations (the same generator, drawn in the same order),
lapseRatePiecewise_two with the default range and the full first-guess list, idw, the height and two other proxies active on the same
synthetic proxy rasters.  k_multidetrend_fit and k_multidetrend_cells at 200 stations, next to k_glocal_areas / k_glocal_cells and
k_localdetrend_proxies of profiles/glocal_timing.json on the same stations (read from that file, not measured again); the fit once more
at 1 024 stations (the 200 and 824 more of the same generator); and k_multidetrend_points at the 200 stations' own places.
usage: python scripts/multidetrend_timing.py [--launches 20] [--warmup 3] [--out profiles/multidetrend_timing.json]"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                           # noqa: E402
from criteria3d_amd import capi, localdetrend as ld, localproxies as lp, meteo, multidetrend as md  # noqa: E402

CONFIGURED, POSITION = [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1]
SLOTS = meteo.MAX_PROXIES
OTHERS = 2


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multidetrend_timing.json"))
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
            m = 2.0 + 0.01 * k * c_ + 0.004 * r_
        elif k % 3 == 2:
            m = np.where(prng.uniform(size=dem.shape) < 0.4, prng.uniform(0.05, 1.0, dem.shape), 0.0)
        else:
            m = np.sin(0.01 * k * c_) * np.cos(0.013 * r_)
        maps.append(np.round(m, 3).astype(np.float32))
    sf = capi.load_product()
    md.bind(sf)
    meteo.initialize(sf, dem, xll, yll, cs, maps, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    rng = np.random.default_rng(24)
    others = lp.make_others([None] + [dict(range=[-1.0, -40.0, 1.0, 50.0])] * (SLOTS - 1))

    def draw(n):
        x = np.round(xll + rng.uniform(-20000.0, cols * cs + 20000.0, n), 2)
        y = np.round(yll + rng.uniform(-20000.0, rows * cs + 20000.0, n), 2)
        h = np.round(rng.uniform(20.0, 1500.0, n), 1).astype(np.float32)
        t = np.round(np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0)) + rng.normal(0.0, 0.6, n), 1).astype(np.float32)
        return x, y, h, t

    def proxy_table(h):
        pv = np.zeros((SLOTS, len(h)), np.float32)
        pv[0] = h
        for k in range(1, SLOTS):
            pv[k] = np.round(np.where(prng.uniform(size=len(h)) < 0.4, prng.uniform(0.05, 1.0, len(h)), 0.0) if k % 3 == 2 else prng.uniform(0.0, 10.0, len(h)), 2)
        return pv

    draw(40)                                                                    # the generator's order: the 40 are drawn and dropped
    x, y, h, t = draw(200)
    pv = proxy_table(h)
    more = draw(meteo.MAX_STATIONS - 200)
    x4, y4, h4, t4 = (np.concatenate([p, q]) for p, q in zip((x, y, h, t), more))
    pv4 = np.concatenate([pv, proxy_table(more[2])], axis=1)
    proxies = [dict(active=1, isHeight=1)] + [dict(active=int(k <= OTHERS), isHeight=0) for k in range(1, SLOTS)]
    runs = []
    for sx, sy, st, spv in ((x, y, t, pv), (x4, y4, t4, pv4)):
        n = len(sx)
        area = np.float32((np.float32(sx.max()) - np.float32(sx.min())) * (np.float32(sy.max()) - np.float32(sy.min())))
        fit = ld.make_fit("piecewiseTwo", CONFIGURED, POSITION, (float(st.min()), float(st.max())), 8)
        ms = []
        for k in range(a.warmup + a.launches):
            md.interpolate(sf, "airT", "idw", sx, sy, st, spv, area, fit, proxies, others, download=False)
            md.points(sf, sx, sy, spv[0], spv)
            if k >= a.warmup:
                ms.append(md.kernel_ms(sf))
        got = md.get_fit(sf)
        runs.append(dict(kernels=list(md.KERNELS), stations=n, others=OTHERS, **stats([m[0] for m in ms], "fit_ms"), **stats([m[1] for m in ms], "cells_ms"),
                         **stats([m[2] for m in ms], "points_ms"), points=n, kept=got["kept"], height_significant=int(got["significant"]),
                         proxies_significant=int(got["proxy_significant"].sum()), fit_share_of_the_call=float(np.median([m[0] / (m[0] + m[1]) for m in ms])),
                         bytes_held=md.bytes_held(sf)))
        print(json.dumps(runs[-1]), flush=True)
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    beside = json.loads((ROOT / "profiles" / "glocal_timing.json").read_text())["runs"]
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_localdetrend.inc", "sf3d_localproxies.inc", "sf3d_multidetrend.inc",
                                                                                 "sf3d_multidetrend_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(rows), cols=int(cols), cells=int(dem.size), valid_cells=int(inside.sum()), cell_size=cs, launches=a.launches, warmup=a.warmup,
               function="piecewiseTwo", method="idw", first_guesses=len(fit["first_guess"]), runs=runs, beside_from_glocal_timing=beside,
               fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
