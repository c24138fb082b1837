"""Time glocal detrending on the Ravone DEM (519 x 1208 cells), HIP events around each launch, medians of 20 launches after 3 warm-ups:
the 200 seeded stations of scripts/localproxies_timing.py (the same generator, drawn in the same order), lapseRatePiecewise_two with the
default range and the full first-guess list, idw, the height and two other proxies active on synthetic proxy rasters; 4 and 16 macro
areas - bands of columns that overlap their neighbours by half, each naming its share of the stations by their rank in x - and, beside them,
sf3d_localproxies_interpolate (local detrending, minPointsLocalDetrending 8) on the same stations and proxies.
usage: python scripts/glocal_timing.py [--launches 20] [--warmup 3] [--areas 4 16] [--out profiles/glocal_timing.json]"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                                           # noqa: E402
from criteria3d_amd import capi, glocal as gl, localdetrend as ld, localproxies as lp, meteo  # noqa: E402

CONFIGURED, POSITION = [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015], [0, 1, 1, 1]
SLOTS = meteo.MAX_PROXIES
OTHERS = 2


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def band_areas(shape, n_areas, x, xll, cs):
    """n_areas bands of columns, each reaching half a band into its neighbours, the weight falling off from the band's middle.  The
    stations lie far around the raster, so a band takes its share of them by rank: sorted by x, band a names the ranks from half a share
    before its own to half a share after it (2 n / n_areas stations away from the ends: every station is named by two bands)"""
    rows, cols = shape
    width = cols / n_areas
    order = np.argsort(x, kind="stable")
    out = []
    for a in range(n_areas):
        lo, hi = max(0, int((a - 0.5) * width)), min(cols, int((a + 1.5) * width))
        c = np.arange(lo, hi)
        w = np.round(0.2 + 0.8 * (1.0 - np.abs((c - (lo + hi - 1) / 2.0) / ((hi - lo) / 2.0))), 3).astype(np.float32)
        cells = (np.arange(rows)[:, None] * cols + c[None, :]).astype(np.float32)
        share = len(x) / n_areas
        named = order[max(0, int((a - 0.5) * share)):min(len(x), int((a + 1.5) * share))]
        out.append(dict(cells=cells.ravel(), weights=np.broadcast_to(w, cells.shape).ravel().copy(), stations=np.sort(named).astype(np.int32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--areas", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glocal_timing.json"))
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
    gl.bind(sf)
    meteo.initialize(sf, dem, xll, yll, cs, maps, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    rng = np.random.default_rng(24)
    others = lp.make_others([None] + [dict(range=[-1.0, -40.0, 1.0, 50.0])] * (SLOTS - 1))
    for n in (40, 200):                                                         # the generator's order: the 40 are drawn and dropped
        x = np.round(xll + rng.uniform(-20000.0, cols * cs + 20000.0, n), 2)
        y = np.round(yll + rng.uniform(-20000.0, rows * cs + 20000.0, n), 2)
        h = np.round(rng.uniform(20.0, 1500.0, n), 1).astype(np.float32)
        t = np.round(np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0)) + rng.normal(0.0, 0.6, n), 1).astype(np.float32)
    pv = np.zeros((SLOTS, n), np.float32)
    pv[0] = h
    for k in range(1, SLOTS):
        pv[k] = np.round(np.where(prng.uniform(size=n) < 0.4, prng.uniform(0.05, 1.0, n), 0.0) if k % 3 == 2 else prng.uniform(0.0, 10.0, n), 2)
    area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
    proxies = [dict(active=1, isHeight=1)] + [dict(active=int(k <= OTHERS), isHeight=0) for k in range(1, SLOTS)]
    fit = ld.make_fit("piecewiseTwo", CONFIGURED, POSITION, (float(t.min()), float(t.max())), 8)
    index = np.arange(n, dtype=np.int32)
    runs = []
    for n_areas in a.areas:
        gl.set_areas(sf, band_areas(dem.shape, n_areas, x, xll, cs))
        ms = []
        for k in range(a.warmup + a.launches):
            gl.interpolate(sf, "airT", "idw", index, x, y, t, pv, area, fit, proxies, others, download=False)
            if k >= a.warmup:
                ms.append(gl.kernel_ms(sf))
        got = gl.get_area_fit(sf)
        runs.append(dict(kernels=list(gl.KERNELS), stations=n, areas=n_areas, others=OTHERS, **stats([m[0] for m in ms], "areas_ms"), **stats([m[1] for m in ms], "cells_ms"),
                         fitted_mean=float(got["fitted"].mean()), kept_mean=float(got["kept"].mean()), height_significant=int(got["significant"].sum()),
                         bytes_held=gl.bytes_held(sf)))
        print(json.dumps(runs[-1]), flush=True)
    ms = []
    for k in range(a.warmup + a.launches):
        lp.interpolate(sf, "airT", "idw", x, y, t, pv, area, fit, proxies, others, download=False)
        if k >= a.warmup:
            ms.append(lp.kernel_ms(sf))
    runs.append(dict(kernels=[lp.KERNEL], stations=n, others=OTHERS, minPointsLocalDetrending=8, **stats(ms, "kernel_ms")))
    print(json.dumps(runs[-1]), flush=True)
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_localdetrend.inc", "sf3d_localproxies.inc", "sf3d_glocal.inc",
                                                                                 "sf3d_glocal_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(rows), cols=int(cols), cells=int(dem.size), valid_cells=int(inside.sum()), cell_size=cs, launches=a.launches, warmup=a.warmup,
               function="piecewiseTwo", method="idw", first_guesses=len(fit["first_guess"]), runs=runs, fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
