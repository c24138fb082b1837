"""Time topographic distance on the Ravone DEM (519 x 1208 cells), HIP events around each launch, medians of 20 launches after 3 warm-ups:
k_topodist_maps for 16 and 64 stations placed in and around the raster, with the number of DEM samples the walks take (counted on the host
from the float distances, as gis::topographicDistance counts its steps); k_meteo_idw_td against k_meteo_idw for the same station list and
method (air temperature with the height proxy, Kh 10), once with every station carrying its map (a look-up per cell and station) and once
map-less (a walk per cell and station, two for the Shepard methods, whose neighbour search asks for every distance twice).
usage: python scripts/topodist_timing.py [--launches 20] [--warmup 3] [--out profiles/topodist_timing.json]"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, meteo, topodist             # noqa: E402

KH = 10


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def samples_walked(dem, flag, xll, yll, cs, x, y) -> int:
    """sum over DEM cells and stations of nrStep = int(distance / float(cellSize)) (0 below one cell size)"""
    cx, cy = meteo.cell_centres(dem.shape, xll, yll, cs)
    valid = dem != np.float32(flag)
    gx, gy = cx[valid].astype(np.float32), cy[valid].astype(np.float32)
    total = 0
    for sx, sy in zip(x.astype(np.float32), y.astype(np.float32)):
        dx, dy = sx - gx, sy - gy
        d = np.sqrt(dx * dx + dy * dy)
        total += int(np.trunc(d / np.float32(cs))[d >= np.float32(cs)].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topodist_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    cs, xll, yll = float(z["cellsize"]), float(z["xllcorner"]), float(z["yllcorner"])
    valid = int((dem != np.float32(flag)).sum())
    sf = capi.load_product()
    meteo.initialize(sf, dem, xll, yll, cs, [None], flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    settings = dict(rainfallThreshold=0.2, useTopographicDistance=1, proxies=[dict(active=1, isHeight=1, inversion=0, slope=-0.0065)])
    rng = np.random.default_rng(22)
    low, high = float(dem[dem != np.float32(flag)].min()), float(dem[dem != np.float32(flag)].max())
    maps_runs, idw_runs = [], []
    for n in (16, 64):
        x = np.round(xll + rng.uniform(-0.2, 1.2, n) * dem.shape[1] * cs, 3)
        y = np.round(yll + rng.uniform(-0.2, 1.2, n) * dem.shape[0] * cs, 3)
        zs = np.round(rng.uniform(low, high, n), 1)
        v = np.round(rng.uniform(4.0, 26.0, n), 2).astype(np.float32)
        area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
        walked = samples_walked(dem, flag, xll, yll, cs, x, y)
        ms = []
        for h in range(a.warmup + a.launches):
            topodist.compute(sf, x, y, zs)
            if h >= a.warmup:
                ms.append(topodist.kernel_ms(sf, "k_topodist_maps"))
        med = float(np.median(ms)) * 1e-3
        maps_runs.append(dict(stations=n, dem_samples_walked=walked, **stats(ms, "kernel_ms"), dem_samples_per_s=float(walked / med),
                              maps_bytes=topodist.bytes_held(sf)))
        every, none = np.arange(n, dtype=np.int32), np.full(n, -1, np.int32)
        for method in ("idw", "shepard"):
            plain = []
            for h in range(a.warmup + a.launches):
                meteo.interpolate(sf, "airT", method, x, y, v, area, dict(settings, useTopographicDistance=0), download=False)
                if h >= a.warmup:
                    plain.append(meteo.kernel_ms(sf))
            row = dict(stations=n, method=method, kh=KH, **stats(plain, "k_meteo_idw_ms"))
            for name, index in (("with_maps", every), ("map_less", none)):
                ms = []
                for h in range(a.warmup + a.launches):
                    topodist.interpolate(sf, "airT", method, x, y, zs, v, index, area, settings, KH, download=False)
                    if h >= a.warmup:
                        ms.append(topodist.kernel_ms(sf, "k_meteo_idw_td"))
                row.update(stats(ms, f"k_meteo_idw_td_{name}_ms"))
            row["map_less_dem_samples_walked"] = walked * (1 if method == "idw" else 2)
            idw_runs.append(row)
    sf.lib.sf3d_kernel_timing(0)
    meteo.clean(sf)
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_meteo.inc", "sf3d_topodist.inc", "sf3d_topodist_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=valid, cell_size=cs, launches=a.launches,
               warmup=a.warmup, k_topodist_maps=maps_runs, k_meteo_idw_td=idw_runs, measured_on_host="not measured", fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
