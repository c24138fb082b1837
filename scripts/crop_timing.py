"""Time the hourly ET0 / daily crop maps on the Ravone DEM (519 x 1208 cells): k_et0_hour and k_crop_day alone (HIP events around the
launch), the sf3d_crop_compute_hour call with its five H2D copies against the call that reads the maps sf3d_snow_compute_hour left on
the device (host clock), and - for scale only - the numpy restatements of criteria3d_amd.crop on the same grid, NOT the reference's
OpenMP loops.
usage: python scripts/crop_timing.py [--launches 20] [--warmup 3] [--out profiles/crop_C5_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, crop, project3d as p3, snow  # noqa: E402

ET0_BYTES_PER_CELL = 11 * 4                                  # 8 floats read (5 inputs, DEM, 2 extremes), 3 written
DAY_BYTES_PER_CELL = 10 * 4                                  # DEM, crop index, 4 state maps read; 4 state maps written
HBM_BYTES_PER_S = 8e12


def forcing(dem, flag, hour, rng):
    valid = dem != np.float32(flag)
    f = lambda v: np.where(valid, v, flag).astype(np.float32)
    shape = dem.shape
    return dict(airT=f(8.0 + 0.5 * hour + rng.uniform(-2, 2, shape)), relHum=f(rng.uniform(40, 100, shape)), windInt=f(rng.uniform(0, 8, shape)),
                globalRad=f(rng.uniform(0, 500, shape)), transmissivity=f(rng.uniform(0.1, 0.8, shape)))


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crop_C5_timing.json"))
    a = ap.parse_args()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    inp = p3.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz")
    units = p3.crop_table(json.loads((ROOT / "tests" / "golden" / "ravone_crops.json").read_text())["crop"], inp.land_units)
    unit_index = p3.land_unit_index(inp).astype(np.int32)
    assert unit_index.shape == dem.shape
    rng = np.random.default_rng(5)
    sf = capi.load_product()
    crop.initialize(sf, dem, unit_index, units, 44.5, flag)
    crop.set_degree_days(sf, np.where(dem != np.float32(flag), np.float32(900.0), np.float32(flag)), 150)
    snow.initialize(sf, dem, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    n = a.warmup + a.launches
    et0_us, day_us, call_ms, reuse_ms, day_call_ms = [], [], [], [], []
    for h in range(n):
        met = forcing(dem, flag, h, rng)
        t0 = time.perf_counter()
        crop.compute_hour(sf, met)
        t1 = time.perf_counter()
        if h >= a.warmup:
            et0_us.append(crop.kernel_ms(sf, crop.KERNEL_ET0_HOUR) * 1e3)
            call_ms.append((t1 - t0) * 1e3)
    explicit = crop.get_et0(sf)
    snow.compute_hour(sf, dict(met, prec=met["relHum"] * np.float32(0), beamRad=met["globalRad"], clearSkyTransmissivity=0.75))
    for h in range(n):
        t0 = time.perf_counter()
        crop.compute_hour(sf, None)
        t1 = time.perf_counter()
        if h >= a.warmup:
            reuse_ms.append((t1 - t0) * 1e3)
    same = bool(np.array_equal(explicit.view(np.uint32), crop.get_et0(sf).view(np.uint32)))
    state = {k: crop.get_state(sf, k) for k in crop.STATE}
    for d in range(n):
        crop.set_state(sf, "dailyTmin", state["dailyTmin"])
        crop.set_state(sf, "dailyTmax", state["dailyTmax"])
        t0 = time.perf_counter()
        crop.daily_update(sf, 150 + d)
        t1 = time.perf_counter()
        if d >= a.warmup:
            day_us.append(crop.kernel_ms(sf, crop.KERNEL_CROP_DAY) * 1e3)
            day_call_ms.append((t1 - t0) * 1e3)
    sf.lib.sf3d_kernel_timing(0)
    lai = crop.get_state(sf, "lai")
    snow.clean(sf)
    crop.clean(sf)
    # host figure: the numpy restatements on the whole grid, once
    t0 = time.perf_counter()
    crop.restate_et0_hour(dem, met, flag)
    crop.restate_daily_temperatures(state["dailyTmin"], state["dailyTmax"], met["airT"], flag)
    host_hour = time.perf_counter() - t0
    t0 = time.perf_counter()
    crop.restate_crop_day(state, dem, unit_index, units, 44.5, 150, 150, flag)
    host_day = time.perf_counter() - t0
    cells = dem.size
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_crop.inc", "sf3d_crop_api.inc"))
    frac = lambda per_cell, us: float(cells * per_cell / (np.median(us) * 1e-6) / HBM_BYTES_PER_S)
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(cells), valid_cells=int((dem != np.float32(flag)).sum()),
               launches=a.launches, warmup=a.warmup, measured_on_gpu=dict(
                   k_et0_hour=dict(stats(et0_us, "kernel_us"), model_bytes=int(cells * ET0_BYTES_PER_CELL), fraction_of_8TBps=frac(ET0_BYTES_PER_CELL, et0_us)),
                   k_crop_day=dict(stats(day_us, "kernel_us"), model_bytes=int(cells * DAY_BYTES_PER_CELL), fraction_of_8TBps=frac(DAY_BYTES_PER_CELL, day_us)),
                   hourly_call_with_its_five_uploads=stats(call_ms, "call_ms"), hourly_call_reading_the_snow_uploads=stats(reuse_ms, "call_ms"),
                   daily_call=stats(day_call_ms, "call_ms"), et0_of_both_hourly_calls_equal=same, cells_with_lai=int((lai > 0).sum())),
               measured_on_host=dict(what="criteria3d_amd.crop restatements (numpy, the C library's exp / pow element by element, one thread; not the reference's OpenMP loops)",
                                     seconds_per_hour=float(host_hour), seconds_per_day=float(host_day)),
               fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
