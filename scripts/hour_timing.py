"""Time the raster stages of one hour on the Ravone DEM (519 x 1208 cells) over the DEM's node model, host-fed against in place, in the same
run: the humidity from the dew point, the snow hour, the ET0 hour, the roots, the sink hour and the hour's totals.  Host-fed: every
stage's input maps lie on the host and go through the host-pointer entry points (what a caller did before include/sf3d_hour.h; for the
humidity and the totals, which had no entry point, only the copies such a caller needs are timed - two maps down and one up, three maps
down - not its loop over the cells).  In place: the calls of include/sf3d_hour.h, nothing handed over.  Host clock around the calls, HIP
events for k_hour_relhum, k_hour_totals and k_hour_pond.  20 repetitions after 3 warm-ups, medians.  Recorded, not asserted.
usage: python scripts/hour_timing.py [--launches 20] [--warmup 3] [--out profiles/hour_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, catchment as cm, crop, hour, meteo, radiation as rad, root, sinks, snow  # noqa: E402


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hour_timing.json"))
    a = ap.parse_args()
    from tests import crop_cases as cc
    from tests import sink_cases as sc
    pin = sc.load_pin()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    valid = dem != np.float32(flag)
    rng = np.random.default_rng(21)
    f = lambda v: np.where(valid, v, flag).astype(np.float32)
    m = cm.dem_model_fast(dem, cell=4.0, nodata=flag, depth=0.95)
    thick = np.concatenate([[0.0], np.array(m.meta["layers"])])
    centre = np.concatenate([[0.0], np.cumsum(thick[1:]) - 0.5 * thick[1:]])
    columns = np.asarray(m.meta["index"]).astype(np.int32)
    r, c = np.mgrid[0:dem.shape[0], 0:dem.shape[1]]
    units, soils = pin["unit_list"], pin["soil_list"]
    crop_index = np.where(valid, c // 4 % len(units), -1).astype(np.int32)
    soil_index = np.where(valid, r // 8 % 2, -1).astype(np.int32)
    sf = capi.load_product()
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1)
    sinks.set_columns(sf, columns, thick)
    crop_units = cc.load_pin()["unit_list"]
    crop_units = [crop_units[k % len(crop_units)] for k in range(len(units))]
    xll, yll = 683000.0, 4927000.0
    header = dict(nrows=dem.shape[0], ncols=dem.shape[1], xllcorner=xll, yllcorner=yll, cellsize=4.0)
    lat, lon = rad.latlon_maps(header, dem=dem, flag=flag)
    slope, aspect = f(rng.uniform(0, 35, dem.shape)), f(rng.uniform(0, 360, dem.shape))
    meteo.initialize(sf, dem, xll, yll, 4.0, (), flag)
    rad.initialize(sf, dem, xll, yll, 4.0, f(lat), f(lon), slope, aspect, flag=flag)
    snow.initialize(sf, dem, flag)
    snow.set_state(sf, "swe", f(rng.uniform(0, 30, dem.shape)))
    snow.reset(sf)
    crop.initialize(sf, dem, crop_index, crop_units, 44.5, flag)
    crop.set_state(sf, "degreeDays", f(10.0 + ((r * 7 + c * 3) % 1500)))
    crop.set_state(sf, "lai", f(0.25 * ((r + 2 * c) % 17)))
    root.initialize(sf, dem, crop_index, soil_index, units, soils, centre, thick, flag)
    sinks.initialize(sf, dem, 4.0, crop_index, soil_index, pin["sink_units"], pin["sink_soils"], centre, thick, 0.95, flag)
    air = f(rng.uniform(2, 14, dem.shape))
    for name, v in (("airT", air), ("prec", f(rng.uniform(0, 3, dem.shape))), ("dewT", f(air - rng.uniform(0.5, 12, dem.shape))),
                    ("windInt", f(rng.uniform(0, 8, dem.shape))), ("transmissivity", f(rng.uniform(0.2, 0.72, dem.shape)))):
        meteo.set_map(sf, name, v)
    rad.compute_hour(sf, (2021, 3, 20, 10, 0, 0), None)
    hour.relative_humidity(sf, download=False)
    hour.set_ponds(sf, slope, crop_index, np.full(len(units), 0.01), np.full(len(units), 4.0), np.ones(len(units), np.int32), True, flag)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    names = ("humidity", "snow", "et0", "roots", "sinks", "totals")
    fed, placed = {n: [] for n in names}, {n: [] for n in names}
    kernels = dict(k_hour_relhum=[], k_hour_totals=[], k_hour_pond=[])

    def timed(store, name, call):
        t0 = time.perf_counter()
        out = call()
        store[name].append((time.perf_counter() - t0) * 1e3)
        return out
    for h in range(a.warmup + a.launches):
        f_, p_ = ({n: [] for n in names}, {n: [] for n in names}) if h < a.warmup else (fed, placed)
        # ---- host-fed: the maps lie on the host
        met = dict(airT=meteo.get_map(sf, "airT"), prec=meteo.get_map(sf, "prec"), relHum=meteo.get_map(sf, "relHum"), windInt=meteo.get_map(sf, "windInt"),
                   globalRad=rad.get_map(sf, "global"), beamRad=rad.get_map(sf, "beam"), transmissivity=meteo.get_map(sf, "transmissivity"), clearSkyTransmissivity=0.75)
        timed(f_, "humidity", lambda: (meteo.get_map(sf, "airT"), meteo.get_map(sf, "dewT"), meteo.set_map(sf, "relHum", met["relHum"])))
        timed(f_, "snow", lambda: snow.compute_hour(sf, met))
        timed(f_, "et0", lambda: crop.compute_hour(sf, met, 0.75))
        et0, lai, dd, liquid = crop.get_et0(sf), crop.get_state(sf, "lai"), crop.get_state(sf, "degreeDays"), snow.get_output(sf, "liquid")
        timed(f_, "roots", lambda: root.compute(sf, dd))
        timed(f_, "sinks", lambda: sinks.compute_hour(sf, et0, lai, dd, liquid))
        timed(f_, "totals", lambda: (sinks.get_actual(sf), snow.get_output(sf, "liquid")))
        # ---- in place
        timed(p_, "humidity", lambda: hour.relative_humidity(sf, download=False))
        if h >= a.warmup:
            kernels["k_hour_relhum"].append(hour.kernel_ms(sf, hour.KERNEL_RELHUM) * 1e3)
        timed(p_, "snow", lambda: hour.snow_hour(sf, None, 0.75))
        timed(p_, "et0", lambda: hour.et0_hour(sf, 0.75))
        timed(p_, "roots", lambda: root.compute(sf, None))
        timed(p_, "sinks", lambda: hour.sink_hour(sf))
        tot = timed(p_, "totals", lambda: hour.totals(sf))
        if h >= a.warmup:
            kernels["k_hour_totals"].append(hour.kernel_ms(sf, hour.KERNEL_TOTALS) * 1e3)
        hour.update_ponds(sf, download=False)
        if h >= a.warmup:
            kernels["k_hour_pond"].append(hour.kernel_ms(sf, hour.KERNEL_POND) * 1e3)
    sf.lib.sf3d_kernel_timing(0)
    sf.lib.sf3d_clean()
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / n).read_bytes() for n in ("sf3d_hour.inc", "sf3d_hour_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=int(valid.sum()), nodes=int(m.n),
               launches=a.launches, warmup=a.warmup, host_fed={n: stats(v, "call_ms") for n, v in fed.items()}, in_place={n: stats(v, "call_ms") for n, v in placed.items()},
               host_fed_hour_ms_median=float(sum(np.median(v) for v in fed.values())), in_place_hour_ms_median=float(sum(np.median(v) for v in placed.values())),
               kernels={n: stats(v, "kernel_us") for n, v in kernels.items()}, totals_m3_per_hour=[float(v) for v in tot],
               note="host_fed humidity and totals: the copies alone (2 maps down + 1 up; 2 double maps + 1 float map down), not the caller's loop over the cells",
               fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
