"""Time the root maps on the Ravone DEM (519 x 1208 cells) with the project's land-unit and soil maps: k_root_cell alone (HIP events
around the launch), the one-off k_root_table build, k_root_gather for all layers, the sf3d_root_compute call with its degree-day upload
against the call that reads the crop block's map (host clock), the number of distinct (unit, soil, rooted atoms) keys against the cell
count, and - for scale only - the Python restatement of criteria3d_amd.root on a sample of rows, NOT the reference's loop.  The Ravone
crops are trees (static roots: one key per pair); a second scenario puts the growing units of the root pin on the same DEM.
usage: python scripts/root_timing.py [--launches 20] [--warmup 3] [--out profiles/root_C5_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, crop, project3d as p3, root  # noqa: E402

CELL_BYTES_PER_CELL = 4 * 4 + 2 * 8 + 3 * 4                  # DEM, degree days, two indices read; length, depth, first, last, key written
HBM_BYTES_PER_S = 8e12


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def scenario(sf, name, dem, flag, crop_index, soil_index, units, soils, layer_depth, layer_thickness, dd, a, crop_units=None):
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    t0 = time.perf_counter()
    root.initialize(sf, dem, crop_index, soil_index, units, soils, layer_depth, layer_thickness, flag)
    init_ms = (time.perf_counter() - t0) * 1e3
    table_us = root.kernel_ms(sf, root.KERNEL_TABLE) * 1e3
    n = a.warmup + a.launches
    cell_us, call_ms, reuse_ms, gather_us, gather_call_ms = [], [], [], [], []
    for h in range(n):
        t0 = time.perf_counter()
        root.compute(sf, dd)
        t1 = time.perf_counter()
        if h >= a.warmup:
            cell_us.append(root.kernel_ms(sf, root.KERNEL_CELL) * 1e3)
            call_ms.append((t1 - t0) * 1e3)
    uploaded = root.get_length(sf)
    keys = root.get_keys(sf)
    same = None
    if crop_units is not None:                               # the crop block on the same raster holds the degree days: NULL form
        crop.initialize(sf, dem, np.where(crop_index < 0, 0, crop_index).astype(np.int32), crop_units, 44.5, flag)
        crop.set_state(sf, "degreeDays", dd)
        for h in range(n):
            t0 = time.perf_counter()
            root.compute(sf, None)
            t1 = time.perf_counter()
            if h >= a.warmup:
                reuse_ms.append((t1 - t0) * 1e3)
        same = bool(np.array_equal(uploaded.view(np.uint64), root.get_length(sf).view(np.uint64)))
        crop.clean(sf)
    for h in range(max(3, a.launches // 4)):
        t0 = time.perf_counter()
        dens = root.get_density(sf, -1)
        t1 = time.perf_counter()
        if h >= 1:
            gather_us.append(root.kernel_ms(sf, root.KERNEL_GATHER) * 1e3)
            gather_call_ms.append((t1 - t0) * 1e3)
    sf.lib.sf3d_kernel_timing(0)
    rows = root.table_rows(sf)
    root.clean(sf)
    cells = dem.size
    computed = int((keys >= 0).sum())
    res = dict(scenario=name, computed_cells=computed, distinct_keys=int(len(np.unique(keys[keys >= 0]))), table_rows=int(rows), layers=int(len(layer_depth)),
               k_root_cell=dict(stats(cell_us, "kernel_us"), model_bytes=int(cells * CELL_BYTES_PER_CELL),
                                fraction_of_8TBps=float(cells * CELL_BYTES_PER_CELL / (np.median(cell_us) * 1e-6) / HBM_BYTES_PER_S)),
               k_root_table_once=dict(kernel_us=float(table_us), initialize_call_ms=float(init_ms)),
               k_root_gather_all_layers=dict(stats(gather_us, "kernel_us"), **stats(gather_call_ms, "call_with_d2h_ms")),
               compute_call_with_its_upload=stats(call_ms, "call_ms"), cells_with_density=int((dens.max(axis=0) > 0).sum()))
    if reuse_ms:
        res["compute_call_reading_the_crop_block"] = stats(reuse_ms, "call_ms")
        res["length_of_both_calls_equal"] = same
    return res, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "root_C5_timing.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from tests import root_cases as rc
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    inp = p3.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz")
    rows = json.loads((ROOT / "tests" / "golden" / "ravone_crops.json").read_text())["crop"]
    units = p3.root_table(rows, inp.land_units)
    crop_units = p3.crop_table(rows, inp.land_units)
    soils = p3.soil_root_table(inp.soils)
    unit_index = p3.land_unit_index(inp).astype(np.int32)
    unit_index[np.isin(unit_index, [k for k, u in enumerate(units) if not u["isCrop"]])] = -1          # isCrop: no transpiration, no roots
    by_id = {int(s["id"]): k for k, s in enumerate(inp.soils)}
    soil_index = np.vectorize(lambda v: by_id.get(int(v), -1))(inp.soil_map).astype(np.int32)          # setSoilIndexMap
    thickness, centre = p3.soil_layers(0.95)
    valid = dem != np.float32(flag)
    r, c = np.mgrid[0:dem.shape[0], 0:dem.shape[1]]
    dd = np.where(valid, (10.0 + ((r * 7 + c * 3) % 1500)).astype(np.float32), np.float32(flag)).astype(np.float32)
    sf = capi.load_product()
    project, _ = scenario(sf, "the project's land units (trees: static roots)", dem, flag, unit_index, soil_index, units, soils, centre, thickness, dd, a, crop_units)
    pin = rc.load_pin()
    stripes = np.where(valid, (c // 4 % len(pin["unit_list"])), -1).astype(np.int32)
    growing, keys = scenario(sf, "the eight units of the root pin in stripes (growing roots)", dem, flag, stripes, soil_index, pin["unit_list"], soils, centre,
                             thickness, dd, a)
    # host figure: the Python restatement on 8 rows, scaled
    r0 = dem.shape[0] // 2
    t0 = time.perf_counter()
    root.restate_root_maps(dem[r0:r0 + 8], stripes[r0:r0 + 8], soil_index[r0:r0 + 8], pin["unit_list"], soils, centre, thickness, dd[r0:r0 + 8], flag)
    host = (time.perf_counter() - t0) * dem.shape[0] / 8
    # what the per-cell form would evaluate every hour: two exp per rooted atom and pass of a cardioid cell (one pass suffices when the thin layers are stored)
    n_of_key = keys[keys >= 0]
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_root.inc", "sf3d_root_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=int(valid.sum()), launches=a.launches,
               warmup=a.warmup, measured_on_gpu=[project, growing],
               measured_on_host=dict(what="criteria3d_amd.root restatement (plain Python doubles, one density vector per distinct (unit, soil, length), one thread; scaled "
                                          "from 8 rows; not the reference's loop)", seconds_per_hour=float(host)),
               computed_cells_per_distinct_key=float(len(n_of_key) / max(len(np.unique(n_of_key)), 1)), fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
