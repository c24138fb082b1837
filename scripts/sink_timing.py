"""Time the hourly water sinks on the Ravone DEM (519 x 1208 cells) over the DEM's node model: k_sink_hour alone (HIP events around the
launch), the sf3d_sink_compute_hour call with every input resident on the device (NULL maps: the crop, snow and root blocks), and
sf3d_sink_apply, beside the path they replace, measured in the same run: sf3d_root_get_density of all layers (the download a host-side
assembly starts with) plus the upload of N sinks through sf3d_set_node_water_sink_source node by node.  20 launches after 3 warm-ups.
Then an hour of 10 mm rain with soil cracking (sf3d_sink_set_cracking: k_sink_hour_crack) and without, alternating, on the same inputs; the
soil nodes are dry (-800 / -150 m in alternate layers) so that the two clay soils of the raster do crack.  --library times another build of
the product library (the parent commit's, for one): a library without sf3d_sink_set_cracking gives the plain hour only.
usage: python scripts/sink_timing.py [--launches 20] [--warmup 3] [--library libsf3d_hip.so] [--out profiles/sink_C5_timing.json]"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np                                           # noqa: E402
from criteria3d_amd import capi, catchment as cm, crop, root, sinks, snow  # noqa: E402


def stats(v, unit):
    return {f"{unit}_min": float(min(v)), f"{unit}_median": float(np.median(v)), f"{unit}_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sink_C5_timing.json"))
    ap.add_argument("--library", default=None, help="another build of the product library (default: the tree's)")
    a = ap.parse_args()
    from tests import crop_cases as cc
    from tests import sink_cases as sc
    from tests.snow_cases import melt_forcing
    pin = sc.load_pin()
    z = np.load(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")
    dem, flag = z["dem"].astype(np.float32), float(z["nodata"])
    valid = dem != np.float32(flag)
    m = cm.dem_model_fast(dem, cell=4.0, nodata=flag, depth=0.95)
    thick = np.concatenate([[0.0], np.array(m.meta["layers"])])
    centre = np.concatenate([[0.0], np.cumsum(thick[1:]) - 0.5 * thick[1:]])
    columns = np.asarray(m.meta["index"]).astype(np.int32)
    r, c = np.mgrid[0:dem.shape[0], 0:dem.shape[1]]
    units, soils = pin["unit_list"], pin["soil_list"]
    crop_index = np.where(valid, c // 4 % len(units), -1).astype(np.int32)
    soil_index = np.where(valid, r // 8 % 2, -1).astype(np.int32)          # the two deep soils of the pin
    dd = np.where(valid, (10.0 + ((r * 7 + c * 3) % 1500)), flag).astype(np.float32)
    lai = np.where(valid, 0.25 * ((r + 2 * c) % 17), flag).astype(np.float32)
    sf = capi.SF3D(Path(a.library).resolve()) if a.library else capi.load_product()
    if not hasattr(sf.lib, "sf3d_sink_set_cracking"):         # a build from before soil cracking: bind what it has
        for name in [k for k in sinks.SIGNATURES if "crack" in k]:
            del sinks.SIGNATURES[name]
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1)
    layer_of_node = np.repeat(np.arange(len(thick)), [int(np.count_nonzero(columns[l] >= 0)) for l in range(len(thick))])
    assert len(layer_of_node) == m.n and np.all(np.diff(columns[columns >= 0]) > 0)      # layer-major numbering
    psi = np.where(layer_of_node % 2 == 1, -800.0, -150.0)    # dry soil nodes
    psi[:m.ns] = 0.0
    sf.set_matric_potential_bulk(0, psi)
    sinks.set_columns(sf, columns, thick)
    crop_units = cc.load_pin()["unit_list"]
    snow.initialize(sf, dem, flag)
    crop.initialize(sf, dem, np.where(crop_index < 0, 0, crop_index) % len(crop_units), crop_units, 44.5, flag)
    root.initialize(sf, dem, crop_index, soil_index, units, soils, centre, thick, flag)
    sinks.initialize(sf, dem, 4.0, crop_index, soil_index, pin["sink_units"], pin["sink_soils"], centre, thick, 0.95, flag)
    for met in melt_forcing(dem.shape, dem, flag)[11:13]:
        snow.compute_hour(sf, met)
        crop.compute_hour(sf, None)
    crop.set_state(sf, "degreeDays", dd)
    crop.set_state(sf, "lai", lai)
    root.compute(sf, None)
    sf.check(sf.lib.sf3d_kernel_timing(1), "timing")
    kernel_us, call_ms, apply_ms, density_ms, setter_ms = [], [], [], [], []
    for h in range(a.warmup + a.launches):
        t0 = time.perf_counter()
        sinks.compute_hour(sf, None, None, None, None)
        t1 = time.perf_counter()
        sinks.apply(sf)
        t2 = time.perf_counter()
        if h >= a.warmup:
            kernel_us.append(sinks.kernel_ms(sf) * 1e3); call_ms.append((t1 - t0) * 1e3); apply_ms.append((t2 - t1) * 1e3)
    q = sinks.get_node_sinks(sf, m.n)
    evaporation, transpiration = sinks.get_actual(sf)
    cracked = None
    if hasattr(sf.lib, "sf3d_sink_set_cracking"):             # the cracked hour and the plain hour in turn, on the same inputs
        from tests.golden.make_soil_cracking import TEXTURE
        crack_soils = [dict(totalDepth=so["totalDepth"], clay=[t[0] for t in tx], silt=[t[1] for t in tx], coarseFragments=[1.0 - f for f in so["soilFraction"]],
                            organicMatter=[t[2] for t in tx]) for so, tx in zip(soils, TEXTURE)]
        crack_us, plain_us = [], []
        rain = np.where(valid, 10.0, flag).astype(np.float32)      # [mm]: more than the ponds hold (2 mm), so that the dry clay does crack
        for h in range(a.warmup + a.launches):
            sinks.set_cracking(sf, crack_soils)
            sinks.compute_hour(sf, None, None, None, rain)
            if h >= a.warmup:
                crack_us.append(sinks.kernel_ms(sf) * 1e3)
            if h == a.warmup + a.launches - 1:
                prec_surface, crack_water = sinks.get_crack(sf)
                q_crack = sinks.get_node_sinks(sf, m.n)
            sinks.set_cracking(sf, None)
            sinks.compute_hour(sf, None, None, None, rain)
            if h >= a.warmup:
                plain_us.append(sinks.kernel_ms(sf) * 1e3)
        q_plain = sinks.get_node_sinks(sf, m.n)
        assert np.array_equal(q_plain[m.ns:], q[m.ns:])              # cracking off again: below the surface the plain hour's bits
        q = q_plain
        cracked = dict(rain_mm=10.0, k_sink_hour_crack=stats(crack_us, "kernel_us"), k_sink_hour_alternating=stats(plain_us, "kernel_us"),
                       cells_cracking=int(np.count_nonzero((crack_water != flag) & (crack_water > 0))),
                       nodes_filled=int(np.count_nonzero(q_crack[m.ns:] > q[m.ns:])))
    for h in range(max(3, a.launches // 4)):                  # the replaced path: the density download, then N single setters
        t0 = time.perf_counter()
        root.get_density(sf, -1)
        t1 = time.perf_counter()
        sf.set_sink_source_bulk(0, q)                         # sf3d_set_nodes_water_sink_source: the node-by-node setter in one C loop
        t2 = time.perf_counter()
        if h >= 1:
            density_ms.append((t1 - t0) * 1e3); setter_ms.append((t2 - t1) * 1e3)
    sf.lib.sf3d_kernel_timing(0)
    sf.lib.sf3d_clean()
    src = b"".join((ROOT / "criteria3d_amd" / "csrc" / f).read_bytes() for f in ("sf3d_sink.inc", "sf3d_sink_api.inc"))
    res = dict(workload="Ravone DEM", rows=int(dem.shape[0]), cols=int(dem.shape[1]), cells=int(dem.size), valid_cells=int(valid.sum()), nodes=int(m.n),
               layers=int(len(thick)), launches=a.launches, warmup=a.warmup,
               k_sink_hour=stats(kernel_us, "kernel_us"), compute_call_inputs_resident=stats(call_ms, "call_ms"), apply_call=stats(apply_ms, "call_ms"),
               replaced_path=dict(root_get_density_all_layers=stats(density_ms, "call_ms"), upload_of_n_sinks_through_the_setter=stats(setter_ms, "call_ms")),
               nodes_with_a_sink=int(np.count_nonzero(q)), cells_evaporating=int(np.count_nonzero((evaporation != flag) & (evaporation > 0))),
               cells_transpiring=int(np.count_nonzero((transpiration != flag) & (transpiration > 0))), soil_cracking=cracked,
               library=Path(a.library).name if a.library else "libsf3d_hip.so", fingerprint=hashlib.sha256(src).hexdigest()[:16])
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
