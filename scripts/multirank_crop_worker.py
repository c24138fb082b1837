"""One rank of a multi-rank run of the HIP product that runs the hourly ET0 / daily crop maps (include/sf3d_crop.h) on a window of the
Ravone project; all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the rank's maps after
the hours and after the day, the state before the first hour and the owner of every node (tests/test_gpu_crop.py merges them).
usage: python scripts/multirank_crop_worker.py <rank> <world> <port> <hours> <outfile>"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch.distributed as dist
from criteria3d_amd import capi, catchment as cm, crop, maps

rank, world, port, hours, outfile = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = str(port)
dist.init_process_group("gloo", rank=rank, world_size=world)


def allgather(b):
    out = [None] * world
    dist.all_gather_object(out, b)
    return out


from tests.scenarios import ravone_project_model          # noqa: E402
from tests import crop_cases as cc                          # noqa: E402
sf = capi.load_product()
sf.check(sf.lib.sf3d_set_device(int(os.environ.get("SF3D_TEST_DEVICE", "0"))), "set_device")
m = ravone_project_model((980, 1060, 330, 420))
sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
cm.build(sf, m, threads=1, dist=(rank, world, allgather))
maps.bind(sf)
col, thick = maps.columns(m)
sf.check(sf.lib.sf3d_set_output_columns(col.shape[1], col.shape[0], col.ctypes.data_as(maps.pi32), thick.ctypes.data_as(capi.pd)), "set_output_columns")
idx = np.asarray(m.meta["index"])[0]
flag = -9999.0
dem = np.where(idx >= 0, m.z[np.maximum(idx, 0)], flag).astype(np.float32)
units = cc.load_pin()["unit_list"]
unit_index = (np.arange(dem.size).reshape(dem.shape) % len(units)).astype(np.int32)
crop.initialize(sf, dem, unit_index, units, 44.5, flag)
crop.set_degree_days(sf, np.where(idx >= 0, np.float32(800.0), np.float32(flag)), 200)
res = {"owner": sf.owner_map(world, m.n)}
res.update({"initial_" + n: crop.get_state(sf, n) for n in crop.STATE})
for met in cc.small_forcing(dem.shape, dem, flag)[:hours]:
    crop.compute_hour(sf, met)
res.update({"hour_" + n: crop.get_state(sf, n) for n in crop.STATE})
res["et0"] = crop.get_et0(sf)
crop.daily_update(sf, 200)
res.update({n: crop.get_state(sf, n) for n in crop.STATE})
np.savez(outfile, **res)
dist.barrier()
sf.lib.sf3d_clean()
dist.destroy_process_group()
