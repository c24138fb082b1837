"""One rank of a multi-rank run of the HIP product that runs the hourly snow model (include/sf3d_snow.h) on a window of the Ravone project;
all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the rank's thirteen maps, the state
before the first hour and the owner of every node (tests/test_gpu_snow.py merges them).
usage: python scripts/multirank_snow_worker.py <rank> <world> <port> <hours> <outfile>"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch.distributed as dist
from criteria3d_amd import capi, catchment as cm, maps, snow

rank, world, port, hours, outfile = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = str(port)
dist.init_process_group("gloo", rank=rank, world_size=world)


def allgather(b):
    out = [None] * world
    dist.all_gather_object(out, b)
    return out


from tests.scenarios import ravone_project_model          # noqa: E402
from tests.snow_cases import melt_forcing                   # noqa: E402
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
snow.initialize(sf, dem, flag)
res = {"owner": sf.owner_map(world, m.n)}
res.update({"initial_" + n: snow.get_state(sf, n) for n in snow.STATE})
for met in melt_forcing(dem.shape, dem, flag)[:hours]:
    snow.compute_hour(sf, met)
res.update(snow.all_maps(sf))
np.savez(outfile, **res)
dist.barrier()
sf.lib.sf3d_clean()
dist.destroy_process_group()
