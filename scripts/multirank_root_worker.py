"""One rank of a multi-rank run of the HIP product that computes the root maps (include/sf3d_root.h) on the 24 x 32 raster of the root
pin, over a catchment model of the same raster; all ranks may share one GPU.  The control plane is torch.distributed with the gloo
backend.  Saves the rank's maps and the owner of every node (tests/test_gpu_root.py merges them).
usage: python scripts/multirank_root_worker.py <rank> <world> <port> <map> <outfile>"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch.distributed as dist
from criteria3d_amd import capi, catchment as cm, maps, root

rank, world, port, which, outfile = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = str(port)
dist.init_process_group("gloo", rank=rank, world_size=world)


def allgather(b):
    out = [None] * world
    dist.all_gather_object(out, b)
    return out


from tests import root_cases as rc                          # noqa: E402
sf = capi.load_product()
sf.check(sf.lib.sf3d_set_device(int(os.environ.get("SF3D_TEST_DEVICE", "0"))), "set_device")
pin = rc.load_pin()
rows, cols = pin["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
cm.build(sf, m, threads=1, dist=(rank, world, allgather))
maps.bind(sf)
col, thick = maps.columns(m)
sf.check(sf.lib.sf3d_set_output_columns(col.shape[1], col.shape[0], col.ctypes.data_as(maps.pi32), thick.ctypes.data_as(capi.pd)), "set_output_columns")
rc.initialize(sf, pin)
root.compute(sf, pin["degree_days"][which])
res = root.all_maps(sf)
res["keys"] = root.get_keys(sf)
res["owner"] = sf.owner_map(world, m.n)
np.savez(outfile, **res)
dist.barrier()
sf.lib.sf3d_clean()
dist.destroy_process_group()
