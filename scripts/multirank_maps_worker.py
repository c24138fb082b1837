"""One rank of a multi-rank run of the HIP product that takes the output maps (include/sf3d_maps.h) after a stretch of the 25 mm hour on a
window of the Ravone project; all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the
rank's maps, the owner of every node and the per-node getter values of the nodes it owns (tests/test_gpu_output_maps.py merges them).
usage: python scripts/multirank_maps_worker.py <rank> <world> <port> <steps> <outfile>    (SF3D_TEST_SPARSE_BUILD=1: strip-local build)"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch.distributed as dist
from criteria3d_amd import capi, catchment as cm, maps

rank, world, port, steps, outfile = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = str(port)
dist.init_process_group("gloo", rank=rank, world_size=world)


def allgather(b):
    out = [None] * world
    dist.all_gather_object(out, b)
    return out


from tests.scenarios import ravone_project_model          # noqa: E402
sf = capi.load_product()
sf.check(sf.lib.sf3d_set_device(int(os.environ.get("SF3D_TEST_DEVICE", "0"))), "set_device")
m = ravone_project_model((980, 1060, 330, 420))
sparse = os.environ.get("SF3D_TEST_SPARSE_BUILD") == "1"
sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
cm.build(sf, m, threads=1, dist=(rank, world, allgather), sparse=sparse)
cm.run_hour(sf, m, 25.0, max_steps=steps)
maps.set_output(sf, m)
res = {"owner": sf.owner_map(world, m.n)}
for var in maps.LAYER_VARIABLES + (maps.FACTOR_OF_SAFETY,) + maps.COLUMN_VARIABLES:
    res[f"map_{var}"] = maps.output_maps(sf, m, var)
mine = np.nonzero(res["owner"] == rank)[0]
for var, name in maps.GETTERS.items():
    fn = getattr(sf.lib, name)
    res[f"get_{var}"] = np.array([fn(int(i), maps.FIELD_CAPACITY) if var == maps.WATER_DEFICIT else fn(int(i)) for i in mine], np.float64)
res["mine"] = mine
np.savez(outfile, **res)
dist.barrier()
sf.lib.sf3d_clean()
dist.destroy_process_group()
