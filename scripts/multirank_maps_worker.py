"""One rank of a multi-rank run of the HIP product that takes the output maps (include/sf3d_maps.h) after a stretch of the 25 mm hour on a
window of the Ravone project; all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the
rank's maps, the owner of every node and the per-node getter values of the nodes it owns (tests/test_gpu_output_maps.py merges them).
usage: python scripts/multirank_maps_worker.py <rank> <world> <port> <steps> <outfile>    (SF3D_TEST_SPARSE_BUILD=1: strip-local build)"""
import os
import multirank_common as mc
import numpy as np
from criteria3d_amd import catchment as cm, maps
from tests.scenarios import ravone_project_model

rank, world, steps, outfile = mc.start()
m = ravone_project_model((980, 1060, 330, 420))
sf = mc.build(m, columns=False, sparse=os.environ.get("SF3D_TEST_SPARSE_BUILD") == "1")
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
mc.finish(sf, outfile, res)
