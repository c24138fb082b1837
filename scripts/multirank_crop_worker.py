"""One rank of a multi-rank run of the HIP product that runs the hourly ET0 / daily crop maps (include/sf3d_crop.h) on a window of the
Ravone project; all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the rank's maps after
the hours and after the day, the state before the first hour and the owner of every node (tests/test_gpu_crop.py merges them).
usage: python scripts/multirank_crop_worker.py <rank> <world> <port> <hours> <outfile>"""
import multirank_common as mc
import numpy as np
from criteria3d_amd import crop
from tests.scenarios import ravone_project_model
from tests import crop_cases as cc

rank, world, hours, outfile = mc.start()
m = ravone_project_model((980, 1060, 330, 420))
sf = mc.build(m)
flag = -9999.0
idx, dem = mc.surface_dem(m, flag)
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
mc.finish(sf, outfile, res)
