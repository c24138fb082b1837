"""One rank of a multi-rank run of the HIP product that runs the hourly snow model (include/sf3d_snow.h) on a window of the Ravone project;
all ranks may share one GPU.  The control plane is torch.distributed with the gloo backend.  Saves the rank's thirteen maps, the state
before the first hour and the owner of every node (tests/test_gpu_snow.py merges them).
usage: python scripts/multirank_snow_worker.py <rank> <world> <port> <hours> <outfile>"""
import multirank_common as mc
from criteria3d_amd import snow
from tests.scenarios import ravone_project_model
from tests.snow_cases import melt_forcing

rank, world, hours, outfile = mc.start()
m = ravone_project_model((980, 1060, 330, 420))
sf = mc.build(m)
flag = -9999.0
idx, dem = mc.surface_dem(m, flag)
snow.initialize(sf, dem, flag)
res = {"owner": sf.owner_map(world, m.n)}
res.update({"initial_" + n: snow.get_state(sf, n) for n in snow.STATE})
for met in melt_forcing(dem.shape, dem, flag)[:hours]:
    snow.compute_hour(sf, met)
res.update(snow.all_maps(sf))
mc.finish(sf, outfile, res)
