"""One rank of a multi-rank run of the HIP product that computes the topographic distance maps of the pin's 7 x 37 raster
(include/sf3d_topodist.h) and interpolates one case of the pin with them, over a catchment model of the same raster; all ranks may share
one GPU.  Saves the rank's maps, its interpolated map, directly returned and through the meteo block's getter, and the owner of every
node (tests/test_gpu_topodist.py merges them).
usage: python scripts/multirank_topodist_worker.py <rank> <world> <port> <case> <outfile>"""
import numpy as np

import multirank_common as mc
from criteria3d_amd import catchment as cm, meteo, topodist
from tests import topodist_cases as cases

rank, world, which, outfile = mc.start()
r = cases.load_pin()["relief"]
rows, cols = r["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
cases.initialize(sf, r)
c = r["cases"][which]
index = cases.hold(sf, r, c["mode"])
res = dict(maps=np.stack([topodist.get_map(sf, i) for i in range(len(r["x"]))]), map=cases.interpolate(sf, r, c, index), got=meteo.get_map(sf, c["var"]),
           owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
