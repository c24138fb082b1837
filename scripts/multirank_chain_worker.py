"""One rank of a multi-rank run of the HIP product that drives the snow, crop and root blocks one after the other in one process
(tests/raster_chain.py) over a catchment model of the root pin's 24 x 32 raster, then the snow block on a raster of another size; all
ranks may share one GPU.  Saves the rank's maps and the owner of every node (tests/test_gpu_raster_chain.py merges them).
usage: python scripts/multirank_chain_worker.py <rank> <world> <port> 0 <outfile>"""
import multirank_common as mc
from criteria3d_amd import catchment as cm
from tests import raster_chain, root_cases as rc

rank, world, _, outfile = mc.start()
pin = rc.load_pin()
rows, cols = pin["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
res = raster_chain.run(sf, pin)
res.update(raster_chain.run_small(sf))
res["owner"] = sf.owner_map(world, m.n)
mc.finish(sf, outfile, res)
