"""One rank of a multi-rank run of the HIP product that drives one hour device to device (include/sf3d_hour.h) on a 7 x 37 raster - the
meteo maps, the humidity from the dew point, radiation, snow, ET0, roots and sinks in place, the hour's totals - and then the day's ponds,
over the node model of the raster (tests/hour_cases.py); all ranks may share one GPU.  Saves the rank's maps, totals, node ponds and the
owner of every node (tests/test_gpu_hour.py merges them).
usage: python scripts/multirank_hour_worker.py <rank> <world> <port> 0 <outfile>"""
import multirank_common as mc
from tests import hour_cases as hc
from tests import sink_cases as sc

rank, world, _, outfile = mc.start()
case = hc.world(sc.load_pin(), (7, 37))
m = sc.node_model(case)
sf = mc.build(m, columns=False)
sc.set_state(sf, case, m)
res = hc.chain(sf, case, m)
res["owner"] = sf.owner_map(world, m.n)
mc.finish(sf, outfile, res)
