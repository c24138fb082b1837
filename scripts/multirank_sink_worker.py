"""One rank of a multi-rank run of the HIP product that computes one hour of the water-sink pin (include/sf3d_sink.h) on its 24 x 32
raster, over the pin's node model; all ranks may share one GPU.  Saves the rank's node sinks, both actual maps and the owner of every
node (tests/test_gpu_sink.py merges them).
usage: python scripts/multirank_sink_worker.py <rank> <world> <port> <hour> <outfile>"""
import multirank_common as mc
from criteria3d_amd import sinks
from tests import root_cases as rc
from tests import sink_cases as sc

rank, world, which, outfile = mc.start()
pin = sc.load_pin()
m = sc.node_model(pin)
sf = mc.build(m, columns=False)
sc.set_state(sf, pin, m)
rc.initialize(sf, pin)
sc.initialize(sf, pin)
sc.hour(sf, pin, which)
evaporation, transpiration = sinks.get_actual(sf)
res = dict(sinks=sinks.get_node_sinks(sf, m.n), evaporation=evaporation, transpiration=transpiration, owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
