"""One rank of a multi-rank run of the HIP product that computes one hour of the soil-cracking pin (include/sf3d_sink.h with
sf3d_sink_set_cracking) on its 24 x 32 raster, over the pin's node model; all ranks may share one GPU.  Saves the rank's node sinks, both
actual maps, both cracking maps and the owner of every node (tests/test_gpu_crack.py merges them).
usage: python scripts/multirank_crack_worker.py <rank> <world> <port> <hour> <outfile>"""
import multirank_common as mc
from tests import crack_cases as kc
from tests import sink_cases as sc

rank, world, which, outfile = mc.start()
pin = kc.load_pin()
m = sc.node_model(pin)
sf = mc.build(m, columns=False)
kc.set_state(sf, pin)
kc.initialize(sf, pin)
sc.hour(sf, pin, which)
res = dict(kc.outputs(sf, m.n), owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
