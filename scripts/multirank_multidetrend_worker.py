"""One rank of a multi-rank run of the HIP product that interpolates one case of the pin of multiple detrending without areas on its
7 x 37 raster (include/sf3d_multidetrend.h), over a catchment model of the same raster; all ranks may share one GPU.  Every rank runs the
one fit; the cell loop runs over the rows the rank owns; the points are evaluated by every rank.  Saves the rank's map, directly returned
and through the meteo block's getter, the fit's kept count, the points and the owner of every node (tests/test_gpu_multidetrend.py merges
them).
usage: python scripts/multirank_multidetrend_worker.py <rank> <world> <port> <case> <outfile>"""
import multirank_common as mc
from criteria3d_amd import catchment as cm, meteo, multidetrend as md
from tests import multidetrend_cases as cases

rank, world, which, outfile = mc.start()
r = cases.load_pin()["relief"]
rows, cols = r["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
cases.initialize(sf, r)
c = r["cases"][which]
res = dict(map=cases.interpolate(sf, c), got=meteo.get_map(sf, c["var"]), kept=md.get_fit(sf)["kept"], points=cases.points(sf, c), owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
