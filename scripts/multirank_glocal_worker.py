"""One rank of a multi-rank run of the HIP product that interpolates one case of the pin of glocal detrending on its 7 x 37 raster
(include/sf3d_glocal.h), over a catchment model of the same raster; all ranks may share one GPU.  Every rank fits every macro area; the
cell loop runs over the rows the rank owns.  Saves the rank's map, directly returned and through the meteo block's getter, the areas'
kept counts and the owner of every node (tests/test_gpu_glocal.py merges them).
usage: python scripts/multirank_glocal_worker.py <rank> <world> <port> <case> <outfile>"""
import multirank_common as mc
from criteria3d_amd import catchment as cm, glocal as gl, meteo
from tests import glocal_cases as cases

rank, world, which, outfile = mc.start()
r = cases.load_pin()["relief"]
rows, cols = r["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
cases.initialize(sf, r)
c = r["cases"][which]
res = dict(map=cases.interpolate(sf, c), got=meteo.get_map(sf, c["var"]), kept=gl.get_area_fit(sf)["kept"], owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
