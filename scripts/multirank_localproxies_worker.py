"""One rank of a multi-rank run of the HIP product that interpolates one case of the pin of local detrending with every proxy on its
7 x 37 raster (include/sf3d_localproxies.h), over a catchment model of the same raster; all ranks may share one GPU.  Saves the rank's
map, directly returned and through the meteo block's getter, the interpolated count and the proxies' slopes per cell, and the owner of
every node (tests/test_gpu_localproxies.py merges them).
usage: python scripts/multirank_localproxies_worker.py <rank> <world> <port> <case> <outfile>"""
import multirank_common as mc
from criteria3d_amd import catchment as cm, localproxies as lp, meteo
from tests import localproxies_cases as cases

rank, world, which, outfile = mc.start()
r = cases.load_pin()["relief"]
rows, cols = r["dem"].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
cases.initialize(sf, r)
c = r["cases"][which]
res = dict(map=cases.interpolate(sf, c), got=meteo.get_map(sf, c["var"]), interpolated=lp.get_interpolated(sf), slope=lp.get_proxy_fit(sf)["slope"],
           owner=sf.owner_map(world, m.n))
mc.finish(sf, outfile, res)
