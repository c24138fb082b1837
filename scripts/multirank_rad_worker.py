"""One rank of a multi-rank run of the HIP product that computes two hours of a radiation pin (include/sf3d_rad.h; "places": the 16 x 24
rasters of rad_rsun_places.npz, else the 24 x 32 ones of rad_rsun.npz), over a catchment model of the same raster; all ranks may share one GPU.  Each rank writes the cells it owns - its shadow rays
read the whole DEM - and leaves the others at the flag.  Saves the rank's five maps after each hour and the owner of every node
(tests/test_gpu_rad.py merges them).
usage: python scripts/multirank_rad_worker.py <rank> <world> <port> <first case> [places] <outfile>"""
import sys

import numpy as np

import multirank_common as mc
from criteria3d_amd import catchment as cm, radiation as rad
from tests import rad_cases as cases

rank, world, which, outfile = mc.start()
places = outfile == "places"
if places:
    outfile = sys.argv[6]
pin = cases.load_places_pin() if places else cases.load_pin()
first, second = pin["cases"][which], pin["cases"][which + 1]
assert second["keep"] and first["raster"] == second["raster"]
r = first["raster"]
rows, cols = pin["dem"][r].shape
m = cm.catchment_model(cols, rows, 4)
sf = mc.build(m)
geo = pin["geo"][r] if places else pin["geo"]        # (xll, yll, cell size): one per raster in the places pin
rad.initialize(sf, pin["dem"][r], geo[0], geo[1], geo[2], pin["lat"][r], pin["lon"][r], pin["slope"][r], pin["aspect"][r], settings=first["settings"],
               flag=float(pin["flag"]))
res = dict(owner=sf.owner_map(world, m.n))
for k, case in enumerate((first, second)):
    rad.compute_hour(sf, case["when"], pin["transmissivity"][case["transmissivity"]])
    res[f"hour{k}"] = np.stack([rad.get_map(sf, n) for n in rad.MAPS])
mc.finish(sf, outfile, res)
