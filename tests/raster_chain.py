"""What tests/test_gpu_raster_chain.py and scripts/multirank_chain_worker.py share (no tests here): the snow, crop and root blocks driven one
after the other in one process, on the 24 x 32 raster of the root pin and then the snow block alone on a 3 x 11 raster."""
import numpy as np

from criteria3d_amd import crop, root, snow
from tests import crop_cases as cc
from tests import root_cases as rc
from tests.snow_cases import melt_forcing

SNOW_MAPS = snow.STATE + snow.OUTPUT
CROP_MAPS = crop.MAPS
ROOT_MAPS = rc.OUTPUTS + ("keys",)
SMALL_SHAPE = (3, 11)


def run(sf, pin) -> dict:
    """every map of the three blocks by name after a cold and a warm hour, the day's update and the root maps from the crop block's degree
    days; "initial_<name>": the snow and crop state before the first hour"""
    dem, flag = pin["dem"], float(pin["flag"])
    units = cc.load_pin()["unit_list"]
    unit_index = (np.arange(dem.size).reshape(dem.shape) % len(units)).astype(np.int32)
    snow.initialize(sf, dem, flag)
    crop.initialize(sf, dem, unit_index, units, 44.5, flag)
    rc.initialize(sf, pin)
    res = {"initial_" + n: snow.get_state(sf, n) for n in snow.STATE}
    res.update({"initial_" + n: crop.get_state(sf, n) for n in crop.STATE})
    for met in melt_forcing(dem.shape, dem, flag)[11:13]:             # the last cold hour and the first warm one
        snow.compute_hour(sf, met)
        crop.compute_hour(sf, None)                                   # the inputs the snow block holds
    crop.daily_update(sf, 150)
    root.compute(sf, None)                                            # the degree days the crop block holds
    res.update(snow.all_maps(sf))
    res.update(crop.all_maps(sf))
    res.update(root.all_maps(sf))
    res["keys"] = root.get_keys(sf)
    return res


def run_small(sf) -> dict:
    """the snow maps after one warm hour on a raster that is not the column table's: no rank leaves a cell out"""
    flag = -9999.0
    dem = (100.0 + 7.0 * np.arange(SMALL_SHAPE[0] * SMALL_SHAPE[1], dtype=np.float32)).reshape(SMALL_SHAPE)
    dem[1, 4] = flag
    snow.initialize(sf, dem, flag)
    snow.compute_hour(sf, melt_forcing(dem.shape, dem, flag)[12])
    return {"small_" + n: v for n, v in snow.all_maps(sf).items()}
