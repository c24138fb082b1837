"""The snow, crop and root blocks share one ownership mask on the host and one mask buffer on the device: two ranks sharing the GPU drive all
three blocks in one process (scripts/multirank_chain_worker.py) and merge, bit for bit, to what the single rank gives for the same
calls; a raster that is not the column table's is computed on every cell by every rank."""
import numpy as np
import pytest

from criteria3d_amd import crop, root, snow
from tests import ranks as mr
from tests import raster_chain
from tests import root_cases as rc
from tests.raster_helpers import bits as _bits

pytestmark = pytest.mark.gpu


def test_two_ranks_chain_the_three_blocks_and_merge_to_the_single_rank_maps(product, tmp_path):
    ranks = mr.run("scripts/multirank_chain_worker.py", 2, mr.PORTS["chain"], [0], tmp_path)
    pin = rc.load_pin()
    single = raster_chain.run(product, pin)
    single.update(raster_chain.run_small(product))
    snow.clean(product); crop.clean(product); root.clean(product)
    rows, cols = pin["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)                # both ranks own cells
    flag = float(pin["flag"])
    # what another rank's cells hold: the flag in the snow outputs, ET0 and the root maps (-1 in the keys), the state as it was elsewhere
    for r, res in enumerate(ranks):
        mine = cell_owner == r
        for n in snow.OUTPUT + ("et0", "length", "depth"):
            assert np.all(res[n][~mine] == flag), (n, r)
        assert np.all(res["density"][:, ~mine] == flag) and np.all(res["keys"][~mine] == -1), r
        assert np.all(res["first"][~mine] == int(flag)) and np.all(res["last"][~mine] == int(flag)), r
        for n in snow.STATE + crop.STATE:
            assert np.array_equal(_bits(res[n][~mine]), _bits(res["initial_" + n][~mine])), (n, r)          # untouched
    # merged by cell owner: the single rank's maps, bit for bit
    for n in raster_chain.SNOW_MAPS + raster_chain.CROP_MAPS + raster_chain.ROOT_MAPS:
        merged = mr.merge([res[n] for res in ranks], cell_owner, 0)
        assert merged.shape == single[n].shape and merged.dtype == single[n].dtype, n
        bad = _bits(merged) != _bits(single[n])
        print(f"{n}: {int(bad.sum())} values differ")
        assert not bad.any(), (n, int(bad.sum()))
    # the chain computed something in every block
    assert np.count_nonzero(single["snowMelt"] > 0) > 300 and np.count_nonzero(single["liquid"] > 0) > 300
    assert np.count_nonzero(single["et0"] > 0) > 300 and np.count_nonzero(single["degreeDays"] > 0) > 100
    assert np.count_nonzero(single["length"] > 0) > 100 and np.count_nonzero(single["density"] > 0) > 100
    # the 3 x 11 raster is not the column table's: no mask, every rank computes every cell
    for n in raster_chain.SNOW_MAPS:
        for r, res in enumerate(ranks):
            assert res["small_" + n].shape == raster_chain.SMALL_SHAPE
            assert np.array_equal(_bits(res["small_" + n]), _bits(single["small_" + n])), (n, r)
    assert np.count_nonzero(single["small_liquid"] > 0) == 32
