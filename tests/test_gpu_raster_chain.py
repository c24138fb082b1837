"""The snow, crop and root blocks share one ownership mask on the host and one mask buffer on the device: two ranks sharing the GPU drive all
three blocks in one process (scripts/multirank_chain_worker.py) and merge, bit for bit, to what the single rank gives for the same
calls; a raster that is not the column table's is computed on every cell by every rank."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from criteria3d_amd import crop, root, snow
from tests import raster_chain
from tests import root_cases as rc
from tests.raster_helpers import bits as _bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_two_ranks_chain_the_three_blocks_and_merge_to_the_single_rank_maps(product, tmp_path):
    world, port = 2, 29775
    outs = [tmp_path / f"chain_r{r}.npz" for r in range(world)]
    env = {**os.environ, "SF3D_DIST_TIMEOUT_S": os.environ.get("SF3D_DIST_TIMEOUT_S", "60")}
    procs = [subprocess.Popen([sys.executable, str(ROOT / "scripts" / "multirank_chain_worker.py"), str(r), str(world), str(port), "0", str(outs[r])],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(pr.returncode == 0 for pr in procs), "\n".join(logs)
    ranks = [np.load(o) for o in outs]
    pin = rc.load_pin()
    single = raster_chain.run(product, pin)
    single.update(raster_chain.run_small(product))
    snow.clean(product); crop.clean(product); root.clean(product)
    rows, cols = pin["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    owner = np.full(rows * cols * 4, 255, np.int64)
    for r, res in enumerate(ranks):
        owner[res["owner"] == r] = r
    cell_owner = owner[idx]
    assert set(np.unique(cell_owner)) == {0, 1}                           # both ranks own cells
    assert all(np.count_nonzero(cell_owner == r) > 0 for r in range(world))
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
        merged = np.array(single[n])
        merged[...] = 0
        for r, res in enumerate(ranks):
            merged[..., cell_owner == r] = res[n][..., cell_owner == r]
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
