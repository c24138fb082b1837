"""The hourly meteo maps from station data on the device (include/sf3d_meteo.h, k_meteo_idw) against the compiled-reference pin
tests/golden/meteo_idw.npz: every cell of every case and method bit for bit; the getter against the map returned directly; a second
variable leaves the first one's map alone; a meteo call between the snow hour and the crop hour that reads its maps changes neither
(the shared mask buffer and stream); two ranks sharing the GPU merge to the single-rank map; 257 x 3 cells with 1 024 stations against
the restatement, every method (the LDS staging loop and the tail block at the cap); 3 x 11 and 1 x 300 cells with 300 stations against the
restatement, every method (less than a wave, a partial second block, a staging pass that ends inside the block)."""
import numpy as np
import pytest

from criteria3d_amd import capi, crop, meteo, snow
from tests import ranks as mr
from tests import crop_cases as cc
from tests import meteo_cases as mc
from tests.raster_helpers import bits
from tests.snow_cases import melt_forcing

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pin():
    return mc.load_pin()


def _same(got, want, what):
    bad = bits(got) != bits(want)
    if bad.any():
        print(f"{what}: {int(bad.sum())} values differ")
    assert np.array_equal(bits(got), bits(want)), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def test_every_cell_of_every_case_equals_the_pin(product, pin):
    mc.initialize(product, pin)
    flag = float(pin["flag"])
    for v in meteo.VARIABLES:
        assert np.all(meteo.get_map(product, v) == flag)                 # before the first call: the flag
    for k, c in enumerate(pin["cases"]):
        _same(mc.interpolate(product, c), c["want"], f"case {k} {mc.case_name(c)}")
    meteo.clean(product)


def test_getter_and_a_second_variable(product, pin):
    mc.initialize(product, pin)
    a, b = pin["cases"][15], next(c for c in pin["cases"] if c["var"] == meteo.AIR_REL_HUMIDITY and len(c["x"]) == 40)
    direct = mc.interpolate(product, a)
    _same(meteo.get_map(product, a["var"]), direct, "getter")
    assert mc.interpolate(product, b, download=False) is None            # stays on the device
    _same(meteo.get_map(product, b["var"]), b["want"], "second variable through the getter")
    _same(meteo.get_map(product, a["var"]), direct, "first variable after the second call")
    hour = meteo.interpolate_hour(product, {meteo.VARIABLES[c["var"]]: (c["x"], c["y"], c["value"], c["area"], c["settings"])
                                            for c in pin["cases"] if c["set"] == 5 and c["method"] == meteo.SHEPARD and c["var"] in (1, 2, 3, 4)
                                            or c is pin["cases"][16]}, "shepard")
    assert list(hour) == ["airT", "prec", "relHum", "windInt", "globalRad"]
    _same(hour["airT"], pin["cases"][16]["want"], "interpolate_hour airT")
    meteo.clean(product)
    assert product.lib.sf3d_meteo_get_map(0, direct.size, direct.ctypes.data_as(meteo.pf32)) != 0      # after clean: not initialised


def test_a_meteo_call_between_the_snow_and_the_crop_hour_changes_neither(product, pin):
    dem, flag = pin["dem"], float(pin["flag"])
    units = cc.load_pin()["unit_list"]
    unit_index = (np.arange(dem.size).reshape(dem.shape) % len(units)).astype(np.int32)

    def chain(with_meteo):
        snow.initialize(product, dem, flag)
        crop.initialize(product, dem, unit_index, units, 44.5, flag)
        if with_meteo:
            mc.initialize(product, pin)
        for met in melt_forcing(dem.shape, dem, flag)[11:13]:
            snow.compute_hour(product, met)
            if with_meteo:
                _same(mc.interpolate(product, pin["cases"][17]), pin["cases"][17]["want"], "meteo inside the chain")
            crop.compute_hour(product, None)                              # reads what the snow hour left on the device
        res = dict(snow.all_maps(product))
        res.update(crop.all_maps(product))
        snow.clean(product); crop.clean(product); meteo.clean(product)
        return res
    without, with_ = chain(False), chain(True)
    assert set(without) == set(with_) and len(without) > 10
    for n in without:
        a, b = np.ascontiguousarray(without[n]), np.ascontiguousarray(with_[n])
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), n          # the bytes
    assert np.count_nonzero(without["et0"] > 0) > 300


def test_two_ranks_merge_to_the_single_rank_map(product, pin, tmp_path):
    which = 16                                                            # shepard, 40 stations, air temperature with both proxies
    ranks = mr.run("scripts/multirank_meteo_worker.py", 2, mr.PORTS["meteo"], [which], tmp_path)
    rows, cols = pin["dem"].shape
    idx = np.arange(rows * cols).reshape(rows, cols)                      # the surface node of every cell of catchment_model(cols, rows, 4)
    cell_owner = mr.cell_owner(ranks, idx, rows * cols * 4)
    flag = np.float32(pin["flag"])
    for r, res in enumerate(ranks):
        _same(res["got"], res["map"], f"rank {r} getter")
    merged = mr.merge([res["map"] for res in ranks], cell_owner, flag, others=flag, what="map")      # another rank's cells: the flag
    _same(merged, pin["cases"][which]["want"], "merged ranks")            # what the single rank gives (the first test): the pin
    assert np.count_nonzero(merged != flag) > 600


@pytest.mark.parametrize("method", ["idw", "shepard", "shepard_modified"])
def test_1024_stations_on_257_x_3_cells_against_the_restatement(product, pin, method):
    r = mc.cap_raster(pin)
    assert len(r["x"]) == meteo.MAX_STATIONS and r["dem"].size % 256 == 3
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], float(r["flag"]))
    got = meteo.interpolate(product, "airT", method, r["x"], r["y"], r["value"], r["area"], r["settings"])
    want = meteo.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], "airT", method, r["x"], r["y"], r["value"], r["area"],
                                     r["settings"], float(r["flag"]))
    _same(got, want, f"1024 stations, {method}")
    assert got.flat[0] == r["flag"] and got.flat[-1] != r["flag"] and np.count_nonzero(got != r["flag"]) == r["dem"].size - 2
    with pytest.raises(capi.SF3DError):                                   # one station beyond the cap
        meteo.interpolate(product, "airT", method, np.append(r["x"], 0.0), np.append(r["y"], 0.0), np.append(r["value"], 0.0), r["area"], r["settings"])
    meteo.clean(product)


@pytest.mark.parametrize("method", meteo.METHODS)
@pytest.mark.parametrize("shape", mc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_300_stations_on_small_rasters_against_the_restatement(product, pin, shape, method):
    """33 cells: less than a wave; one row of 300: a partial second block.  300 stations: the second pass of the LDS staging loop ends at
    lane 44.  The single row holds every neighbourhood size of shepardSearchNeighbour (tests/test_meteo_host.py)."""
    r = mc.small_raster(pin, shape)
    flag = r["flag"]
    meteo.initialize(product, r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], float(flag))
    got = meteo.interpolate(product, "airT", method, r["x"], r["y"], r["value"], r["area"], r["settings"])
    want = meteo.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], r["proxy_maps"], "airT", method, r["x"], r["y"], r["value"], r["area"],
                                     r["settings"], float(flag))
    print(f"{shape} {method}: {int((bits(got) != bits(want)).sum())} values differ")
    _same(got, want, f"300 stations on {shape}, {method}")
    assert got.flat[0] == flag and got.flat[-1] != flag and np.count_nonzero(got != flag) == r["dem"].size - 2
    meteo.clean(product)
