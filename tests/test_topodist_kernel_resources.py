"""Registers, scratch and LDS of the three topographic distance kernels, read from the code object inside the built product library (no
GPU needed): the walk keeps its position and its maximum in registers; k_meteo_idw_td holds k_meteo_idw's station table in LDS and beside
it only the stations' heights (floats) and map indices; k_topodist_maps and k_topodist_matrix declare no LDS and use none."""
from criteria3d_amd import meteo
from tests.kernel_notes import kernel_resources

MAPS = "_Z15k_topodist_maps12TopoMapsView"
IDW_TD = "_Z14k_meteo_idw_td11TopoIdwView"
MATRIX = "_Z17k_topodist_matrix14TopoMatrixView"


def test_topodist_kernels_have_no_scratch_and_no_spills():
    for name in (MAPS, IDW_TD, MATRIX):
        r = kernel_resources(name)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["threads"] == 256, (name, r)


def test_lds_is_the_station_table_with_heights_and_map_indices():
    r = kernel_resources(IDW_TD)
    assert 0 < r["lds"] <= meteo.MAX_STATIONS * (8 + 8 + 4 + 4 + 4), r      # x, y: doubles; value, z: floats; mapIndex: int32; no math tables
    assert kernel_resources(MAPS)["lds"] == 0 and kernel_resources(MATRIX)["lds"] == 0
