"""Registers, scratch and LDS of k_localdetrend, read from the code object inside the built product library (no GPU needed): a wave per
cell holds the Marquardt fit of one first guess per lane - the 6 x 6 normal matrix, the gradient, the parameters and their scratch vectors
as doubles - in registers, with no scratch and no spill; the LDS is the block's station table, four selected lists, four tables of fit
records and four rows of lane maxima, as DESIGN.md 24 states it."""
from criteria3d_amd import localdetrend as ld, meteo
from tests.kernel_notes import kernel_resources

KERNEL = "_Z14k_localdetrend16LocalDetrendView"
CELLS_PER_BLOCK = 4
STATION_TABLE = meteo.MAX_STATIONS * (8 + 8 + 4 + 4)                                   # x, y: doubles; height, value: floats
SELECTED_LIST = meteo.MAX_STATIONS * (2 + 4 + 4 + 4 + 4)                               # index (16 bits), distance, value, height, weight
FIT_RECORDS = ld.MAX_FIRST_GUESS * (ld.MAX_PARAMETERS + 2) * 8                         # parameters, R2, RMSE: doubles
LANE_MAXIMA = 64 * 4
LDS = STATION_TABLE + CELLS_PER_BLOCK * (SELECTED_LIST + FIT_RECORDS + LANE_MAXIMA)     # 107 264 bytes: DESIGN.md 24
VGPR = 188


def test_localdetrend_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources(KERNEL)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["threads"] == 256, r


def test_lds_is_what_the_design_states_and_fits_a_compute_unit():
    r = kernel_resources(KERNEL)
    assert LDS == 107264 and 0 < r["lds"] <= LDS < 160 * 1024, r


def test_vgprs_are_what_the_design_states():
    r = kernel_resources(KERNEL)
    assert r["vgpr"] == VGPR, r                    # one block of four waves a compute unit (the LDS decides that): up to 512 would do
