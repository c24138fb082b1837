"""Registers, scratch and LDS of k_localdetrend_proxies, read from the code object inside the built product library (no GPU needed): the
conditions of DESIGN.md 25.  The parameter vectors and the normal matrix of the proxies' fit live in LDS, so seven other proxies need no
scratch; the LDS is k_localdetrend's (tests/test_localdetrend_kernel_resources.py, which guards that kernel unchanged) and, on top of it,
a row of station values per other proxy shared by the block, and per cell the membership bytes and the fit's nine parameter vectors; the
normal matrix takes the room of the elevation fit's records."""
from criteria3d_amd import localproxies as lp, meteo
from tests.kernel_notes import kernel_resources
from tests.test_localdetrend_kernel_resources import CELLS_PER_BLOCK, FIT_RECORDS, LDS as LDS_HEIGHT_ALONE

KERNEL = "_Z22k_localdetrend_proxies16LocalProxiesView"
PARAMETERS = 2 * lp.MAX_OTHERS                                                          # slope and intercept per proxy
PROXY_ROWS = lp.MAX_OTHERS * meteo.MAX_STATIONS * 4                                     # floats, shared by the block's four cells
MEMBERSHIP = meteo.MAX_STATIONS                                                         # a byte per list entry: the fit bit, the interpolated bit
VECTORS = 9 * PARAMETERS * 8                                                            # p, p + d, (p + d) - d, delta, min, max, lambda, change, new
LDS = LDS_HEIGHT_ALONE + PROXY_ROWS + CELLS_PER_BLOCK * (MEMBERSHIP + VECTORS)           # 144 064 bytes: DESIGN.md 25


def test_proxies_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources(KERNEL)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["threads"] == 256, r


def test_lds_equals_the_formula_and_fits_a_compute_unit():
    r = kernel_resources(KERNEL)
    assert LDS == 144064 and r["lds"] == LDS < 160 * 1024, r
    assert (PARAMETERS * PARAMETERS + PARAMETERS) * 8 <= FIT_RECORDS                      # the normal matrix and the gradient in the fit records' room


def test_vgprs_leave_room_for_four_waves():
    r = kernel_resources(KERNEL)
    assert r["vgpr"] <= 256, r                     # one block of four waves a compute unit (the LDS decides that), a wave a SIMD
