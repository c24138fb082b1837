"""Registers, scratch and LDS of k_multidetrend_fit, k_multidetrend_cells and k_multidetrend_points, read from the code object inside
the built product library (no GPU needed): the conditions of DESIGN.md 27.  k_multidetrend_fit is ONE wave: the call's list, the fit
records of the first guesses, the proxies' membership bytes and nine parameter vectors lie in LDS - a quarter of k_glocal_areas', which
holds them for four waves; the station table stays in global memory.  The two other kernels are a thread per cell / per point with the
meteo block's ten-slot neighbour list in registers and the kept stations staged by the block, as k_meteo_idw stages the call's."""
from criteria3d_amd import localdetrend as ld, localproxies as lp, meteo
from tests.kernel_notes import kernel_resources

FIT = "_Z18k_multidetrend_fit19MultiDetrendFitView"
CELLS = "_Z20k_multidetrend_cells21MultiDetrendCellsView"
POINTS = "_Z21k_multidetrend_points22MultiDetrendPointsView"
LIST = meteo.MAX_STATIONS * (2 + 4 + 4 + 4 + 4)                                         # station index (16 bits), place, value, height, weight
FIT_RECORDS = ld.MAX_FIRST_GUESS * (ld.MAX_PARAMETERS + 2) * 8                          # parameters, R2, RMSE: doubles
MEMBERSHIP = meteo.MAX_STATIONS                                                         # a byte per list entry
VECTORS = 9 * 2 * lp.MAX_OTHERS * 8                                                     # p, p + d, (p + d) - d, delta, min, max, lambda, change, new
FIT_LDS = LIST + FIT_RECORDS + MEMBERSHIP + VECTORS                                     # 22 448 bytes: DESIGN.md 27
KEPT_LDS = meteo.MAX_STATIONS * (8 + 8 + 4)                                             # the kept stations: x, y doubles, the detrended value


def test_the_three_kernels_have_no_scratch_and_no_spills():
    for kernel, threads in ((FIT, 64), (CELLS, 256), (POINTS, 256)):
        r = kernel_resources(kernel)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (kernel, r)
        assert r["threads"] == threads, (kernel, r)


def test_lds_equals_the_formula_and_fits_a_compute_unit():
    assert FIT_LDS == 22448 and kernel_resources(FIT)["lds"] == FIT_LDS < 160 * 1024
    assert KEPT_LDS == 20480 and kernel_resources(CELLS)["lds"] == KEPT_LDS and kernel_resources(POINTS)["lds"] == KEPT_LDS
    assert kernel_resources("_Z11k_meteo_idw9MeteoView")["lds"] == KEPT_LDS              # the same table
    assert (2 * lp.MAX_OTHERS * 2 * lp.MAX_OTHERS + 2 * lp.MAX_OTHERS) * 8 <= FIT_RECORDS   # the normal matrix and the gradient in the fit records' room


def test_vgprs_are_what_the_design_states():
    assert kernel_resources(FIT)["vgpr"] == 172                                         # DESIGN.md 27, from the first build; one wave, so occupancy is no question
    assert kernel_resources(CELLS)["vgpr"] == 122
    assert kernel_resources(POINTS)["vgpr"] == 122
