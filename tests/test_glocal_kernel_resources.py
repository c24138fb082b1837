"""Registers, scratch and LDS of k_glocal_areas and k_glocal_cells, read from the code object inside the built product library (no GPU
needed): the conditions of DESIGN.md 26.  k_glocal_areas is a wave per macro area: the area's list, the fit records of the first
guesses, the proxies' membership bytes and nine parameter vectors lie in LDS per wave - the call's point table stays in global memory,
so there is no station table and no row of proxy values in LDS, and no selection, so no lane maxima; the normal matrix takes the room of
the fit records as in k_localdetrend_proxies.  k_glocal_cells is a thread per cell with the meteo block's ten-slot neighbour list in
registers and no LDS at all."""
from criteria3d_amd import localdetrend as ld, localproxies as lp, meteo
from tests.kernel_notes import kernel_resources

AREAS = "_Z14k_glocal_areas15GlocalAreasView"
CELLS = "_Z14k_glocal_cells15GlocalCellsView"
AREAS_PER_BLOCK = 4
AREA_LIST = meteo.MAX_STATIONS * (2 + 4 + 4 + 4 + 4)                                    # point index (16 bits), place in the area's list, value, height, weight
FIT_RECORDS = ld.MAX_FIRST_GUESS * (ld.MAX_PARAMETERS + 2) * 8                          # parameters, R2, RMSE: doubles
MEMBERSHIP = meteo.MAX_STATIONS                                                         # a byte per list entry
VECTORS = 9 * 2 * lp.MAX_OTHERS * 8                                                     # p, p + d, (p + d) - d, delta, min, max, lambda, change, new
LDS = AREAS_PER_BLOCK * (AREA_LIST + FIT_RECORDS + MEMBERSHIP + VECTORS)                # 89 792 bytes: DESIGN.md 26


def test_both_kernels_have_no_scratch_and_no_spills():
    for kernel in (AREAS, CELLS):
        r = kernel_resources(kernel)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (kernel, r)
        assert r["threads"] == 256, (kernel, r)


def test_lds_equals_the_formula_and_fits_a_compute_unit():
    assert LDS == 89792 and kernel_resources(AREAS)["lds"] == LDS < 160 * 1024
    assert kernel_resources(CELLS)["lds"] == 0
    assert (2 * lp.MAX_OTHERS * 2 * lp.MAX_OTHERS + 2 * lp.MAX_OTHERS) * 8 <= FIT_RECORDS   # the normal matrix and the gradient in the fit records' room


def test_vgprs_are_what_the_design_states():
    assert kernel_resources(AREAS)["vgpr"] == 192                                       # DESIGN.md 26; the LDS allows one block a compute unit: a wave a SIMD
    assert kernel_resources(CELLS)["vgpr"] == 154
