"""Registers, scratch and LDS of k_hour_relhum, k_hour_totals and k_hour_pond, read from the code object inside the built product library
(no GPU needed): one thread per cell, no spills, and exactly the LDS each kernel declares - the math tables of fm_init for the inlined pow
and exp of k_hour_relhum, the reduction buffer of k_hour_totals (three totals x 256 doubles), none for k_hour_pond."""
import pytest

from tests.kernel_notes import MATH_TABLES, kernel_resources

BLOCK = 256                                     # SF3D_BLOCK
TOTALS_BUFFER = 3 * BLOCK * 8                   # __shared__ double sm[HOUR_TOTALS][SF3D_BLOCK]


@pytest.mark.parametrize("kernel,lds", [("_Z13k_hour_relhum14HourRelhumView", MATH_TABLES), ("_Z13k_hour_totals14HourTotalsView", TOTALS_BUFFER),
                                        ("_Z11k_hour_pond12HourPondView", 0)])
def test_hour_kernels_have_no_scratch_and_no_spills(kernel, lds):
    r = kernel_resources(kernel)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == lds, r
    assert r["threads"] == BLOCK and r["vgpr"] <= 128, r       # the other raster kernels' bound: at least 4 waves per SIMD
