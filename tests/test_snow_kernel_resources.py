"""Registers and scratch of k_snow_hour, read from the code object inside the built product library (no GPU needed): one thread per cell
with three inlined pow, three exp and three log of the C library's algorithms - it must not spill."""
from tests.kernel_notes import MATH_TABLES, kernel_resources


def test_snow_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z11k_snow_hour8SnowView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == MATH_TABLES, r              # the pow / exp / log tables, nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
