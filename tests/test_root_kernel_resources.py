"""Registers, scratch and LDS of k_root_cell, k_root_table and k_root_gather, read from the code object inside the built product library
(no GPU needed): one thread per cell / per table row with the inlined exp of the C library's algorithm - they must not spill, the thin
layers are recomputed and not kept in per-thread arrays (no scratch), and the only LDS beyond the math tables is the unit table of
k_root_cell."""
import ctypes

import pytest

from criteria3d_amd import root
from tests.kernel_notes import MATH_TABLES, kernel_resources


@pytest.mark.parametrize("kernel,lds", [("_Z11k_root_cell8RootView", MATH_TABLES + root.MAX_UNITS * ctypes.sizeof(root.Unit)),
                                        ("_Z12k_root_table13RootTableView", MATH_TABLES),
                                        ("_Z13k_root_gather8RootView", 0)])
def test_root_kernels_have_no_scratch_and_no_spills(kernel, lds):
    r = kernel_resources(kernel)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == lds, r                                   # the math tables (+ 64 units x 48 B in k_root_cell), nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
