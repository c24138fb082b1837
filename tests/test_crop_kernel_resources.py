"""Registers, scratch and LDS of k_et0_hour and k_crop_day, read from the code object inside the built product library (no GPU needed):
one thread per cell with inlined pow / exp / log of the C library's algorithms - they must not spill, and the only LDS beyond the math
tables is the crop table of k_crop_day."""
import ctypes

import pytest

from criteria3d_amd import crop
from tests.kernel_notes import MATH_TABLES, kernel_resources


@pytest.mark.parametrize("kernel,lds", [("_Z10k_et0_hour8CropView", MATH_TABLES),
                                        ("_Z10k_crop_day8CropView", MATH_TABLES + crop.MAX_UNITS * ctypes.sizeof(crop.Unit))])
def test_crop_kernels_have_no_scratch_and_no_spills(kernel, lds):
    r = kernel_resources(kernel)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == lds, r                                   # the math tables (+ 64 units x 96 B in k_crop_day), nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
