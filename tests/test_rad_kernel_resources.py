"""Registers, scratch and LDS of k_rad_hour, read from the code object inside the built product library (no GPU needed): the sun position,
the shadow march and the radiation arms live in registers - no scratch, no spills - and the only LDS is the exp / pow tables of fm_init
(refraction and the Rayleigh thickness call pow, the beam and Reindl's correction exp); powf's two small tables stay in global memory."""
from tests.kernel_notes import MATH_TABLES, kernel_resources


def test_rad_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z10k_rad_hour7RadView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == MATH_TABLES, r
    assert r["vgpr"] <= 128, r                     # the figure DESIGN 19 quotes; two waves per SIMD at 256 threads a block hold up to 128
    assert r["threads"] == 256, r


def test_trig_hook_has_no_scratch():
    r = kernel_resources("_Z10k_rad_trigiPKdS0_Pdj")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
