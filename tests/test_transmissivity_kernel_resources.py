"""Registers, scratch and LDS of k_transmissivity_points, read from the code object inside the built product library (no GPU needed): the
evaluation is rad_eval of k_rad_hour and lives in registers as it does there - no scratch, no spills, at most 128 VGPRs at 256 threads
a block - and beyond the exp / pow tables of fm_init the LDS holds only the hand-over of the evaluations to the lane that adds them up:
256 doubles, 256 floats and 256 bytes."""
from tests.kernel_notes import MATH_TABLES, kernel_resources

HAND_OVER = 256 * 8 + 256 * 4 + 256


def test_transmissivity_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z23k_transmissivity_points6TrView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == MATH_TABLES + HAND_OVER, r
    assert r["vgpr"] <= 128, r                     # two waves per SIMD at 256 threads a block hold up to 128, as k_rad_hour's bound
    assert r["threads"] == 256, r


def test_rad_kernel_keeps_its_bounds_beside_the_shared_evaluation():
    r = kernel_resources("_Z10k_rad_hour7RadView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == MATH_TABLES and r["vgpr"] <= 128, r
