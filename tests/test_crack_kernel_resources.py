"""Registers, scratch and LDS of k_sink_hour_crack, read from the code object inside the built product library (no GPU needed): the hour
with soil cracking keeps no per-thread array of layers either (the second loop of computeSoilCracking evaluates a layer's void volume again
instead of keeping voidVolumeList), so there is no scratch and nothing spills; the only LDS is the math tables of exp."""
from tests.kernel_notes import MATH_TABLES, kernel_resources


def test_crack_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z17k_sink_hour_crack13SinkCrackView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == MATH_TABLES, r
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
