"""Registers, scratch and LDS of k_sink_hour, read from the code object inside the built product library (no GPU needed): one thread per
cell walks its column without a per-thread array of layers (the redistribution and the final loop of assignTranspiration evaluate
layerTranspiration again instead of keeping it), so there is no scratch and nothing spills; the only LDS is the math tables of exp."""
from tests.kernel_notes import MATH_TABLES, kernel_resources


def test_sink_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z11k_sink_hour8SinkView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == MATH_TABLES, r
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
