"""Registers, scratch and LDS of k_meteo_idw, read from the code object inside the built product library (no GPU needed): the ten-slot
neighbour list, the direction terms and the weights live in registers (constant indices after full unrolling: no scratch, no spills), and
the only LDS is the station table of the 1 024-station cap - x and y as doubles, the value as float."""
from criteria3d_amd import meteo
from tests.kernel_notes import kernel_resources


def test_meteo_kernel_has_no_scratch_and_no_spills():
    r = kernel_resources("_Z11k_meteo_idw9MeteoView")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert 0 < r["lds"] <= meteo.MAX_STATIONS * (8 + 8 + 4), r          # no math tables: the kernel calls no exp / log / pow
    assert r["threads"] == 256, r
