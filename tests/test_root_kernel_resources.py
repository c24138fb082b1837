"""Registers, scratch and LDS of k_root_cell, k_root_table and k_root_gather, read from the code object inside the built product library
(no GPU needed): one thread per cell / per table row with the inlined exp of the C library's algorithm - they must not spill, the thin
layers are recomputed and not kept in per-thread arrays (no scratch), and the only LDS beyond the math tables is the unit table of
k_root_cell."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from criteria3d_amd import build, root

LLVM = Path("/opt/rocm/lib/llvm/bin")
MATH_TABLES = 7 * 128 * 8                       # the pow / exp / log tables of fm_init


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    tmp = tmp_path_factory.mktemp("root_co")
    lib = build.build_product()
    so = tmp / "libsf3d_hip.so"
    shutil.copy(lib, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=tmp)
    co = [p for p in tmp.iterdir() if "gfx950" in p.name]
    assert len(co) == 1, [p.name for p in tmp.iterdir()]
    return subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co[0])], check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("kernel,lds", [("_Z11k_root_cell8RootView", MATH_TABLES + root.MAX_UNITS * ctypes.sizeof(root.Unit)),
                                        ("_Z12k_root_table13RootTableView", MATH_TABLES),
                                        ("_Z13k_root_gather8RootView", 0)])
def test_root_kernels_have_no_scratch_and_no_spills(notes, kernel, lds):
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", notes)[1:] if re.search(r"\.name:\s+" + kernel + r"\b", b)]
    assert len(blocks) == 1
    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    r = dict(scratch=g("private_segment_fixed_size"), vgpr=g("vgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
             lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    print(kernel, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == lds, r                                   # the math tables (+ 64 units x 48 B in k_root_cell), nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
