"""Registers and scratch of k_snow_hour, read from the code object inside the built product library (no GPU needed): one thread per cell
with three inlined pow, three exp and three log of the C library's algorithms - it must not spill."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from criteria3d_amd import build

LLVM = Path("/opt/rocm/lib/llvm/bin")


def test_snow_kernel_has_no_scratch_and_no_spills(tmp_path):
    if not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    lib = build.build_product()
    so = tmp_path / "libsf3d_hip.so"
    shutil.copy(lib, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    co = [p for p in tmp_path.iterdir() if "gfx950" in p.name]
    assert len(co) == 1, [p.name for p in tmp_path.iterdir()]
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co[0])], check=True, capture_output=True, text=True).stdout
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", notes)[1:] if re.search(r"\.name:\s+_Z11k_snow_hour8SnowView\b", b)]
    assert len(blocks) == 1
    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    r = dict(scratch=g("private_segment_fixed_size"), vgpr=g("vgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
             lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == 7 * 128 * 8, r              # the pow / exp / log tables, nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
