"""Registers, scratch and LDS of k_et0_hour and k_crop_day, read from the code object inside the built product library (no GPU needed):
one thread per cell with inlined pow / exp / log of the C library's algorithms - they must not spill, and the only LDS beyond the math
tables is the crop table of k_crop_day."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from criteria3d_amd import build, crop

LLVM = Path("/opt/rocm/lib/llvm/bin")
MATH_TABLES = 7 * 128 * 8                       # the pow / exp / log tables of fm_init


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    tmp = tmp_path_factory.mktemp("crop_co")
    lib = build.build_product()
    so = tmp / "libsf3d_hip.so"
    shutil.copy(lib, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], check=True, capture_output=True, cwd=tmp)
    co = [p for p in tmp.iterdir() if "gfx950" in p.name]
    assert len(co) == 1, [p.name for p in tmp.iterdir()]
    return subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co[0])], check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("kernel,lds", [("_Z10k_et0_hour8CropView", MATH_TABLES),
                                        ("_Z10k_crop_day8CropView", MATH_TABLES + crop.MAX_UNITS * ctypes.sizeof(crop.Unit))])
def test_crop_kernels_have_no_scratch_and_no_spills(notes, kernel, lds):
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", notes)[1:] if re.search(r"\.name:\s+" + kernel + r"\b", b)]
    assert len(blocks) == 1
    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    r = dict(scratch=g("private_segment_fixed_size"), vgpr=g("vgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
             lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    print(kernel, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == lds, r                                   # the math tables (+ 64 units x 96 B in k_crop_day), nothing else
    assert r["threads"] == 256 and r["vgpr"] <= 128, r          # at least 4 waves per SIMD
