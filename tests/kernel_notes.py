"""Helper of the kernel-resource tests (no tests here): what the gfx950 code object inside the built product library records about a
kernel.  Only the notes of the code object are read."""
import functools
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

from criteria3d_amd import build

LLVM = Path("/opt/rocm/lib/llvm/bin")
MATH_TABLES = 7 * 128 * 8                       # the pow / exp / log tables of fm_init


@functools.lru_cache(maxsize=None)
def _notes() -> str:
    if not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-readelf").exists():
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    with tempfile.TemporaryDirectory(prefix="sf3d_co") as tmp:
        tmp = Path(tmp)
        shutil.copy(build.build_product(), tmp / "libsf3d_hip.so")
        subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", "libsf3d_hip.so"], check=True, capture_output=True, cwd=tmp)
        co = [p for p in tmp.iterdir() if "gfx950" in p.name]
        assert len(co) == 1, [p.name for p in tmp.iterdir()]
        return subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co[0])], check=True, capture_output=True, text=True).stdout


def kernel_resources(mangled: str) -> dict:
    """scratch, vgpr, vgpr_spill, sgpr_spill, lds (bytes) and threads (largest workgroup) of the kernel with this mangled name"""
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", _notes())[1:] if re.search(r"\.name:\s+" + re.escape(mangled) + r"\b", b)]
    assert len(blocks) == 1, (mangled, len(blocks))
    g = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    r = dict(scratch=g("private_segment_fixed_size"), vgpr=g("vgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
             lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    print(mangled, r)
    return r
