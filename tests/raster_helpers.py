"""What the tests of the raster blocks and the output maps share (a plain module, no fixtures)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def bits(a):
    """the bit patterns of a 4- or 8-byte float array; an integer array as it is"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def need_glibc_set(product):
    if product.lib.sf3d_libm_set() != 1:
        pytest.skip("this build evaluates the 0.50-ulp routines, not the C library's bits (-DSF3D_LIBM_GLIBC=0): bit identity with the compiled reference is not its contract")


# ---- the host programs of the raster blocks (tests/<block>_host.cpp over tests/host_io.h): the per-cell text the device compiles, on a CPU

def build_host_program(block: str, directory, sanitize: bool = False) -> Path:
    """tests/<block>_host.cpp with the flags of the product's host side (no FMA contraction); sanitize: address and undefined behaviour.
    The program is run on its own, never loaded into another process."""
    exe = Path(directory) / (f"{block}_host_san" if sanitize else f"{block}_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", *extra, f"-I{ROOT / 'include'}", f"-I{ROOT / 'criteria3d_amd' / 'csrc'}",
                    str(ROOT / "tests" / f"{block}_host.cpp"), "-o", str(exe), "-lm"], check=True)
    return exe


def run_host_program(exe, directory, name: str, parts) -> bytes:
    """writes `parts` (arrays and bytes, in order) as the program's input, runs it and returns its output; the program must exit 0 and write
    nothing to stderr (a sanitized build reports there)"""
    src, dst = Path(directory) / f"{name}.in", Path(directory) / f"{name}.out"
    with open(src, "wb") as f:
        for p in parts:
            f.write(p if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p).tobytes())
    res = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, (Path(exe).name, name, res.returncode, res.stderr[-3000:])
    return dst.read_bytes()


class Reader:
    """takes arrays off a program's output in order"""
    def __init__(self, raw: bytes):
        self.raw, self.at = raw, 0

    def take(self, dtype, *shape):
        count = int(np.prod(shape)) if shape else 1
        a = np.frombuffer(self.raw, dtype, count, self.at).reshape(shape if shape else (1,)).copy()
        self.at += a.nbytes
        return a

    def done(self) -> bool:
        return self.at == len(self.raw)


def differing(a, b) -> np.ndarray:
    """where two arrays differ in their bits; a NaN equals any NaN, as in tests/test_gpu_fastmath.py same_bits (the payload of an invalid
    operation is the hardware's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    bad = bits(a) != bits(b)
    if a.dtype.kind == "f":
        bad &= ~(np.isnan(a) & np.isnan(b))
    return bad
