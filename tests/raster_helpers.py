"""What the tests of the raster blocks, the output maps and the host programs share (a plain module, no fixtures)."""
import re
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


# ---- the host programs (tests/<block>_host.cpp; those with an input file over tests/host_io.h): the text the device compiles, on a CPU

# the product's host side (no FMA contraction: only the explicit fma calls of the radiation text become instructions with -mfma), every
# warning an error; -pthread for the plan program's stage threads
HOST_FLAGS = ("-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread")


def build_host_program(block: str, directory, sanitize: bool = False) -> Path:
    """tests/<block>_host.cpp with HOST_FLAGS; sanitize: address and undefined behaviour.  The program is run on its own, never loaded into
    another process."""
    exe = Path(directory) / (f"{block}_host_san" if sanitize else f"{block}_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", *HOST_FLAGS, *extra, f"-I{ROOT / 'include'}", f"-I{ROOT / 'criteria3d_amd' / 'csrc'}", str(ROOT / "tests" / f"{block}_host.cpp"),
                    "-o", str(exe), "-lm"], check=True)
    return exe


def write_parts(path, parts) -> None:
    """`parts` (arrays and bytes, in order) as a program's input file"""
    with open(path, "wb") as f:
        for p in parts:
            f.write(p if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p).tobytes())


def run_host_program(exe, directory, name: str, parts) -> bytes:
    """writes `parts` as the program's input, runs it and returns its output; the program must exit 0 and write nothing to stderr (a
    sanitized build reports there)"""
    src, dst = Path(directory) / f"{name}.in", Path(directory) / f"{name}.out"
    write_parts(src, parts)
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
    """where two arrays differ in their bits; a NaN equals any NaN (the payload of an invalid operation is the hardware's, its sign and
    payload are not promised by sf3d_glibcmath.inc)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    bad = bits(a) != bits(b)
    if a.dtype.kind == "f":
        bad &= ~(np.isnan(a) & np.isnan(b))
    return bad


def same(got: dict, want: dict, what: str, quantities: dict) -> None:
    """every quantity of a local-detrending table {name: rule}, cell by cell.  "bits": the raw patterns, no NaN allowed to stand for
    another; "nan": the bits, a NaN equals any NaN (the bits of a NaN are the compiler's choice); "value": counts and booleans, by =="""
    for q, rule in quantities.items():
        a, b = np.asarray(got[q]), np.asarray(want[q])
        assert a.shape == b.shape, (what, q, a.shape, b.shape)
        if rule == "value":
            bad = a != b
        else:
            assert a.dtype == b.dtype, (what, q, a.dtype, b.dtype)
            bad = differing(a, b) if rule == "nan" else bits(a) != bits(b)
        assert not bad.any(), (what, q, int(bad.sum()), np.argwhere(bad)[:4].tolist(), a[bad][:4], b[bad][:4])


# ---- a library's exports and a header's declarations

def exported_names(lib, kinds: str = "") -> set:
    """the names a shared library defines and exports; kinds: only those whose nm type letter is among these ("T": code)"""
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip() and (not kinds or line.split()[-2] in kinds)}


def header_text(header: str) -> str:
    """include/<header> without its comments"""
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)


def declared_entry_points(header: str, prefix: str) -> list:
    """the functions include/<header> declares under a prefix, sorted"""
    return sorted(set(re.findall(rf"\b({prefix}[a-z0-9_]+)\s*\(", header_text(header))))
