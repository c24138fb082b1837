"""The trigonometry of the radiation block (criteria3d_amd/csrc/sf3d_trig.inc), host build of the same source text, against the C library.

sin / cos / tan / acos (double) are faithful routines of their own, not the library's: both sides err by less than one ulp, so they are
never more than one ulp apart - the bar here, on more than 10^7 seeded arguments per function: |x| <= 200 for sin / cos / tan and
[-1, 1] for acos, with the neighbourhoods of the multiples of pi/2 and of +-1.  The share of arguments on which the two differ at all is
measured and written to the test's output (DESIGN 19 quotes it).

acosf and powf ARE the library's (the compiled reference calls them: solPos.cpp:603, 637, 752, 825): the same bits on 10^7 arguments.
tests/test_gpu_rad.py then holds the device build against this host build."""
import ctypes
import json
import platform
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
N = 2_600_000          # per range; every function sees four ranges
NAMES = ("sin", "cos", "tan", "acos")

pytestmark = pytest.mark.skipif(platform.machine() != "x86_64" or platform.libc_ver()[0] != "glibc",
                                reason="compares with glibc's x86-64 routines")


def build_trig_host(directory):
    """the host build of sf3d_trig.inc as a shared library (also used by tests/test_gpu_rad.py)"""
    out = Path(directory) / "libtrig.so"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-Wall", "-Werror",
                    f"-I{ROOT / 'criteria3d_amd' / 'csrc'}", str(ROOT / "tests" / "trig_host.c"), "-o", str(out), "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.tr_count_diff_acosf.restype = ctypes.c_size_t
    lib.tr_count_diff_powf.restype = ctypes.c_size_t
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_trig_host(tmp_path_factory.mktemp("trig"))


def near(rng, centres, n, widths=(1e-3, 1e-7, 1e-11, 1e-15)):
    """n arguments in relative and absolute neighbourhoods of `centres`, the centres and their floating-point neighbours included"""
    c = rng.choice(centres, n)
    w = rng.choice(widths, n)
    x = c + rng.uniform(-1, 1, n) * w * np.maximum(np.abs(c), 1.0)
    k = min(n, 3 * len(centres))
    edge = np.concatenate([centres, np.nextafter(centres, np.inf), np.nextafter(centres, -np.inf)])
    x[:k] = edge[:k]
    return x


def trig_ranges(seed):
    rng = np.random.default_rng(seed)
    multiples = np.arange(-127, 128) * (np.pi / 2)
    return {
        "|x| <= 200": rng.uniform(-200, 200, N),
        "the radiation block's angles (degrees x pi / 180, |x| <= 2 pi)": rng.uniform(-360, 360, N) * 0.0174532925,
        "around the multiples of pi/2": np.clip(near(rng, multiples, N), -200, 200),
        "small and tiny": rng.choice([-1, 1], N) * np.exp(rng.uniform(-700, 0, N)),
    }


def acos_ranges(seed):
    rng = np.random.default_rng(seed)
    return {
        "[-1, 1]": rng.uniform(-1, 1, N),
        "around +-1": np.clip(near(rng, np.array([-1.0, 1.0]), N), -1, 1),
        "around +-0.5 and 0": near(rng, np.array([-0.5, 0.0, 0.5]), N),
        "small and tiny": rng.choice([-1, 1], N) * np.exp(rng.uniform(-700, 0, N)),
    }


@pytest.mark.parametrize("which", range(4), ids=NAMES)
def test_faithful_routine_is_never_more_than_one_ulp_from_libm(lib, which, tmp_path):
    ranges = acos_ranges(40 + which) if which == 3 else trig_ranges(40 + which)
    total, differ, report = 0, 0, {}
    for name, x in ranges.items():
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(3)
        lib.tr_compare(which, ptr(x), ctypes.c_size_t(x.size), ptr(out))
        report[name] = {"arguments": int(x.size), "max_ulp": out[0], "differ": int(out[1]), "share": out[1] / x.size}
        print(f"{NAMES[which]:>4} {name}: max {out[0]:.0f} ulp at {float(out[2]).hex()}, {int(out[1])} of {x.size} differ ({out[1] / x.size:.3%})")
        total += x.size
        differ += int(out[1])
    print(json.dumps({"function": NAMES[which], "arguments": total, "differ": differ, "share": differ / total}))
    assert total > 10_000_000
    for name, r in report.items():
        assert r["max_ulp"] <= 1, (NAMES[which], name, r)


def test_special_values(lib):
    for which in range(4):
        x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1.5, -1.5, 5e-324, 2.0 ** -27, np.pi / 4, -np.pi / 4], np.float64)
        out = np.zeros(3)
        lib.tr_compare(which, ptr(x), ctypes.c_size_t(x.size), ptr(out))
        assert out[0] <= 1, (NAMES[which], out)
    y = np.zeros(2)
    x = np.array([0.0, -0.0])
    lib.tr_eval(0, ptr(x), ptr(y), ctypes.c_size_t(2))
    assert np.array_equal(np.signbit(y), [False, True])           # sin keeps the sign of zero
    lib.tr_eval(1, ptr(x), ptr(y), ctypes.c_size_t(2))
    assert np.array_equal(y, [1.0, 1.0])


def test_acosf_is_the_librarys_acosf_bit_for_bit(lib):
    rng = np.random.default_rng(50)
    total = 0
    for name, x in {
        "[-1, 1]": rng.uniform(-1, 1, 4 * N),
        "around +-1, +-0.5 and 0": np.clip(near(rng, np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), N, widths=(1e-2, 1e-4, 1e-6, 1e-7)), -1, 1),
        "small and tiny": rng.choice([-1, 1], N) * np.exp(rng.uniform(-100, 0, N)),
        "edges": np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.0000001, -1.0000001, 2.0, np.inf, np.nan, 2.0 ** -26, 2.0 ** -27, 1e-45]),
    }.items():
        x = np.ascontiguousarray(x, dtype=np.float32)
        first = np.zeros(2, np.float32)
        bad = lib.tr_count_diff_acosf(ptr(x), ctypes.c_size_t(x.size), ptr(first))
        assert bad == 0, (name, bad, float(first[0]).hex())
        total += x.size
    assert total > 10_000_000


def test_powf_is_the_librarys_powf_bit_for_bit(lib):
    rng = np.random.default_rng(51)
    total = 0
    for name, (x, e) in {
        "Kasten's air mass: (96.07995 - zenith)^-1.6364 (solPos.cpp:825)": (rng.uniform(3.0, 97.0, 4 * N), np.full(4 * N, -1.6364)),
        "bases around one": (1 + rng.uniform(-0.3, 0.4, N), rng.uniform(-60, 60, N)),
        "wide": (np.exp(rng.uniform(-20, 20, N)), rng.uniform(-4, 4, N)),
    }.items():
        x = np.ascontiguousarray(x, dtype=np.float32)
        e = np.ascontiguousarray(e, dtype=np.float32)
        first = np.zeros(2, np.float32)
        bad = lib.tr_count_diff_powf(ptr(x), ptr(e), ctypes.c_size_t(x.size), ptr(first))
        assert bad == 0, (name, bad, [float(v).hex() for v in first])
        total += x.size
    assert total > 10_000_000
