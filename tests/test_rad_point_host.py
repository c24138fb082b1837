"""The point function of the radiation kernel (criteria3d_amd/csrc/sf3d_rad.inc with sf3d_trig.inc and sf3d_rad_setup.inc), compiled for the
host as tests/rad_host.cpp, over every case of the compiled-reference pins (tests/golden/rad_rsun.npz and rad_rsun_places.npz): the same
text the device compiles equals the reference in every cell, map and case - zero exclusions - before any GPU runs it.  The double sin / cos / tan of
sf3d_trig.inc are not the C library's (tests/test_trig_host.py: within one ulp, a few per cent of the arguments differ), so this
equality is expected, not guaranteed by construction: a failure here that traces to a last-place trig difference is a finding about
the routine's rounding."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import rad_cases

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "golden"))


@pytest.fixture(scope="module")
def rad_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rad_host") / "rad_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-Werror", "-Wno-unused-function",
                    f"-I{ROOT / 'criteria3d_amd' / 'csrc'}", str(ROOT / "tests" / "rad_host.cpp"), "-o", str(exe), "-lm"], check=True)
    return exe


def _every_cell(rad_host, tmp_path, pin):
    """rad_host over every raster of a pin, each with its own geo -> the number of cases checked"""
    import make_rad_rsun as gen
    checked = 0
    for raster in range(len(pin["dem"])):
        cases = [c for c in pin["cases"] if c["raster"] == raster]
        case_list = [(c["name"], raster, c["settings"], c["when"], c["keep"], c["transmissivity"]) for c in cases]
        static = (pin["lat"][raster], pin["lon"][raster], pin["slope"][raster], pin["aspect"][raster])
        with open(tmp_path / f"in{raster}.bin", "wb") as f:
            gen.write_input(f, pin["dem"][raster], pin["flag"], rad_cases.pin_geo(pin, raster), case_list, list(pin["transmissivity"]), static=static)
        subprocess.run([str(rad_host), str(tmp_path / f"in{raster}.bin"), str(tmp_path / f"out{raster}.bin")], check=True)
        n = pin["dem"][raster].size
        rec = np.fromfile(tmp_path / f"out{raster}.bin", np.float32).reshape(len(cases), 1 + 5 * n)
        for k, case in enumerate(cases):
            status = int(rec[k, :1].view(np.int32)[0])
            assert status == (1 if "refuses" in case["name"] else 0), case["name"]
            got = rec[k, 1:].reshape(5, *pin["dem"][raster].shape)
            same = rad_cases.same_bits(got, rad_cases.pin_maps(pin, case))
            assert same.all(), (case["name"], int((~same).sum()), np.argwhere(~same)[:4].tolist())
            checked += 1
    return checked


def test_host_build_of_the_kernels_point_function_equals_the_pin_in_every_cell(rad_host, tmp_path):
    pin = rad_cases.load_pin()
    assert _every_cell(rad_host, tmp_path, pin) == len(pin["cases"]) >= 40


def test_host_build_of_the_kernels_point_function_equals_the_places_pin_in_every_cell(rad_host, tmp_path):
    """radsHour, radsCell and rad_point at the other places, dates and edited cells: no exclusions"""
    pin = rad_cases.load_places_pin()
    assert _every_cell(rad_host, tmp_path, pin) == len(pin["cases"]) >= 36
