"""The point function of the radiation kernel (criteria3d_amd/csrc/sf3d_rad.inc with sf3d_trig.inc and sf3d_rad_setup.inc), compiled for the
host as tests/rad_host.cpp, over every case of the compiled-reference pins (tests/golden/rad_rsun.npz and rad_rsun_places.npz): the same
text the device compiles equals the reference in every cell, map and case - zero exclusions - before any GPU runs it.  The double sin / cos / tan of
sf3d_trig.inc are not the C library's (tests/test_trig_host.py: within one ulp, a few per cent of the arguments differ), so this
equality is expected, not guaranteed by construction: a failure here that traces to a last-place trig difference is a finding about
the routine's rounding."""
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import rad_cases
from tests.raster_helpers import Reader, build_host_program, differing, run_host_program

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "golden"))


@pytest.fixture(scope="module")
def rad_host(tmp_path_factory):
    return build_host_program("rad", tmp_path_factory.mktemp("rad_host"))


def _every_cell(rad_host, tmp_path, pin):
    """rad_host over every raster of a pin, each with its own geo -> the number of cases checked"""
    import make_rad_rsun as gen
    checked = 0
    for raster in range(len(pin["dem"])):
        cases = [c for c in pin["cases"] if c["raster"] == raster]
        case_list = [(c["name"], raster, c["settings"], c["when"], c["keep"], c["transmissivity"]) for c in cases]
        static = (pin["lat"][raster], pin["lon"][raster], pin["slope"][raster], pin["aspect"][raster])
        with open(tmp_path / f"pin{raster}.bin", "wb") as f:                 # the format is the pin driver's
            gen.write_input(f, pin["dem"][raster], pin["flag"], rad_cases.pin_geo(pin, raster), case_list, list(pin["transmissivity"]), static=static)
        out = Reader(run_host_program(rad_host, tmp_path, f"raster{raster}", [(tmp_path / f"pin{raster}.bin").read_bytes()]))
        for case in cases:
            status = int(out.take(np.int32)[0])
            assert status == (1 if "refuses" in case["name"] else 0), case["name"]
            got = out.take(np.float32, 5, *pin["dem"][raster].shape)
            same = ~differing(got, rad_cases.pin_maps(pin, case))
            assert same.all(), (case["name"], int((~same).sum()), np.argwhere(~same)[:4].tolist())
            checked += 1
        assert out.done()
    return checked


def test_host_build_of_the_kernels_point_function_equals_the_pin_in_every_cell(rad_host, tmp_path):
    pin = rad_cases.load_pin()
    assert _every_cell(rad_host, tmp_path, pin) == len(pin["cases"]) >= 40


def test_host_build_of_the_kernels_point_function_equals_the_places_pin_in_every_cell(rad_host, tmp_path):
    """radsHour, radsCell and rad_point at the other places, dates and edited cells: no exclusions"""
    pin = rad_cases.load_places_pin()
    assert _every_cell(rad_host, tmp_path, pin) == len(pin["cases"]) >= 36


def test_host_build_runs_both_pins_clean_under_the_sanitizers(tmp_path):
    """the program has its own main and is not loaded into python; a sanitizer report ends it with a non-zero status and text on stderr"""
    exe = build_host_program("rad", tmp_path, sanitize=True)
    for pin in (rad_cases.load_pin(), rad_cases.load_places_pin()):
        assert _every_cell(exe, tmp_path, pin) == len(pin["cases"])
