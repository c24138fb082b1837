#!/usr/bin/env python3
"""Generate tests/golden/relhum_dew.npz: the compiled-reference pin of the relative humidity from the dew point -
relHumFromTdew(float, float) (agrolib/meteo/meteo.cpp:301-315), what Crit3DHourlyMeteoMaps::computeRelativeHumidityMap
(agrolib/project/meteoMaps.cpp:301-321) evaluates per cell.  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_relhum_dew.py --reference <CRITERIA3D tree>

The driver below is this project's own text: it reads float pairs, calls the reference's relHumFromTdew on each, and walks one small raster
with the rule of the map loop (the emptied grid keeps its flag where either input holds the flag; isEqual of basicMath.h).  It is compiled
with plain `g++ -O2` together with the reference's agrolib/meteo/meteo.cpp WHERE IT LIES into a scratch directory (unused functions are
dropped at link time), and only data is recorded: the seeded pairs, the raster's two input maps, the results and the arm table.

Pairs (seeded, quantised to 1/16 degC): air temperature in [-40, 50], dew point from 70 degC below it to 5 degC above it - saturated pairs
(100), very dry pairs that reach the max(1.f, ..) floor, NODATA in either input.  The raster (7 x 37) has a flag other than -9999, cells
that hold it in either map and cells that hold NODATA.  The restatement (criteria3d_amd/hour.py) must equal the pin bit for bit before the
fixture is written."""
import argparse
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
OUT = HERE / "relhum_dew.npz"
PAIRS = 6000
SHAPE = (7, 37)
FLAG = -32768.0
NODATA = -9999.0

DRIVER = r"""
// driver of the relative humidity pin: see make_relhum_dew.py
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "basicMath.h"
#include "commonConstants.h"
#include "meteo.h"

static std::vector<float> readMap(FILE* f, size_t n) { std::vector<float> v(n); if (fread(v.data(), 4, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    int dims[2]; float flag;
    if (!in || !out || fread(dims, 4, 2, in) != 2 || fread(&flag, 4, 1, in) != 1) return 2;
    const size_t pairs = (size_t)dims[0], cells = (size_t)dims[1];
    std::vector<float> td = readMap(in, pairs), t = readMap(in, pairs), airT = readMap(in, cells), dewT = readMap(in, cells);
    std::vector<float> rh(pairs), map(cells, flag);                    // emptyGrid
    for (size_t k = 0; k < pairs; ++k) rh[k] = relHumFromTdew(td[k], t[k]);
    for (size_t c = 0; c < cells; ++c)
        if (! isEqual(airT[c], flag) && ! isEqual(dewT[c], flag)) map[c] = relHumFromTdew(dewT[c], airT[c]);
    fwrite(rh.data(), 4, pairs, out);
    fwrite(map.data(), 4, cells, out);
    fclose(out);
    return 0;
}
"""


def inputs(seed=20261020):
    rng = np.random.default_rng(seed)
    q = lambda v: (np.round(np.asarray(v) * 16) / 16).astype(np.float32)
    t = q(rng.uniform(-40.0, 50.0, PAIRS))
    td = q(t - rng.uniform(-5.0, 70.0, PAIRS))
    t[:40], td[:40] = q(np.linspace(-40, 50, 40)), q(np.linspace(-40, 50, 40))          # Td == T
    t[40:80], td[40:80] = q(np.linspace(20, 50, 40)), np.float32(-40.0)                  # the driest pairs
    td[80:90] = NODATA
    t[90:100] = NODATA
    td[100:103], t[100:103] = NODATA, NODATA
    air = q(rng.uniform(-40.0, 50.0, SHAPE))
    dew = q(air - rng.uniform(-5.0, 70.0, SHAPE))
    air[0, 0] = FLAG; dew[0, 0] = FLAG
    air[3, 18] = FLAG
    dew[3, 19] = FLAG
    air[rng.random(SHAPE) < 0.04] = FLAG
    dew[rng.random(SHAPE) < 0.04] = FLAG
    air[6, 30], dew[6, 31] = NODATA, NODATA                                              # the function's own test, second
    dew[6, 32], air[6, 32] = np.float32(12.0), np.float32(12.0)
    dew[6, 36], air[6, 36] = np.float32(-38.0), np.float32(49.0)                         # the last lane: the floor
    return td, t, air.astype(np.float32), dew.astype(np.float32)


def arm_table(td, t, rh, flag_cells=None):
    eq = lambda a, v=NODATA: np.abs(a.astype(np.float64) - v) < 1e-5
    nodata = eq(td) | eq(t)
    arms = {"NODATA in": int(np.count_nonzero(nodata)), "100": int(np.count_nonzero(~nodata & (rh == 100))), "floor": int(np.count_nonzero(~nodata & (rh == 1))),
            "between": int(np.count_nonzero(~nodata & (rh > 1) & (rh < 100)))}
    if flag_cells is not None:
        arms["flag cell"] = int(np.count_nonzero(flag_cells))
    return arms


def main():
    from criteria3d_amd import hour
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    ref = Path(a.reference)
    td, t, air, dew = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        inc = [f"-I{ref / 'agrolib' / sub}" for sub in ("mathFunctions", "meteo", "crit3dDate", "gis", "utilities")]
        cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               str(ref / "agrolib" / "meteo" / "meteo.cpp"), "-o", str(work / "relhum_pin"), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        with open(work / "in.bin", "wb") as f:
            np.array([PAIRS, air.size], np.int32).tofile(f)
            np.array([FLAG], np.float32).tofile(f)
            for m in (td, t, air, dew):
                np.ascontiguousarray(m, np.float32).tofile(f)
        subprocess.run([str(work / "relhum_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True)
        raw = np.fromfile(work / "out.bin", np.float32)
    rh, rh_map = raw[:PAIRS], raw[PAIRS:].reshape(SHAPE)
    assert np.isfinite(rh).all() and np.isfinite(rh_map).all(), "a compared value is inf / NaN"
    flag_cells = (air == np.float32(FLAG)) | (dew == np.float32(FLAG))
    arms = arm_table(td, t, rh)
    map_arms = arm_table(dew[~flag_cells], air[~flag_cells], rh_map[~flag_cells], flag_cells)
    for name, table in (("pairs", arms), ("raster", map_arms)):
        print(name, table)
        empty = [k for k, v in table.items() if v == 0]
        assert not empty, f"{name}: arms never reached: {empty}"
    assert np.all(rh_map[flag_cells] == np.float32(FLAG))
    # the restatement equals the pin bit for bit before the fixture is written
    bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    assert np.array_equal(bits(hour.rel_hum_from_tdew(td, t)), bits(rh)), "the restatement differs from the reference on the pairs"
    assert np.array_equal(bits(hour.restate_relative_humidity(air, dew, FLAG)), bits(rh_map)), "the restatement differs from the reference on the raster"
    names = list(map_arms)
    np.savez_compressed(OUT, dew_t=td, air_t=t, rel_hum=rh, flag=np.float32(FLAG), map_air_t=air, map_dew_t=dew, map_rel_hum=rh_map,
                        arm_names=np.array(names), arm_counts=np.array([arms.get(k, 0) + map_arms[k] for k in names], np.int64),      # pairs and raster together
                        map_arm_counts=np.array([map_arms[k] for k in names], np.int64))
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
