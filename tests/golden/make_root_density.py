#!/usr/bin/env python3
"""Generate tests/golden/root_density.npz: the compiled-reference pin of the root depth and root density maps - the two calls
Project3D::assignTranspiration makes for every crop cell, every hour (src/project3D/project3D.cpp:2487-2498):
Crit3DCrop::computeRootLength3D (agrolib/crop/crop.cpp:651-691, over root::getRootLengthDD, agrolib/crop/root.cpp:139-170) and
root::computeRootDensity3D (root.cpp:505-633, over cardioidDistribution / cylindricalDistribution, root.cpp:255-364), each cell on a
fresh copy of cropList[unit].  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_root_density.py --reference <CRITERIA3D tree>

The driver below is this project's own text: one Crit3DCrop per land unit and one Crit3DSoil per soil with their public fields set from
the tables, the cell loop around the reference's two functions, and a counter per arm.  It is compiled with
`g++ -O2 -ffunction-sections -fdata-sections -Wl,--gc-sections` together with the reference's agrolib/crop/{crop,development,root}.cpp,
soil/soil.cpp, mathFunctions/{basicMath,gammaFunction}.cpp and crit3dDate/crit3dDate.cpp WHERE THEY LIE into a scratch directory, and
only data is recorded: the DEM window, the index maps, the root-unit and soil tables, the layer grid, the degree-day maps, the results
(root length, root depth, first / last root layer, root density of every layer) and the arm table.  A cell that is not computed (no DEM
value, no crop index, no soil index, degree days at the flag) holds the flag in every result.

The lunette values recorded for test_root_host are the driver's own evaluation of the formula of root.cpp:277-284 with the pin build's
compiler and C library (atan2, sqrt) - the reference keeps lunette[] local to cardioidDistribution; what pins it is the density."""
import argparse
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from criteria3d_amd import project3d  # noqa: E402

OUT = HERE / "root_density.npz"
ROW0, COL0, NROWS, NCOLS = 8, 280, 24, 32             # the snow and crop pins' window of ravone_dem_519x1208.npz
COMPUTATION_DEPTH = 0.95                              # the Ravone project's imposed computation depth: it cuts the 1.2 m and 1.5 m soils
CYLINDER, CARDIOID, GAMMA = 0, 1, 2                   # rootDistributionType (agrolib/crop/root.h:11)
LINEAR, EXPONENTIAL, LOGISTIC = 0, 1, 2               # rootGrowthType (root.h:14)
UNIT_FIELDS = ("rootShape", "growth", "isRootStatic", "degreeDaysRootGrowth", "shapeDeformation", "rootDepthMin", "rootDepthMax", "degreeDaysEmergence")
# synthetic land units (numbers in the range of a crop database)
UNITS = (
    (CARDIOID, LOGISTIC, 0, 1200, 1.5, 0.05, 1.0, 120.0),      # an annual: deformation inside [1, 2]
    (CYLINDER, LINEAR, 0, 600, 0.7, 0.0, 0.6, 0.0),            # linear growth from the surface, deformation below 1
    (CARDIOID, LOGISTIC, 1, 1400, 2.5, 0.02, 0.5, -9999.0),    # a grass: static, deformation above 2
    (GAMMA, LOGISTIC, 1, 1200, 1.0, 0.05, 2.0, -9999.0),       # a tree: static, gamma shape, deeper than every soil
    (CYLINDER, LOGISTIC, 0, 1000, 1.6, 0.1, 1.4, 30.0),
    (CARDIOID, LINEAR, 0, 800, 0.0, 0.05, 2.5, 50.0),          # deformation 0 (the Ravone crops'), deeper than every soil
    (GAMMA, LOGISTIC, 0, 900, 1.2, 0.0, 0.8, 100.0),
    (CYLINDER, LOGISTIC, 1, 1200, 1.3, 0.035, 3.0, -9999.0),   # a tree whose roots start 3.5 cm down: the atom clamp on the 0.29 m soil (4 + 26 > 29)
)
# synthetic soils: total depth, horizons (upper, lower, coarse fragments)
SOILS = (
    (1.5, ((0.0, 0.5, 0.1), (0.5, 0.75, 0.0), (0.75, 1.5, 0.02))),      # differing coarse fragments: the renormalisation runs
    (1.2, ((0.0, 0.4, 0.0), (0.4, 1.2, 0.0))),                          # none: it does not
    (0.6, ((0.0, 0.25, 0.02), (0.25, 0.6, 0.3))),                       # the layers below 0.6 m have no horizon
    (0.29, ((0.0, 0.29, 0.0),)),                                        # int(0.29 * 100) + 1 = 29 atoms
    (0.04, ((0.0, 0.04, 0.05),)),                                       # shallower than the tree's and the crops' rootDepthMin: length <= 0
)

DRIVER = r"""
// driver of the root pin: see make_root_density.py
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "soil.h"
#include "crop.h"
#include "root.h"

enum { A_NO_DEM, A_NO_CROP, A_NO_SOIL, A_DD_FLAG, A_COMPUTED, A_STATIC, A_DD_NOT_POSITIVE, A_DD_UP_TO_ONE, A_LINEAR, A_LOGISTIC, A_GROWTH_ENDED, A_MAX_BEYOND_SOIL,
       A_LENGTH_NOT_POSITIVE, A_TOO_SHORT, A_CYLINDER, A_CARDIOID, A_GAMMA, A_DEF_BELOW_1, A_DEF_INSIDE, A_DEF_ABOVE_2, A_MIN_ZERO, A_MIN_NONZERO, A_CLAMP,
       A_RENORMALISED, A_NOT_RENORMALISED, A_LAYER_WITHOUT_HORIZON, A_ROOT_LAYERS_FOUND, A_COUNT };
static const char* armNames[A_COUNT] = {
    "cell: outside the DEM", "cell: no crop index", "cell: no soil index", "cell: degree days at the flag", "cell: computed",
    "length: static roots", "length: degree days <= 0", "length: degree days in (0, 1]", "length: linear growth", "length: logistic growth",
    "length: beyond degreeDaysRootGrowth", "length: rootDepthMax beyond the soil depth", "density: length <= 0 (early return)",
    "density: roots too short (0 rooted atoms)", "density: cylinder", "density: cardioid", "density: gamma unit (becomes a cardioid)",
    "density: shapeDeformation < 1", "density: shapeDeformation in [1, 2]", "density: shapeDeformation > 2", "density: rootDepthMin zero",
    "density: rootDepthMin non-zero", "density: atom clamp (top + rooted > nrAtoms)", "density: renormalised (coarse fragments differ)",
    "density: not renormalised", "density: a layer below the last horizon", "density: first / last root layer found" };
static long arms[A_COUNT];

template <class T> static void rd(FILE* f, T* p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb"); FILE* lun = fopen(argv[3], "wb");
    int dims[7]; float flag;
    if (!in || !out || !lun) return 2;
    rd(in, dims, 7); rd(in, &flag, 1);
    const int nrows = dims[0], ncols = dims[1], nUnits = dims[2], nSoils = dims[3], nrLayers = dims[4], nMaps = dims[5], nLun = dims[6];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> dem(n); rd(in, dem.data(), n);
    std::vector<int> cropIndex(n), soilIndex(n); rd(in, cropIndex.data(), n); rd(in, soilIndex.data(), n);
    std::vector<double> layerDepth(nrLayers), layerThickness(nrLayers); rd(in, layerDepth.data(), nrLayers); rd(in, layerThickness.data(), nrLayers);
    std::vector<Crit3DCrop> cropList(nUnits);
    for (int u = 0; u < nUnits; ++u) {
        int iv[4]; double dv[4]; rd(in, iv, 4); rd(in, dv, 4);
        Crit3DCrop& c = cropList[u];
        c.roots.rootShape = rootDistributionType(iv[0]); c.roots.growth = rootGrowthType(iv[1]);
        c.type = iv[2] ? TREE : HERBACEOUS_ANNUAL;                      // isRootStatic()
        c.roots.degreeDaysRootGrowth = iv[3];
        c.roots.shapeDeformation = dv[0]; c.roots.rootDepthMin = dv[1]; c.roots.rootDepthMax = dv[2]; c.degreeDaysEmergence = dv[3];
        if (c.isRootStatic() != (iv[2] != 0)) return 4;
    }
    std::vector<soil::Crit3DSoil> soilList(nSoils);
    for (int s = 0; s < nSoils; ++s) {
        double td; int nh; rd(in, &td, 1); rd(in, &nh, 1);
        soilList[s].totalDepth = td; soilList[s].nrHorizons = nh; soilList[s].horizon.resize(nh);
        for (int h = 0; h < nh; ++h) { double v[3]; rd(in, v, 3); soilList[s].horizon[h].upperDepth = v[0]; soilList[s].horizon[h].lowerDepth = v[1]; soilList[s].horizon[h].coarseFragments = v[2]; }
    }
    // lunette[] of cardioidDistribution (root.cpp:277-284) for a few numbers of rooted atoms: this driver's own evaluation
    for (int k = 0; k < nLun; ++k) {
        int m; rd(in, &m, 1);
        for (int i = 0; i < m; ++i) {
            double sinAlfa = 1.0 - double(i+1.0) / double((unsigned)m);
            double v = std::max(0.0, 1.0 - sinAlfa * sinAlfa);
            double cosAlfa = std::max(std::sqrt(v), 0.0001);
            double alfa = atan2(sinAlfa, cosAlfa);
            double l = ((PI / 2.0) - alfa - sinAlfa * cosAlfa) / PI;
            fwrite(&l, 8, 1, lun);
        }
    }
    fclose(lun);
    const double dflag = double(flag);
    std::vector<double> length(n), depth(n), density((size_t)nrLayers * n);
    std::vector<int> first(n), last(n);
    for (int k = 0; k < nMaps; ++k) {
        std::vector<float> dd(n); rd(in, dd.data(), n);
        for (size_t c = 0; c < n; ++c) {
            length[c] = depth[c] = dflag; first[c] = last[c] = int(flag);
            for (int l = 0; l < nrLayers; ++l) density[(size_t)l * n + c] = dflag;
            if (isEqual(dem[c], flag)) { arms[A_NO_DEM]++; continue; }
            if (cropIndex[c] < 0) { arms[A_NO_CROP]++; continue; }
            if (soilIndex[c] < 0) { arms[A_NO_SOIL]++; continue; }
            double currentDegreeDays = double(dd[c]);
            if (isEqual(currentDegreeDays, NODATA) || isEqual(dd[c], flag)) { arms[A_DD_FLAG]++; continue; }
            arms[A_COMPUTED]++;
            Crit3DCrop currentCrop = cropList[cropIndex[c]];                       // a fresh copy
            const soil::Crit3DSoil& currentSoil = soilList[soilIndex[c]];
            const bool gamma = currentCrop.roots.rootShape == GAMMA_DISTRIBUTION;
            currentCrop.computeRootLength3D(currentDegreeDays, currentSoil.totalDepth);
            root::computeRootDensity3D(currentCrop, currentSoil, nrLayers, layerDepth, layerThickness);
            const Crit3DRoot& r = currentCrop.roots;
            length[c] = r.currentRootLength; depth[c] = r.rootDepth; first[c] = r.firstRootLayer; last[c] = r.lastRootLayer;
            if ((int)r.rootDensity.size() != nrLayers) return 5;
            for (int l = 0; l < nrLayers; ++l) density[(size_t)l * n + c] = r.rootDensity[l];
            // the arms, from the same inputs
            if (currentCrop.isRootStatic()) arms[A_STATIC]++;
            else if (currentDegreeDays <= 0) arms[A_DD_NOT_POSITIVE]++;
            else if (currentDegreeDays > r.degreeDaysRootGrowth) arms[A_GROWTH_ENDED]++;
            else if (currentDegreeDays <= 1) arms[A_DD_UP_TO_ONE]++;
            else if (r.growth == LINEAR) arms[A_LINEAR]++;
            else if (r.growth == LOGISTIC) arms[A_LOGISTIC]++;
            if (r.rootDepthMax > currentSoil.totalDepth) arms[A_MAX_BEYOND_SOIL]++;
            if (r.currentRootLength <= 0) { arms[A_LENGTH_NOT_POSITIVE]++; continue; }
            const int nrAtoms = int(currentSoil.totalDepth * 100) + 1;
            const int top = int(round(r.rootDepthMin / 0.01));
            const int rooted = int(round(std::min(r.currentRootLength, currentSoil.totalDepth) / 0.01));
            if (rooted == 0) { arms[A_TOO_SHORT]++; continue; }
            if (gamma) arms[A_GAMMA]++;
            if (r.rootShape == CYLINDRICAL_DISTRIBUTION) arms[A_CYLINDER]++; else arms[A_CARDIOID]++;
            if (r.shapeDeformation < 1) arms[A_DEF_BELOW_1]++; else if (r.shapeDeformation > 2) arms[A_DEF_ABOVE_2]++; else arms[A_DEF_INSIDE]++;
            if (r.rootDepthMin == 0) arms[A_MIN_ZERO]++; else arms[A_MIN_NONZERO]++;
            if (top + rooted > nrAtoms) { arms[A_CLAMP]++; if (nrAtoms - top <= 0) return 6; }
            bool without = false, differ = false;
            for (int l = 0; l < nrLayers; ++l) {
                int h = currentSoil.getHorizonIndex(layerDepth[l]);
                if (h == int(NODATA)) without = true;
                else if (currentSoil.horizon[h].coarseFragments != 0) differ = true;
            }
            if (without) arms[A_LAYER_WITHOUT_HORIZON]++;
            if (differ) arms[A_RENORMALISED]++; else arms[A_NOT_RENORMALISED]++;
            if (r.firstRootLayer != NODATA && r.lastRootLayer != NODATA) arms[A_ROOT_LAYERS_FOUND]++;
        }
        fwrite(length.data(), 8, n, out); fwrite(depth.data(), 8, n, out); fwrite(first.data(), 4, n, out); fwrite(last.data(), 4, n, out);
        fwrite(density.data(), 8, density.size(), out);
    }
    fclose(out);
    printf("{");
    for (int a = 0; a < A_COUNT; ++a) printf("%s\"%s\": %ld", a ? ", " : "", armNames[a], arms[a]);
    printf("}\n");
    return 0;
}
"""
LUNETTE_M = (1, 2, 7, 29, 120)


def index_maps(dem, flag):
    """land units in vertical stripes of four columns, soils in horizontal bands of two rows (every pair occurs); blocks without either"""
    crop = (np.arange(NCOLS) // 4 % len(UNITS))[None, :].repeat(NROWS, 0).astype(np.int32)
    crop[12:, :] = np.roll(crop[12:, :], 4, axis=1)
    soil = (np.arange(NROWS) // 2 % len(SOILS))[:, None].repeat(NCOLS, 1).astype(np.int32)
    soil[10:, :] = (soil[10:, :] + 1) % len(SOILS)
    crop[2:4, 5:11] = -1
    soil[14:16, 20:27] = -1
    crop[21, 0:3] = -1
    soil[21, 1:5] = -1
    return crop, soil


def degree_day_maps(dem, flag):
    """a handful of float maps on quarter-degree steps: the flag, <= 0, (0, 1], the first degrees (roots too short), the growth phase, beyond"""
    valid = np.abs(dem.astype(np.float64) - float(flag)) >= 1e-5
    r, c = np.mgrid[0:NROWS, 0:NCOLS]
    maps = []
    m = np.full(dem.shape, 0.0)                         # the year's start: nothing, a negative value, fractions of a degree, the first degrees
    m[:, 0::4] = -5.0
    m[:, 1::4] = 0.5
    m[:, 2::4] = 1.0
    m[:, 3::4] = 1.25 + 0.75 * (r[:, 3::4] % 8)
    m[5, :] = flag
    maps.append(m)
    maps.append(10.0 + 12.5 * ((r * 3 + c // 4 * 5) % 40))               # early growth: every unit walks through many numbers of rooted atoms
    maps.append(300.0 + 22.25 * ((r * 5 + c // 4 * 3) % 40))             # the growth phase up to and across degreeDaysRootGrowth
    m = 550.0 + 50.0 * (r % 16)                                          # around every unit's degreeDaysRootGrowth, on it and one step beyond
    m[17, :] = flag
    maps.append(m)
    maps.append(np.full(dem.shape, 3000.0))                              # the season's end: every root full grown
    return np.stack([np.where(valid, x, flag).astype(np.float32) for x in maps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    ref = Path(a.reference)
    d = np.load(HERE / "ravone_dem_519x1208.npz")
    flag = np.float32(d["nodata"])
    dem = d["dem"][ROW0:ROW0 + NROWS, COL0:COL0 + NCOLS].astype(np.float32)
    crop_index, soil_index = index_maps(dem, flag)
    dd = degree_day_maps(dem, flag)
    thickness, centre = project3d.soil_layers(COMPUTATION_DEPTH)
    layer_depth, layer_thickness = np.array(centre, np.float64), np.array(thickness, np.float64)
    nl = len(thickness)
    agro = ref / "agrolib"
    srcs = [agro / "crop" / "crop.cpp", agro / "crop" / "development.cpp", agro / "crop" / "root.cpp", agro / "soil" / "soil.cpp",
            agro / "mathFunctions" / "basicMath.cpp", agro / "mathFunctions" / "gammaFunction.cpp", agro / "crit3dDate" / "crit3dDate.cpp"]
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        inc = [f"-I{agro / sub}" for sub in ("mathFunctions", "crit3dDate", "gis", "utilities", "crop", "soil")]
        cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"), *map(str, srcs),
               "-o", str(work / "root_pin"), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        with open(work / "in.bin", "wb") as f:
            np.array([NROWS, NCOLS, len(UNITS), len(SOILS), nl, len(dd), len(LUNETTE_M)], np.int32).tofile(f)
            np.array([flag], np.float32).tofile(f)
            dem.tofile(f)
            crop_index.tofile(f)
            soil_index.tofile(f)
            layer_depth.tofile(f)
            layer_thickness.tofile(f)
            for u in UNITS:
                np.array(u[:4], np.int32).tofile(f)
                np.array(u[4:], np.float64).tofile(f)
            for total, horizons in SOILS:
                np.array([total], np.float64).tofile(f)
                np.array([len(horizons)], np.int32).tofile(f)
                np.array(horizons, np.float64).tofile(f)
            for m in LUNETTE_M:
                np.array([m], np.int32).tofile(f)
            dd.tofile(f)
        r = subprocess.run([str(work / "root_pin"), str(work / "in.bin"), str(work / "out.bin"), str(work / "lun.bin")], check=True, capture_output=True, text=True)
        arms = json.loads(r.stdout)
        n = NROWS * NCOLS
        rec = np.dtype([("length", np.float64, (NROWS, NCOLS)), ("depth", np.float64, (NROWS, NCOLS)), ("first", np.int32, (NROWS, NCOLS)),
                        ("last", np.int32, (NROWS, NCOLS)), ("density", np.float64, (nl, NROWS, NCOLS))])
        out = np.fromfile(work / "out.bin", rec)
        assert len(out) == len(dd) and rec.itemsize == n * (8 + 8 + 4 + 4 + 8 * nl)
        lunette = np.fromfile(work / "lun.bin", np.float64)
        assert len(lunette) == sum(LUNETTE_M)
        # which log / exp / atan2 of the two functions are calls of the library in this build, which constants are folded
        dis = subprocess.run(["objdump", "-d", "--no-show-raw-insn", str(work / "root_pin")], capture_output=True, text=True, check=True).stdout
        calls = {}
        for fn in ("getRootLengthDD", "cardioidDistribution", "cylindricalDistribution", "computeRootDensity3D", "computeRootLength3D"):
            body = re.search(r"<_Z\w*" + fn + r"\w*>:\n(.*?)\n\n", dis, re.S)
            calls[fn] = sorted(set(re.findall(r"call\s+\w+ <(\w+)@plt>", body.group(1)))) if body else None
        print("library calls:", calls)

    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    for name in rec.names:
        assert np.isfinite(out[name]).all(), f"{name} holds inf / NaN: change the tables"
    empty = [k for k, v in arms.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"
    soil_horizons = np.full((len(SOILS), max(len(h) for _, h in SOILS), 3), -9999.0)
    for s, (_, hz) in enumerate(SOILS):
        soil_horizons[s, :len(hz)] = hz
    save = dict(dem=dem, flag=flag, crop_index=crop_index, soil_index=soil_index, unit_fields=np.array(UNIT_FIELDS), units=np.array(UNITS, np.float64),
                soil_total_depth=np.array([s[0] for s in SOILS]), soil_nr_horizons=np.array([len(s[1]) for s in SOILS], np.int32), soil_horizons=soil_horizons,
                layer_depth=layer_depth, layer_thickness=layer_thickness, degree_days=dd, length=out["length"], depth=out["depth"], first=out["first"],
                last=out["last"], density=out["density"], lunette_m=np.array(LUNETTE_M, np.int32), lunette=lunette,
                window=np.array([ROW0, COL0, NROWS, NCOLS], np.int32), arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64),
                library_calls=np.array(json.dumps(calls)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(dd)} degree-day maps, {nl} layers")
    assert OUT.stat().st_size <= (HERE / "snow_brooks.npz").stat().st_size
    return 0


if __name__ == "__main__":
    sys.exit(main())
