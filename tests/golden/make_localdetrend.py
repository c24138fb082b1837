#!/usr/bin/env python3
"""Generate tests/golden/localdetrend.npz: the compiled-reference pin of air and dew-point temperature with local detrending - the cell
loop of Project::interpolationDemLocalDetrending (agrolib/project/project.cpp:3226-3254) on Crit3DInterpolationSettings: localSelection,
preInterpolation (multipleDetrendingMain) and interpolate() for every DEM cell, with the map value, the selected count, localRadius, the
significance flag, float(R2) and the fitted parameters of every cell; and what setMultipleDetrendingHeightTemperatureRange and
calculateFirstGuessCombinations make of a configured range.  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_localdetrend.py --reference <CRITERIA3D tree>

The driver below is this project's own text.  It is compiled with `g++ -std=c++17 -O2 -fopenmp -ffunction-sections -fdata-sections
-Wl,--gc-sections` together with the reference's agrolib/interpolation/{interpolation,interpolationSettings,interpolationPoint,
spatialControl}.cpp, meteo/{meteo,meteoPoint,quality}.cpp, gis/*.cpp, mathFunctions/*.cpp and crit3dDate/*.cpp WHERE THEY LIE into a
scratch directory, and only data is recorded.  It reads and writes the files of tests/localdetrend_host.cpp (tests/localdetrend_cases.py).

Two rasters of 500 m cells at UTM-sized coordinates: `relief`, 7 x 37 cells with a real elevation range and flag cells, whose stations
reach tens of kilometres out so that the 7.5 km rings matter, and `tiny`, 5 x 9 cells with a dozen stations and short first-guess lists,
on which the Python restatement of criteria3d_amd/localdetrend.py is held against the reference bit for bit before anything is written.
The arms named below are counted (from the restatement on `tiny`, from the recorded outcome on `relief`): none may be empty."""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from criteria3d_amd import localdetrend as ld, meteo  # noqa: E402
from tests import localdetrend_cases as lc  # noqa: E402
from tests.raster_helpers import same  # noqa: E402

OUT = HERE / "localdetrend.npz"
FLAG = np.float32(-9999.0)

DRIVER = r"""
// driver of the local detrending pin: see make_localdetrend.py
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "crit3dDate.h"
#include "gis.h"
#include "meteo.h"
#include "meteoPoint.h"
#include "interpolationSettings.h"
#include "interpolationPoint.h"
#include "interpolation.h"

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
template <class T> static void wr(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short output\n"); exit(3); } }

static const meteoVariable refVar[7] = { airTemperature, precipitation, airRelHumidity, windScalarIntensity, globalIrradiance, atmTransmissivity, airDewTemperature };
static const TInterpolationMethod refMethod[3] = { idw, shepard, shepard_modified };
static const TFittingFunction refFunction[3] = { piecewiseTwo, piecewiseThreeFree, piecewiseThree };
enum { MAXP = 6, MAXG = 31 };

// ranges <in> <out>: per check int32 function, nParameters; int32 position[nParameters]; double range[2 * nParameters], pointsRange[2]
//                    -> int32 nCombinations; double range[2 * nParameters]; double combinations[nCombinations][nParameters]
static int ranges(FILE* in, FILE* out)
{
    int count; rd(in, &count, 1);
    for (int k = 0; k < count; ++k) {
        int iv[2]; rd(in, iv, 2);
        const int np = iv[1];
        std::vector<int> position(np); rd(in, position.data(), np);
        std::vector<double> range(2 * np); rd(in, range.data(), 2 * np);
        double pointsRange[2]; rd(in, pointsRange, 2);
        Crit3DInterpolationSettings settings;
        settings.initialize();
        settings.setUseMultipleDetrending(true);
        settings.setUseLocalDetrending(true);
        Crit3DProxy height;
        height.setName("elevation");
        height.setFittingFunctionName(refFunction[iv[0]]);
        height.setFittingParametersRange(range);
        height.setFittingFirstGuess(position);
        settings.addProxy(height, true);
        settings.setPointsRange(pointsRange[0], pointsRange[1]);
        if (!setMultipleDetrendingHeightTemperatureRange(settings)) return 4;
        const std::vector<double> got = settings.getProxy(0)->getFittingParametersRange();
        const std::vector<std::vector<double>> combos = settings.getProxy(0)->getFirstGuessCombinations();
        const int n = (int)combos.size();
        wr(out, &n, 1); wr(out, got.data(), got.size());
        for (const auto& c : combos) wr(out, c.data(), c.size());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    FILE* in = fopen(argv[2], "rb"); FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    if (!strcmp(argv[1], "ranges")) { const int e = ranges(in, out); fclose(out); return e; }
    int dims[3]; float flag; double geo[3];
    rd(in, dims, 3); rd(in, &flag, 1); rd(in, geo, 3);
    const int nrows = dims[0], ncols = dims[1], nCases = dims[2];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> demv(n); rd(in, demv.data(), n);

    gis::Crit3DRasterGrid dem;
    dem.header->nrRows = nrows; dem.header->nrCols = ncols; dem.header->cellSize = geo[2]; dem.header->invCellSize = 1.0 / geo[2];
    dem.header->llCorner.x = geo[0]; dem.header->llCorner.y = geo[1]; dem.header->flag = flag;
    dem.initializeGrid(flag);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) dem.value[r][c] = demv[(size_t)r * ncols + c];
    dem.isLoaded = true;

    for (int k = 0; k < nCases; ++k) {
        int iv[8]; float fv[2]; double table[(3 + MAXG) * MAXP];
        rd(in, iv, 8); rd(in, fv, 2); rd(in, table, (3 + MAXG) * MAXP);
        const int var = iv[0], method = iv[1], function = iv[2], np = iv[3], nGuess = iv[4], minLocal = iv[5], useDetrending = iv[6], m = iv[7];
        std::vector<double> sx(m), sy(m); std::vector<float> sh(m), sv(m);
        rd(in, sx.data(), m); rd(in, sy.data(), m); rd(in, sh.data(), m); rd(in, sv.data(), m);

        Crit3DInterpolationSettings settings;
        settings.initialize();
        settings.setInterpolationMethod(refMethod[method]);
        settings.setUseThermalInversion(false);
        settings.setUseMultipleDetrending(true);
        settings.setUseLocalDetrending(true);
        settings.setMinPointsLocalDetrending(minLocal);
        settings.setUseDoNotRetrend(useDetrending == 0);
        settings.setCurrentDEM(&dem);
        settings.setPointsBoundingBoxArea(fv[1]);
        Crit3DProxy height;
        height.setName("elevation");
        height.setGrid(&dem);
        height.setFittingFunctionName(refFunction[function]);
        std::vector<double> range(2 * np);
        for (int j = 0; j < np; ++j) { range[j] = table[j]; range[np + j] = table[MAXP + j]; }
        height.setFittingParametersRange(range);
        height.setStdDevThreshold(fv[0]);
        std::vector<std::vector<double>> combos(nGuess, std::vector<double>(np));
        for (int g = 0; g < nGuess; ++g) for (int j = 0; j < np; ++j) combos[g][j] = table[(3 + g) * MAXP + j];
        height.setFirstGuessCombinations(combos);
        settings.addProxy(height, true);
        settings.setCurrentCombination(settings.getSelectedCombination());
        // the delta the reference forms from the range is the one the table hands to the other builds
        for (int j = 0; j < np; ++j) {
            const double delta = (range[np + j] - range[j]) / 800;
            if (memcmp(&delta, &table[2 * MAXP + j], sizeof(double)) != 0) { fprintf(stderr, "case %d: parametersDelta[%d] differs\n", k, j); return 4; }
        }
        Crit3DMeteoSettings meteoSettings;
        Crit3DClimateParameters climateParameters;
        std::vector<Crit3DMeteoPoint> meteoPoints;
        Crit3DTime myTime;
        std::string errorStr;

        std::vector<Crit3DInterpolationDataPoint> points(m);
        for (int i = 0; i < m; ++i) {
            points[i].index = i; points[i].isActive = true; points[i].value = sv[i];
            points[i].point->utm.x = sx[i]; points[i].point->utm.y = sy[i]; points[i].point->z = sh[i];
            points[i].proxyValues.push_back(sh[i]);
        }

        std::vector<float> map(n, flag), radius(n, NODATA), r2(n, NODATA);
        std::vector<uint32_t> count(n, 0);
        std::vector<int32_t> significant(n, 0);
        std::vector<double> parameters(n * MAXP, NODATA);
        // the cell loop of interpolationDemLocalDetrending, project.cpp:3222-3254
        Crit3DInterpolationSettings mySettings = settings;
        std::vector<double> proxyValues(mySettings.getProxyNr());
        const auto t0 = std::chrono::steady_clock::now();
        long cells = 0;
        for (long row = 0; row < nrows; row++) {
            for (long col = 0; col < ncols; col++) {
                const size_t c = (size_t)row * ncols + col;
                float z = dem.value[row][col];
                if (isEqual(z, flag)) continue;
                double x, y;
                gis::getUtmXYFromRowCol(*dem.header, row, col, &x, &y);
                getProxyValuesXY(x, y, mySettings, proxyValues);
                if (proxyValues[0] != z) { fprintf(stderr, "case %d: the height proxy of cell %ld %ld is not the DEM value\n", k, row, col); return 4; }
                std::vector<Crit3DInterpolationDataPoint> subset;
                localSelection(points, subset, x, y, mySettings, false);
                preInterpolation(subset, mySettings, &meteoSettings, &climateParameters, meteoPoints, refVar[var], myTime, errorStr);
                map[c] = interpolate(subset, mySettings, &meteoSettings, refVar[var], x, y, z, proxyValues, true);
                count[c] = (uint32_t)subset.size();
                radius[c] = mySettings.getLocalRadius();
                significant[c] = mySettings.getCurrentCombination().isProxySignificant(0) ? 1 : 0;
                r2[c] = mySettings.getProxy(0)->getRegressionR2();
                const std::vector<std::vector<double>> fitted = mySettings.getFittingParameters();
                if (!fitted.empty()) {
                    if (!significant[c] || (int)fitted.front().size() != np) { fprintf(stderr, "case %d: parameters without significance\n", k); return 4; }
                    for (int j = 0; j < np; ++j) parameters[c * MAXP + j] = fitted.front()[j];
                } else if (significant[c]) { fprintf(stderr, "case %d: significance without parameters\n", k); return 4; }
                mySettings.clearFitting();
                mySettings.setCurrentCombination(mySettings.getSelectedCombination());
                ++cells;
            }
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d %ld %.6f\n", k, cells, seconds);
        wr(out, map.data(), n); wr(out, count.data(), n); wr(out, radius.data(), n); wr(out, significant.data(), n); wr(out, r2.data(), n);
        wr(out, parameters.data(), n * MAXP);
    }
    fclose(out);
    return 0;
}
"""

# setChosenElevationFunction's defaults (interpolationSettings.cpp:231-306): the configured range (minima, then maxima; the temperature
# slots are set from the point range) and the first-guess positions
H0_MIN, H0_MAX, DELTA_MIN, DELTA_MAX, SLOPE_MIN, SLOPE_MAX, INV_MIN, INV_MAX = -350.0, 2500.0, 300.0, 1000.0, 0.002, 0.007, -0.01, -0.0015
DEFAULTS = {
    ld.PIECEWISE_TWO: ([0.0, 0.0, SLOPE_MIN, INV_MIN, H0_MAX, 0.0, SLOPE_MAX, INV_MAX], [0, 1, 1, 1]),
    ld.PIECEWISE_THREE: ([H0_MIN, 0.0, DELTA_MIN, SLOPE_MIN, INV_MIN, H0_MAX, 0.0, DELTA_MAX, SLOPE_MAX, INV_MAX], [0, 1, 1, 1, 1]),
    ld.PIECEWISE_THREE_FREE: ([H0_MIN, 0.0, DELTA_MIN, SLOPE_MIN, INV_MIN, INV_MIN, H0_MAX, 0.0, DELTA_MAX, SLOPE_MAX, INV_MAX, INV_MAX], [0, 1, 1, 1, 1, 1]),
}


def short_delta(function):
    """a configured range whose height difference (parameter 2) starts at 0, with the first guess at its minimum: par[2] is raised to 10"""
    rng, pos = DEFAULTS[function]
    rng, pos = list(rng), list(pos)
    rng[2] = 0.0
    pos[1] = 0                  # calculateFirstGuessCombinations reads the position of parameter 2's steps from slot 1
    pos[2] = 0
    return rng, pos


def bounding_box_area(x, y):
    return np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))


def temperature(h, rng, noise=0.6):
    """an inversion below 350 m, -5.5 K / km above, and noise"""
    t = np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0))
    return np.round(t + rng.normal(0.0, noise, len(h)), 1).astype(np.float32)


def raster_relief():
    rows, cols, cs = 7, 37, 500.0
    xll, yll = 681000.0, 4925000.0
    r, c = np.mgrid[0:rows, 0:cols]
    dem = 60.0 + 38.0 * c + 90.0 * np.sin(c / 4.3) * (1 + 0.2 * r) + 420.0 * np.exp(-((c - 25.0) / 3.5) ** 2) - 25.0 * r
    dem = np.round(dem, 1).astype(np.float32)
    for rc in ((0, 0), (0, 1), (2, 15), (3, 15), (4, 16), (6, 36), (5, 30), (1, 21)):
        dem[rc] = FLAG
    return dem, xll, yll, cs


def raster_tiny():
    rows, cols, cs = 5, 9, 500.0
    xll, yll = 681000.0, 4925000.0
    r, c = np.mgrid[0:rows, 0:cols]
    dem = np.round(150.0 + 95.0 * c - 30.0 * r + 60.0 * np.sin(1.7 * c + r), 1).astype(np.float32)
    dem[1, 4] = FLAG
    dem[4, 0] = FLAG
    return dem, xll, yll, cs


def stations(rng, xll, yll, cs, shape, n_near, n_far, reach):
    """n_near stations within 3 km of the raster's west end, n_far up to `reach` metres around it; heights 20 .. 1 900 m"""
    rows, cols = shape
    x = np.concatenate([xll + rng.uniform(-1500.0, 3000.0, n_near), xll + rng.uniform(-reach, cols * cs + reach, n_far)])
    y = np.concatenate([yll + rng.uniform(0.0, rows * cs, n_near), yll + rng.uniform(-reach, rows * cs + reach, n_far)])
    h = np.round(np.concatenate([rng.uniform(20.0, 700.0, n_near), rng.uniform(20.0, 1900.0, n_far)]), 1).astype(np.float32)
    return np.round(x, 2), np.round(y, 2), h


def fit_of(function, rng_pos, points_range, min_local, threshold=ld.NODATA, first_guess=None, keep=None):
    fit = ld.make_fit(function, rng_pos[0], rng_pos[1], points_range, min_local, threshold)
    if keep is not None:
        fit["first_guess"] = fit["first_guess"][:keep]
    if first_guess is not None:
        fit["first_guess"] = first_guess
    return fit


def case(label, var, method, fit, x, y, h, v, use_detrending=1):
    return dict(label=label, var=meteo.VARIABLES.index(var), method=method, fit=fit, useDetrending=use_detrending, x=np.asarray(x, np.float64), y=np.asarray(y, np.float64),
                height=np.asarray(h, np.float32), value=np.asarray(v, np.float32), area=bounding_box_area(np.asarray(x), np.asarray(y)))


def relief_cases(rng, dem, xll, yll, cs):
    x, y, h = stations(rng, xll, yll, cs, dem.shape, 12, 26, 42000.0)
    t = temperature(h, rng)
    pr = (float(t.min()), float(t.max()))
    centre = lambda row, col: (xll + cs * (col + 0.5), yll + cs * (dem.shape[0] - row - 0.5))
    out = []
    out.append(case("plain", "airT", meteo.IDW, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], pr, 8), x, y, h, t))
    out.append(case("raised", "airT", meteo.SHEPARD, fit_of(ld.PIECEWISE_THREE, short_delta(ld.PIECEWISE_THREE), pr, 5), x, y, h, t))
    out.append(case("raised", "airT", meteo.SHEPARD_MODIFIED, fit_of(ld.PIECEWISE_THREE_FREE, short_delta(ld.PIECEWISE_THREE_FREE), pr, 8), x, y, h, t))
    dew = (t - np.float32(3.5)).astype(np.float32)
    out.append(case("rings", "dewT", meteo.SHEPARD_MODIFIED, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (float(dew.min()), float(dew.max())), 20), x, y, h, dew))
    s = np.r_[0:len(x):2, 1:7:2]                                    # 22 stations: no more than minPoints (24), no fewer than minPointsLocalDetrending
    out.append(case("all", "airT", meteo.IDW, fit_of(ld.PIECEWISE_THREE, DEFAULTS[ld.PIECEWISE_THREE], pr, 20), x[s], y[s], h[s], t[s]))
    out.append(case("threshold", "airT", meteo.SHEPARD, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], pr, 5, threshold=2000.0), x, y, h, t))
    flat = np.full(len(x), 16.0, np.float32)                        # a power of two: the weighted mean is exact, the total deviation 0
    out.append(case("equal", "dewT", meteo.IDW, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (16.0, 16.0), 8), x, y, h, flat))
    vee = np.round(6.0 + 0.012 * np.abs(h - 900.0) + rng.normal(0.0, 0.3, len(h)), 1).astype(np.float32)
    out.append(case("vee", "airT", meteo.SHEPARD_MODIFIED, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (float(vee.min()), float(vee.max())), 8), x, y, h, vee))
    # a first guess near the optimum but below the minimum of parameter 1 (a point range that begins above the stations' values): every
    # step is clamped back to a worse place, the iteration cap ends the fit
    base = fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (16.0, float(t.max()) + 4.0), 5)
    low = [list(g) for g in base["first_guess"][:3]]
    low[1][1] = 10.5
    out.append(case("cap", "airT", meteo.IDW, dict(base, first_guess=low), x, y, h, t))
    # minPoints + 1 stations, two of them on one cell centre: beyondLastPoint ends that cell's loop short of minPoints
    cx, cy = centre(3, 6)
    bx, by, bh = np.append(x[:5], [cx, cx]), np.append(y[:5], [cy, cy]), np.append(h[:5], [float(dem[3, 6]), float(dem[3, 6]) + 40.0]).astype(np.float32)
    bt = temperature(bh, rng)
    out.append(case("beyond", "airT", meteo.SHEPARD_MODIFIED, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (float(bt.min()), float(bt.max())), 5), bx, by, bh, bt))
    gaps = h.copy()
    gaps[1::3] = np.float32(ld.NODATA)
    out.append(case("gaps", "airT", meteo.IDW, fit_of(ld.PIECEWISE_THREE_FREE, DEFAULTS[ld.PIECEWISE_THREE_FREE], pr, 8), x, y, gaps, t))
    out.append(case("noretrend", "dewT", meteo.SHEPARD, fit_of(ld.PIECEWISE_THREE_FREE, DEFAULTS[ld.PIECEWISE_THREE_FREE], (float(dew.min()), float(dew.max())), 5), x, y, h,
                    dew, use_detrending=0))
    return out


def tiny_cases(rng, dem, xll, yll, cs):
    x, y, h = stations(rng, xll, yll, cs, dem.shape, 5, 7, 16000.0)
    t = temperature(h, rng)
    pr = (float(t.min()), float(t.max()))
    out = []
    out.append(case("plain", "airT", meteo.IDW, fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], pr, 5, keep=4), x, y, h, t))
    out.append(case("raised", "dewT", meteo.SHEPARD, fit_of(ld.PIECEWISE_THREE, short_delta(ld.PIECEWISE_THREE), pr, 5, keep=3), x, y, h, t))
    out.append(case("raised", "airT", meteo.SHEPARD_MODIFIED, fit_of(ld.PIECEWISE_THREE_FREE, short_delta(ld.PIECEWISE_THREE_FREE), pr, 8, keep=3), x, y, h, t))
    base = fit_of(ld.PIECEWISE_TWO, DEFAULTS[ld.PIECEWISE_TWO], (16.0, float(t.max()) + 4.0), 5)
    low = [list(g) for g in base["first_guess"][:2]]
    low[1][1] = 10.5
    gaps = h.copy()
    gaps[2] = np.float32(ld.NODATA)
    out.append(case("cap", "airT", meteo.SHEPARD_MODIFIED, dict(base, first_guess=low), x, y, gaps, t))
    return out


def run_cases(exe, work, r, cases):
    src, dst = work / f"{r['name']}.in", work / f"{r['name']}.out"
    lc.write_input(src, r, cases)
    res = subprocess.run([str(exe), "cases", str(src), str(dst)], check=True, capture_output=True, text=True)
    timing = [line.split() for line in res.stdout.strip().splitlines()]
    return lc.read_output(dst, r, cases), [(int(c), float(s)) for _, c, s in timing]


def run_ranges(exe, work, checks):
    src, dst = work / "ranges.in", work / "ranges.out"
    with open(src, "wb") as f:
        np.array([len(checks)], np.int32).tofile(f)
        for c in checks:
            n = ld.PARAMETERS[c["function"]]
            np.array([c["function"], n], np.int32).tofile(f)
            np.array(c["position"], np.int32).tofile(f)
            np.array(c["configured"], np.float64).tofile(f)
            np.array(c["points_range"], np.float64).tofile(f)
    subprocess.run([str(exe), "ranges", str(src), str(dst)], check=True)
    raw = np.fromfile(dst, np.uint8)
    pos = 0
    for c in checks:
        n = ld.PARAMETERS[c["function"]]
        count = int(raw[pos:pos + 4].view(np.int32)[0])
        pos += 4
        c["want_range"] = raw[pos:pos + 16 * n].view(np.float64).tolist()
        pos += 16 * n
        c["want_combinations"] = raw[pos:pos + 8 * n * count].view(np.float64).reshape(count, n).tolist()
        pos += 8 * n * count
    assert pos == raw.size
    return checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    agro = Path(a.reference) / "agrolib"
    srcs = [agro / "interpolation" / f for f in ("interpolation.cpp", "interpolationSettings.cpp", "interpolationPoint.cpp", "spatialControl.cpp")]
    srcs += [agro / "meteo" / f for f in ("meteo.cpp", "meteoPoint.cpp", "quality.cpp")]
    for sub in ("gis", "mathFunctions", "crit3dDate"):
        srcs += sorted((agro / sub).glob("*.cpp"))
    rng = np.random.default_rng(20261020)
    save, arms, cpu = {}, {}, []
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        exe = work / "localdetrend_pin"
        inc = [f"-I{agro / sub}" for sub in ("interpolation", "meteo", "gis", "mathFunctions", "crit3dDate", "utilities")]
        cmd = ["g++", "-w", "-std=c++17", "-O2", "-fopenmp", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               *map(str, srcs), "-o", str(exe), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)

        # ---- what stays with the caller: the range and the first-guess list
        checks = []
        for function, (rng_, pos) in DEFAULTS.items():
            checks.append(dict(function=function, configured=rng_, position=pos, points_range=[3.25, 21.5]))
            checks.append(dict(function=function, configured=short_delta(function)[0], position=short_delta(function)[1], points_range=[-7.0, 12.75]))
        checks.append(dict(function=ld.PIECEWISE_THREE, configured=DEFAULTS[ld.PIECEWISE_THREE][0], position=[2, 2, 1, 0, 1], points_range=[0.5, 30.0]))
        checks.append(dict(function=ld.PIECEWISE_TWO, configured=DEFAULTS[ld.PIECEWISE_TWO][0], position=[1, 0, 2, 1], points_range=[0.5, 30.0]))
        for c in run_ranges(exe, work, checks):
            mine = ld.height_temperature_range(c["function"], c["configured"], c["points_range"])
            assert np.array_equal(np.array(mine).view(np.uint64), np.array(c["want_range"]).view(np.uint64)), ("range", c)
            combos = ld.first_guess_combinations(c["function"], mine, c["position"])
            assert np.array_equal(np.array(combos).view(np.uint64), np.array(c["want_combinations"]).view(np.uint64)), ("first guesses", c)
            assert len(combos) <= ld.MAX_FIRST_GUESS
        assert max(len(c["want_combinations"]) for c in checks) == ld.MAX_FIRST_GUESS

        for name, (dem, xll, yll, cs), maker in (("relief", raster_relief(), relief_cases), ("tiny", raster_tiny(), tiny_cases)):
            r = dict(name=name, dem=dem, xll=xll, yll=yll, cell_size=cs, flag=FLAG)
            cases = maker(rng, dem, xll, yll, cs)
            got, timing = run_cases(exe, work, r, cases)
            inside = dem != FLAG
            for k, (c, g) in enumerate(zip(cases, got)):
                what = f"{name} {k} {lc.case_name(c)}"
                assert np.isfinite(g["value"]).all(), (what, "a map holds inf / NaN: change the tables")
                assert (g["value"][~inside] == FLAG).all() and (g["count"][inside] > 0).all(), what
                print(f"  {what}: significant {int(g['significant'].sum())}/{int(inside.sum())}, count {g['count'][inside].min()}..{g['count'].max()}, "
                      f"{timing[k][1]:.3f} s")
                cpu.append(dict(raster=name, case=lc.case_name(c), stations=len(c["x"]), cells=timing[k][0], seconds=timing[k][1],
                                seconds_per_1000_cells=1000.0 * timing[k][1] / timing[k][0]))
                # the arms the recorded outcome shows
                key = lambda s: arms.__setitem__(s, arms.get(s, 0) + 1)
                need = ld.min_points(c["fit"]["minPointsLocalDetrending"])
                if len(c["x"]) <= need:
                    key("all stations selected")
                key(f"function {ld.FUNCTIONS[c['fit']['function']]}")
                key(f"method {meteo.METHODS[c['method']]}")
                key(f"variable {meteo.VARIABLES[c['var']]}")
                key(f"minPointsLocalDetrending {c['fit']['minPointsLocalDetrending']}")
                if (c["value"] == c["value"][0]).all() and not np.isfinite(g["r2"][inside]).any():
                    key("all station values equal: R2 is x / 0")
                if (g["r2"][g["significant"]] < 0).any():
                    key("bestR2 < 0: the fit is repeated from the RMSE index")
                if c["fit"]["function"] != ld.PIECEWISE_TWO and (g["parameters"][g["significant"]][:, 2] == 10.0).any():
                    key(f"{ld.FUNCTIONS[c['fit']['function']]}: par[2] raised to 10")
            if name == "tiny":
                # ---- the restatement, bit for bit, on every cell; its arms
                for k, (c, g) in enumerate(zip(cases, got)):
                    t0 = time.time()
                    mine = lc.restated(r, c, arms=arms)
                    same(mine, g, f"restatement {k} {lc.case_name(c)}", lc.QUANTITIES)
                    if c["method"] == meteo.SHEPARD:
                        assert not mine["ties"].any(), "two selected stations at one float distance in a shepardIdw case: move a station"
                    print(f"  restatement {k}: equal ({time.time() - t0:.1f} s)")
            else:
                # the selection's arms on the large raster, from the restated selection alone (it equals the recorded count and radius)
                cx, cy = meteo.cell_centres(dem.shape, xll, yll, cs)
                for k, (c, g) in enumerate(zip(cases, got)):
                    ties = False
                    for row, col in np.argwhere(inside):
                        sel, d, w, radius = ld.local_selection(cx[row, col], cy[row, col], c["x"], c["y"], c["fit"]["minPointsLocalDetrending"], c["area"], arms)
                        assert len(sel) == g["count"][row, col] and np.float32(radius) == g["radius"][row, col], (k, row, col)
                        ties = ties or (d is not None and len(set(np.array(d).tolist())) < len(d))
                        elevation = int((c["height"][sel] != np.float32(ld.NODATA)).sum())
                        if not g["significant"][row, col]:
                            if elevation < max(ld.MIN_NR, c["fit"]["minPointsLocalDetrending"]):
                                arms["height not significant: fewer elevation points than minPointsLocalDetrending"] = \
                                    arms.get("height not significant: fewer elevation points than minPointsLocalDetrending", 0) + 1
                            elif c["fit"]["stdDevThreshold"] != ld.NODATA:
                                arms["height not significant: standard deviation below the threshold"] = \
                                    arms.get("height not significant: standard deviation below the threshold", 0) + 1
                    if c["method"] == meteo.SHEPARD:
                        assert not ties, "two selected stations at one float distance in a shepardIdw case: move a station"
            save.update({f"{name}_dem": dem, f"{name}_geo": np.array([xll, yll, cs], np.float64),
                         f"{name}_cases": np.array(json.dumps([dict(label=c["label"], var=c["var"], method=c["method"], fit=c["fit"], useDetrending=c["useDetrending"],
                                                                    area=float(c["area"])) for c in cases]))})
            for k, (c, g) in enumerate(zip(cases, got)):
                n_par = len(c["fit"]["min"])
                assert (g["parameters"][..., n_par:] == ld.NODATA).all() and g["count"].max() < 65536
                save.update({f"{name}_c{k}_x": c["x"], f"{name}_c{k}_y": c["y"], f"{name}_c{k}_h": c["height"], f"{name}_c{k}_v": c["value"], f"{name}_c{k}_map": g["value"],
                             f"{name}_c{k}_count": g["count"].astype(np.uint16), f"{name}_c{k}_radius": g["radius"], f"{name}_c{k}_sig": g["significant"].astype(np.uint8),
                             f"{name}_c{k}_r2": g["r2"], f"{name}_c{k}_par": g["parameters"][..., :n_par].copy()})
        for f in (1, 2):
            if ld.RAISED[f]:
                arms[f"{ld.FUNCTIONS[f]}: par[2] raised to 10"] = arms.get(f"{ld.FUNCTIONS[f]}: par[2] raised to 10", 0) + ld.RAISED[f]

    must = ["all stations selected", "one ring suffices", "several 7 500 m rings", "the step drops to 1 000 m", "beyondLastPoint ends the loop short of minPoints",
            "a station on the cell centre", "height not significant: standard deviation below the threshold",
            "height not significant: fewer elevation points than minPointsLocalDetrending", "the fit ends on |diffSSE| <= epsilon", "the fit ends on the iteration cap",
            "a parameter clamped to its range", "a later first guess replaces the best fit", "bestR2 < 0: the fit is repeated from the RMSE index",
            "all station values equal: R2 is x / 0", "piecewiseThreeFree: par[2] raised to 10", "piecewiseThree: par[2] raised to 10"]
    must += [f"function {n}" for n in ld.FUNCTIONS] + [f"method {n}" for n in meteo.METHODS] + ["variable airT", "variable dewT"]
    must += [f"minPointsLocalDetrending {n}" for n in (5, 8, 20)]
    for k in must:
        arms.setdefault(k, 0)
    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k in must if arms[k] == 0]
    assert not empty, f"arms never reached: {empty}"
    save.update(flag=FLAG, arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64), cpu=np.array(json.dumps(cpu)),
                ranges=np.array(json.dumps(checks)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < (1 << 18)
    return 0


if __name__ == "__main__":
    sys.exit(main())
