#!/usr/bin/env python3
"""Generate tests/golden/multidetrend.npz: the compiled-reference pin of air and dew-point temperature with multiple detrending and no
sub-option - what Project::interpolationDem (agrolib/project/project.cpp:3113-3150) computes on Crit3DInterpolationSettings with the
height and up to seven other proxies: the map of interpolationRaster, the one fit of preInterpolation (the height's flag / float(R2) /
parameters, per proxy slot flag, slope and intercept, the kept stations and their detrended values) and interpolate() at a list of
points, as computeResiduals and interpolationOutputPoints call it.  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_multidetrend.py --reference <CRITERIA3D tree>

The driver below is this project's own text.  It is compiled as that of make_glocal.py is (the same sources of the reference WHERE THEY
LIE, into a scratch directory), and only data is recorded.  It calls the reference's preInterpolation, getProxyValuesXY and interpolate,
and restates the twenty-line loops of interpolationRaster (agrolib/project/interpolationCmd.cpp:354-395, with the reference's
gis::getUtmXYFromRowColSinglePrecision) and of computeResiduals (agrolib/interpolation/spatialControl.cpp:102-160) around them, because
interpolationCmd.cpp sits in the Qt library.  The height's range and first guesses are the reference's own (from the configured range,
the first-guess positions and the points' range); the driver refuses a case whose table (localdetrend.make_fit) differs from them.  It
reads and writes the files of tests/multidetrend_host.cpp (tests/multidetrend_cases.py), a side file with what the reference builds the
table from, and a side file with what getProxyValuesXY gives at every point, which multidetrend.proxy_values_xy is held to.

The two rasters of make_localdetrend.py with the seven synthetic proxy rasters of localproxies_cases.synthetic_rasters.  The Python
restatement of criteria3d_amd/multidetrend.py is held against the driver bit for bit on `tiny` before anything is written, and it names
and counts the arms there.  None of MUST may be empty, except what UNREACHED explains."""
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
sys.path.insert(0, str(HERE))
from criteria3d_amd import localdetrend as ld, meteo, multidetrend as md  # noqa: E402
from tests import multidetrend_cases as mc, localproxies_cases as pc  # noqa: E402
from tests.raster_helpers import same, write_parts  # noqa: E402
import make_localdetrend as base  # noqa: E402
import make_localproxies as mp  # noqa: E402
import make_glocal as mg  # noqa: E402

OUT = HERE / "multidetrend.npz"
FLAG = base.FLAG
S = pc.SLOTS

DRIVER = r"""
// driver of the multiple detrending pin: see make_multidetrend.py
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
static const char* proxyName[8] = { "elevation", "seaDistance", "urban", "orogIndex", "water", "valley", "green", "aspect" };
enum { MAXP = 6, MAXG = 31, S = 8 };

static void grid(gis::Crit3DRasterGrid& g, int nrows, int ncols, const double* geo, float flag, const float* values)
{
    g.header->nrRows = nrows; g.header->nrCols = ncols; g.header->cellSize = geo[2]; g.header->invCellSize = 1.0 / geo[2];
    g.header->llCorner.x = geo[0]; g.header->llCorner.y = geo[1]; g.header->flag = flag;
    g.initializeGrid(flag);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) g.value[r][c] = values[(size_t)r * ncols + c];
    g.isLoaded = true;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb"); FILE* cfg = fopen(argv[3], "rb"); FILE* xy = fopen(argv[4], "wb");
    if (!in || !out || !cfg || !xy) return 2;
    int dims[3]; float flag; double geo[3];
    rd(in, dims, 3); rd(in, &flag, 1); rd(in, geo, 3);
    const int nrows = dims[0], ncols = dims[1], nCases = dims[2];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> demv(n), mapsv(S * n);
    rd(in, demv.data(), n); rd(in, mapsv.data(), S * n);
    gis::Crit3DRasterGrid dem;
    grid(dem, nrows, ncols, geo, flag, demv.data());
    std::vector<gis::Crit3DRasterGrid> maps(S);
    for (int p = 1; p < S; ++p) grid(maps[p], nrows, ncols, geo, flag, mapsv.data() + (size_t)p * n);

    for (int k = 0; k < nCases; ++k) {
        int iv[8], options[5], active[S]; float fv[2], threshold[S]; double range[S][4], table[(3 + MAXG) * MAXP];
        rd(in, iv, 8); rd(in, options, 5); rd(in, active, S); rd(in, fv, 2); rd(in, threshold, S); rd(in, &range[0][0], S * 4); rd(in, table, (3 + MAXG) * MAXP);
        const int var = iv[0], method = iv[1], function = iv[2], np = iv[3], nGuess = iv[4], useDetrending = iv[6], m = iv[7];
        std::vector<double> sx(m), sy(m); std::vector<float> pv((size_t)S * m), sv(m);
        rd(in, sx.data(), m); rd(in, sy.data(), m); rd(in, pv.data(), (size_t)S * m); rd(in, sv.data(), m);
        int nPoints; rd(in, &nPoints, 1);
        if (nPoints < 0) return 4;
        std::vector<float> px(nPoints), py(nPoints), pz(nPoints), ppv((size_t)S * nPoints);
        rd(in, px.data(), nPoints); rd(in, py.data(), nPoints); rd(in, pz.data(), nPoints); rd(in, ppv.data(), (size_t)S * nPoints);
        int position[MAXP]; double configured[2 * MAXP], pointsRange[2];
        rd(cfg, position, MAXP); rd(cfg, configured, 2 * MAXP); rd(cfg, pointsRange, 2);

        Crit3DInterpolationSettings settings;
        settings.initialize();
        settings.setInterpolationMethod(refMethod[method]);
        settings.setUseThermalInversion(false);
        settings.setUseMultipleDetrending(true);
        settings.setUseLocalDetrending(false);
        settings.setUseGlocalDetrending(false);
        settings.setUseDoNotRetrend(useDetrending == 0);
        settings.setCurrentDEM(&dem);
        settings.setPointsBoundingBoxArea(fv[1]);
        settings.setPointsRange(pointsRange[0], pointsRange[1]);
        for (int p = 0; p < S; ++p) {
            Crit3DProxy proxy;
            proxy.setName(proxyName[p]);
            if (p == 0) {
                proxy.setGrid(&dem);
                proxy.setFittingFunctionName(refFunction[function]);
                proxy.setFittingParametersRange(std::vector<double>(configured, configured + 2 * np));
                proxy.setFittingFirstGuess(std::vector<int>(position, position + np));
                proxy.setStdDevThreshold(fv[0]);
            } else {
                proxy.setGrid(&maps[p]);
                proxy.setFittingFunctionName(linear);
                proxy.setFittingParametersRange({range[p][0], range[p][1], range[p][2], range[p][3]});
                proxy.setStdDevThreshold(threshold[p]);
            }
            settings.addProxy(proxy, active[p] != 0);
        }
        if (getProxyPragaName(proxyName[0]) != proxyHeight) return 4;
        for (int p = 1; p < S; ++p) if (getProxyPragaName(proxyName[p]) == proxyHeight) return 4;
        Crit3DMeteoSettings meteoSettings;
        Crit3DClimateParameters climateParameters;
        std::vector<Crit3DMeteoPoint> meteoPoints;
        Crit3DTime myTime;
        std::string errorStr;

        std::vector<Crit3DInterpolationDataPoint> points(m);
        for (int i = 0; i < m; ++i) {
            points[i].index = i; points[i].isActive = true; points[i].value = sv[i];
            points[i].point->utm.x = sx[i]; points[i].point->utm.y = sy[i]; points[i].point->z = pv[i];
            for (int p = 0; p < S; ++p) points[i].proxyValues.push_back(pv[(size_t)p * m + i]);
        }

        // Project::interpolationDem, project.cpp:3113-3150: the one fit
        settings.setCurrentCombination(settings.getSelectedCombination());
        const auto t0 = std::chrono::steady_clock::now();
        if (!preInterpolation(points, settings, &meteoSettings, &climateParameters, meteoPoints, refVar[var], myTime, errorStr)) return 4;
        if (active[0]) {
            // the table of the case is what the reference fitted with
            const std::vector<double> got = settings.getProxy(0)->getFittingParametersRange();
            const std::vector<std::vector<double>> combos = settings.getProxy(0)->getFirstGuessCombinations();
            if ((int)combos.size() != nGuess || (int)got.size() != 2 * np) { fprintf(stderr, "case %d: %zu first guesses, the table holds %d\n", k, combos.size(), nGuess); return 4; }
            for (int j = 0; j < np; ++j) {
                if (got[j] != table[j] || got[np + j] != table[MAXP + j]) { fprintf(stderr, "case %d: the range differs at %d\n", k, j); return 4; }
                for (int g = 0; g < nGuess; ++g) if (combos[g][j] != table[(3 + g) * MAXP + j]) { fprintf(stderr, "case %d: first guess %d differs at %d\n", k, g, j); return 4; }
            }
        }
        Crit3DProxyCombination combination = settings.getCurrentCombination();
        const std::vector<std::vector<double>> fitted = settings.getFittingParameters();
        if (fitted.size() != settings.getFittingFunction().size()) { fprintf(stderr, "case %d: the undefined arm\n", k); return 5; }
        int32_t significant = active[0] && combination.isProxySignificant(0) ? 1 : 0;
        float r2 = active[0] ? settings.getProxy(0)->getRegressionR2() : (float)NODATA;
        std::vector<int32_t> psig(S, 0), stationKept(m, 0);
        std::vector<double> parameters(MAXP, NODATA), slope(S, NODATA), intercept(S, NODATA);
        std::vector<float> detrended(m, NODATA);
        size_t at = 0;
        if (significant) {
            if (fitted.empty() || (int)fitted.front().size() != np) { fprintf(stderr, "case %d: significance without parameters\n", k); return 4; }
            for (int j = 0; j < np; ++j) parameters[j] = fitted.front()[j];
            at = 1;
        }
        for (int p = 1; p < S; ++p) {
            if (!(active[p] && combination.isProxySignificant(p))) continue;
            if (at >= fitted.size() || fitted[at].size() != 2) { fprintf(stderr, "case %d: a significant proxy without its line\n", k); return 4; }
            psig[p] = 1; slope[p] = fitted[at][0]; intercept[p] = fitted[at][1];
            ++at;
        }
        if (at != fitted.size()) { fprintf(stderr, "case %d: %zu parameter vectors, %zu significant proxies\n", k, fitted.size(), at); return 4; }
        const uint32_t counts[2] = { (uint32_t)m, (uint32_t)points.size() };
        for (size_t i = 0; i < points.size(); ++i) { detrended[points[i].index] = points[i].value; stationKept[points[i].index] = 1; }

        // interpolationRaster, interpolationCmd.cpp:370-392, serially
        gis::Crit3DRasterGrid raster;
        if (!raster.initializeGrid(dem)) return 4;
        std::vector<double> proxyValues(settings.getProxyNr());
        for (long row = 0; row < raster.header->nrRows; row++) {
            for (long col = 0; col < raster.header->nrCols; col++) {
                float z = dem.value[row][col];
                if (!isEqual(z, raster.header->flag)) {
                    float x, y;
                    gis::getUtmXYFromRowColSinglePrecision(*(raster.header), row, col, &x, &y);
                    if (getUseDetrendingVar(refVar[var])) getProxyValuesXY(x, y, settings, proxyValues);
                    raster.value[row][col] = interpolate(points, settings, &meteoSettings, refVar[var], x, y, z, proxyValues, true);
                }
            }
        }
        // computeResiduals, spatialControl.cpp:113-157: interpolate() at every point with the point's own proxy values
        std::vector<float> pout(nPoints, NODATA), xyValues((size_t)S * nPoints, NODATA);
        for (int i = 0; i < nPoints; ++i) {
            std::vector<double> myProxyValues(S);
            for (int p = 0; p < S; ++p) myProxyValues[p] = ppv[(size_t)p * nPoints + i];
            pout[i] = interpolate(points, settings, &meteoSettings, refVar[var], px[i], py[i], pz[i], myProxyValues, false);
            std::vector<double> here(settings.getProxyNr());
            getProxyValuesXY(px[i], py[i], settings, here);
            for (int p = 0; p < S; ++p) xyValues[(size_t)p * nPoints + i] = (float)here[p];
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d %d %.6f\n", k, m, seconds);
        std::vector<float> map(n);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) map[(size_t)r * ncols + c] = raster.value[r][c];
        const int status = 0;
        wr(out, &status, 1);
        wr(out, map.data(), n); wr(out, &significant, 1); wr(out, &r2, 1); wr(out, parameters.data(), MAXP);
        wr(out, psig.data(), S); wr(out, slope.data(), S); wr(out, intercept.data(), S);
        wr(out, counts, 2); wr(out, detrended.data(), m); wr(out, stationKept.data(), m);
        wr(out, &status, 1);
        wr(out, pout.data(), nPoints);
        wr(xy, xyValues.data(), (size_t)S * nPoints);
    }
    fclose(out); fclose(xy);
    return 0;
}
"""

EXTRA = 3                                       # the points `with_points` adds behind the stations


def case(r, label, var, method, fit, x, y, pv, v, active, oth=None, use_detrending=1):
    return mc.with_points(r, mp.case(label, var, method, fit, x, y, pv, v, active, oth, use_detrending))


def tiny_cases(rng, r):
    dem, xll, yll, cs = r["dem"], r["xll"], r["yll"], r["cell_size"]
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 10, 14, 16000.0)                     # 24 stations
    pv = mp.station_proxies(rng, x, y, h, xll, yll)
    t = mp.temperature(rng, pv)
    pr = (float(t.min()), float(t.max()))
    two = lambda threshold=ld.NODATA: mg.glocal_fit(ld.PIECEWISE_TWO, pr, threshold)
    add = lambda *a, **k: out.append(case(r, *a, **k))
    out = []
    add("height", "airT", meteo.IDW, two(), x, y, pv, t, mp.act(0))
    add("one", "dewT", meteo.SHEPARD, two(), x, y, pv, (t - np.float32(3.5)).astype(np.float32), mp.act(0, 1))
    add("three-others", "airT", meteo.SHEPARD_MODIFIED, two(), x, y, pv, t, mp.act(0, 1, 3, 5))
    # the urban fraction (flag holes in its raster): the stations where it is 0 are erased for all-zero proxies; the cells of the holes
    # lack a significant proxy; the holes of slot 5, which is not active here, do not matter
    add("urban", "airT", meteo.IDW, two(), x, y, pv, t, mp.act(0, 2))
    # slot 5 active and flat at the stations (not significant): the cell of its raster's hole lacks only it, and is retrended
    flat5 = pv.copy()
    flat5[5] = np.float32(20.0)
    flat5[5][:3] = np.float32(20.01)
    add("flat-valley", "airT", meteo.SHEPARD, two(), x, y, flat5, t, mp.act(0, 1, 5), mp.others(thresholds={5: 1.0}))
    gaps = pv.copy()
    gaps[1][[2, 9, 15]] = np.float32(ld.NODATA)
    gaps[3][[4, 11]] = np.float32(ld.NODATA)
    add("gaps", "airT", meteo.IDW, two(), x, y, gaps, t, mp.act(0, 1, 2, 3))
    add("noheight", "airT", meteo.IDW, two(), x, y, gaps, t, mp.act(1, 2))
    add("flatheight", "dewT", meteo.IDW, two(5000.0), x, y, pv, t, mp.act(0, 1, 3))
    few = pv.copy()
    few[0][4:] = np.float32(ld.NODATA)
    add("fewheights", "airT", meteo.IDW, two(), x, y, few, t, mp.act(0, 1))
    missing = pv.copy()
    missing[0][[1, 7, 20]] = np.float32(ld.NODATA)
    add("noheightvalue", "airT", meteo.SHEPARD, two(), x, y, missing, t, mp.act(0))
    add("three", "airT", meteo.IDW, mg.glocal_fit(ld.PIECEWISE_THREE, pr), x, y, pv, t, mp.act(0, 1))
    add("free", "airT", meteo.SHEPARD, mg.glocal_fit(ld.PIECEWISE_THREE_FREE, pr), x, y, pv, t, mp.act(0))
    add("allfail", "airT", meteo.SHEPARD, two(), x, y, pv, t, mp.act(0, 1, 5), mp.others(thresholds={1: 1000.0, 5: 1000.0}))
    # slot 1 has no value at stations 0, 1, 2: the prunings erase them.  Slot 5 holds its two far values there: its deviation passes the
    # first pass only.  Slot 7 is flat but for two stations, the pruned ones lie at its mean: its deviation passes the second pass only,
    # and its one NODATA, never pruned, enters the fit as -9999: detrendingOtherProxies erases that station
    sec = pv.copy()
    sec[1][[0, 1, 2]] = np.float32(ld.NODATA)
    sec[5] = np.float32(20.0) + np.round(rng.uniform(-0.5, 0.5, len(x)), 2).astype(np.float32)
    sec[5][0], sec[5][1] = np.float32(60.0), np.float32(-20.0)
    sec[7] = np.float32(0.5)
    sec[7][4], sec[7][5] = np.float32(-0.6), np.float32(1.6)
    sec[7][8] = np.float32(ld.NODATA)
    add("secondpass", "airT", meteo.IDW, two(), x, y, sec, t, mp.act(0, 1, 5, 7), mp.others(thresholds={5: 5.0, 7: 0.335}))
    # slot 4 is 0 at every station: it passes the first pass (no threshold), every station is erased for all-zero proxies, and
    # interpolate() has no point left: -9999 in every cell and at every point, and the call succeeds
    zero = pv.copy()
    zero[4] = np.float32(0.0)
    add("allzero", "airT", meteo.IDW, two(), x, y, zero, t, mp.act(0, 4))
    add("noretrend", "airT", meteo.IDW, two(), x, y, pv, t, mp.act(0, 1), use_detrending=0)
    return out


def relief_cases(rng, r):
    dem, xll, yll, cs = r["dem"], r["xll"], r["yll"], r["cell_size"]
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 12, 40, 42000.0)                     # 52 stations
    pv = mp.station_proxies(rng, x, y, h, xll, yll)
    pv[1][3::11] = np.float32(ld.NODATA)
    pv[3][7::13] = np.float32(ld.NODATA)
    t = mp.temperature(rng, pv)
    pr = (float(t.min()), float(t.max()))
    add = lambda *a, **k: out.append(case(r, *a, **k))
    out = []
    add("height", "airT", meteo.IDW, mg.glocal_fit(ld.PIECEWISE_TWO, pr), x, y, pv, t, mp.act(0))
    add("two", "dewT", meteo.SHEPARD, mg.glocal_fit(ld.PIECEWISE_TWO, pr), x, y, pv, (t - np.float32(3.5)).astype(np.float32), mp.act(0, 1, 2))
    add("four", "airT", meteo.SHEPARD_MODIFIED, mg.glocal_fit(ld.PIECEWISE_THREE, pr), x, y, pv, t, mp.act(0, 1, 2, 3, 5))
    add("all", "airT", meteo.IDW, mg.glocal_fit(ld.PIECEWISE_THREE_FREE, pr), x, y, pv, t, mp.act(*range(S)))
    add("noheight", "dewT", meteo.IDW, mg.glocal_fit(ld.PIECEWISE_TWO, pr), x, y, pv, t, mp.act(2, 5))
    return out


def run_cases(exe, work, r, cases):
    src, dst, cfg, xy = (work / f"{r['name']}.{e}" for e in ("in", "out", "cfg", "xy"))
    mc.write_input(src, r, cases)
    parts = []
    for c in cases:
        f = c["fit"]
        n = len(f["min"])
        parts += [np.array(f["position"] + [0] * (ld.MAX_PARAMETERS - n), np.int32), np.array(f["configured"] + [0.0] * (2 * ld.MAX_PARAMETERS - 2 * n), np.float64),
                  np.array(f["points_range"], np.float64)]
    write_parts(cfg, parts)
    res = subprocess.run([str(exe), str(src), str(dst), str(cfg), str(xy)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    timing = [line.split() for line in res.stdout.strip().splitlines()]
    raw, at, here = np.fromfile(xy, np.float32), 0, []
    for c in cases:
        k = S * len(c["points"]["x"])
        here.append(raw[at:at + k].reshape(S, -1))
        at += k
    assert at == len(raw)
    return mc.read_output(dst, r, cases), [float(s) for _, _, s in timing], here


MUST = ["the height not active", "the height not significant: fewer than five heights", "the height not significant: the standard deviation",
        "the height significant alone", "the height significant with 1 other proxies", "the height significant with 3 other proxies",
        "the height withdrawn by isVectorNodataOrZero", "no other proxy active", "every proxy fails the first pass: the list untouched",
        "a proxy fails only the second pass", "a proxy passes only the second pass",
        "a station erased by detrendingOtherProxies: NODATA entered the fit as a predictor", "a station pruned for NODATA",
        "a station pruned from interpolation only: all significant values 0", "an erased station absent from the map's neighbours",
        "a station with a NODATA height while the height is significant", "a place lacking a significant proxy: value kept, retrend 0",
        "a cell lacking only a non-significant active proxy", "a cell whose interpolate() gives NODATA", "useDetrending 0",
        "a point: a station at its own coordinates", "a point: an erased station still evaluated", "a point on a cell centre", "a point outside the raster",
        "a point with a NODATA value of a significant proxy"]
MUST += [f"method {n}" for n in meteo.METHODS] + ["variable airT", "variable dewT"] + [f"function {n}" for n in ld.FUNCTIONS]
# arms the reference does not reach: why, from its text, for the notes of the pin
UNREACHED = {
    "the height withdrawn by isVectorNodataOrZero":
        "multipleDetrendingElevationFitting (interpolation.cpp:1939) withdraws a valid height only where isEqual(R2, NODATA), and "
        "bestFittingMarquardt_nDimension (furtherMathFunctions.cpp:1360-1427) returns NODATA only with no first guess - the entry point refuses a table "
        "without one - or a weighted R2 = 1 - residuals / total within 1e-5 of -9999, which no station list built here gives",
}


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
    rng = np.random.default_rng(20261021)
    save, arms, notes = {}, {}, []
    key = lambda s, n=1: arms.__setitem__(s, arms.get(s, 0) + n)
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        exe = work / "multidetrend_pin"
        inc = [f"-I{agro / sub}" for sub in ("interpolation", "meteo", "gis", "mathFunctions", "crit3dDate", "utilities")]
        cmd = ["g++", "-w", "-std=c++17", "-O2", "-fopenmp", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               *map(str, srcs), "-o", str(exe), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)

        for name, maker in (("relief", relief_cases), ("tiny", tiny_cases)):
            r = mg.make_raster(name, rng)
            cases = maker(rng, r)
            got, timing, here = run_cases(exe, work, r, cases)
            inside = r["dem"] != FLAG
            for k, (c, g) in enumerate(zip(cases, got)):
                what = f"{name} {k} {mc.case_name(c)}"
                assert g["status"] == 0 and g["points_status"] == 0, (what, g["status"], g["points_status"])
                assert (g["value"][~inside] == FLAG).all() and not np.isnan(g["value"]).any(), (what, "a map holds NaN or a value outside the DEM")
                nodata_cells = int(((g["value"] == FLAG) & inside).sum())
                print(f"  {what}: height significant {int(g['significant'])}, r2 {float(g['r2']):.3f}, proxies {g['proxy_significant'].astype(int).tolist()}, "
                      f"fitted {g['fitted']}, kept {g['kept']}, NODATA cells {nodata_cells}, NODATA points {int((g['points'] == FLAG).sum())}, {timing[k]:.4f} s")
                key(f"method {meteo.METHODS[c['method']]}")
                key(f"variable {meteo.VARIABLES[c['var']]}")
                key(f"function {ld.FUNCTIONS[c['fit']['function']]}")
                key("a cell whose interpolate() gives NODATA", nodata_cells)
                # getProxyValuesXY of the reference at every point against multidetrend.proxy_values_xy
                q = c["points"]
                mine = md.proxy_values_xy(r["dem"], r["xll"], r["yll"], r["cell_size"], mc.maps_of(r), mc.proxies_of(c), q["x"], q["y"], float(FLAG))
                assert np.array_equal(mine.view(np.uint32), here[k].view(np.uint32)), (what, "proxy_values_xy differs from getProxyValuesXY")
                m = len(c["x"])
                sig = [p for p in range(S) if (p == 0 and g["significant"]) or g["proxy_significant"][p]]
                key("a point: a station at its own coordinates", m)
                key("a point: an erased station still evaluated", int(((g["points"][:m] != FLAG) & ~g["station_kept"]).sum()))
                key("a point on a cell centre", int(g["points"][m] != FLAG))
                key("a point outside the raster", int(g["points"][m + 1] != FLAG and (here[k][:, m + 1] == FLAG).all()))
                key("a point with a NODATA value of a significant proxy", int(bool(sig) and g["points"][m + 2] != FLAG))
                # an erased station is absent from the map's neighbours: moving its value leaves the map alone (checked by the restatement
                # on tiny: it interpolates over the kept list only); here: the count
                key("an erased station absent from the map's neighbours", int(g["fitted"] - g["kept"]) if g["kept"] else 0)
            if name == "tiny":
                for k, (c, g) in enumerate(zip(cases, got)):
                    t0 = time.time()
                    mine = mc.restated(r, c, arms=arms)
                    same(mine, g, f"restatement {k} {mc.case_name(c)}", mc.QUANTITIES)
                    print(f"  restatement {k}: equal ({time.time() - t0:.1f} s)")
            save.update({f"{name}_dem": r["dem"], f"{name}_maps": r["maps"], f"{name}_geo": np.array([r["xll"], r["yll"], r["cell_size"]], np.float64),
                         f"{name}_cases": np.array(json.dumps([dict(label=c["label"], var=c["var"], method=c["method"], fit=c["fit"], useDetrending=c["useDetrending"],
                                                                    area=float(c["area"]), active=c["active"], others=c["others"]) for c in cases]))})
            for k, (c, g) in enumerate(zip(cases, got)):
                n_par = len(c["fit"]["min"])
                assert (g["parameters"][n_par:] == ld.NODATA).all()
                q = c["points"]
                save.update({f"{name}_c{k}_x": c["x"], f"{name}_c{k}_y": c["y"], f"{name}_c{k}_pv": c["proxy_values"], f"{name}_c{k}_v": c["value"],
                             f"{name}_c{k}_map": g["value"], f"{name}_c{k}_sig": np.uint8(g["significant"]), f"{name}_c{k}_r2": np.float32(g["r2"]),
                             f"{name}_c{k}_par": g["parameters"][:n_par].copy(), f"{name}_c{k}_psig": g["proxy_significant"].astype(np.uint8),
                             f"{name}_c{k}_slope": g["slope"], f"{name}_c{k}_icpt": g["intercept"], f"{name}_c{k}_fitted": np.uint16(g["fitted"]),
                             f"{name}_c{k}_kept": np.uint16(g["kept"]), f"{name}_c{k}_det": g["detrended"], f"{name}_c{k}_skept": g["station_kept"].astype(np.uint8),
                             f"{name}_c{k}_px": q["x"][-EXTRA:], f"{name}_c{k}_py": q["y"][-EXTRA:], f"{name}_c{k}_pz": q["z"][-EXTRA:],
                             f"{name}_c{k}_ppv": q["values"][:, -EXTRA:], f"{name}_c{k}_pout": g["points"]})
            notes.append(f"{name}: the reference took {sum(timing):.4f} s for {len(cases)} cases (fit, map and points) in the driver")

    for k in MUST:
        arms.setdefault(k, 0)
    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k in MUST if arms[k] == 0 and k not in UNREACHED]
    assert not empty, f"arms never reached: {empty}"
    for k, why in UNREACHED.items():
        if arms[k] == 0:
            notes.append(f"arm not reached with the reference: {k}: {why}")
    notes.append("the points of a case are its stations at their own float coordinates with their own proxy values, then the three recorded points")
    save.update(flag=FLAG, arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64), notes=np.array(json.dumps(notes)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < (1 << 18)
    return 0


if __name__ == "__main__":
    sys.exit(main())
