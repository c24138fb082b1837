#!/usr/bin/env python3
"""Generate tests/golden/localproxies.npz: the compiled-reference pin of air and dew-point temperature with local detrending and every
active proxy - the cell loop of Project::interpolationDemLocalDetrending (agrolib/project/project.cpp:3226-3254) on
Crit3DInterpolationSettings with the height and up to seven other proxies: getProxyValuesXY, localSelection, preInterpolation
(multipleDetrendingMain) and interpolate() for every DEM cell, with the map value, the selected count, the interpolated count,
localRadius, the height's flag / float(R2) / parameters and per proxy slot flag, slope and intercept of every cell.  Run by hand where the
reference tree is present; no test calls it:

    python tests/golden/make_localproxies.py --reference <CRITERIA3D tree>

The driver below is this project's own text.  It is compiled as that of make_localdetrend.py is (the same sources of the reference WHERE
THEY LIE, into a scratch directory), and only data is recorded.  It reads and writes the files of tests/localproxies_host.cpp
(tests/localproxies_cases.py).  The driver itself refuses a cell in the one arm the reference leaves undefined (fitting functions and
fitting parameters of different length).

The two rasters of make_localdetrend.py with seven synthetic proxy rasters each (tests/localproxies_cases.synthetic_rasters: planes,
patchy 0 / fraction maps, bounded indices; flag holes in two of them).  The Python restatement of criteria3d_amd/localproxies.py is held
against the reference bit for bit on every cell of `tiny` before anything is written, and it names and counts the arms there; the arms
that the recorded outcome shows are counted on both rasters.  None of MUST may be empty."""
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
from criteria3d_amd import localdetrend as ld, localproxies as lp, meteo  # noqa: E402
from tests import localproxies_cases as pc  # noqa: E402
from tests.raster_helpers import same  # noqa: E402
import make_localdetrend as base  # noqa: E402

OUT = HERE / "localproxies.npz"
FLAG = base.FLAG
S = pc.SLOTS

DRIVER = r"""
// driver of the local detrending pin with every proxy: see make_localproxies.py
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
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
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
        int iv[8], active[S]; float fv[2], threshold[S]; double range[S][4], table[(3 + MAXG) * MAXP];
        rd(in, iv, 8); rd(in, active, S); rd(in, fv, 2); rd(in, threshold, S); rd(in, &range[0][0], S * 4); rd(in, table, (3 + MAXG) * MAXP);
        const int var = iv[0], method = iv[1], function = iv[2], np = iv[3], nGuess = iv[4], minLocal = iv[5], useDetrending = iv[6], m = iv[7];
        std::vector<double> sx(m), sy(m); std::vector<float> pv((size_t)S * m), sv(m);
        rd(in, sx.data(), m); rd(in, sy.data(), m); rd(in, pv.data(), (size_t)S * m); rd(in, sv.data(), m);

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
        for (int p = 0; p < S; ++p) {
            Crit3DProxy proxy;
            proxy.setName(proxyName[p]);
            if (p == 0) {
                proxy.setGrid(&dem);
                proxy.setFittingFunctionName(refFunction[function]);
                std::vector<double> r(2 * np);
                for (int j = 0; j < np; ++j) { r[j] = table[j]; r[np + j] = table[MAXP + j]; }
                proxy.setFittingParametersRange(r);
                proxy.setStdDevThreshold(fv[0]);
                std::vector<std::vector<double>> combos(nGuess, std::vector<double>(np));
                for (int g = 0; g < nGuess; ++g) for (int j = 0; j < np; ++j) combos[g][j] = table[(3 + g) * MAXP + j];
                proxy.setFirstGuessCombinations(combos);
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
        settings.setCurrentCombination(settings.getSelectedCombination());
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

        std::vector<float> map(n, flag), radius(n, NODATA), r2(n, NODATA);
        std::vector<uint32_t> count(n, 0), interpolated(n, 0);
        std::vector<int32_t> significant(n, 0), psig(n * S, 0);
        std::vector<double> parameters(n * MAXP, NODATA), slope(n * S, NODATA), intercept(n * S, NODATA);
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
                for (int p = 0; p < S; ++p) {
                    const float cell = p == 0 ? z : mapsv[(size_t)p * n + c];
                    const double want = !active[p] || cell == flag ? (double)NODATA : (double)cell;
                    if (proxyValues[p] != want) { fprintf(stderr, "case %d: the proxy %d of cell %ld %ld is not the raster's value\n", k, p, row, col); return 4; }
                }
                std::vector<Crit3DInterpolationDataPoint> subset;
                localSelection(points, subset, x, y, mySettings, false);
                count[c] = (uint32_t)subset.size();
                preInterpolation(subset, mySettings, &meteoSettings, &climateParameters, meteoPoints, refVar[var], myTime, errorStr);
                map[c] = interpolate(subset, mySettings, &meteoSettings, refVar[var], x, y, z, proxyValues, true);
                interpolated[c] = (uint32_t)subset.size();
                radius[c] = mySettings.getLocalRadius();
                Crit3DProxyCombination combination =mySettings.getCurrentCombination();
                significant[c] = active[0] && combination.isProxySignificant(0) ? 1 : 0;
                r2[c] = active[0] ? mySettings.getProxy(0)->getRegressionR2() : (float)NODATA;
                const std::vector<std::vector<double>> fitted = mySettings.getFittingParameters();
                // the arm the reference leaves undefined: functions and parameters of different length
                if (fitted.size() != mySettings.getFittingFunction().size()) { fprintf(stderr, "case %d cell %ld %ld: the undefined arm\n", k, row, col); return 5; }
                size_t at = 0;
                if (significant[c]) {
                    if (fitted.empty() || (int)fitted.front().size() != np) { fprintf(stderr, "case %d: significance without parameters\n", k); return 4; }
                    for (int j = 0; j < np; ++j) parameters[c * MAXP + j] = fitted.front()[j];
                    at = 1;
                }
                for (int p = 1; p < S; ++p) {
                    if (!(active[p] && combination.isProxySignificant(p))) continue;
                    if (at >= fitted.size() || fitted[at].size() != 2) { fprintf(stderr, "case %d: a significant proxy without its line\n", k); return 4; }
                    psig[c * S + p] = 1; slope[c * S + p] = fitted[at][0]; intercept[c * S + p] = fitted[at][1];
                    ++at;
                }
                if (at != fitted.size()) { fprintf(stderr, "case %d cell %ld %ld: %zu parameter vectors, %zu significant proxies\n", k, row, col, fitted.size(), at); return 4; }
                mySettings.clearFitting();
                mySettings.setCurrentCombination(mySettings.getSelectedCombination());
                ++cells;
            }
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d %ld %.6f\n", k, cells, seconds);
        wr(out, map.data(), n); wr(out, count.data(), n); wr(out, interpolated.data(), n); wr(out, radius.data(), n); wr(out, significant.data(), n); wr(out, r2.data(), n);
        wr(out, parameters.data(), n * MAXP); wr(out, psig.data(), n * S); wr(out, slope.data(), n * S); wr(out, intercept.data(), n * S);
    }
    fclose(out);
    return 0;
}
"""

DEFAULT_RANGE = [-1.0, -40.0, 1.0, 50.0]        # interpolationSettings.cpp:251
CAP_SEARCH = 800                                # set-ups tried for a fit that the iteration cap ends


def others(ranges=None, thresholds=None) -> list:
    """the `others` of a case: the default range and no threshold per slot unless given ({slot: ...})"""
    ranges, thresholds = ranges or {}, thresholds or {}
    return lp.make_others([None] + [dict(range=ranges.get(p, DEFAULT_RANGE), stdDevThreshold=thresholds.get(p, ld.NODATA)) for p in range(1, S)])


def station_proxies(rng, x, y, h, xll, yll):
    """the stations' value of every slot: slot 0 the height, a plane of the coordinates, a patchy 0 / fraction, bounded indices ..."""
    n = len(x)
    pv = np.zeros((S, n), np.float32)
    pv[0] = h
    pv[1] = np.round(2.0 + (x - xll) / 1000.0 * 0.9 + (y - yll) / 1000.0 * 0.3, 2)
    pv[2] = np.where(rng.uniform(size=n) < 0.55, np.round(rng.uniform(0.05, 1.0, n), 2), 0.0)
    pv[3] = np.round(rng.uniform(-1.0, 1.0, n), 3)
    pv[4] = np.round(rng.uniform(0.0, 1.0, n), 3)
    pv[5] = np.round(30.0 - (x - xll) / 1000.0 * 0.5 + rng.normal(0.0, 2.0, n), 2)
    pv[6] = np.where(rng.uniform(size=n) < 0.4, np.round(rng.uniform(0.1, 1.0, n), 2), 0.0)
    pv[7] = np.round(rng.uniform(-1.0, 1.0, n), 3)
    return pv


def temperature(rng, pv):
    t = base.temperature(pv[0], rng, 0.4).astype(np.float64)
    t = t + 0.08 * pv[1] - 1.5 * pv[2] + 0.8 * pv[3] - 0.6 * pv[4] + 0.05 * pv[5] + 0.7 * pv[6] - 0.4 * pv[7]
    return np.round(t, 1).astype(np.float32)


def case(label, var, method, fit, x, y, pv, v, active, oth=None, use_detrending=1):
    return dict(label=label, var=meteo.VARIABLES.index(var), method=method, fit=fit, useDetrending=use_detrending, x=np.asarray(x, np.float64), y=np.asarray(y, np.float64),
                proxy_values=np.asarray(pv, np.float32), value=np.asarray(v, np.float32), area=base.bounding_box_area(np.asarray(x), np.asarray(y)),
                active=[int(a) for a in active], others=oth or others())


def act(*slots):
    return [1 if p in slots else 0 for p in range(S)]


def relief_cases(rng, dem, xll, yll, cs):
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 12, 26, 42000.0)
    pv = station_proxies(rng, x, y, h, xll, yll)
    pv[1][3::11] = np.float32(ld.NODATA)
    pv[3][7::13] = np.float32(ld.NODATA)
    t = temperature(rng, pv)
    pr = (float(t.min()), float(t.max()))
    two = lambda n: base.fit_of(ld.PIECEWISE_TWO, base.DEFAULTS[ld.PIECEWISE_TWO], pr, n, keep=6)
    out = []
    out.append(case("none", "airT", meteo.IDW, two(8), x, y, pv, t, act(0)))
    out.append(case("one", "airT", meteo.SHEPARD_MODIFIED, two(8), x, y, pv, t, act(0, 1)))
    out.append(case("two", "dewT", meteo.SHEPARD, two(12), x, y, pv, (t - np.float32(3.5)).astype(np.float32), act(0, 1, 2)))
    out.append(case("four", "airT", meteo.IDW, base.fit_of(ld.PIECEWISE_THREE, base.DEFAULTS[ld.PIECEWISE_THREE], pr, 20, keep=4), x, y, pv, t, act(0, 1, 2, 3, 5)))
    out.append(case("cap", "airT", meteo.SHEPARD_MODIFIED, two(20), x, y, pv, t, act(*range(S))))
    out.append(case("noheight", "dewT", meteo.IDW, two(12), x, y, pv, t, act(2, 5)))
    out.append(case("urban", "airT", meteo.SHEPARD, two(12), x, y, pv, t, act(0, 2), others(ranges={2: [-3.0, -5.0, 0.0, 5.0]})))
    return out


def tiny_cases(rng, dem, xll, yll, cs):
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 6, 8, 16000.0)                       # 14 stations
    pv = station_proxies(rng, x, y, h, xll, yll)
    t = temperature(rng, pv)
    pr = (float(t.min()), float(t.max()))
    fit = lambda n, threshold=ld.NODATA: base.fit_of(ld.PIECEWISE_TWO, base.DEFAULTS[ld.PIECEWISE_TWO], pr, n, threshold=threshold, keep=3)
    out = []
    out.append(case("none", "airT", meteo.IDW, fit(5), x, y, pv, t, act(0)))
    out.append(case("one", "dewT", meteo.SHEPARD, fit(5), x, y, pv, t, act(0, 1)))
    gaps = pv.copy()
    gaps[1][[2, 9]] = np.float32(ld.NODATA)
    out.append(case("two", "airT", meteo.SHEPARD_MODIFIED, fit(8), x, y, gaps, t, act(0, 1, 2)))
    out.append(case("four", "airT", meteo.IDW, fit(8), x, y, gaps, t, act(0, 1, 3, 4, 5)))
    out.append(case("cap", "airT", meteo.IDW, fit(12), x, y, pv, t, act(*range(S))))
    out.append(case("noheight", "airT", meteo.SHEPARD_MODIFIED, fit(8), x, y, pv, t, act(1, 2)))
    # the height fails its validity (a threshold no deviation reaches), the others are fitted on the values as they are
    out.append(case("flatheight", "airT", meteo.IDW, fit(8, threshold=5000.0), x, y, pv, t, act(0, 1, 3)))
    # first pass: slot 3 has fewer than five values, slot 4's deviation is below its threshold, slot 1 carries on
    few = pv.copy()
    few[3][3:] = np.float32(ld.NODATA)
    out.append(case("firstpass", "airT", meteo.IDW, fit(12), x, y, few, t, act(0, 1, 3, 4), others(thresholds={4: 3.0})))
    # every proxy fails: the list untouched
    out.append(case("allfail", "airT", meteo.SHEPARD, fit(8), x, y, pv, t, act(0, 1, 5), others(thresholds={1: 1000.0, 5: 1000.0})))
    # the urban fraction alone: the stations where it is 0 leave the interpolated list, not the fit; its slope is kept in a range the
    # fit wants to leave (clamped), the urban raster has a flag hole where the retrend is then 0
    out.append(case("urban", "airT", meteo.IDW, fit(12), x, y, pv, t, act(0, 2), others(ranges={2: [-0.5, -40.0, 1.0, 50.0]})))
    out.append(case("urbanmax", "airT", meteo.IDW, fit(12), x, y, pv, t, act(0, 2), others(ranges={2: [-8.0, -40.0, -3.0, 50.0]})))
    # every station selected (14 <= unsigned(12 * 1.2f)).  Slot 1 has no value at stations 0, 1, 2: they leave both lists.
    #  - slot 5 holds its two far values there: its deviation passes the first pass only;
    #  - slot 7 is flat but for two stations, the pruned ones lie at its mean: its deviation passes the second pass only, and its one
    #    NODATA, never pruned, enters the fit as -9999 and the station is erased afterwards.
    sec = pv.copy()
    sec[1][[0, 1, 2]] = np.float32(ld.NODATA)
    sec[5] = np.float32(20.0) + np.round(rng.uniform(-0.5, 0.5, len(x)), 2).astype(np.float32)
    sec[5][0], sec[5][1] = np.float32(60.0), np.float32(-20.0)
    sec[7] = np.float32(0.5)
    sec[7][4], sec[7][5] = np.float32(-0.6), np.float32(1.6)
    sec[7][8] = np.float32(ld.NODATA)
    out.append(case("secondpass", "airT", meteo.IDW, fit(11), x, y, sec, t, act(0, 1, 5, 7), others(thresholds={5: 5.0, 7: 0.45})))
    # too few fit points: eleven stations keep a value of slot 1, minPointsLocalDetrending is 12
    out.append(case("fewfit", "dewT", meteo.SHEPARD_MODIFIED, fit(12), x, y, sec, t, act(0, 1)))
    # a fit that the iteration cap ends is rare: the intercepts of several proxies are collinear, and it takes proxies of very different
    # magnitudes with a slope range the fit wants to leave.  A seeded search over set-ups of that kind, every station selected and the
    # height not active, so that one cell decides for all; nothing else is bent
    cx, cy = meteo.cell_centres(dem.shape, xll, yll, cs)
    narrow = others(ranges={p: [0.2, -40.0, 1.0, 50.0] for p in (1, 3, 4, 5)})
    for attempt in range(1, CAP_SEARCH + 1):
        scaled = pv.copy()
        for p, scale in zip((1, 3, 4, 5), rng.permutation([10.0, 10.0, 100.0, 1000.0])):
            scaled[p] = np.round(rng.uniform(0.0, 1.0, len(x)) * scale, 2)
        tt = np.round(rng.normal(10.0, 4.0, len(x)), 1).astype(np.float32)
        c = case("capfit", "airT", meteo.IDW, fit(12), x, y, scaled, tt, act(1, 3, 4, 5), narrow)
        seen = {}
        lp.interpolate_cell(c["method"], cx[0, 0], cy[0, 0], dem[0, 0], lp.cell_proxy_values(dem, [None] * S, FLAG)[0, 0], c["x"], c["y"], c["proxy_values"], c["value"],
                            c["area"], c["fit"], pc.proxies_of(c), c["others"], True, seen)
        if seen.get("the proxies' fit ends on the iteration cap"):
            out.append(c)
            print(f"  the iteration cap: set-up {attempt} of the seeded search")
            break
    else:
        print(f"  the iteration cap: none of {CAP_SEARCH} set-ups reaches it")
    return out


def run_cases(exe, work, r, cases):
    src, dst = work / f"{r['name']}.in", work / f"{r['name']}.out"
    pc.write_input(src, r, cases)
    res = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    timing = [line.split() for line in res.stdout.strip().splitlines()]
    return pc.read_output(dst, r, cases), [(int(c), float(s)) for _, c, s in timing]


MUST = ["0 other proxies active", "1 other proxies active", "2 other proxies active", "4 other proxies active", f"{lp.MAX_OTHERS} other proxies active",
        "the height not active", "the height not significant with others significant", "a proxy fails the first pass for count",
        "a proxy fails the first pass for deviation", "every proxy fails the first pass: the list untouched", "a station pruned for NODATA",
        "a station pruned from interpolation only: all significant values 0", "interpolated count < selected count", "a proxy fails only the second pass",
        "a proxy passes only the second pass", "a station erased by detrendingOtherProxies: NODATA entered the fit as a predictor", "too few fit points",
        "a proxy parameter clamped at its minimum", "a proxy parameter clamped at its maximum", "the proxies' fit ends on the iteration cap",
        "the proxies' fit ends on |diffSSE| <= epsilon", "the cell's proxy NODATA for a significant proxy: retrend 0",
        "the cell's proxy NODATA for a proxy that is not significant"]
MUST += [f"method {n}" for n in meteo.METHODS] + ["variable airT", "variable dewT"]


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
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        exe = work / "localproxies_pin"
        inc = [f"-I{agro / sub}" for sub in ("interpolation", "meteo", "gis", "mathFunctions", "crit3dDate", "utilities")]
        cmd = ["g++", "-w", "-std=c++17", "-O2", "-fopenmp", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               *map(str, srcs), "-o", str(exe), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)

        for name, (dem, xll, yll, cs), maker in (("relief", base.raster_relief(), relief_cases), ("tiny", base.raster_tiny(), tiny_cases)):
            maps = pc.synthetic_rasters(dem.shape, rng)
            holes = ((1, 2), (3, 6), (2, 7)) if name == "tiny" else ((1, 3), (4, 20), (5, 8), (2, 30))
            for rc in holes:
                maps[2][rc] = FLAG                                   # the urban fraction
            maps[5][holes[0]] = FLAG
            r = dict(name=name, dem=dem, maps=maps, xll=xll, yll=yll, cell_size=cs, flag=FLAG)
            cases = maker(rng, dem, xll, yll, cs)
            got, timing = run_cases(exe, work, r, cases)             # the driver exits with 5 on a cell in the undefined arm
            inside = dem != FLAG
            key = lambda s, n=1: arms.__setitem__(s, arms.get(s, 0) + n)
            for k, (c, g) in enumerate(zip(cases, got)):
                what = f"{name} {k} {pc.case_name(c)}"
                assert (g["value"][~inside] == FLAG).all() and (g["count"][inside] > 0).all(), what
                assert not np.isnan(g["value"]).any(), (what, "a map holds NaN: change the tables")
                print(f"  {what}: height significant {int(g['significant'].sum())}/{int(inside.sum())}, proxies significant "
                      f"{g['proxy_significant'].sum(axis=(0, 1)).tolist()}, count {g['count'][inside].min()}..{g['count'].max()}, interpolated "
                      f"{g['interpolated'][inside].min()}..{g['interpolated'].max()}, {timing[k][1]:.3f} s")
                key(f"method {meteo.METHODS[c['method']]}")
                key(f"variable {meteo.VARIABLES[c['var']]}")
                key("interpolated count < selected count", int((g["interpolated"] < g["count"]).sum()))
                if name == "relief":                                 # on `tiny` the restatement counts these per cell
                    key(f"{sum(c['active'][1:])} other proxies active", int(inside.sum()))
                    if not c["active"][0]:
                        key("the height not active", int(inside.sum()))
            if name == "tiny":
                for k, (c, g) in enumerate(zip(cases, got)):
                    t0 = time.time()
                    mine = pc.restated(r, c, arms=arms)
                    same(mine, g, f"restatement {k} {pc.case_name(c)}", pc.QUANTITIES)
                    if c["method"] == meteo.SHEPARD:
                        assert not mine["ties"].any(), "two listed stations at one float distance in a shepardIdw case: move a station"
                    print(f"  restatement {k}: equal ({time.time() - t0:.1f} s)")
            else:
                cx, cy = meteo.cell_centres(dem.shape, xll, yll, cs)
                for k, (c, g) in enumerate(zip(cases, got)):
                    if c["method"] != meteo.SHEPARD:
                        continue
                    for row, col in np.argwhere(inside):
                        sel, d, w, radius = ld.local_selection(cx[row, col], cy[row, col], c["x"], c["y"], c["fit"]["minPointsLocalDetrending"], c["area"])
                        assert len(sel) == g["count"][row, col] and d is not None and len(set(np.array(d).tolist())) == len(d), \
                            "two selected stations at one float distance in a shepardIdw case: move a station"
            save.update({f"{name}_dem": dem, f"{name}_maps": maps, f"{name}_geo": np.array([xll, yll, cs], np.float64),
                         f"{name}_cases": np.array(json.dumps([dict(label=c["label"], var=c["var"], method=c["method"], fit=c["fit"], useDetrending=c["useDetrending"],
                                                                    area=float(c["area"]), active=c["active"], others=c["others"]) for c in cases]))})
            for k, (c, g) in enumerate(zip(cases, got)):
                n_par = len(c["fit"]["min"])
                assert (g["parameters"][..., n_par:] == ld.NODATA).all() and g["count"].max() < 65536
                save.update({f"{name}_c{k}_x": c["x"], f"{name}_c{k}_y": c["y"], f"{name}_c{k}_pv": c["proxy_values"], f"{name}_c{k}_v": c["value"],
                             f"{name}_c{k}_map": g["value"], f"{name}_c{k}_count": g["count"].astype(np.uint16), f"{name}_c{k}_interp": g["interpolated"].astype(np.uint16),
                             f"{name}_c{k}_radius": g["radius"], f"{name}_c{k}_sig": g["significant"].astype(np.uint8), f"{name}_c{k}_r2": g["r2"],
                             f"{name}_c{k}_par": g["parameters"][..., :n_par].copy(), f"{name}_c{k}_psig": g["proxy_significant"].astype(np.uint8),
                             f"{name}_c{k}_slope": g["slope"], f"{name}_c{k}_icpt": g["intercept"]})

    for k in MUST:
        arms.setdefault(k, 0)
    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k in MUST if arms[k] == 0]
    assert not empty, f"arms never reached: {empty}"
    notes.append("no recorded cell is in the arm the reference leaves undefined: the driver compares the lengths of the fitting functions and parameters on every cell")
    save.update(flag=FLAG, arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64), notes=np.array(json.dumps(notes)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < (1 << 18)
    return 0


if __name__ == "__main__":
    sys.exit(main())
