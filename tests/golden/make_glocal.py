#!/usr/bin/env python3
"""Generate tests/golden/glocal.npz: the compiled-reference pin of air and dew-point temperature with glocal detrending - what
Project::interpolationDemGlocalDetrending (agrolib/project/project.cpp:3267-3384) computes on Crit3DInterpolationSettings with macro areas,
the height and up to seven other proxies: the map, and per macro area the height's flag / float(R2) / parameters, per proxy slot flag,
slope and intercept, the fitted and kept counts and the rebuilt subset's detrended values.  Run by hand where the reference tree is
present; no test calls it:

    python tests/golden/make_glocal.py --reference <CRITERIA3D tree>

The driver below is this project's own text.  It is compiled as that of make_localproxies.py is (the same sources of the reference WHERE
THEY LIE, into a scratch directory), and only data is recorded.  It restates the area and cell loops of project.cpp:3321-3380 SERIALLY,
the areas in index order - the reference's loop is an OpenMP loop whose order is not defined - and calls the reference's preInterpolation
(glocalDetrendingFitting), setMultipleDetrendingHeightTemperatureRange, macroAreaDetrending, getSignificantProxyValuesXY and interpolate.
The height's range and first guesses are the reference's own (from the configured range, the first-guess positions and the points'
range); the driver refuses a case whose table (localdetrend.make_fit) differs from them.  float(R2) of an area is not kept by the
reference beyond the next area's fit: the driver reads it from multipleDetrendingElevationFitting(.., false) on a copy of the settings.
It reads and writes the files of tests/glocal_host.cpp (tests/glocal_cases.py) and a side file with what the reference builds the table from.

The two rasters of make_localdetrend.py with the seven synthetic proxy rasters of localproxies_cases.synthetic_rasters and 3 to 5 macro
areas whose weight maps overlap.  The Python restatement of criteria3d_amd/glocal.py is held against the driver bit for bit on `tiny`
before anything is written, and it names and counts the arms there.  None of MUST may be empty, except what UNREACHED explains."""
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
from criteria3d_amd import glocal as gl, localdetrend as ld, meteo  # noqa: E402
from tests import glocal_cases as gc, localproxies_cases as pc  # noqa: E402
from tests.raster_helpers import same, write_parts  # noqa: E402
import make_localdetrend as base  # noqa: E402
import make_localproxies as mp  # noqa: E402

OUT = HERE / "glocal.npz"
FLAG = base.FLAG
S = pc.SLOTS

DRIVER = r"""
// driver of the glocal detrending pin: see make_glocal.py
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
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb"); FILE* cfg = fopen(argv[3], "rb");
    if (!in || !out || !cfg) return 2;
    int dims[3]; float flag; double geo[3];
    rd(in, dims, 3); rd(in, &flag, 1); rd(in, geo, 3);
    const int nrows = dims[0], ncols = dims[1], nCases = dims[2];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> demv(n), mapsv(S * n);
    rd(in, demv.data(), n); rd(in, mapsv.data(), S * n);
    int adims[3]; rd(in, adims, 3);
    const int nAreas = adims[0], nAreaCells = adims[1], nList = adims[2];
    std::vector<uint32_t> cellOffset(nAreas + 1), stationOffset(nAreas + 1);
    std::vector<float> cell(nAreaCells), weight(nAreaCells);
    std::vector<int32_t> stationIndex(nList);
    rd(in, cellOffset.data(), nAreas + 1); rd(in, cell.data(), nAreaCells); rd(in, weight.data(), nAreaCells);
    rd(in, stationOffset.data(), nAreas + 1); rd(in, stationIndex.data(), nList);
    gis::Crit3DRasterGrid dem;
    grid(dem, nrows, ncols, geo, flag, demv.data());
    std::vector<gis::Crit3DRasterGrid> maps(S);
    for (int p = 1; p < S; ++p) grid(maps[p], nrows, ncols, geo, flag, mapsv.data() + (size_t)p * n);
    const int areasOk = 1;
    wr(out, &areasOk, 1);

    for (int k = 0; k < nCases; ++k) {
        int iv[8], options[3], active[S]; float fv[2], threshold[S]; double range[S][4], table[(3 + MAXG) * MAXP];
        rd(in, iv, 8); rd(in, options, 3); rd(in, active, S); rd(in, fv, 2); rd(in, threshold, S); rd(in, &range[0][0], S * 4); rd(in, table, (3 + MAXG) * MAXP);
        const int var = iv[0], method = iv[1], function = iv[2], np = iv[3], nGuess = iv[4], useDetrending = iv[6], m = iv[7];
        std::vector<int32_t> pointIndex(m);
        std::vector<double> sx(m), sy(m); std::vector<float> pv((size_t)S * m), sv(m);
        rd(in, pointIndex.data(), m); rd(in, sx.data(), m); rd(in, sy.data(), m); rd(in, pv.data(), (size_t)S * m); rd(in, sv.data(), m);
        int position[MAXP]; double configured[2 * MAXP], pointsRange[2];
        rd(cfg, position, MAXP); rd(cfg, configured, 2 * MAXP); rd(cfg, pointsRange, 2);

        Crit3DInterpolationSettings settings;
        settings.initialize();
        settings.setInterpolationMethod(refMethod[method]);
        settings.setUseThermalInversion(false);
        settings.setUseMultipleDetrending(true);
        settings.setUseLocalDetrending(false);
        settings.setUseGlocalDetrending(true);
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
        std::vector<Crit3DMacroArea> areas(nAreas);
        for (int a = 0; a < nAreas; ++a) {
            areas[a].setMeteoPoints(std::vector<int>(stationIndex.begin() + stationOffset[a], stationIndex.begin() + stationOffset[a + 1]));
            std::vector<float> cells;
            for (uint32_t c = cellOffset[a]; c < cellOffset[a + 1]; ++c) { cells.push_back(cell[c]); cells.push_back(weight[c]); }
            areas[a].setAreaCellsDEM(cells);
        }
        settings.setMacroAreas(areas);
        Crit3DMeteoSettings meteoSettings;
        Crit3DClimateParameters climateParameters;
        std::vector<Crit3DMeteoPoint> meteoPoints;
        Crit3DTime myTime;
        std::string errorStr;

        std::vector<Crit3DInterpolationDataPoint> points(m);
        for (int i = 0; i < m; ++i) {
            points[i].index = pointIndex[i]; points[i].isActive = true; points[i].value = sv[i];
            points[i].point->utm.x = sx[i]; points[i].point->utm.y = sy[i]; points[i].point->z = pv[i];
            for (int p = 0; p < S; ++p) points[i].proxyValues.push_back(pv[(size_t)p * m + i]);
        }

        // interpolationDemGlocalDetrending, project.cpp:3285-3319
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
        gis::Crit3DRasterGrid raster;
        raster.initializeGrid(*dem.header);
        if (!setMultipleDetrendingHeightTemperatureRange(settings)) return 4;
        int elevationPos = NODATA;
        for (unsigned int pos = 0; pos < settings.getCurrentCombination().getProxySize(); pos++)
            if (getProxyPragaName(settings.getProxy(pos)->getName()) == proxyHeight) elevationPos = pos;

        std::vector<int32_t> significant(nAreas, 0), psig((size_t)nAreas * S, 0), stationKept(nList, 0);
        std::vector<float> r2(nAreas, NODATA), detrended(nList, NODATA);
        std::vector<uint32_t> fitted(nAreas, 0), kept(nAreas, 0);
        std::vector<double> parameters((size_t)nAreas * MAXP, NODATA), slope((size_t)nAreas * S, NODATA), intercept((size_t)nAreas * S, NODATA);

        // the area and cell loops of project.cpp:3321-3380, serially
        Crit3DInterpolationSettings mySettings = settings;
        std::vector<double> proxyValues(mySettings.getProxyNr());
        bool isOk = true;
        for (int areaIndex = 0; areaIndex < mySettings.getMacroAreasSize(); areaIndex++) {
            Crit3DMacroArea macroArea = mySettings.getMacroArea(areaIndex);
            std::vector<float> areaCells = macroArea.getAreaCellsDEM();
            std::vector<Crit3DInterpolationDataPoint> subset;
            const std::vector<int> listed = macroArea.getMeteoPoints();
            if (listed.empty()) { if (!areaCells.empty()) return 4; continue; }

            // what the area holds: recorded also where it has no cells (the reference's loop skips it there)
            {
                Crit3DInterpolationSettings scratch = settings;
                std::vector<Crit3DInterpolationDataPoint> fitSubset;
                for (size_t l = 0; l < listed.size(); ++l)
                    for (int i = 0; i < m; ++i) if (points[i].index == listed[l]) { fitSubset.push_back(points[i]); break; }
                fitted[areaIndex] = (uint32_t)fitSubset.size();
                if (active[0]) {
                    scratch.setCurrentCombination(scratch.getSelectedCombination());
                    scratch.clearFitting();
                    if (!multipleDetrendingElevationFitting(0, fitSubset, scratch, refVar[var], errorStr, false)) return 4;
                    r2[areaIndex] = scratch.getProxy(0)->getRegressionR2();
                }
            }
            macroAreaDetrending(macroArea, refVar[var], mySettings, &meteoSettings, meteoPoints, points, subset, elevationPos);
            Crit3DProxyCombination combination = macroArea.getCombination();
            const std::vector<std::vector<double>> fittedParameters = macroArea.getParameters();
            size_t at = 0;
            significant[areaIndex] = active[0] && combination.isProxySignificant(0) ? 1 : 0;
            if (significant[areaIndex]) {
                if (fittedParameters.empty() || (int)fittedParameters.front().size() != np) { fprintf(stderr, "case %d: significance without parameters\n", k); return 4; }
                for (int j = 0; j < np; ++j) parameters[(size_t)areaIndex * MAXP + j] = fittedParameters.front()[j];
                at = 1;
            }
            for (int p = 1; p < S; ++p) {
                if (!(active[p] && combination.isProxySignificant(p))) continue;
                if (at >= fittedParameters.size() || fittedParameters[at].size() != 2) { fprintf(stderr, "case %d: a significant proxy without its line\n", k); return 4; }
                psig[(size_t)areaIndex * S + p] = 1; slope[(size_t)areaIndex * S + p] = fittedParameters[at][0]; intercept[(size_t)areaIndex * S + p] = fittedParameters[at][1];
                ++at;
            }
            if (at != fittedParameters.size()) { fprintf(stderr, "case %d area %d: %zu parameter vectors, %zu significant proxies\n", k, areaIndex, fittedParameters.size(), at); return 5; }
            kept[areaIndex] = (uint32_t)subset.size();
            for (size_t i = 0; i < subset.size(); ++i)
                for (size_t l = 0; l < listed.size(); ++l)
                    if (listed[l] == subset[i].index) { detrended[stationOffset[areaIndex] + l] = subset[i].value; stationKept[stationOffset[areaIndex] + l] = 1; }

            if (areaCells.empty()) continue;
            for (std::size_t cellIndex = 0; cellIndex < areaCells.size(); cellIndex = cellIndex + 2) {
                int row = int(areaCells[cellIndex] / dem.header->nrCols);
                int col = int(areaCells[cellIndex]) % dem.header->nrCols;
                float z = dem.value[row][col];
                if (isEqual(z, dem.header->flag)) continue;
                double x, y;
                gis::getUtmXYFromRowCol(*dem.header, row, col, &x, &y);
                if (!getSignificantProxyValuesXY(x, y, mySettings, proxyValues)) { raster.value[row][col] = NODATA; continue; }
                double interpolatedValue = interpolate(subset, mySettings, &meteoSettings, refVar[var], x, y, z, proxyValues, true);
                if (isEqual(interpolatedValue, NODATA)) isOk = false;
                if (isEqual(raster.value[row][col], NODATA)) raster.value[row][col] = interpolatedValue * areaCells[cellIndex + 1];
                else raster.value[row][col] += interpolatedValue * areaCells[cellIndex + 1];
            }
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d %d %.6f\n", k, nAreas, seconds);
        std::vector<float> map(n);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) map[(size_t)r * ncols + c] = raster.value[r][c];
        const int status = isOk ? 0 : 1;
        wr(out, &status, 1);
        wr(out, map.data(), n); wr(out, significant.data(), nAreas); wr(out, r2.data(), nAreas); wr(out, parameters.data(), (size_t)nAreas * MAXP);
        wr(out, psig.data(), (size_t)nAreas * S); wr(out, slope.data(), (size_t)nAreas * S); wr(out, intercept.data(), (size_t)nAreas * S);
        wr(out, fitted.data(), nAreas); wr(out, kept.data(), nAreas); wr(out, detrended.data(), nList); wr(out, stationKept.data(), nList);
    }
    fclose(out);
    return 0;
}
"""


def glocal_fit(function, points_range, threshold=ld.NODATA, rng_pos=None):
    """the fit of a case as the reference builds it: every first-guess combination; with the configuration the driver hands the reference"""
    configured, position = rng_pos or base.DEFAULTS[function]
    fit = ld.make_fit(function, configured, position, points_range, 0, threshold)
    fit["configured"], fit["position"], fit["points_range"] = [float(v) for v in configured], [int(v) for v in position], [float(v) for v in points_range]
    return fit


def case(label, var, method, fit, index, x, y, pv, v, active, oth=None, use_detrending=1):
    c = mp.case(label, var, method, fit, x, y, pv, v, active, oth, use_detrending)
    c["point_index"] = np.asarray(index, np.int32)
    return c


def weight_maps(shape, layout) -> list:
    """per area None or a weight map on the DEM: layout[a] = (first column, last column + 1, peak weight) - a band whose weight falls off
    from its middle; bands overlap, the weights do not add up to 1, and the columns no band reaches are covered by none"""
    rows, cols = shape
    out = []
    for band in layout:
        if band is None:
            out.append(None)
            continue
        lo, hi, peak = band
        w = np.zeros(shape, np.float32)
        for c in range(lo, hi):
            w[:, c] = np.float32(round(peak * (0.35 + 0.65 * (1.0 - abs((c - (lo + hi - 1) / 2.0) / max(1.0, (hi - lo) / 2.0)))), 3))
        w[0, lo] = FLAG                                                      # a NODATA of the map: skipped
        out.append(w)
    return out


def header(dem, xll, yll, cs) -> dict:
    return dict(nrows=dem.shape[0], ncols=dem.shape[1], xllcorner=xll, yllcorner=yll, cellsize=cs, nodata_value=float(FLAG))


def make_raster(name, rng):
    dem, xll, yll, cs = base.raster_tiny() if name == "tiny" else base.raster_relief()
    maps = pc.synthetic_rasters(dem.shape, rng)
    holes = ((1, 2), (3, 6), (2, 7)) if name == "tiny" else ((1, 3), (4, 20), (5, 8), (2, 30))
    for rc in holes:
        maps[2][rc] = FLAG
    maps[5][holes[0]] = FLAG
    return dict(name=name, dem=dem, maps=maps, xll=xll, yll=yll, cell_size=cs, flag=FLAG)


def tiny_world(rng):
    r = make_raster("tiny", rng)
    dem, xll, yll, cs = r["dem"], r["xll"], r["yll"], r["cell_size"]
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 10, 14, 16000.0)                     # 24 stations
    pv = mp.station_proxies(rng, x, y, h, xll, yll)
    t = mp.temperature(rng, pv)
    n = len(x)
    index = (np.arange(n) * 2 + 5).astype(np.int32)
    ids = [f"st{i}" for i in range(int(index.max()) + 1)]
    order = np.argsort(x)
    west, mid, east = order[:11], order[6:18], order[13:]
    lists = [west, mid, east, order[::2][:6]]                                                 # the fourth area has no weight map
    # columns 0-4, 2-7, 4-7: cells under one, two and (column 4) three areas; column 8 under none
    layout = [(0, 5, 0.9), (2, 8, 0.7), (4, 8, 0.5), None]
    r["areas"] = gl.areas_from_maps(header(dem, xll, yll, cs), weight_maps(dem.shape, layout), [[ids[index[i]] for i in l] for l in lists], ids)
    return r, x, y, pv, t, index


def tiny_cases(rng, r, x, y, pv, t, index):
    pr = (float(t.min()), float(t.max()))
    two = lambda threshold=ld.NODATA: glocal_fit(ld.PIECEWISE_TWO, pr, threshold)
    out = []
    out.append(case("height", "airT", meteo.IDW, two(), index, x, y, pv, t, mp.act(0)))
    out.append(case("one", "dewT", meteo.SHEPARD, two(), index, x, y, pv, (t - np.float32(3.5)).astype(np.float32), mp.act(0, 1)))
    # slot 2 (urban, flag holes in its raster) is flat at the western stations: significant in the other areas only, so the cells of its
    # holes are set to NODATA by one area and not by another
    flat = pv.copy()
    west = np.argsort(x)[:11]
    flat[2][west] = np.float32(0.3)
    flat[2][west[:2]] = np.float32(0.31)
    out.append(case("urban", "airT", meteo.SHEPARD_MODIFIED, two(), index, x, y, flat, t, mp.act(0, 2), mp.others(thresholds={2: 0.05})))
    # the same at the eastern stations: the area that sets the holes of columns 6 and 7 to NODATA comes first, the next one fills them again
    east = np.argsort(x)[13:]
    flat_east = pv.copy()
    flat_east[2][east] = np.float32(0.3)
    flat_east[2][east[:2]] = np.float32(0.31)
    out.append(case("urban-east", "airT", meteo.IDW, two(), index, x, y, flat_east, t, mp.act(0, 2), mp.others(thresholds={2: 0.05})))
    gaps = flat.copy()
    gaps[1][[2, 9, 15]] = np.float32(ld.NODATA)
    gaps[3][[4, 11]] = np.float32(ld.NODATA)
    out.append(case("gaps", "airT", meteo.IDW, two(), index, x, y, gaps, t, mp.act(0, 1, 2, 3), mp.others(thresholds={2: 0.05})))
    out.append(case("noheight", "airT", meteo.IDW, two(), index, x, y, gaps, t, mp.act(1, 2), mp.others(thresholds={2: 0.05})))
    out.append(case("flatheight", "dewT", meteo.IDW, two(5000.0), index, x, y, pv, t, mp.act(0, 1, 3)))
    out.append(case("three", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_THREE, pr), index, x, y, pv, t, mp.act(0, 1)))
    out.append(case("free", "airT", meteo.SHEPARD, glocal_fit(ld.PIECEWISE_THREE_FREE, pr), index, x, y, pv, t, mp.act(0)))
    # temperatures that rise with the height against the slopes the range allows: a fit worse than the mean
    up = np.round(2.0 + 0.012 * pv[0] + rng.normal(0.0, 0.5, len(x)), 1).astype(np.float32)
    out.append(case("rising", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_TWO, (float(up.min()), float(up.max()))), index, x, y, pv, up, mp.act(0)))
    # temperatures that do not depend on the height: the slopes the range forces make every fit worse than the mean
    level = np.round(10.0 + rng.normal(0.0, 0.2, len(x)), 1).astype(np.float32)
    out.append(case("level", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_TWO, (float(level.min()), float(level.max()))), index, x, y, pv, level, mp.act(0)))
    vee = np.round(6.0 + 0.012 * np.abs(pv[0] - 900.0) + rng.normal(0.0, 0.3, len(x)), 1).astype(np.float32)
    out.append(case("vee", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_THREE, (float(vee.min()), float(vee.max()))), index, x, y, pv, vee, mp.act(0)))
    out.append(case("vee-free", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_THREE_FREE, (float(vee.min()), float(vee.max())), rng_pos=base.short_delta(ld.PIECEWISE_THREE_FREE)),
                    index, x, y, pv, vee, mp.act(0)))
    return out


def relief_world(rng):
    r = make_raster("relief", rng)
    dem, xll, yll, cs = r["dem"], r["xll"], r["yll"], r["cell_size"]
    x, y, h = base.stations(rng, xll, yll, cs, dem.shape, 12, 40, 42000.0)                     # 52 stations
    pv = mp.station_proxies(rng, x, y, h, xll, yll)
    pv[1][3::11] = np.float32(ld.NODATA)
    pv[3][7::13] = np.float32(ld.NODATA)
    t = mp.temperature(rng, pv)
    n = len(x)
    index = rng.permutation(200)[:n].astype(np.int32)
    ids = [f"st{i}" for i in range(200)]
    order = np.argsort(x)
    lists = [order[:16], order[10:30], order[24:42], order[36:], order[::3]]
    layout = [(0, 12, 0.8), (8, 22, 0.6), (18, 30, 0.9), (26, 36, 0.5), (4, 34, 0.2)]
    r["areas"] = gl.areas_from_maps(header(dem, xll, yll, cs), weight_maps(dem.shape, layout), [[ids[index[i]] for i in l] for l in lists], ids)
    return r, x, y, pv, t, index


def relief_cases(rng, r, x, y, pv, t, index):
    pr = (float(t.min()), float(t.max()))
    out = []
    out.append(case("height", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_TWO, pr), index, x, y, pv, t, mp.act(0)))
    out.append(case("two", "dewT", meteo.SHEPARD, glocal_fit(ld.PIECEWISE_TWO, pr), index, x, y, pv, (t - np.float32(3.5)).astype(np.float32), mp.act(0, 1, 2)))
    out.append(case("four", "airT", meteo.SHEPARD_MODIFIED, glocal_fit(ld.PIECEWISE_THREE, pr), index, x, y, pv, t, mp.act(0, 1, 2, 3, 5)))
    out.append(case("all", "airT", meteo.IDW, glocal_fit(ld.PIECEWISE_THREE_FREE, pr), index, x, y, pv, t, mp.act(*range(S))))
    out.append(case("noheight", "dewT", meteo.IDW, glocal_fit(ld.PIECEWISE_TWO, pr), index, x, y, pv, t, mp.act(2, 5)))
    return out


def run_cases(exe, work, r, cases):
    src, dst, cfg = work / f"{r['name']}.in", work / f"{r['name']}.out", work / f"{r['name']}.cfg"
    gc.write_input(src, r, cases)
    parts = []
    for c in cases:
        f = c["fit"]
        n = len(f["min"])
        parts += [np.array(f["position"] + [0] * (ld.MAX_PARAMETERS - n), np.int32), np.array(f["configured"] + [0.0] * (2 * ld.MAX_PARAMETERS - 2 * n), np.float64),
                  np.array(f["points_range"], np.float64)]
    write_parts(cfg, parts)
    res = subprocess.run([str(exe), str(src), str(dst), str(cfg)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    timing = [line.split() for line in res.stdout.strip().splitlines()]
    return gc.read_output(dst, r, cases), [float(s) for _, _, s in timing]


MUST = ["a cell visited by its area number 1", "a cell visited by its area number 2", "a cell visited by its area number 3", "a DEM cell covered by no area",
        "an area without a weight map", "weights that do not add up to 1", "a cell set to NODATA by a later area",
        "a cell set to NODATA by an earlier area and then refilled", "the height not active", "the height not significant",
        "the height significant with others significant", "a first guess skipped for leaving its range", "the double-inversion rule refuses a better R2",
        "bestR2 < 0 with the refit", "the maximum clamp with lambda >= 1000 not clamping", "a station pruned in the fit of step 1 but present in the rebuilt subset",
        "a station erased by detrendingOtherProxies in step 2", "a proxy significant in one area and not in another"]
MUST += [f"method {n}" for n in meteo.METHODS] + ["variable airT", "variable dewT"] + [f"function {n}" for n in ld.FUNCTIONS]
# arms the reference alone does not reach on these rasters: why, for the notes of the pin
UNREACHED = {}


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
        exe = work / "glocal_pin"
        inc = [f"-I{agro / sub}" for sub in ("interpolation", "meteo", "gis", "mathFunctions", "crit3dDate", "utilities")]
        cmd = ["g++", "-w", "-std=c++17", "-O2", "-fopenmp", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               *map(str, srcs), "-o", str(exe), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)

        for name, world, maker in (("relief", relief_world, relief_cases), ("tiny", tiny_world, tiny_cases)):
            r, x, y, pv, t, index = world(rng)
            cases = maker(rng, r, x, y, pv, t, index)
            got, timing = run_cases(exe, work, r, cases)
            inside = r["dem"] != FLAG
            total = np.zeros(r["dem"].shape, np.float64)
            for area in r["areas"]:
                if len(area["cells"]) == 0:
                    key("an area without a weight map")
                for cell, w in zip(area["cells"], area["weights"]):
                    total[gl.cell_row_col(cell, r["dem"].shape[1])] += float(w)
            key("weights that do not add up to 1", int(((total != 0) & (np.abs(total - 1.0) > 1e-3) & inside).sum()))
            for k, (c, g) in enumerate(zip(cases, got)):
                what = f"{name} {k} {gc.case_name(c)}"
                assert g["status"] == 0, (what, g["status"])
                assert (g["value"][~inside] == FLAG).all() and not np.isnan(g["value"]).any(), (what, "a map holds NaN or a value outside the DEM")
                print(f"  {what}: height significant {g['significant'].astype(int).tolist()}, r2 {np.round(g['r2'], 3).tolist()}, proxies "
                      f"{g['proxy_significant'].astype(int).sum(axis=0).tolist()}, fitted {g['fitted'].tolist()}, kept {g['kept'].tolist()}, NODATA cells "
                      f"{int(((g['value'] == FLAG) & inside).sum())}, {timing[k]:.4f} s")
                key(f"method {meteo.METHODS[c['method']]}")
                key(f"variable {meteo.VARIABLES[c['var']]}")
                key(f"function {ld.FUNCTIONS[c['fit']['function']]}")
                with_stations = g["fitted"] > 0
                mixed = (g["proxy_significant"][with_stations].any(axis=0) & ~g["proxy_significant"][with_stations].all(axis=0)).sum()
                key("a proxy significant in one area and not in another", int(mixed))
                if name == "relief":                                 # on `tiny` the restatement counts these
                    key("the height not active", 0 if c["active"][0] else int(with_stations.sum()))
                    key("a station erased by detrendingOtherProxies in step 2", int((g["fitted"] - g["kept"]).sum()))
            if name == "tiny":
                for k, (c, g) in enumerate(zip(cases, got)):
                    t0 = time.time()
                    mine = gc.restated(r, c, arms=arms)
                    assert not mine["failed"]
                    same(mine, g, f"restatement {k} {gc.case_name(c)}", gc.QUANTITIES)
                    print(f"  restatement {k}: equal ({time.time() - t0:.1f} s)")
            f = gl.flat_areas(r["areas"])
            save.update({f"{name}_dem": r["dem"], f"{name}_maps": r["maps"], f"{name}_geo": np.array([r["xll"], r["yll"], r["cell_size"]], np.float64),
                         f"{name}_cell_offset": f["cell_offset"], f"{name}_cell": f["cell"], f"{name}_weight": f["weight"], f"{name}_station_offset": f["station_offset"],
                         f"{name}_station_index": f["station_index"],
                         f"{name}_cases": np.array(json.dumps([dict(label=c["label"], var=c["var"], method=c["method"], fit=c["fit"], useDetrending=c["useDetrending"],
                                                                    area=float(c["area"]), active=c["active"], others=c["others"]) for c in cases]))})
            for k, (c, g) in enumerate(zip(cases, got)):
                n_par = len(c["fit"]["min"])
                assert (g["parameters"][..., n_par:] == ld.NODATA).all()
                save.update({f"{name}_c{k}_index": c["point_index"], f"{name}_c{k}_x": c["x"], f"{name}_c{k}_y": c["y"], f"{name}_c{k}_pv": c["proxy_values"],
                             f"{name}_c{k}_v": c["value"], f"{name}_c{k}_map": g["value"], f"{name}_c{k}_sig": g["significant"].astype(np.uint8), f"{name}_c{k}_r2": g["r2"],
                             f"{name}_c{k}_par": g["parameters"][..., :n_par].copy(), f"{name}_c{k}_psig": g["proxy_significant"].astype(np.uint8),
                             f"{name}_c{k}_slope": g["slope"], f"{name}_c{k}_icpt": g["intercept"], f"{name}_c{k}_fitted": g["fitted"].astype(np.uint16),
                             f"{name}_c{k}_kept": g["kept"].astype(np.uint16), f"{name}_c{k}_det": g["detrended"], f"{name}_c{k}_skept": g["station_kept"].astype(np.uint8)})
            notes.append(f"{name}: the reference's serial loop took {sum(timing):.4f} s for {len(cases)} cases in the driver")

    for k in MUST:
        arms.setdefault(k, 0)
    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k in MUST if arms[k] == 0 and k not in UNREACHED]
    assert not empty, f"arms never reached: {empty}"
    for k, why in UNREACHED.items():
        if arms[k] == 0:
            notes.append(f"arm not reached with the reference alone on these rasters: {k}: {why}")
    notes.append("the areas are visited in index order: the reference's OpenMP loop has no defined order, the driver runs it serially")
    save.update(flag=FLAG, arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64), notes=np.array(json.dumps(notes)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < (1 << 18)
    return 0


if __name__ == "__main__":
    sys.exit(main())
