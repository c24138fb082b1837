#!/usr/bin/env python3
"""Generate tests/golden/topodist.npz: the compiled-reference pin of topographic distance - gis::topographicDistanceMap
(agrolib/gis/gis.cpp:1650-1675) for every station, the library function interpolate() (agrolib/interpolation/interpolation.cpp:2502-2560)
under getUseTD() for every DEM cell with the stations' maps set, unset (nullptr) and mixed, the topoDistance of computeDistances
(:208-256) between the stations themselves, and topographicDistanceOptimize (:2297-2368).  Run by hand where the reference tree is
present; no test calls it:

    python tests/golden/make_topodist.py --reference <CRITERIA3D tree>

The driver below is this project's own text.  It is compiled with `g++ -std=c++17 -O2 -fopenmp -ffunction-sections -fdata-sections
-Wl,--gc-sections` together with the reference's agrolib/interpolation/{interpolation,interpolationSettings,interpolationPoint,
spatialControl}.cpp, meteo/{meteo,meteoPoint,quality}.cpp, gis/*.cpp, mathFunctions/*.cpp and crit3dDate/*.cpp WHERE THEY LIE into a
scratch directory, and only data is recorded: the rasters and their georeference, the stations, the case tables and the results.

Two rasters: 7 x 37 cells of 20 m with relief and flag cells, and 5 x 9 cells of 0.4 m at the same UTM-sized coordinates, where the float
of a cell centre lies in another cell than its own (asserted below): the rule by which computeDistances looks a station's map up.

Before anything is written the Python restatements of criteria3d_amd/topodist.py are held against the reference bit for bit, and the arms
named below are counted from them: none may be empty."""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from criteria3d_amd import meteo, topodist  # noqa: E402

OUT = HERE / "topodist.npz"
FLAG = np.float32(-9999.0)
MAX_KH = 128
MODES = ("none", "all", "mixed", "hand")              # which stations carry a map: nullptr everywhere, every one, the mixed list, every one with the hand-made map

DRIVER = r"""
// driver of the topographic distance pin: see make_topodist.py
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "gis.h"
#include "meteo.h"
#include "meteoPoint.h"
#include "interpolationSettings.h"
#include "interpolationPoint.h"
#include "interpolation.h"
#include "spatialControl.h"

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }
template <class T> static void wr(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short output\n"); exit(3); } }

static const meteoVariable refVar[7] = { airTemperature, precipitation, airRelHumidity, windScalarIntensity, globalIrradiance, atmTransmissivity, airDewTemperature };
static const TInterpolationMethod refMethod[3] = { idw, shepard, shepard_modified };

static void fillGrid(gis::Crit3DRasterGrid& g, const gis::Crit3DRasterGrid& like, const float* values)
{
    g.initializeGrid(like);
    for (int r = 0; r < like.header->nrRows; ++r) for (int c = 0; c < like.header->nrCols; ++c) g.value[r][c] = values[(size_t)r * like.header->nrCols + c];
    g.isLoaded = true;
}

static void settingsFor(Crit3DInterpolationSettings& settings, gis::Crit3DRasterGrid* dem, int method, int useTD, int kh, int heightActive, float slope, float area)
{
    settings.initialize();
    settings.setInterpolationMethod(refMethod[method]);
    settings.setUseTD(useTD != 0);
    settings.setTopoDist_Kh(kh);
    settings.setTopoDist_maxKh(MAX_KH_VALUE);
    settings.setCurrentDEM(dem);
    settings.setUseThermalInversion(false);
    settings.setPointsBoundingBoxArea(area);
    Crit3DProxy height;
    height.setName("elevation"); height.setRegressionSlope(slope);
    settings.addProxy(height, heightActive != 0);
    settings.setCurrentCombination(settings.getSelectedCombination());
    settings.setSignificantCurrentCombination(0, true);
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int timing = argc > 3 ? atoi(argv[3]) : 0;          // repeat topographicDistanceMap (a host figure for scale)
    int dims[6]; float flag; double geo[3];
    rd(in, dims, 6); rd(in, &flag, 1); rd(in, geo, 3);
    const int nrows = dims[0], ncols = dims[1], m = dims[2], nCases = dims[3], hand = dims[4], nOpt = dims[5];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> demv(n), handMap(n);
    rd(in, demv.data(), n);
    std::vector<double> sx(m), sy(m), sz(m);
    rd(in, sx.data(), m); rd(in, sy.data(), m); rd(in, sz.data(), m);
    rd(in, handMap.data(), n);
    std::vector<int> mixed(m); rd(in, mixed.data(), m);

    gis::Crit3DRasterGrid dem;
    dem.header->nrRows = nrows; dem.header->nrCols = ncols; dem.header->cellSize = geo[2]; dem.header->invCellSize = 1.0 / geo[2];
    dem.header->llCorner.x = geo[0]; dem.header->llCorner.y = geo[1]; dem.header->flag = flag;
    dem.initializeGrid(flag);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) dem.value[r][c] = demv[(size_t)r * ncols + c];
    dem.isLoaded = true;

    // the maps
    std::vector<gis::Crit3DPoint> pts(m);
    std::vector<gis::Crit3DRasterGrid> maps(m);
    gis::Crit3DRasterGrid handGrid; fillGrid(handGrid, dem, handMap.data());
    std::vector<float> row(n);
    for (int i = 0; i < m; ++i) {
        pts[i].utm.x = sx[i]; pts[i].utm.y = sy[i]; pts[i].z = sz[i];
        for (int rep = 0; rep <= timing; ++rep) gis::topographicDistanceMap(pts[i], dem, &maps[i]);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) row[(size_t)r * ncols + c] = maps[i].value[r][c];
        wr(out, row.data(), n);
    }
    auto mapOf = [&](int mode, int i) -> gis::Crit3DRasterGrid* {
        if (mode == 0 || (mode == 2 && !mixed[i])) return nullptr;
        return (mode == 3 && i == hand) ? &handGrid : &maps[i];
    };

    // the cases: interpolate() on every DEM cell
    for (int k = 0; k < nCases; ++k) {
        int iv[6]; float fv[3];
        rd(in, iv, 6); rd(in, fv, 3);
        std::vector<float> value(m); rd(in, value.data(), m);
        const int var = iv[0], method = iv[1], kh = iv[2], mode = iv[3], useTD = iv[4], heightActive = iv[5];
        Crit3DInterpolationSettings settings;
        settingsFor(settings, &dem, method, useTD, kh, heightActive, fv[2], fv[1]);
        Crit3DMeteoSettings meteoSettings;
        meteoSettings.setRainfallThreshold(fv[0]);
        std::vector<Crit3DInterpolationDataPoint> points(m);
        for (int i = 0; i < m; ++i) {
            points[i].index = i; points[i].isActive = true; points[i].value = value[i];
            *(points[i].point) = pts[i];
            points[i].topographicDistance = mapOf(mode, i);
        }
        std::vector<float> map(n, flag);
        for (int r = 0; r < nrows; ++r)
            for (int c = 0; c < ncols; ++c) {
                const float z = dem.value[r][c];
                if (isEqual(z, flag)) continue;
                double x, y;
                gis::getUtmXYFromRowCol(*dem.header, r, c, &x, &y);
                std::vector<double> proxyValues(1, NODATA);
                if (heightActive) proxyValues[0] = z;
                map[(size_t)r * ncols + c] = interpolate(points, settings, &meteoSettings, refVar[var], float(x), float(y), z, proxyValues, true);
            }
        wr(out, map.data(), n);
    }

    // the station matrix, per mode: the topoDistance of computeDistances for station i at station j's float position
    long matrixChecks = 0;
    for (int mode = 0; mode < 4; ++mode) {
        std::vector<float> matrix((size_t)m * m);
        Crit3DInterpolationSettings settings;
        settingsFor(settings, &dem, 0, 1, 1, 0, 0.f, 1.f);
        std::vector<Crit3DInterpolationDataPoint> points(m);
        for (int i = 0; i < m; ++i) { points[i].index = i; points[i].isActive = true; points[i].value = 1.f; *(points[i].point) = pts[i]; points[i].topographicDistance = mapOf(mode, i); }
        for (int j = 0; j < m; ++j) {
            const float x = float(sx[j]), y = float(sy[j]), z = float(sz[j]);
            for (int i = 0; i < m; ++i) {
                const float d = gis::computeDistance(x, y, float(sx[i]), float(sy[i]));
                float topo = NODATA;
                gis::Crit3DRasterGrid* g = mapOf(mode, i);
                if (g != nullptr && !gis::isOutOfGridXY(x, y, g->header)) {
                    int r, c;
                    gis::getRowColFromXY(*(g->header), x, y, &r, &c);
                    topo = g->value[r][c];
                }
                if (isEqual(topo, NODATA)) topo = gis::topographicDistance(x, y, z, float(sx[i]), float(sy[i]), float(sz[i]), d, dem);
                matrix[(size_t)j * m + i] = topo;
            }
            // the same through the library's own computeDistances with kh = 1
            std::vector<float> dist = computeDistances(airTemperature, points, settings, x, y, z, false);
            for (int i = 0; i < m; ++i) {
                float d = gis::computeDistance(x, y, float(sx[i]), float(sy[i]));
                d += (1 * matrix[(size_t)j * m + i]);
                if (d != dist[i]) { fprintf(stderr, "station matrix disagrees with computeDistances at %d %d\n", j, i); return 4; }
                matrixChecks++;
            }
        }
        wr(out, matrix.data(), matrix.size());
    }

    // topographicDistanceOptimize
    for (int k = 0; k < nOpt; ++k) {
        int iv[5]; float fv[2];
        rd(in, iv, 5); rd(in, fv, 2);
        const int var = iv[0], method = iv[1], mode = iv[2], heightActive = iv[3], ns = iv[4];
        std::vector<int> sub(ns); rd(in, sub.data(), ns);
        std::vector<float> value(ns), observed(ns); rd(in, value.data(), ns); rd(in, observed.data(), ns);
        Crit3DInterpolationSettings settings;
        settingsFor(settings, &dem, method, 1, 0, heightActive, fv[1], fv[0]);
        Crit3DMeteoSettings meteoSettings;
        meteoSettings.setRainfallThreshold(0.2f);
        std::vector<Crit3DInterpolationDataPoint> points(ns);
        std::vector<Crit3DMeteoPoint> meteoPoints(ns);
        for (int i = 0; i < ns; ++i) {
            const int s = sub[i];
            points[i].index = i; points[i].isActive = true; points[i].value = value[i]; *(points[i].point) = pts[s];
            points[i].topographicDistance = mapOf(mode, s);
            if (heightActive) points[i].proxyValues.push_back(float(sz[s]));
            meteoPoints[i].active = true; meteoPoints[i].quality = quality::accepted; meteoPoints[i].currentValue = observed[i];
            meteoPoints[i].point = pts[s]; meteoPoints[i].lapseRateCode = primary;
            meteoPoints[i].isInsideDem = !gis::isOutOfGridXY(sx[s], sy[s], dem.header);
            if (heightActive) meteoPoints[i].proxyValues.push_back(float(sz[s]));
        }
        topographicDistanceOptimize(refVar[var], meteoPoints, points, settings, &meteoSettings);
        const int kh = settings.getTopoDist_Kh();
        const std::vector<float>& a = settings.getKh_series();
        const std::vector<float>& b = settings.getKh_error_series();
        const int len = (int)a.size();
        wr(out, &kh, 1); wr(out, &len, 1); wr(out, a.data(), a.size()); wr(out, b.data(), b.size());
    }
    fclose(out);
    printf("{\"matrix checks\": %ld}\n", matrixChecks);
    return 0;
}
"""


def bounding_box_area(x, y):
    """(xMax - xMin) * (yMax - yMin) as computeOptimalDataRange hands it to setPointsBoundingBoxArea (spatialControl.cpp:568): a float"""
    return np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))


def raster_relief():
    """7 x 37 cells of 20 m: a ridge across a slope, a pit, flag cells"""
    rows, cols, cs = 7, 37, 20.0
    xll, yll = 681230.0, 4925470.0
    r, c = np.mgrid[0:rows, 0:cols]
    dem = 120.0 + 3.5 * c + 9.0 * np.sin(c / 3.1) * (1 + 0.3 * r) + 60.0 * np.exp(-((c - 22.0) / 2.5) ** 2) - 4.0 * r
    dem = np.round(dem, 2).astype(np.float32)
    dem[3, 9] = np.float32(35.5)                                        # a pit
    for rc in ((0, 0), (0, 1), (2, 15), (3, 15), (4, 16), (6, 36), (5, 30), (1, 21)):
        dem[rc] = FLAG
    st = []                                                             # (x, y, z)
    cx = lambda col: xll + cs * (col + 0.5)
    cy = lambda row: yll + cs * (rows - row - 0.5)
    st.append((cx(5) + 3.1, cy(2) - 4.2, 131.0))                        # inside
    st.append((cx(30) - 6.3, cy(5) + 1.7, 262.4))                       # inside, high ground
    st.append((xll - 333.3, cy(3) + 2.2, 118.0))                        # outside: west
    st.append((xll + cols * cs + 270.9, cy(1) - 7.7, 301.0))            # east
    st.append((cx(12) + 0.4, yll + rows * cs + 191.3, 150.0))           # north
    st.append((cx(25) - 0.9, yll - 207.4, 190.0))                       # south
    st.append((cx(8) + 4.0, cy(4) + 5.0, 140.0))                        # within one cell of a DEM cell centre
    st.append((xll + cs * 18.0, cy(3), 170.0))                          # on a cell border
    st.append((cx(14) + 1.0, cy(1) + 1.0, 10.0))                        # below every cell
    st.append((cx(20) - 2.0, cy(5) - 3.0, 900.0))                       # above every cell
    st.append((cx(27) + 7.7, cy(2) - 6.1, float(dem[4, 11])))           # at exactly a cell's height
    st.append((cx(15) + 2.5, cy(2) + 1.5, 160.0))                       # over a flag cell
    st.append((xll - 0.6 * cs, yll - 0.7 * cs, 125.0))                  # left of and below the lower-left corner within one cell: int() truncates to 0
    x, y, z = (np.round(np.array(a, np.float64), 3) for a in zip(*st))
    return dem, xll, yll, cs, x, y, z


def raster_tiny():
    """5 x 9 cells of 0.4 m at UTM-sized coordinates: the float of y (ulp 0.5 m) leaves the cell"""
    rows, cols, cs = 5, 9, 0.4
    xll, yll = 681230.13, 4925470.27
    r, c = np.mgrid[0:rows, 0:cols]
    dem = np.round(200.0 + 0.35 * c - 0.22 * r + 0.4 * np.sin(1.7 * c + r), 3).astype(np.float32)
    dem[1, 4] = FLAG
    dem[4, 0] = FLAG
    st = [(xll + 1.3, yll + 0.9, 200.1), (xll + 2.9, yll + 1.7, 201.7), (xll - 5.2, yll + 0.3, 199.0), (xll + 6.6, yll + 4.4, 203.0), (xll + 1.7, yll - 3.9, 150.0),
          (xll + 2.1, yll + 1.1, 600.0)]
    x, y, z = (np.round(np.array(a, np.float64), 3) for a in zip(*st))
    return dem, xll, yll, cs, x, y, z


def case_table(n, rng, tiny):
    """dicts of var, method, kh, mode, useTD, heightActive, slope, threshold, value"""
    values = dict(airT=np.round(rng.uniform(4.0, 26.0, n), 2), relHum=np.round(rng.uniform(-40.0, 150.0, n), 1), windInt=np.round(rng.uniform(-3.0, 6.0, n), 2),
                  prec=np.round(rng.uniform(0.0, 1.2, n) ** 3, 3))
    out = []
    add = lambda var, method, kh, mode, td=1: out.append(dict(var=var, method=method, kh=kh, mode=mode, useTD=td, heightActive=int(var == "airT"), slope=-0.0065,
                                                             threshold=0.2, value=values[var].astype(np.float32)))
    if tiny:
        for mode in ("none", "all", "mixed"):
            for method in range(3):
                add("airT", method, 3, mode)
        add("relHum", meteo.IDW, 1, "all")
        return out
    for mode in ("none", "all", "mixed"):
        for method in range(3):
            for kh in (0, 1, 7, 40):
                add("airT", method, kh, mode)
    for var in ("relHum", "windInt"):
        for method in range(3):
            add(var, method, 5, "mixed")
        add(var, meteo.SHEPARD, 1, "all")
        add(var, meteo.IDW, 23, "none")
    for method in range(3):                                             # not a TD variable: kh is ignored
        add("prec", method, 9, "all")
    add("prec", meteo.IDW, 0, "none")
    for method in range(3):                                             # a hand-made map in the place of the computed one
        add("airT", method, 4, "hand")
    add("airT", meteo.SHEPARD, 6, "all", td=0)                          # useTD off: kh is ignored
    return out


def run_raster(agro, work, name, dem, xll, yll, cs, x, y, z, cases, opts, hand, mixed, hand_map, timing=0):
    exe = work / "topodist_pin"
    n = len(x)
    area = bounding_box_area(x, y)
    with open(work / f"{name}.in", "wb") as f:
        np.array([dem.shape[0], dem.shape[1], n, len(cases), hand, len(opts)], np.int32).tofile(f)
        np.array([FLAG], np.float32).tofile(f)
        np.array([xll, yll, cs], np.float64).tofile(f)
        dem.tofile(f)
        for a in (x, y, z):
            a.astype(np.float64).tofile(f)
        hand_map.astype(np.float32).tofile(f)
        mixed.astype(np.int32).tofile(f)
        for c in cases:
            c["area"] = area
            np.array([meteo.VARIABLES.index(c["var"]), c["method"], c["kh"], MODES.index(c["mode"]), c["useTD"], c["heightActive"]], np.int32).tofile(f)
            np.array([c["threshold"], area, c["slope"]], np.float32).tofile(f)
            c["value"].tofile(f)
        for o in opts:
            o["area"] = bounding_box_area(x[o["sub"]], y[o["sub"]])
            np.array([meteo.VARIABLES.index(o["var"]), o["method"], MODES.index(o["mode"]), o["heightActive"], len(o["sub"])], np.int32).tofile(f)
            np.array([o["area"], o["slope"]], np.float32).tofile(f)
            np.asarray(o["sub"], np.int32).tofile(f)
            o["value"].astype(np.float32).tofile(f)
            o["observed"].astype(np.float32).tofile(f)
    r = subprocess.run([str(exe), str(work / f"{name}.in"), str(work / f"{name}.out"), str(timing)], check=True, capture_output=True, text=True)
    print(name, r.stdout.strip())
    raw = np.fromfile(work / f"{name}.out", np.uint8)
    cells = dem.size
    pos = 0

    def take(count, dtype):
        nonlocal pos
        a = raw[pos:pos + count * 4].view(dtype).copy()
        pos += count * 4
        return a
    maps = take(n * cells, np.float32).reshape(n, *dem.shape)
    case_maps = take(len(cases) * cells, np.float32).reshape(len(cases), *dem.shape)
    matrices = take(4 * n * n, np.float32).reshape(4, n, n)
    opt_out = []
    for _ in opts:
        kh, ln = take(2, np.int32)
        opt_out.append((int(kh), take(ln, np.float32), take(ln, np.float32)))
    assert pos == raw.size
    return maps, case_maps, matrices, opt_out


def settings_of(c):
    return dict(allZero=0, rainfallThreshold=c.get("threshold", 0.2), useDetrending=1, useTopographicDistance=c.get("useTD", 1),
                proxies=[dict(active=c["heightActive"], isHeight=1, inversion=0, slope=c["slope"], lapseRateH0=meteo.NODATA, lapseRateH1=meteo.NODATA,
                              inversionLapseRate=meteo.NODATA)])


def mode_maps(mode, maps, mixed, hand, hand_map):
    """(list of maps, map index per station) of a mode"""
    held = [hand_map if (mode == "hand" and i == hand) else maps[i] for i in range(len(maps))]
    if mode == "none":
        index = np.full(len(maps), -1, np.int32)
    elif mode == "mixed":
        index = np.where(mixed != 0, np.arange(len(maps)), -1).astype(np.int32)
    else:
        index = np.arange(len(maps), dtype=np.int32)
    return held, index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    ap.add_argument("--timing", type=int, default=0, help="repeat topographicDistanceMap this many times (a host figure for scale)")
    a = ap.parse_args()
    agro = Path(a.reference) / "agrolib"
    srcs = [agro / "interpolation" / f for f in ("interpolation.cpp", "interpolationSettings.cpp", "interpolationPoint.cpp", "spatialControl.cpp")]
    srcs += [agro / "meteo" / f for f in ("meteo.cpp", "meteoPoint.cpp", "quality.cpp")]
    for sub in ("gis", "mathFunctions", "crit3dDate"):
        srcs += sorted((agro / sub).glob("*.cpp"))
    rng = np.random.default_rng(20261020)
    save, arms = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER.replace("MAX_KH_VALUE", str(MAX_KH)))
        inc = [f"-I{agro / sub}" for sub in ("interpolation", "meteo", "gis", "mathFunctions", "crit3dDate", "utilities")]
        cmd = ["g++", "-w", "-std=c++17", "-O2", "-fopenmp", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               *map(str, srcs), "-o", str(work / "topodist_pin"), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        for name, (dem, xll, yll, cs, x, y, z) in (("relief", raster_relief()), ("tiny", raster_tiny())):
            tiny = name == "tiny"
            n = len(x)
            hand = 1
            mixed = (np.arange(n) % 3 != 1).astype(np.int32)                    # every third station has no map
            hand_map = np.where(dem == FLAG, FLAG, np.round(rng.uniform(0.0, 80.0, dem.shape), 1)).astype(np.float32)
            hand_map[2, 3] = np.float32(meteo.NODATA)                           # a NODATA value inside a map: the walk
            cases = case_table(n, rng, tiny)
            opts = []
            if not tiny:
                t = np.round(rng.uniform(8.0, 24.0, n), 2).astype(np.float32)
                rh = np.round(rng.uniform(35.0, 95.0, n), 1).astype(np.float32)
                full, part = np.arange(n), np.array([0, 1, 3, 4, 6, 7, 9, 10])
                slope = np.float32(-0.0065)
                # air temperature: the interpolation points hold detrended values (value - z * slope), the meteo points the observed ones
                det = lambda s: (t[s] - (np.float32(z[s]).astype(np.float64) * float(slope)).astype(np.float32)).astype(np.float32)
                opts.append(dict(var="airT", method=meteo.IDW, mode="all", heightActive=1, slope=-0.0065, sub=full, value=det(full), observed=t[full]))
                opts.append(dict(var="relHum", method=meteo.SHEPARD_MODIFIED, mode="mixed", heightActive=0, slope=0.0, sub=part, value=rh[part], observed=rh[part]))
                opts.append(dict(var="airT", method=meteo.SHEPARD, mode="none", heightActive=1, slope=-0.0065, sub=part, value=det(part), observed=t[part]))
            maps, case_maps, matrices, opt_out = run_raster(agro, work, name, dem, xll, yll, cs, x, y, z, cases, opts, hand, mixed, hand_map, 0 if tiny else a.timing)
            assert not np.isnan(case_maps).any() and not np.isinf(case_maps).any(), "a map holds inf / NaN: change the tables"

            # ---- the restatements, bit for bit
            walk_arms = {}
            for i in range(n):
                mine = topodist.restate_map(dem, xll, yll, cs, x[i], y[i], z[i], FLAG, arms=walk_arms)
                assert np.array_equal(mine.view(np.uint32), maps[i].view(np.uint32)), (name, "map", i)
            for k, v in walk_arms.items():
                arms[f"walk: {k}"] = arms.get(f"walk: {k}", 0) + v
            for k, c in enumerate(cases):
                held, index = mode_maps(c["mode"], maps, mixed, hand, hand_map)
                got = {}
                mine = topodist.restate_interpolate(dem, xll, yll, cs, [None], c["var"], c["method"], x, y, z, c["value"], c["area"], settings_of(c), c["kh"],
                                                    held, index, FLAG, arms=got)
                bad = mine.view(np.uint32) != case_maps[k].view(np.uint32)
                assert not bad.any(), (name, "case", k, c["var"], c["method"], c["kh"], c["mode"], int(bad.sum()), mine[bad][:3], case_maps[k][bad][:3])
                for key, v in got.items():
                    arms[f"interpolate: {key}"] = arms.get(f"interpolate: {key}", 0) + v
            for mi, mode in enumerate(MODES):
                held, index = mode_maps(mode, maps, mixed, hand, hand_map)
                mine = topodist.restate_station_matrix(dem, xll, yll, cs, FLAG, x, y, z, held, index)
                assert np.array_equal(mine.view(np.uint32), matrices[mi].view(np.uint32)), (name, "matrix", mode)
            series_note = []
            for o, (kh, ks, es) in zip(opts, opt_out):
                held, index = mode_maps(o["mode"], maps, mixed, hand, hand_map)
                s = o["sub"]
                matrix = topodist.restate_station_matrix(dem, xll, yll, cs, FLAG, x[s], y[s], z[s], held, index[s])
                inside = ~((x[s] < xll) | (y[s] < yll) | (x[s] >= xll + dem.shape[1] * cs) | (y[s] >= yll + dem.shape[0] * cs))
                pv = [[float(np.float32(zz))] for zz in z[s]] if o["heightActive"] else None
                my_kh, series = topodist.optimize_kh(o["var"], o["method"], x[s], y[s], z[s], o["value"], o["observed"], matrix, o["area"], settings_of(o), MAX_KH,
                                                     pv, inside)
                assert my_kh == kh, (name, "optimize", o["var"], my_kh, kh)
                mk, me = np.array([p[0] for p in series], np.float32), np.array([p[1] for p in series], np.float32)
                assert np.array_equal(mk.view(np.uint32), ks.view(np.uint32)), (mk, ks)
                series_note.append(bool(np.array_equal(me.view(np.uint32), es.view(np.uint32))))
                assert series_note[-1], ("the Kh error series differs", me, es)
                print(f"  optimize {o['var']} {meteo.METHODS[o['method']]} {o['mode']}: Kh {kh}, {len(ks)} evaluations, errors {es.min():.4f} .. {es.max():.4f}")
            if tiny:                                                            # the look-up rule: a DEM cell whose float centre lies in another cell
                cx, cy = meteo.cell_centres(dem.shape, xll, yll, cs)
                _, row, col, ok = topodist._lookup([], [], dem.shape, xll, yll, cs, cx.ravel().astype(np.float32), cy.ravel().astype(np.float32))
                r0, c0 = np.mgrid[0:dem.shape[0], 0:dem.shape[1]]
                moved = ((row != r0.ravel()) | (col != c0.ravel()) | ~ok) & (dem.ravel() != FLAG)
                arms["look-up: the float centre of a DEM cell lies in another cell"] = int((moved & ok).sum())
                arms["look-up: the float centre of a DEM cell lies outside the grid"] = int((moved & ~ok).sum())
                assert (moved & ok).any(), "no DEM cell of the tiny raster looks another cell up: move the raster"
            save.update({f"{name}_dem": dem, f"{name}_geo": np.array([xll, yll, cs], np.float64), f"{name}_x": x, f"{name}_y": y, f"{name}_z": z,
                         f"{name}_maps": maps, f"{name}_hand": np.int32(hand), f"{name}_hand_map": hand_map, f"{name}_mixed": mixed,
                         f"{name}_case_var": np.array([meteo.VARIABLES.index(c["var"]) for c in cases], np.int32),
                         f"{name}_case_method": np.array([c["method"] for c in cases], np.int32), f"{name}_case_kh": np.array([c["kh"] for c in cases], np.int32),
                         f"{name}_case_mode": np.array([MODES.index(c["mode"]) for c in cases], np.int32),
                         f"{name}_case_values": np.array([c["value"] for c in cases], np.float32),
                         f"{name}_case_settings": np.array(json.dumps([settings_of(c) for c in cases])),
                         f"{name}_case_area": np.array([c["area"] for c in cases], np.float32), f"{name}_case_maps": case_maps, f"{name}_matrices": matrices})
            if opts:
                save.update({"opt_table": np.array(json.dumps([dict(var=o["var"], method=o["method"], mode=o["mode"], heightActive=o["heightActive"], slope=o["slope"],
                                                                   sub=[int(q) for q in o["sub"]], area=float(o["area"])) for o in opts])),
                             "opt_kh": np.array([kh for kh, _, _ in opt_out], np.int32)})
                for k, (o, (kh, ks, es)) in enumerate(zip(opts, opt_out)):
                    save.update({f"opt{k}_value": o["value"], f"opt{k}_observed": o["observed"], f"opt{k}_series_kh": ks, f"opt{k}_series_error": es})

    names = {"walk: first": "walk from the cell (the cell is the lower end)", "walk: second": "walk from the station (or a tie)", "walk: below": "distance below a cell size",
             "walk: flag": "sample on a flag cell", "walk: outside": "sample outside the grid", "interpolate: map hit": "map hit",
             "interpolate: map miss": "map miss falling back to the walk", "interpolate: input order": "Shepard list by input order",
             "interpolate: insertion": "Shepard list by insertion"}
    table = {names.get(k, k): v for k, v in arms.items()}
    for k in names.values():
        table.setdefault(k, 0)
    width = max(map(len, table))
    for k, v in table.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k in names.values() if table[k] == 0]
    assert not empty, f"arms never reached: {empty}"
    save.update(flag=FLAG, modes=np.array(MODES), max_kh=np.int32(MAX_KH), arm_names=np.array(list(table)), arm_counts=np.array(list(table.values()), np.int64))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    assert OUT.stat().st_size < (1 << 20)
    return 0


if __name__ == "__main__":
    sys.exit(main())
