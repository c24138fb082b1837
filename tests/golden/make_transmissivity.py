#!/usr/bin/env python3
"""Generate the compiled-reference pin of the station transmissivity and its window: tests/golden/transmissivity.npz holds what
computeTransmissivity (agrolib/solarRadiation/transmissivity.cpp:105-169, over radiation::computePointTransmissivity,
solarRadiation.cpp:1265-1367) and radiation::estimateTransmissivityWindow (:835-922) of the compiled reference return.  Run by hand
where the reference tree is present; no test calls it:

    python tests/golden/make_transmissivity.py --reference <CRITERIA3D tree>

The driver below is this project's own text: it builds a Crit3DRasterGrid from a float array, sets Crit3DRadiationSettings through its
setters, makes one Crit3DMeteoPoint per station with an hourly (or half-hourly) series of globalIrradiance around the time, calls
computeTransmissivity and reads atmTransmissivity back; for the window it calls estimateTransmissivityWindow per station.  It is
compiled with plain `g++ -O2` together with the reference's solarRadiation, gis, mathFunctions, meteo and crit3dDate sources where they
lie, as make_rad_rsun.py does, and only data is recorded: the rasters, the stations, the measured series, the settings and times of
the cases, the float results, the returned bools and the int window widths, and the arm table.

Crit3DRadiationSettings::setGisSettings (radiationSettings.cpp:344-350) copies utmZone, timeZone and isUTC and leaves the start location
at its default (44.501 N), so a caller that sets nothing else gives its stations the latitude of the northern hemisphere whatever the
project's start location says; the driver therefore writes startLocation.latitude into the settings' own copy, which is what
getLatLonFromUtm reads (solarRadiation.cpp:1288).  The product takes latitude and longitude as inputs, so this choice lies with its caller.

Rasters: the two windows of rad_rsun.npz (the scaled one makes both outcomes of computeShadow occur) and the southern raster of
rad_rsun_places.npz (33.93 S, UTM zone 34 south, 2.5 m cells, time zone 2).

Stations (station_sets): sets of 1, 7 and 40.  The set of 7: a cell centre, a point off centre, a flag cell, a point 1 m west of the
raster (out of the DEM by isOutOfGridXY, column 0 by getRowCol's truncation), a point above dem.maximum, the hollow, and a point far
east.  The hollow is chosen by a rule that does not look at the product's output: the valid cell at least four cells from every edge
whose height lies farthest below the mean of its 5 x 5 neighbourhood.  The set of 40: the seven, points outside on the south and the north,
and seeded points over the raster stretched by a fifth on every side; every second station has z = NODATA (resolved through
getValueFromXY: the flag on a flag cell or outside), the others their cell's height plus a mast of 0-10 m.  No candidate is rejected
from computeTransmissivity's cases; from the window cases window_defined() leaves out the stations S_solpos itself refuses, by a rule
that reads the station and the DEM only (its docstring gives the reason).

Measured series (series): per station one of - all there; the centre NODATA; exactly ceil(0.66 width) there; one fewer; NODATA in
backward slots only; in forward slots only; three times clear sky (the clamp at 1.2); all zeros; seeded gaps.

The arm table is judged by criteria3d_amd.transmissivity.restate_points / restate_window, which this script first holds against the
reference bit for bit on every case and station: a restatement that reproduces every value follows the reference's path."""
import argparse
import json
import math
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
from criteria3d_amd import radiation as rad, transmissivity as tr      # noqa: E402

OUT = HERE / "transmissivity.npz"
NODATA = np.float32(-9999.0)

DRIVER = r"""
// driver of the transmissivity pin: see make_transmissivity.py
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "commonConstants.h"
#include "crit3dDate.h"
#include "gis.h"
#include "meteoPoint.h"
#include "radiationSettings.h"
#include "solarRadiation.h"
#include "transmissivity.h"

template <class T> static std::vector<T> readv(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<int> dims = readv<int>(in, 2);
    const float flag = readv<float>(in, 1)[0];
    std::vector<double> geo = readv<double>(in, 3);
    const int utmZone = readv<int>(in, 1)[0];
    const double startLatitude = readv<double>(in, 1)[0];
    const int nrows = dims[0], ncols = dims[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> z = readv<float>(in, n);
    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = geo[2]; header.invCellSize = 1.0 / geo[2]; header.flag = flag;
    header.llCorner.x = geo[0]; header.llCorner.y = geo[1];
    gis::Crit3DRasterGrid dem;
    dem.initializeGrid(header);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) dem.value[r][c] = z[(size_t)r * ncols + c];
    dem.isLoaded = true;
    gis::updateMinMaxRasterGrid(&dem);
    gis::Crit3DGisSettings gisSettings;
    gisSettings.utmZone = utmZone; gisSettings.startLocation.latitude = startLatitude;
    gis::Crit3DRasterGrid paramMap;
    paramMap.initializeGrid(dem, 3.f);                   // a Linke / albedo map: loaded, and never read inside the grid
    const int nCases = readv<int>(in, 1)[0];
    for (int k = 0; k < nCases; ++k) {
        std::vector<int> si = readv<int>(in, 8);
        std::vector<float> sf = readv<float>(in, 17);
        std::vector<int> call = readv<int>(in, 10);      // year, month, day, hour, minute, second, mode, width, step, nPoints
        const int mode = call[6], width = call[7], step = call[8], nPoints = call[9];
        std::vector<double> xyz = readv<double>(in, (size_t)nPoints * 3);
        Crit3DRadiationSettings rs;
        gisSettings.timeZone = si[6]; gisSettings.isUTC = si[7] != 0;
        rs.setGisSettings(&gisSettings);
        rs.gisSettings->startLocation.latitude = startLatitude;      // the setter copies the zone, the time zone and isUTC only (see the docstring)
        rs.setRealSky(si[0] != 0);
        rs.setRealSkyAlgorithm(TradiationRealSkyAlgorithm(si[1]));
        rs.setShadowing(si[2] != 0);
        rs.setLinkeMode(TparameterMode(si[3]));
        rs.setAlbedoMode(TparameterMode(si[4]));
        rs.setTiltMode(TtiltMode(si[5]));
        rs.setLinkeDefault(sf[0]);
        rs.setLinkeMonthly(std::vector<float>(sf.begin() + 1, sf.begin() + 13));
        rs.setAlbedo(sf[13]); rs.setTilt(sf[14]); rs.setAspect(sf[15]); rs.setClearSky(sf[16]);
        if (si[3] == PARAM_MODE_MAP) rs.setLinkeMap(&paramMap);
        if (si[4] == PARAM_MODE_MAP) rs.setAlbedoMap(&paramMap);
        const Crit3DTime t(Crit3DDate(call[2], call[1], call[0]), call[3] * 3600 + call[4] * 60 + call[5]);
        if (mode == 1) {
            for (int p = 0; p < nPoints; ++p) {
                gis::Crit3DPoint point;
                point.utm.x = xyz[3 * p]; point.utm.y = xyz[3 * p + 1]; point.z = xyz[3 * p + 2];
                const int steps = radiation::estimateTransmissivityWindow(&rs, point, t, dem, step);
                fwrite(&steps, 4, 1, out);
            }
            continue;
        }
        std::vector<float> measured = readv<float>(in, (size_t)nPoints * width);
        const int half = (width - 1) / 2;
        std::vector<Crit3DMeteoPoint> stations((size_t)nPoints);
        for (int p = 0; p < nPoints; ++p) {
            Crit3DMeteoPoint& mp = stations[p];
            mp.point.utm.x = xyz[3 * p]; mp.point.utm.y = xyz[3 * p + 1]; mp.point.z = xyz[3 * p + 2];
            mp.initializeObsDataH(3600 / step, 5, t.date.addDays(-2));
            for (int i = 0; i < width; ++i) {
                const Crit3DTime ti = t.addSeconds((i - half) * step);
                if (!mp.setMeteoPointValueH(ti.date, ti.getHour(), ti.getMinutes(), globalIrradiance, measured[(size_t)p * width + i])) return 4;
            }
        }
        const int ret = computeTransmissivity(&rs, stations, width, t, dem) ? 1 : 0;
        fwrite(&ret, 4, 1, out);
        for (int p = 0; p < nPoints; ++p) {
            const float v = stations[p].getMeteoPointValueH(t.date, t.getHour(), t.getMinutes(), atmTransmissivity);
            fwrite(&v, 4, 1, out);
        }
    }
    fclose(out);
    return 0;
}
"""

SETTING_INTS = ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")
MONTHLY = (2.1, 2.2, 8.0, 2.9, 3.2, 3.4, 3.5, 3.3, 2.9, 2.6, 2.3, 2.2)
POINTS, WINDOW = 0, 1
SERIES = ("all there", "centre NODATA", "just enough", "one too few", "backward NODATA", "forward NODATA", "above clear sky", "all zeros", "seeded gaps")


def rasters():
    """[(name, dem, flag, geo, (utmZone, startLatitude), timeZone)]"""
    a, b = np.load(HERE / "rad_rsun.npz"), np.load(HERE / "rad_rsun_places.npz")
    flag = np.float32(a["flag"])
    geo = tuple(float(v) for v in a["geo"])
    south = json.loads(str(b["places"]))[2]
    return [("window", a["dem"][0].astype(np.float32), flag, geo, (32, 44.501), 1),
            ("scaled window", a["dem"][1].astype(np.float32), flag, geo, (32, 44.501), 1),
            ("south", b["dem"].astype(np.float32), flag, tuple(float(v) for v in b["geo"][2]), (south["utmZone"], south["startLatitude"]), south["timeZone"])]


def hollow(dem, flag):
    """the valid cell at least four cells from every edge farthest below the mean of its 5 x 5 neighbourhood (flag cells left out)"""
    rows, cols = dem.shape
    best = (-1e30, None)
    for r in range(4, rows - 4):
        for c in range(4, cols - 4):
            if dem[r, c] == flag:
                continue
            w = dem[r - 2:r + 3, c - 2:c + 3]
            depth = float(w[w != flag].mean()) - float(dem[r, c])
            if depth > best[0]:
                best = (depth, (r, c))
    return best[1]


def station_sets(dem, flag, geo, seed):
    """{1: [...], 7: [...], 40: [...]} of (x, y, z) with z = NODATA on every second station"""
    rows, cols = dem.shape
    xll, yll, cs = geo
    centre = lambda r, c: (xll + cs * (c + 0.5), yll + cs * (rows - r - 0.5))
    valid = dem != flag
    rr, cc = np.argwhere(valid)[len(np.argwhere(valid)) // 2]
    fr, fc = np.argwhere(~valid)[0]
    hr, hc = hollow(dem, flag)
    top = float(dem[valid].max())
    seven = [centre(rr, cc) + (float(dem[rr, cc]) + 2.0,),                                    # a cell centre, z given
             (centre(rr + 2, cc + 3)[0] + 1.3, centre(rr + 2, cc + 3)[1] - 0.7, float(NODATA)),  # off centre, z from the DEM
             centre(fr, fc) + (float(NODATA),),                                               # a flag cell: the height is the flag
             (xll - 1.0, centre(rows // 2, 0)[1], float(NODATA)),                             # out by isOutOfGridXY, column 0 by truncation
             centre(rr - 3, cc - 2) + (top + 50.0,),                                          # above dem.maximum
             centre(hr, hc) + (float(dem[hr, hc]),),                                          # the hollow
             (xll + cs * cols + 300.0, centre(3, 0)[1], 140.0)]                               # far east, z given
    rng = np.random.default_rng(seed)
    forty = list(seven) + [(centre(0, cols // 2)[0], yll - 40.0, float(NODATA)), (centre(0, cols // 3)[0], yll + cs * rows + 0.5, 150.0),
                           (centre(0, 2)[0], yll + cs * rows, float(NODATA))]
    while len(forty) < 40:
        x = xll + cs * cols * rng.uniform(-0.2, 1.2)
        y = yll + cs * rows * rng.uniform(-0.2, 1.2)
        k = len(forty)
        z = float(NODATA)
        if k % 2:
            r, c = (rows - 1) - int((y - yll) / cs), int((x - xll) / cs)
            inside = 0 <= r < rows and 0 <= c < cols and dem[r, c] != flag
            z = (float(dem[r, c]) if inside else 130.0) + float(np.round(rng.uniform(0, 10), 1))
        forty.append((float(np.round(x, 2)), float(np.round(y, 2)), z))
    return {1: seven[:1], 7: seven, 40: forty}


def series(kind, width, rng, scale=600.0):
    """one station's measured series [width] float32"""
    centre = (width - 1) // 2
    m = np.round(rng.uniform(0.05, 1.0, width) * scale).astype(np.float32)
    enough = math.ceil(0.66 * width)
    others = np.array([i for i in range(width) if i != centre], np.int64)
    if kind == "centre NODATA":
        m[centre] = NODATA
    elif kind in ("just enough", "one too few"):
        keep = enough if kind == "just enough" else enough - 1
        drop = rng.permutation(others)[:width - keep]
        m[drop] = NODATA
    elif kind == "backward NODATA":
        m[:centre][::2] = NODATA
    elif kind == "forward NODATA":
        m[centre + 1:][::2] = NODATA
    elif kind == "above clear sky":
        m[:] = np.float32(3000.0)
    elif kind == "all zeros":
        m[:] = 0.0
    elif kind == "seeded gaps":
        m[rng.permutation(others)[:max(0, (width - enough) // 2)]] = NODATA
    return m


def cases(time_zone_south):
    """(name, raster, settings, when, mode, width, step, station set)"""
    S = lambda **kw: dict(kw)
    eq, js, ds = (2021, 3, 20), (2021, 6, 21), (2021, 12, 21)
    total = dict(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY)
    out = []
    for width in (1, 3, 13, 23):
        for step in (3600, 1800):
            out.append((f"noon, width {width}, step {step}", 1, S(), eq + (11, 0, 0), POINTS, width, step, 7))
    out += [
        ("one station at noon", 0, S(), eq + (11, 30, 0), POINTS, 13, 3600, 1),
        ("forty stations, the hour of sunrise", 1, S(), eq + (5, 30, 0), POINTS, 13, 3600, 40),
        ("forty stations, the hour of sunset", 1, S(), eq + (17, 0, 0), POINTS, 13, 1800, 40),
        ("forty stations, a low sun in December", 1, S(), ds + (8, 30, 0), POINTS, 3, 1800, 40),
        ("a window wholly at night", 1, S(), eq + (0, 30, 0), POINTS, 3, 1800, 7),
        ("a window across midnight and sunrise", 1, S(), eq + (3, 0, 0), POINTS, 13, 3600, 7),
        ("a window across the year's end", 0, S(), (2021, 12, 31, 23, 0, 0), POINTS, 23, 3600, 7),
        ("local time (isUTC off), noon", 1, S(isUTC=0), eq + (12, 30, 0), POINTS, 13, 1800, 7),
        ("time zone -12: backward slots in 1949, which S_solpos refuses (the stale value)", 1, S(timeZone=-12), (1950, 1, 1, 13, 0, 0), POINTS, 13, 3600, 7),
        ("time zone -12: half-hour steps back into 1949", 1, S(timeZone=-12), (1950, 1, 1, 12, 30, 0), POINTS, 7, 1800, 7),
        ("time zone -12: the centre is in 1949 (NODATA is added)", 1, S(timeZone=-12), (1950, 1, 1, 11, 0, 0), POINTS, 3, 3600, 7),
        ("forward slots in 2101, which S_solpos refuses", 0, S(), (2100, 12, 31, 21, 0, 0), POINTS, 7, 3600, 7),
        ("total transmissivity, real sky", 1, S(**total), eq + (8, 30, 0), POINTS, 13, 1800, 40),
        ("total transmissivity, clear sky", 1, S(realSky=0, **total), eq + (14, 30, 0), POINTS, 3, 3600, 7),
        ("Linke, clear sky", 1, S(realSky=0), eq + (9, 30, 0), POINTS, 3, 3600, 7),
        ("no shadowing", 1, S(shadowing=0), eq + (7, 30, 0), POINTS, 3, 3600, 7),
        ("monthly Linke (March: 8), a window into April is March still", 1, S(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), (2021, 3, 31, 20, 0, 0), POINTS, 23, 3600, 7),
        ("monthly Linke (June)", 0, S(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), js + (9, 30, 0), POINTS, 3, 1800, 7),
        ("Linke map and albedo map, stations inside", 1, S(linkeMode=rad.MODE_MAP, albedoMode=rad.MODE_MAP), eq + (10, 30, 0), POINTS, 3, 3600, "inside"),
        ("clear sky 0.8", 0, S(clearSky=0.8), js + (15, 0, 0), POINTS, 13, 1800, 7),
        ("south: December noon", 2, S(timeZone=time_zone_south), ds + (10, 0, 0), POINTS, 13, 3600, 40),
        ("south: June morning", 2, S(timeZone=time_zone_south), js + (6, 30, 0), POINTS, 13, 1800, 7),
        ("south: local time, total transmissivity", 2, S(timeZone=time_zone_south, isUTC=0, **total), ds + (16, 30, 0), POINTS, 23, 1800, 7),
    ]
    for name, r, s, when, step, k in (
            ("noon", 1, S(), eq + (11, 0, 0), 3600, 7), ("morning", 1, S(), eq + (6, 30, 0), 3600, 40), ("sunrise", 1, S(), eq + (5, 30, 0), 1800, 7),
            ("before sunrise", 1, S(), eq + (4, 0, 0), 1800, 7), ("before sunrise, hourly", 1, S(), eq + (3, 0, 0), 3600, 7),
            ("midnight", 1, S(), eq + (23, 0, 0), 3600, 7), ("midnight, half-hourly: the cap", 0, S(), ds + (23, 30, 0), 1800, 7),
            ("December afternoon", 0, S(), ds + (14, 30, 0), 1800, 40), ("sunset", 1, S(), js + (18, 30, 0), 1800, 7),
            ("local time", 1, S(isUTC=0), eq + (7, 0, 0), 3600, 7), ("no shadowing", 1, S(shadowing=0), eq + (6, 30, 0), 3600, 7),
            ("total transmissivity", 1, S(**total), eq + (6, 0, 0), 1800, 7), ("monthly Linke", 1, S(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), eq + (6, 30, 0), 1800, 7),
            ("the centre is in 2101: the noon value stays", 0, S(), (2100, 12, 31, 23, 30, 0), 3600, 7),
            ("time zone -12: steps back into 1949", 1, S(timeZone=-12), (1950, 1, 1, 12, 30, 0), 1800, 7),
            ("south: morning", 2, S(timeZone=time_zone_south), ds + (3, 30, 0), 1800, 7), ("south: June evening", 2, S(timeZone=time_zone_south), js + (15, 30, 0), 3600, 40)):
        out.append((f"window: {name}, step {step}", r, s, when, WINDOW, tr.WINDOW_SLOTS, step, k))
    return out


def window_defined(raster, p):
    """the one rule that leaves a station out, and only of the window cases: S_solpos refuses the point itself (a height that resolves to
    the flag gives a pressure above 2000 hPa), so estimateTransmissivityWindow reads a sunPosition no evaluation has set - the reference's
    answer is then whatever its stack holds, and sf3d_transmissivity_window answers SF3D_PARAMETER_ERROR.  The rule reads the station and
    the DEM only.  In computeTransmissivity the same stations stay: every evaluation fails and NODATA is what is added"""
    _, dem, flag, geo, gis, _ = raster
    st = tr.station_points([p[0]], [p[1]], [p[2]], dict(utmZone=gis[0], startLatitude=gis[1]), dem, dict(xllcorner=geo[0], yllcorner=geo[1], cellsize=geo[2]), flag)[0]
    return bool(rad.cell_setup(float(st[2]), rad.f32(st[3]), rad.f32(st[4]), 0.0, 180.0)["ok"])


def build_reference(ref, work):
    (work / "driver.cpp").write_text(DRIVER)
    lib = ref / "agrolib"
    dirs = ("solarRadiation", "gis", "mathFunctions", "meteo", "crit3dDate")
    inc = [f"-I{lib / d}" for d in dirs + ("utilities", "interpolation")]
    srcs = [str(p) for d in dirs for p in sorted((lib / d).glob("*.cpp"))]
    cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"), *srcs, "-o", str(work / "tr_pin"), "-lm"]
    print(" ".join(cmd))
    subprocess.run(cmd, check=True)


def write_case(f, settings, when, mode, width, step, xyz, measured):
    full = rad.settings_dict(settings)
    np.array([full[k] for k in SETTING_INTS], np.int32).tofile(f)
    np.array([full["linke"], *full["linkeMonthly"], full["albedo"], full["tilt"], full["aspect"], full["clearSky"]], np.float32).tofile(f)
    np.array([*when, mode, width, step, len(xyz)], np.int32).tofile(f)
    np.ascontiguousarray(xyz, np.float64).tofile(f)
    if mode == POINTS:
        np.ascontiguousarray(measured, np.float32).tofile(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    ap.add_argument("--out", help="directory to write the fixture to (default: tests/golden)")
    a = ap.parse_args()
    ras = rasters()
    sets = [station_sets(dem, flag, geo, 20261019 + k) for k, (_, dem, flag, geo, _, _) in enumerate(ras)]
    for k, (_, dem, flag, geo, _, _) in enumerate(ras):      # map mode: stations whose row and column are inside (outside the reference indexes out of bounds)
        rows, cols = dem.shape
        ok = lambda p: 0 <= (rows - 1) - int((p[1] - geo[1]) / geo[2]) < rows and 0 <= int((p[0] - geo[0]) / geo[2]) < cols
        sets[k]["inside"] = [p for p in sets[k][40] if ok(p)][:12]
    rng = np.random.default_rng(20261019)
    rows_out = []
    for name, r, s, when, mode, width, step, which in cases(ras[2][5]):
        xyz = np.array(sets[r][which], np.float64)
        if mode == WINDOW:
            xyz = xyz[[window_defined(ras[r], p) for p in xyz]]
        measured, kinds = None, None
        if mode == POINTS:
            kinds = [SERIES[(k + (1 if len(xyz) == 7 else 0)) % len(SERIES)] if len(xyz) > 1 else "all there" for k in range(len(xyz))]
            if "stale" in name or "NODATA is added" in name or "2101" in name or "1949" in name:
                kinds = ["all there" if k % 2 == 0 else kd for k, kd in enumerate(kinds)]
            measured = np.stack([series(kd, width, rng) for kd in kinds])
        rows_out.append(dict(name=name, raster=r, settings=s, when=list(when), mode=mode, width=width, step=step, xyz=xyz, measured=measured, kinds=kinds))

    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        build_reference(Path(a.reference), work)
        for r, (_, dem, flag, geo, gis, _) in enumerate(ras):
            mine = [c for c in rows_out if c["raster"] == r]
            with open(work / "in.bin", "wb") as f:
                np.array(dem.shape, np.int32).tofile(f)
                np.array([flag], np.float32).tofile(f)
                np.array(geo, np.float64).tofile(f)
                np.array([gis[0]], np.int32).tofile(f)
                np.array([gis[1]], np.float64).tofile(f)
                dem.tofile(f)
                np.array([len(mine)], np.int32).tofile(f)
                for c in mine:
                    write_case(f, c["settings"], c["when"], c["mode"], c["width"], c["step"], c["xyz"], c["measured"])
            subprocess.run([str(work / "tr_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True)
            rec = np.fromfile(work / "out.bin", np.int32)
            at = 0
            for c in mine:
                n = len(c["xyz"])
                if c["mode"] == POINTS:
                    c["ret"] = int(rec[at]); at += 1
                    c["result"] = rec[at:at + n].view(np.float32).copy(); at += n
                else:
                    c["result"] = rec[at:at + n].copy(); at += n
            assert at == rec.size

    # the restatement against the reference, bit for bit, and the arms it takes
    counts = {n: 0 for n in tr.ARMS}
    model_counts = {n: 0 for n in rad.ARMS}
    differ = []
    for c in rows_out:
        _, dem, flag, geo, gis, _ = ras[c["raster"]]
        grid = tr.grid_of(dem, flag, *geo)
        st = tr.station_points(c["xyz"][:, 0], c["xyz"][:, 1], c["xyz"][:, 2], dict(utmZone=gis[0], startLatitude=gis[1]), dem,
                               dict(xllcorner=geo[0], yllcorner=geo[1], cellsize=geo[2]), flag)
        c["stations"] = st
        if c["mode"] == POINTS:
            got, n_valid, arms, model, _ = tr.restate_points(grid, c["settings"], c["when"], c["width"], c["step"], st, c["measured"])
            same = got.view(np.uint32) == c["result"].view(np.uint32)
            if not same.all() or (n_valid > 0) != bool(c["ret"]):
                differ.append((c["name"], np.nonzero(~same)[0].tolist(), got[~same].tolist(), c["result"][~same].tolist()))
        else:
            res = [tr.restate_window(grid, c["settings"], c["when"], p, c["step"]) for p in st]
            got = np.array([v[0] for v in res], np.int32)
            arms, model = np.array([v[1] for v in res], np.int64), np.array([v[2] for v in res], np.int64)
            if not np.array_equal(got, c["result"]):
                differ.append((c["name"], np.nonzero(got != c["result"])[0].tolist(), got.tolist(), c["result"].tolist()))
        c["arms"], c["model_arms"] = [int(v) for v in arms], int(np.bitwise_or.reduce(model)) if len(model) else 0
        for n in tr.ARMS:
            counts[n] += int(((arms & tr._A[n]) != 0).sum())
        for n in rad.ARMS:
            model_counts[n] += int(((model & rad._ARM[n]) != 0).sum())
    for d in differ:
        print("DIFFERS:", d)
    assert not differ, f"{len(differ)} cases differ between the restatement and the reference"
    width = max(map(len, counts))
    for k, v in {**counts, **model_counts}.items():
        print(f"  {k:<{width}} {v:>6}")
    empty = [k for k, v in counts.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"
    for n in ("shadow: hit", "shadow: ray left the grid", "shadow: miss (above the highest cell)", "not illuminated", "illuminated"):
        assert model_counts[n] > 0, n

    save = dict(flag=ras[0][2], arm_names=np.array(list(counts)), arm_counts=np.array(list(counts.values()), np.int64),
                model_arm_names=np.array(list(model_counts)), model_arm_counts=np.array(list(model_counts.values()), np.int64),
                rasters=np.array(json.dumps([dict(name=n, geo=list(g), utmZone=z[0], startLatitude=z[1], timeZone=tz) for n, _, _, g, z, tz in ras])))
    for r, (_, dem, _, _, _, _) in enumerate(ras):
        save[f"dem{r}"] = dem
    meta = []
    for k, c in enumerate(rows_out):
        meta.append(dict(name=c["name"], raster=c["raster"], settings=c["settings"], when=c["when"], mode=c["mode"], width=c["width"], step=c["step"],
                         kinds=c["kinds"], ret=c.get("ret"), arms=c["arms"], model_arms=c["model_arms"]))
        save[f"xyz{k}"] = c["xyz"]
        save[f"stations{k}"] = c["stations"]
        save[f"result{k}"] = c["result"]
        if c["mode"] == POINTS:
            save[f"measured{k}"] = c["measured"]
    save["cases"] = np.array(json.dumps(meta))
    out = (Path(a.out) if a.out else HERE) / OUT.name
    np.savez_compressed(out, **save)
    print(f"{out}: {out.stat().st_size} bytes, {len(meta)} cases")
    assert out.stat().st_size <= (HERE / "ravone_window.npz").stat().st_size
    return 0


if __name__ == "__main__":
    sys.exit(main())
