#!/usr/bin/env python3
"""Generate tests/golden/rad_rsun.npz: the compiled-reference pin of the hourly r.sun radiation maps (radiation::computeRadiationDEM,
agrolib/solarRadiation/solarRadiation.cpp:1045-1069, over solPos.cpp, computeShadow and computeRadiationRsun).  Run by hand where the
reference tree is present; no test calls it:

    python tests/golden/make_rad_rsun.py --reference <CRITERIA3D tree>

The driver below is this project's own text: it builds a Crit3DRasterGrid from a float array, lets Crit3DRadiationMaps(dem, gisSettings)
compute latitude, longitude, slope and aspect, sets Crit3DRadiationSettings through its setters, fills the transmissivity map and calls
computeRadiationDEM.  It is compiled with plain `g++ -O2` together with the reference's solarRadiation, gis, mathFunctions, meteo and
crit3dDate sources WHERE THEY LIE into a scratch directory (unused functions are dropped at link time), and only data is recorded: the
two DEMs, the four static maps the reference computes on each, the float32 transmissivity maps, the settings and times of the cases,
the five maps after each case, and the arm table.

Rasters: the 24 x 32 Ravone window at 4 m with its flag cells, and the same window with its elevations scaled about their minimum by the
first factor of SCALES with which, on every case of that raster whose sun stands between 10 and 40 degrees, computeShadow ends both
ways.  Both carry a hand-made flat patch (slope == 0) and one cell whose slope is NODATA (S_solpos refuses its tilt).

The arm table is judged by criteria3d_amd.radiation.restate_radiation_hour, which this script first holds against the reference's maps
bit for bit on every case: a restatement that reproduces every value follows the reference's path through the arms.

No case has left the pin (the issue caps such cases at two, each with argument, both results and reason recorded here): none."""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
from criteria3d_amd import radiation as rad      # noqa: E402

OUT = HERE / "rad_rsun.npz"
ROW0, COL0, NROWS, NCOLS = 8, 280, 24, 32             # window of ravone_dem_519x1208.npz, as the snow pin's
SCALES = (3.0, 4.0, 5.0, 6.0, 8.0)
FLAT = (slice(14, 19), slice(20, 25))                 # 5 x 5 cells at one height: slope 0 on the inner 3 x 3
NODATA_SLOPE = (6, 6)
MAPS = rad.MAPS

DRIVER = r"""
// driver of the radiation pin: see make_rad_rsun.py
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "commonConstants.h"
#include "crit3dDate.h"
#include "gis.h"
#include "radiationSettings.h"
#include "solarRadiation.h"

template <class T> static std::vector<T> readv(FILE* f, size_t n) { std::vector<T> v(n); if (fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static void writeGrid(FILE* f, const gis::Crit3DRasterGrid* g) { for (int r = 0; r < g->header->nrRows; ++r) fwrite(g->value[r], 4, g->header->nrCols, f); }

int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<int> dims = readv<int>(in, 2);
    const float flag = readv<float>(in, 1)[0];
    std::vector<double> geo = readv<double>(in, 3);
    const int nrows = dims[0], ncols = dims[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> z = readv<float>(in, n), slopeEdit = readv<float>(in, n);
    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = geo[2]; header.invCellSize = 1.0 / geo[2]; header.flag = flag;
    header.llCorner.x = geo[0]; header.llCorner.y = geo[1];
    gis::Crit3DRasterGrid dem;
    dem.initializeGrid(header);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) dem.value[r][c] = z[(size_t)r * ncols + c];
    dem.isLoaded = true;
    gis::updateMinMaxRasterGrid(&dem);
    gis::Crit3DGisSettings gisSettings;                  // utmZone 32, start location 44.501 N
    Crit3DRadiationMaps maps(dem, gisSettings);
    writeGrid(out, maps.latMap); writeGrid(out, maps.lonMap); writeGrid(out, maps.slopeMap); writeGrid(out, maps.aspectMap);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) if (slopeEdit[(size_t)r * ncols + c] != 12345.f) maps.slopeMap->value[r][c] = slopeEdit[(size_t)r * ncols + c];
    gis::Crit3DRasterGrid paramMap;
    paramMap.initializeGrid(dem, 3.f);                   // a Linke / albedo map: loaded, and never read inside the grid
    const int nCases = readv<int>(in, 1)[0];
    for (int k = 0; k < nCases; ++k) {
        std::vector<int> si = readv<int>(in, 8);
        std::vector<float> sf = readv<float>(in, 17);
        std::vector<int> when = readv<int>(in, 7);
        std::vector<float> trans = readv<float>(in, n);
        Crit3DRadiationSettings rs;
        gisSettings.timeZone = si[6]; gisSettings.isUTC = si[7] != 0;
        rs.setGisSettings(&gisSettings);
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
        if (!when[6]) maps.initialize();
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) maps.transmissivityMap->value[r][c] = trans[(size_t)r * ncols + c];
        Crit3DTime t(Crit3DDate(when[2], when[1], when[0]), when[3] * 3600 + when[4] * 60 + when[5]);
        if (!radiation::computeRadiationDEM(&rs, dem, &maps, t, false)) return 3;
        writeGrid(out, maps.sunElevationMap); writeGrid(out, maps.globalRadiationMap); writeGrid(out, maps.beamRadiationMap);
        writeGrid(out, maps.diffuseRadiationMap); writeGrid(out, maps.reflectedRadiationMap);
    }
    fclose(out);
    return 0;
}
"""

SETTING_INTS = ("realSky", "realSkyAlgorithm", "shadowing", "linkeMode", "albedoMode", "tiltMode", "timeZone", "isUTC")
MONTHLY = (2.1, 2.2, 8.0, 2.9, 3.2, 3.4, 3.5, 3.3, 2.9, 2.6, 2.3, 2.2)         # March: a Linke factor where the A0 patch applies


def transmissivity_maps(valid, flag, seed=20261018):
    """two seeded maps (quantised to 1/64) with NODATA cells in different places, values on all three arms of Erbs' correlation and above clear sky"""
    rng = np.random.default_rng(seed)
    maps = []
    for k in range(2):
        t = (np.round(rng.uniform(0.05, 0.9, valid.shape) * 64) / 64).astype(np.float32)
        t[:, 11 + 6 * k] = -9999.0
        t[3 + 9 * k, 2:9] = -9999.0
        t[~valid] = flag
        maps.append(t)
    return maps


def cases():
    """(name, raster, settings, when, keep, transmissivity map): the times are UTC, the rasters stand at 44.5 N 11.3 E, time zone 1"""
    out = []
    S = lambda **kw: dict(kw)
    eq, js, ds = (2021, 3, 20), (2021, 6, 21), (2021, 12, 21)
    for r in (0, 1):
        out += [
            (f"r{r} equinox night", r, S(), eq + (2, 30, 0), 0, 0),
            (f"r{r} equinox, the hour of sunrise (low sun in the east)", r, S(), eq + (5, 30, 0), 0, 0),
            (f"r{r} equinox morning", r, S(), eq + (6, 30, 0), 0, 0),
            (f"r{r} equinox morning, second hour on the same maps", r, S(), eq + (7, 30, 0), 1, 1),
            (f"r{r} equinox noon", r, S(), eq + (11, 30, 0), 0, 0),
            (f"r{r} equinox afternoon", r, S(), eq + (15, 30, 0), 0, 0),
            (f"r{r} equinox, the hour of sunset (low sun in the west)", r, S(), eq + (17, 15, 0), 0, 1),
            (f"r{r} equinox, after sunset on the maps of the hour before", r, S(), eq + (18, 30, 0), 1, 1),
            (f"r{r} refracted elevation just above zero", r, S(), None, 0, 0),            # the second is searched below
            (f"r{r} June solstice, early", r, S(), js + (4, 30, 0), 0, 1),
            (f"r{r} June solstice noon", r, S(), js + (11, 30, 0), 0, 0),
            (f"r{r} December solstice morning", r, S(), ds + (8, 30, 0), 0, 0),
            (f"r{r} December solstice noon", r, S(), ds + (11, 30, 0), 0, 1),
        ]
    t = eq + (7, 30, 0)
    out += [
        ("total transmissivity, real sky", 1, S(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY), t, 0, 0),
        ("total transmissivity, clear sky", 1, S(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY, realSky=0), t, 0, 0),
        ("Linke, clear sky", 1, S(realSky=0), t, 0, 0),
        ("no shadowing", 1, S(shadowing=0), t, 0, 0),
        ("fixed tilt 30 deg to the south", 1, S(tiltMode=rad.TILT_FIXED, tilt=30.0, aspect=180.0), t, 0, 0),
        ("fixed tilt 0", 0, S(tiltMode=rad.TILT_FIXED, tilt=0.0, aspect=0.0), t, 0, 1),
        ("monthly Linke (March: 8, the A0 patch)", 1, S(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), t, 0, 0),
        ("monthly Linke (June)", 0, S(linkeMode=rad.MODE_MONTHLY, linkeMonthly=MONTHLY), js + (9, 30, 0), 0, 0),
        ("Linke map", 1, S(linkeMode=rad.MODE_MAP), t, 0, 0),
        ("albedo map", 1, S(albedoMode=rad.MODE_MAP), t, 0, 0),
        ("albedo 0.6, clear sky 0.8", 0, S(albedo=0.6, clearSky=0.8), t, 0, 1),
        ("local time (isUTC off), noon", 0, S(isUTC=0), eq + (12, 30, 0), 0, 0),
        ("UTC, time zone -12: the local date is the day before", 0, S(timeZone=-12), eq + (6, 30, 0), 0, 0),
        ("local time, time zone -12, the same instant", 0, S(timeZone=-12, isUTC=0), (2021, 3, 19, 18, 30, 0), 0, 0),
        ("UTC, time zone 12: the local date is the day after", 0, S(timeZone=12), eq + (18, 30, 0), 0, 0),
        ("UTC, the local date is in the next year", 0, S(), (2021, 12, 31, 23, 30, 0), 0, 0),
        ("a year S_solpos refuses (2101): nothing is written", 0, S(), (2101, 3, 20, 11, 30, 0), 0, 0),
    ]
    return out


def search_low_sun(dem, flag, geo, static, settings):
    """the second of the equinox morning at which most cells have a refracted elevation in (0, 1e-3] degrees"""
    lat, lon, slope, aspect = static
    valid = dem != flag
    cells = [rad.cell_setup(float(dem[r, c]), float(lat[r, c]), float(lon[r, c]), float(slope[r, c]), float(aspect[r, c]))
             for r, c in zip(*np.nonzero(valid))][::7]
    best = (-1, None)
    for sec in range(4 * 3600 + 50 * 60, 5 * 3600 + 40 * 60):
        when = (2021, 3, 20, sec // 3600, (sec % 3600) // 60, sec % 60)
        h = rad.hour_setup(when, settings["timeZone"], bool(settings["isUTC"]))
        mid = rad.sun_position(h, cells[len(cells) // 2])
        if mid is None or not (-0.01 < mid["elevationRefr"] < 0.01):
            continue
        count = sum(1 for c in cells if c["ok"] and 0 < rad.sun_position(h, c)["elevationRefr"] <= 1e-3)
        if count > best[0]:
            best = (count, when)
    assert best[0] > 0, "no second with a refracted elevation in (0, 1e-3]"
    return best[1], best[0]


def run_reference(ref, work, dem, flag, geo, slope_edit, case_list, tmaps):
    (work / "driver.cpp").write_text(DRIVER)
    lib = ref / "agrolib"
    dirs = ("solarRadiation", "gis", "mathFunctions", "meteo", "crit3dDate")
    inc = [f"-I{lib / d}" for d in dirs + ("utilities", "interpolation")]
    srcs = [str(p) for d in dirs for p in sorted((lib / d).glob("*.cpp"))]
    cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"), *srcs, "-o", str(work / "rad_pin"), "-lm"]
    print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    with open(work / "in.bin", "wb") as f:
        write_input(f, dem, flag, geo, case_list, tmaps, slope_edit=slope_edit)
    subprocess.run([str(work / "rad_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True)
    rec = np.fromfile(work / "out.bin", np.float32)
    n = dem.size
    static = rec[:4 * n].reshape(4, *dem.shape)
    maps = rec[4 * n:].reshape(len(case_list), 5, *dem.shape)
    return static, maps


def write_input(f, dem, flag, geo, case_list, tmaps, slope_edit=None, static=None):
    """the input of the driver (slope_edit) and of tests/rad_host.cpp (static: lat, lon, slope, aspect)"""
    np.array(dem.shape, np.int32).tofile(f)
    np.array([flag], np.float32).tofile(f)
    np.array(geo, np.float64).tofile(f)
    dem.astype(np.float32).tofile(f)
    if slope_edit is not None:
        slope_edit.astype(np.float32).tofile(f)
    else:
        for m in static:
            np.ascontiguousarray(m, np.float32).tofile(f)
    np.array([len(case_list)], np.int32).tofile(f)
    for _, _, s, when, keep, tk in case_list:
        full = rad.settings_dict(s)
        np.array([full[k] for k in SETTING_INTS], np.int32).tofile(f)
        np.array([full["linke"], *full["linkeMonthly"], full["albedo"], full["tilt"], full["aspect"], full["clearSky"]], np.float32).tofile(f)
        np.array([*when, keep], np.int32).tofile(f)
        tmaps[tk].tofile(f)


def build_raster(window, flag, scale):
    dem = window.copy()
    valid = dem != flag
    if scale != 1.0:
        lo = dem[valid].min()
        dem[valid] = (lo + (dem[valid] - lo) * np.float32(scale)).astype(np.float32)
    patch = dem[FLAT]
    patch[patch != flag] = np.float32(np.round(np.median(patch[patch != flag])))
    return dem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    ref = Path(a.reference)
    d = np.load(HERE / "ravone_dem_519x1208.npz")
    flag = np.float32(d["nodata"])
    cs = float(d["cellsize"])
    window = d["dem"][ROW0:ROW0 + NROWS, COL0:COL0 + NCOLS].astype(np.float32)
    full_rows = d["dem"].shape[0]
    geo = (float(d["xllcorner"]) + COL0 * cs, float(d["yllcorner"]) + (full_rows - ROW0 - NROWS) * cs, cs)
    valid = window != flag
    assert valid[FLAT].all() and valid[NODATA_SLOPE]
    tmaps = transmissivity_maps(valid, flag)
    slope_edit = np.full(window.shape, 12345.0, np.float32)
    slope_edit[NODATA_SLOPE] = -9999.0
    all_cases = cases()

    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        chosen = None
        for scale in SCALES:
            dems = [build_raster(window, flag, 1.0), build_raster(window, flag, scale)]
            statics, recs, lists = [], [], []
            for r in (0, 1):
                mine = [c for c in all_cases if c[1] == r]
                probe = [c if c[3] is not None else c[:3] + ((2021, 3, 20, 5, 0, 0),) + c[4:] for c in mine]
                static, _ = run_reference(ref, work, dems[r], flag, geo, slope_edit, probe[:1], tmaps)
                slope = static[2].copy()
                slope[NODATA_SLOPE] = -9999.0
                when, count = search_low_sun(dems[r], flag, geo, (static[0], static[1], slope, static[3]), rad.settings_dict(None))
                print(f"raster {r}: refracted elevation in (0, 1e-3] on {count} of the probed cells at {when}")
                mine = [c if c[3] is not None else c[:3] + (when,) + c[4:] for c in mine]
                static, maps = run_reference(ref, work, dems[r], flag, geo, slope_edit, mine, tmaps)
                statics.append(static); recs.append(maps); lists.append(mine)
            # the restatement against the reference, bit for bit, and the arms it takes
            arms_of, ok = [], True
            for r in (0, 1):
                lat, lon, slope, aspect = statics[r]
                slope = slope.copy()
                slope[NODATA_SLOPE] = -9999.0
                prev = None
                for k, (name, _, s, when, keep, tk) in enumerate(lists[r]):
                    got, arms = rad.restate_radiation_hour(dems[r], flag, geo[0], geo[1], geo[2], lat, lon, slope, aspect, when, tmaps[tk], s,
                                                           previous=prev if keep else None)
                    if got is None:
                        got, arms = np.full((5,) + window.shape, flag, np.float32), np.zeros(window.shape, np.int64)
                    same = (got.view(np.uint32) == recs[r][k].view(np.uint32)) | (np.isnan(got) & np.isnan(recs[r][k]))
                    assert same.all(), (name, int((~same).sum()), "cells differ between the restatement and the reference")
                    prev = got
                    arms_of.append((r, name, got, arms))
            both = True
            hit_bit = rad._ARM["shadow: hit"]
            marched = hit_bit | rad._ARM["shadow: ray left the grid"] | rad._ARM["shadow: miss (above the highest cell)"]
            for r, name, got, arms in arms_of:
                rays = (arms & marched) != 0
                if r != 1 or not rays.any():
                    continue
                elev = got[0][rays]
                if 10 <= elev.min() and elev.max() <= 40:
                    hit = int(((arms & hit_bit) != 0).sum())
                    free = int(rays.sum()) - hit
                    print(f"  scale {scale}: {name}: sun at {elev.min():.1f}-{elev.max():.1f} deg, shaded {hit}, not shaded {free}")
                    both = both and hit > 0 and free > 0
            if both:
                chosen = scale
                break
        assert chosen is not None, "no scale gives both outcomes of computeShadow at 10-40 degrees"

    counts = {n: 0 for n in rad.ARMS}
    for r, name, got, arms in arms_of:
        for n in rad.ARMS:
            counts[n] += int(((arms & rad._ARM[n]) != 0).sum())
    width = max(map(len, counts))
    for k, v in counts.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k, v in counts.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"

    case_rows = []
    for r in (0, 1):
        for k, (name, _, s, when, keep, tk) in enumerate(lists[r]):
            case_rows.append(dict(name=name, raster=r, index=k, settings=s, when=list(when), keep=keep, transmissivity=tk))
    save = dict(flag=flag, geo=np.array(geo), window=np.array([ROW0, COL0, NROWS, NCOLS], np.int32), scale=np.float32(chosen),
                dem=np.stack(dems), lat=np.stack([s[0] for s in statics]), lon=np.stack([s[1] for s in statics]),
                slope_reference=np.stack([s[2] for s in statics]), aspect=np.stack([s[3] for s in statics]),
                nodata_slope_cell=np.array(NODATA_SLOPE, np.int32), transmissivity=np.stack(tmaps),
                cases=np.array(json.dumps(case_rows)), maps0=recs[0], maps1=recs[1], map_names=np.array(MAPS),
                arm_names=np.array(list(counts)), arm_counts=np.array(list(counts.values()), np.int64))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, scale {chosen}, {len(case_rows)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
