#!/usr/bin/env python3
"""Generate the compiled-reference pins of the hourly r.sun radiation maps (radiation::computeRadiationDEM,
agrolib/solarRadiation/solarRadiation.cpp:1045-1069, over solPos.cpp, computeShadow and computeRadiationRsun): tests/golden/rad_rsun.npz
(one place, one year: the arms of the radiation model) and tests/golden/rad_rsun_places.npz (other latitudes, longitudes and dates: the
arms of the sun position).  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_rad_rsun.py --reference <CRITERIA3D tree> --pin places
    python tests/golden/make_rad_rsun.py --reference <CRITERIA3D tree> --pin rsun --out <scratch directory>

The second line regenerates rad_rsun.npz elsewhere and compares every array with the committed file, byte for byte (it was equal when
the driver learnt the UTM zone, the start latitude and the edit maps).

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

No case has left the pin (the issue caps such cases at two, each with argument, both results and reason recorded here): none.

rad_rsun_places.npz (make_places).  Per raster the driver reads the UTM zone and gisSettings.startLocation.latitude (its sign is the
hemisphere of utmToLatLon) and edit maps for latMap, lonMap and aspectMap, applied as slopeEdit is: single cells stand where UTM cannot
put them.  Six rasters of 16 x 24 cells, all the cut [4:20, 1:25] of raster 1 of rad_rsun.npz (the scaled window with its flag cells, flat
patch and NODATA slope), each at one place of PLACES: 69.67 N 12.9 E (zone 33, 4 m), 0.23 N 9.2 E (zone 32, 10 m), 33.93 S 18.4 E (zone
34 south, 2.5 m), 37.77 N 122.4 W (zone 10, 4 m, time zone -8), 17.2 S 178.9 W (zone 1 south, 10 m, time zone -12) and the window's own
place with edited cells (EDITS): latitude 90, -90, 89.97; longitude 180, -180, 179.99; latitude 90.5, longitude 180.5 and aspect 361,
which validate() refuses; and the searched cells below.  39 cases (places_cases): polar day at midnight and noon, polar night with a
two-hour chain, the equinox; the zenith at the equator; the sun in the north at the southern place; hours by day and by night in UTC and
one in local time at both western places; 00:05 local time before the true solar midnight; two hours at which the wrapped tstfix
alone makes a cell on the date line dark under a sun 11 degrees high; 29 February 2024 seen from time zone -8 on
both sides, day 366, 2000-02-29, 2100-03-01, 2100-12-31, 1999-12-31 23:30 (ectime < 0), 1951-01-01 (mnlong and mnanom wrap), and 1950-01-01
00:30 in time zone -12, whose local year 1949 S_solpos refuses: the maps of the hour before stay.  As above, the restatement is first held
against the reference bit for bit on every case; then its model arms (rad.ARMS) and sun-position arms (rad.SUN_ARMS) are recorded per
case and counted over the cells with an elevation.  No case has left this pin either: none.

Searches (their results are in the pin's `notes`):
  * elevetr > 85 in most cells: the second of 11:00-12:00 UTC on 2021-03-20 with the highest count (every probed cell at 11:10:50).
  * |ce cl| < 0.001 off the poles needs the sun within 0.057 degrees of the zenith.  Within the hour of the 2021 equinox noon the search
    fails (the sun passes 0.19 degrees from it: highest elevetr 89.806); search_cecl goes on over the noons of 19-23 March and 21-25
    September 2021-2040 and finds 2026-09-22 11:16:02 UTC, where all 339 valid cells take the arm.
  * ca > 1 and ca < -1: at latitude 89.9, where |ce cl| is still 0.0016, the longitudes 9.275 and -171.03 (hour angle near 0 and 180) at
    2021-03-20 11:30 UTC, found by a scan of the longitude in steps of 0.005 degrees; they are cells of the edited raster.
  * cssha > 1 with the sun up: a scan of the latitude from 66 N in steps of 0.002 at December noon finds 66.566 N, where the unrefracted
    geometry has no sunrise and refraction lifts the sun to 0.42 degrees: ssha = 0 keeps the cell dark, any other value would light it.
  * |cz| > 1: NOT REACHED.  The search: for the three hours of the edited raster, 10 000 latitudes within half a degree of the
    declination (steps of 1e-4) with ch = 1, looking for float(sd sl) + float(cd cl) > 1; none exists, so no cell was added.
  * elevref < -9: not reachable by a cell validate() accepts (rad.SUN_ARMS_UNREACHABLE gives the argument), recorded with count 0.

Reached is not held.  An arm counts as reached when a cell takes it; whether a recorded value would change without it is another
question, answered by changing the kernel's text on a scratch copy (DESIGN 19 lists the changes that differ from this pin and those that
do not: both ca clamps, zenref > 93 against 94, hrang > 0 against >= 0, ssha <= 1 against < 1 and the mnlong / mnanom corrections are
taken by cells of this pin, and no recorded value depends on them)."""
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
from criteria3d_amd import radiation as rad      # noqa: E402

OUT = HERE / "rad_rsun.npz"
OUT_PLACES = HERE / "rad_rsun_places.npz"
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
    const int utmZone = readv<int>(in, 1)[0];
    const double startLatitude = readv<double>(in, 1)[0];
    const int nrows = dims[0], ncols = dims[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> z = readv<float>(in, n), latEdit = readv<float>(in, n), lonEdit = readv<float>(in, n), slopeEdit = readv<float>(in, n), aspectEdit = readv<float>(in, n);
    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = geo[2]; header.invCellSize = 1.0 / geo[2]; header.flag = flag;
    header.llCorner.x = geo[0]; header.llCorner.y = geo[1];
    gis::Crit3DRasterGrid dem;
    dem.initializeGrid(header);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) dem.value[r][c] = z[(size_t)r * ncols + c];
    dem.isLoaded = true;
    gis::updateMinMaxRasterGrid(&dem);
    gis::Crit3DGisSettings gisSettings;                  // (initialised to utmZone 32, start location 44.501 N)
    gisSettings.utmZone = utmZone; gisSettings.startLocation.latitude = startLatitude;
    Crit3DRadiationMaps maps(dem, gisSettings);
    writeGrid(out, maps.latMap); writeGrid(out, maps.lonMap); writeGrid(out, maps.slopeMap); writeGrid(out, maps.aspectMap);
    const std::vector<float>* edits[4] = {&latEdit, &lonEdit, &slopeEdit, &aspectEdit};
    gis::Crit3DRasterGrid* edited[4] = {maps.latMap, maps.lonMap, maps.slopeMap, maps.aspectMap};
    for (int m = 0; m < 4; ++m)
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) if ((*edits[m])[(size_t)r * ncols + c] != 12345.f) edited[m]->value[r][c] = (*edits[m])[(size_t)r * ncols + c];
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


def build_reference(ref, work):
    (work / "driver.cpp").write_text(DRIVER)
    lib = ref / "agrolib"
    dirs = ("solarRadiation", "gis", "mathFunctions", "meteo", "crit3dDate")
    inc = [f"-I{lib / d}" for d in dirs + ("utilities", "interpolation")]
    srcs = [str(p) for d in dirs for p in sorted((lib / d).glob("*.cpp"))]
    cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"), *srcs, "-o", str(work / "rad_pin"), "-lm"]
    print(" ".join(cmd))
    subprocess.run(cmd, check=True)


def run_reference(ref, work, dem, flag, geo, slope_edit, case_list, tmaps, gis=None, edits=None):
    """gis: (UTM zone, start latitude), the reference's defaults without; edits: {"lat" / "lon" / "aspect": map, NO_EDIT where the
    reference's value stays}, applied as slope_edit is"""
    with open(work / "in.bin", "wb") as f:
        write_input(f, dem, flag, geo, case_list, tmaps, slope_edit=slope_edit, gis=gis, edits=edits)
    subprocess.run([str(work / "rad_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True)
    rec = np.fromfile(work / "out.bin", np.float32)
    n = dem.size
    static = rec[:4 * n].reshape(4, *dem.shape)
    maps = rec[4 * n:].reshape(len(case_list), 5, *dem.shape)
    return static, maps


NO_EDIT = 12345.0
GIS = (rad.DEFAULT_GIS["utmZone"], rad.DEFAULT_GIS["startLatitude"])


def write_input(f, dem, flag, geo, case_list, tmaps, slope_edit=None, static=None, gis=None, edits=None):
    """the input of the driver (slope_edit, gis, edits) and of tests/rad_host.cpp (static: lat, lon, slope, aspect)"""
    np.array(dem.shape, np.int32).tofile(f)
    np.array([flag], np.float32).tofile(f)
    np.array(geo, np.float64).tofile(f)
    if slope_edit is not None:
        zone, start_latitude = gis or GIS
        np.array([zone], np.int32).tofile(f)
        np.array([start_latitude], np.float64).tofile(f)
    dem.astype(np.float32).tofile(f)
    if slope_edit is not None:
        none = np.full(dem.shape, NO_EDIT, np.float32)
        for m in ((edits or {}).get("lat", none), (edits or {}).get("lon", none), slope_edit, (edits or {}).get("aspect", none)):
            m.astype(np.float32).tofile(f)
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


# ------------------------------------------------------------------------------------------------ the places pin

P_ROW0, P_COL0, P_ROWS, P_COLS = 4, 1, 16, 24          # the cut of raster 1 of rad_rsun.npz: flag cells, the flat patch, the NODATA slope
# (name, UTM zone, start latitude (its sign is the hemisphere), lower left corner (E, N) [m], cell size [m], time zone)
PLACES = (
    ("polar, 69.67 N 12.9 E", 33, 69.67, (420000.0, 7730000.0), 4.0, 1),
    ("equator, 0.23 N 9.2 E", 32, 0.23, (520000.0, 25000.0), 10.0, 1),
    ("south, 33.93 S 18.4 E", 34, -33.93, (262000.0, 6243000.0), 2.5, 2),
    ("west, 37.77 N 122.4 W", 10, 37.77, (551000.0, 4180000.0), 4.0, -8),
    ("date line, 17.2 S 178.9 W", 1, -17.2, (300000.0, 8100000.0), 10.0, -12),
    ("the window of rad_rsun.npz, edited", 32, 44.501, None, 4.0, 1),
)
POLAR, EQUATOR, SOUTH, WEST, DATELINE, EDITED = range(6)
# the edited raster: (row, col, map, value).  Row 1 and row 5 of the cut hold cells with an elevation off the flat patch and the NODATA slope
EDITS = ((1, 6, "lat", 90.0), (1, 7, "lat", -90.0), (1, 8, "lat", 89.97), (1, 9, "lon", 180.0), (1, 10, "lon", -180.0), (1, 11, "lon", 179.99),
         (1, 12, "lat", 90.5), (1, 13, "lon", 180.5), (1, 14, "aspect", 361.0))
EDIT_WHY = {("lat", 90.0): "north pole", ("lat", -90.0): "south pole", ("lat", 89.97): "near the pole: |cd cl| and |ce cl| below 0.001",
            ("lon", 180.0): "date line", ("lon", -180.0): "date line", ("lon", 179.99): "near the date line",
            ("lat", 90.5): "out of validate()'s range", ("lon", 180.5): "out of validate()'s range", ("aspect", 361.0): "out of validate()'s range"}
SEARCHED_ROW = 5                                        # the searched cells of the edited raster (ca clamps, |cz| > 1) go here, from column 6


def places_cases(found):
    """(name, raster, settings, when, keep, transmissivity map); the times are UTC unless the settings say otherwise; found: the searched times"""
    S = lambda r, **kw: dict(kw, timeZone=PLACES[r][5])
    total = dict(realSkyAlgorithm=rad.REALSKY_TOTALTRANSMISSIVITY)
    P, E, Z, W, D, X = POLAR, EQUATOR, SOUTH, WEST, DATELINE, EDITED
    return [
        ("polar: 21 June 2021, midnight (polar day, the sun low in the north)", P, S(P), (2021, 6, 20, 23, 30, 0), 0, 0),
        ("polar: 21 June 2021, morning", P, S(P), (2021, 6, 21, 5, 30, 0), 0, 1),
        ("polar: 21 June 2021, noon", P, S(P), (2021, 6, 21, 11, 30, 0), 0, 0),
        ("polar: 21 June 2021, evening", P, S(P), (2021, 6, 21, 17, 30, 0), 0, 1),
        ("polar: 21 December 2021, an hour of the polar night", P, S(P), (2021, 12, 21, 10, 30, 0), 0, 0),
        ("polar: 21 December 2021, noon (polar night) on the maps of the hour before", P, S(P), (2021, 12, 21, 11, 30, 0), 1, 1),
        ("polar: equinox noon", P, S(P), (2021, 3, 20, 11, 30, 0), 0, 0),
        ("polar: 2024-12-31 11:30, day 366", P, S(P), (2024, 12, 31, 11, 30, 0), 0, 0),
        ("equator: equinox noon", E, S(E), (2021, 3, 20, 11, 30, 0), 0, 0),
        ("equator: the second with elevetr > 85 in most cells", E, S(E), found["zenith"], 0, 1),
        ("equator: the second nearest the zenith (|ce cl| < 0.001 if any)", E, S(E), found["cecl"], 0, 0),
        ("equator: equinox morning", E, S(E), (2021, 3, 20, 6, 30, 0), 0, 0),
        ("equator: equinox evening, total transmissivity", E, S(E, **total), (2021, 3, 20, 16, 30, 0), 0, 1),
        ("equator: 2000-02-29 (the 400-year rule)", E, S(E), (2000, 2, 29, 11, 30, 0), 0, 0),
        ("equator: 1999-12-31 23:30, the local date is 2000-01-01 (ectime < 0)", E, S(E), (1999, 12, 31, 23, 30, 0), 0, 0),
        ("south: 21 December 2021, noon (the sun in the north)", Z, S(Z), (2021, 12, 21, 10, 30, 0), 0, 0),
        ("south: 21 June 2021, morning", Z, S(Z), (2021, 6, 21, 6, 30, 0), 0, 1),
        ("south: 21 June 2021, afternoon on the maps of the morning", Z, S(Z), (2021, 6, 21, 14, 30, 0), 1, 0),
        ("south: fixed tilt 30 deg to the north", Z, S(Z, tiltMode=rad.TILT_FIXED, tilt=30.0, aspect=0.0), (2021, 12, 21, 8, 30, 0), 0, 0),
        ("south: 2100-03-01 (the 100-year rule: day 60)", Z, S(Z), (2100, 3, 1, 10, 30, 0), 0, 0),
        ("south: 2100-12-31 (day 365)", Z, S(Z), (2100, 12, 31, 10, 30, 0), 0, 1),
        ("south: 1951-01-01", Z, S(Z), (1951, 1, 1, 10, 30, 0), 0, 0),
        ("west: 21 June 2021, an hour by day in UTC", W, S(W), (2021, 6, 21, 20, 30, 0), 0, 0),
        ("west: 21 June 2021, an hour by night in UTC", W, S(W), (2021, 6, 21, 8, 30, 0), 0, 0),
        ("west: equinox, morning in UTC", W, S(W), (2021, 3, 20, 15, 30, 0), 0, 1),
        ("west: local time (isUTC off), after noon", W, S(W, isUTC=0), (2021, 3, 20, 12, 30, 0), 0, 0),
        ("west: 2024-02-29 09:30 UTC, the local date is 29 February", W, S(W), (2024, 2, 29, 9, 30, 0), 0, 0),
        ("west: 2024-03-01 00:30 UTC, the local date is 29 February still", W, S(W), (2024, 3, 1, 0, 30, 0), 0, 1),
        ("west: 2022-01-01 03:30 UTC, the local date is in 2021", W, S(W), (2022, 1, 1, 3, 30, 0), 0, 0),
        ("date line: 21 December 2021, an hour by day in UTC", D, S(D), (2021, 12, 21, 23, 30, 0), 0, 0),
        ("date line: 1950-01-01 00:30 UTC, the local year is 1949: S_solpos refuses, the maps stay", D, S(D), (1950, 1, 1, 0, 30, 0), 1, 1),
        ("date line: 21 June 2021, an hour by night in UTC", D, S(D), (2021, 6, 21, 11, 30, 0), 0, 0),
        ("date line: local time (isUTC off), morning, clear sky", D, S(D, isUTC=0, realSky=0), (2021, 9, 22, 9, 30, 0), 0, 0),
        ("date line: afternoon in UTC", D, S(D), (2021, 9, 23, 3, 30, 0), 0, 1),
        ("edited: equinox noon", X, S(X), (2021, 3, 20, 11, 30, 0), 0, 0),
        ("edited: June midnight, 00:05 local time and 23:50 true solar time", X, S(X), (2021, 6, 20, 23, 5, 0), 0, 1),
        ("edited: December noon", X, S(X), (2021, 12, 21, 11, 30, 0), 0, 0),
        # the two hours at which a tstfix wrap decides isIlluminated: the sun stands 11 degrees high over the cell on the date line, and
        # the wrapped tstfix puts sunrise and sunset on the other side of the local time
        ("edited: 21 June 2021 17:30 UTC, the cell at longitude -180 is dark only by the tstfix < -720 wrap", X, S(X), (2021, 6, 21, 17, 30, 0), 0, 1),
        ("edited: 21 June 2021 05:30 UTC in time zone -1, the cell at longitude 180 is dark only by the tstfix > 720 wrap", X, dict(timeZone=-1),
         (2021, 6, 21, 5, 30, 0), 0, 1),
    ]


def _cells(dem, flag, static, step=1):
    lat, lon, slope, aspect = static
    return [rad.cell_setup(float(dem[r, c]), float(lat[r, c]), float(lon[r, c]), float(slope[r, c]), float(aspect[r, c]))
            for r, c in zip(*np.nonzero(dem != flag))][::step]


def search_zenith(dem, flag, static, time_zone):
    """the second of the equinox hour around the local noon at which most cells have elevetr > 85, as search_low_sun does"""
    cells = [c for c in _cells(dem, flag, static, 5) if c["ok"]]
    bit = rad._SUN["refrac: elevetr > 85"]
    best = (-1, None)
    for sec in range(11 * 3600, 12 * 3600, 10):
        when = (2021, 3, 20, sec // 3600, (sec % 3600) // 60, sec % 60)
        h = rad.hour_setup(when, time_zone, True)
        count = sum(1 for c in cells if rad.sun_position(h, c)["sunArms"] & bit)
        if count > best[0]:
            best = (count, when)
    assert best[0] > len(cells) // 2, "no second with elevetr > 85 in most cells"
    return best[1], best[0], len(cells)


def search_cecl(dem, flag, static, time_zone, years=range(2021, 2041)):
    """the second at which the sun stands nearest the zenith of the equator raster: the hour of the 2021 equinox noon first (the nearest
    to the listed case), then the noons of 19-23 March and 21-25 September of `years`, minute by minute on the middle cell, then second by second
    on every cell around the best minute.  -> (when, cells with |ce cl| < 0.001, cells with |cz| > 1, where it was found)"""
    cells = [c for c in _cells(dem, flag, static) if c["ok"]]
    mid = cells[len(cells) // 2]
    bit, czbit = rad._SUN["sazm: default 180 off the poles (|ce cl| < 0.001)"], rad._SUN["|cz| > 1"]

    def seconds(day, secs, who):
        best = (-1, -1.0, None)
        for sec in secs:
            when = day + (sec // 3600, (sec % 3600) // 60, sec % 60)
            h = rad.hour_setup(when, time_zone, True)
            suns = [rad.sun_position(h, c) for c in who]
            key = (sum(1 for s in suns if s["sunArms"] & bit), max(s["elevationRefr"] for s in suns), when)
            best = max(best, key)
        return best
    first = seconds((2021, 3, 20), range(11 * 3600, 12 * 3600), cells[::11])
    if first[0] > 0:
        where = "within the hour of the 2021 equinox noon"
        day, centre = first[2][:3], first[2][3] * 3600 + first[2][4] * 60 + first[2][5]
    else:
        days = [(y, m, d) for y in years for m, ds in ((3, range(19, 24)), (9, range(21, 26))) for d in ds]
        best = max(seconds(day, range(10 * 3600 + 1800, 12 * 3600 + 1800, 60), [mid])[1:] + (day,) for day in days)
        where = (f"not within the hour of the 2021 equinox noon (highest elevetr {first[1]:.3f}: |ce cl| >= 0.001 needs 89.943); "
                 f"searched the noons of 19-23 March and 21-25 September {years[0]}-{years[-1]}")
        day, centre = best[2], best[1][3] * 3600 + best[1][4] * 60 + best[1][5]
    best = seconds(day, range(centre - 90, centre + 91), cells)
    h = rad.hour_setup(best[2], time_zone, True)
    n_cz = sum(1 for c in cells if rad.sun_position(h, c)["sunArms"] & czbit)
    return best[2], best[0], n_cz, where


def search_edited_cells(hours):
    """cells for the edited raster that reach what only rounding reaches: near a pole (latitude +-89.9, where |ce cl| >= 0.001 still) the
    longitudes at which the azimuth's cosine leaves [-1, 1]; and under the sun (latitude = declination) one at which cz does.
    -> [(map edits of one cell, the arm it reaches), ...]; the arms not found are recorded in the pin as never reached"""
    found, log = [], []
    want = ["sazm: ca > 1", "sazm: ca < -1", "|cz| > 1"]
    for h in hours:
        for lat in (89.9, -89.9, 89.5, -89.5):
            for lon in np.arange(-180.0, 180.0, 0.005):
                c = rad.cell_setup(150.0, rad.f32(lat), rad.f32(lon), 20.0, 135.0)
                arms = rad.sun_position(h, c)["sunArms"]
                for n in list(want):
                    if arms & rad._SUN[n]:
                        want.remove(n)
                        found.append((rad.f32(lat), rad.f32(lon), n))
            if not [n for n in want if n.startswith("sazm")]:
                break
        if "|cz| > 1" in want:
            under = lambda lo: rad.sun_position(h, rad.cell_setup(150.0, rad.f32(h["declin"]), rad.f32(lo), 20.0, 135.0))["elevationRefr"]
            lon0 = max(np.arange(-180.0, 180.0, 0.5), key=under)
            f32 = rad.f32
            over = [la for la in (f32(h["declin"] + d) for d in np.arange(-0.5, 0.5, 1e-4))          # cz at ch == 1
                    if f32(f32(h["sd"] * f32(math.sin(rad.RADDEG * la))) + f32(h["cd"] * f32(math.cos(rad.RADDEG * la)))) > 1.0]
            for lat in over[:20]:
                for lon in np.arange(lon0 - 1.0, lon0 + 1.0, 0.002):
                    c = rad.cell_setup(150.0, lat, rad.f32(lon), 20.0, 135.0)
                    if rad.sun_position(h, c)["sunArms"] & rad._SUN["|cz| > 1"]:
                        found.append((lat, rad.f32(lon), "|cz| > 1"))
                        want.remove("|cz| > 1")
                        break
                if "|cz| > 1" not in want:
                    break
    return found, want


def search_polar_night_by_day(h, lon):
    """the latitude at which cssha > 1 (no sunrise by the unrefracted geometry) while refraction lifts the sun above the horizon: with
    ssha = 0 the cell is dark, with any other value it would be lit"""
    bit = rad._SUN["ssha: cssha > 1 (polar night)"]
    for lat in np.arange(66.0, 68.5, 0.002):
        sun = rad.sun_position(h, rad.cell_setup(150.0, rad.f32(lat), lon, 20.0, 135.0))
        if sun["sunArms"] & bit and sun["elevationRefr"] > 0:
            return rad.f32(lat), sun["elevationRefr"]
    return None, None


def make_places(ref, work, out):
    old = np.load(OUT)
    flag = np.float32(old["flag"])
    cut = (slice(P_ROW0, P_ROW0 + P_ROWS), slice(P_COL0, P_COL0 + P_COLS))
    dem = old["dem"][1][cut].astype(np.float32)
    valid = dem != flag
    nodata_slope = (int(old["nodata_slope_cell"][0]) - P_ROW0, int(old["nodata_slope_cell"][1]) - P_COL0)
    flat = (slice(FLAT[0].start - P_ROW0, FLAT[0].stop - P_ROW0), slice(FLAT[1].start - P_COL0, FLAT[1].stop - P_COL0))
    assert (~valid).any() and valid[flat].all() and flat[1].stop <= P_COLS and valid[nodata_slope] and len(np.unique(dem[flat])) == 1
    tmaps = [np.ascontiguousarray(t[cut]) for t in old["transmissivity"]]
    g0 = old["geo"]
    geos = [(p[3][0], p[3][1], p[4]) if p[3] else (float(g0[0]) + P_COL0 * p[4], float(g0[1]) + (NROWS - P_ROW0 - P_ROWS) * p[4], p[4]) for p in PLACES]
    slope_edit = np.full(dem.shape, NO_EDIT, np.float32)
    slope_edit[nodata_slope] = -9999.0

    # the static maps of every raster, the searched times and the searched cells
    probe = [("probe", 0, dict(), (2021, 3, 20, 11, 30, 0), 0, 0)]
    statics = []
    for r, p in enumerate(PLACES):
        static, _ = run_reference(ref, work, dem, flag, geos[r], slope_edit, probe, tmaps, gis=(p[1], p[2]))
        static = static.copy()
        static[2][nodata_slope] = -9999.0
        statics.append(static)
    found, notes = {}, []
    found["zenith"], count, of = search_zenith(dem, flag, statics[EQUATOR], PLACES[EQUATOR][5])
    notes.append(f"equator: elevetr > 85 on {count} of {of} probed cells at {found['zenith']}")
    found["cecl"], n_cecl, n_cz, where = search_cecl(dem, flag, statics[EQUATOR], PLACES[EQUATOR][5])
    notes.append(f"equator: |ce cl| < 0.001 on {n_cecl} cells and |cz| > 1 on {n_cz} cells at {found['cecl']}, {where}")
    cases = places_cases(found)
    hours = [rad.hour_setup(c[3], c[2]["timeZone"], True) for c in cases if c[1] == EDITED]
    searched, missing = search_edited_cells(hours)
    notes.append(f"edited raster: searched cells {[(float(a), float(b), n) for a, b, n in searched]}; not found by the search: {missing}")
    december = next(c for c in cases if c[0] == "edited: December noon")
    lon = float(statics[EDITED][1][SEARCHED_ROW, 6 + len(searched)])
    lat, elev = search_polar_night_by_day(rad.hour_setup(december[3], december[2]["timeZone"], True), lon)
    notes.append(f"edited raster: cssha > 1 with the refracted sun at {elev} degrees at latitude {lat}, longitude {lon}, {december[3]}")
    if lat is not None:
        searched.append((lat, lon, "ssha: cssha > 1 (polar night) with the refracted sun above the horizon"))
    edits = {k: np.full(dem.shape, NO_EDIT, np.float32) for k in ("lat", "lon", "aspect")}
    edit_rows = [dict(row=r, col=c, map=m, value=v, why=EDIT_WHY[(m, v)]) for r, c, m, v in EDITS]
    for k, (lat, lon, why) in enumerate(searched):
        edit_rows += [dict(row=SEARCHED_ROW, col=6 + k, map="lat", value=float(lat), why=why), dict(row=SEARCHED_ROW, col=6 + k, map="lon", value=float(lon), why=why)]
    for e in edit_rows:
        assert valid[e["row"], e["col"]] and (e["row"], e["col"]) != nodata_slope
        edits[e["map"]][e["row"], e["col"]] = e["value"]
    for n in notes:
        print(n)

    # the reference on every raster; the static maps as the cases use them
    recs, lists = [], []
    for r, p in enumerate(PLACES):
        mine = [c for c in cases if c[1] == r]
        static, maps = run_reference(ref, work, dem, flag, geos[r], slope_edit, mine, tmaps, gis=(p[1], p[2]), edits=edits if r == EDITED else None)
        assert np.array_equal(static[[0, 1, 3]], statics[r][[0, 1, 3]])
        if r == EDITED:
            for k, name in ((0, "lat"), (1, "lon"), (3, "aspect")):
                statics[r][k] = np.where(edits[name] != NO_EDIT, edits[name], statics[r][k])
        recs.append(maps); lists.append(mine)

    # the restatement against the reference, bit for bit, and the arms it takes
    counts, sun_counts = {n: 0 for n in rad.ARMS}, {n: 0 for n in rad.SUN_ARMS}
    case_rows, differ = [], []
    for r in range(len(PLACES)):
        lat, lon, slope, aspect = statics[r]
        prev = None
        for k, (name, _, s, when, keep, tk) in enumerate(lists[r]):
            sun_arms = np.zeros(dem.shape, np.int64)
            got, arms = rad.restate_radiation_hour(dem, flag, geos[r][0], geos[r][1], geos[r][2], lat, lon, slope, aspect, when, tmaps[tk], s,
                                                   previous=prev if keep else None, sun_arms=sun_arms)
            if got is None:
                got = prev.copy() if keep else np.full((5,) + dem.shape, flag, np.float32)
                arms = np.zeros(dem.shape, np.int64)
            same = (got.view(np.uint32) == recs[r][k].view(np.uint32)) | (np.isnan(got) & np.isnan(recs[r][k]))
            if not same.all():
                differ.append((name, int((~same).sum()), np.argwhere(~same)[:6].tolist(), got[~same][:6].tolist(), recs[r][k][~same][:6].tolist()))
            prev = recs[r][k]
            for n in rad.ARMS:
                counts[n] += int(((arms & rad._ARM[n]) != 0).sum())
            for n in rad.SUN_ARMS:
                hit = int((((sun_arms & rad._SUN[n]) != 0) & valid).sum())
                sun_counts[n] += hit
            case_rows.append(dict(name=name, raster=r, index=k, settings=s, when=list(when), keep=keep, transmissivity=tk,
                                  arms=int(np.bitwise_or.reduce(arms, axis=None)), sun_arms=int(np.bitwise_or.reduce(sun_arms, axis=None))))
    for d in differ:
        print("DIFFERS:", d)
    assert not differ, f"{len(differ)} cases differ between the restatement and the reference"
    width = max(map(len, sun_counts))
    for k, v in {**counts, **sun_counts}.items():
        print(f"  {k:<{width}} {v:>8}")
    empty = [k for k, v in sun_counts.items() if v == 0]
    assert set(empty) <= set(rad.SUN_ARMS_BY_ROUNDING + rad.SUN_ARMS_UNREACHABLE), f"sun arms never reached: {empty}"
    print(f"sun arms never reached (only rounding reaches them; the searches above failed): {empty}")

    save = dict(flag=flag, cut=np.array([P_ROW0, P_COL0, P_ROWS, P_COLS], np.int32), dem=dem, geo=np.array(geos),
                places=np.array(json.dumps([dict(name=p[0], utmZone=p[1], startLatitude=p[2], timeZone=p[5]) for p in PLACES])),
                lat=np.stack([s[0] for s in statics]), lon=np.stack([s[1] for s in statics]), slope=np.stack([s[2] for s in statics]),
                aspect=np.stack([s[3] for s in statics]), edits=np.array(json.dumps(edit_rows)), notes=np.array(json.dumps(notes)),
                transmissivity=np.stack(tmaps), cases=np.array(json.dumps(case_rows)), map_names=np.array(MAPS),
                arm_names=np.array(list(counts)), arm_counts=np.array(list(counts.values()), np.int64),
                sun_arm_names=np.array(list(sun_counts)), sun_arm_counts=np.array(list(sun_counts.values()), np.int64),
                **{f"maps{r}": recs[r] for r in range(len(PLACES))})
    np.savez_compressed(out, **save)
    print(f"{out}: {out.stat().st_size} bytes, {len(case_rows)} cases")
    assert out.stat().st_size < OUT.stat().st_size
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    ap.add_argument("--pin", choices=("rsun", "places"), default="places", help="which fixture to generate (places reads the committed rad_rsun.npz)")
    ap.add_argument("--out", help="directory to write the fixture to (default: tests/golden); with --pin rsun elsewhere, the arrays are compared with the committed file")
    a = ap.parse_args()
    ref = Path(a.reference)
    out_dir = Path(a.out) if a.out else HERE
    if a.pin == "places":
        with tempfile.TemporaryDirectory() as tmp:
            work = Path(a.keep or tmp)
            work.mkdir(parents=True, exist_ok=True)
            build_reference(ref, work)
            return make_places(ref, work, out_dir / OUT_PLACES.name)
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
        build_reference(ref, work)
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
    out = out_dir / OUT.name
    np.savez_compressed(out, **save)
    print(f"{out}: {out.stat().st_size} bytes, scale {chosen}, {len(case_rows)} cases")
    if out != OUT:
        old, new = np.load(OUT), np.load(out)
        assert sorted(old.files) == sorted(new.files)
        for k in old.files:
            a, b = old[k], new[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        print(f"every one of the {len(old.files)} arrays has the bytes of the committed {OUT.name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
