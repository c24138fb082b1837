#!/usr/bin/env python3
"""Generate tests/golden/crop_et0.npz: the compiled-reference pin of the hourly reference evapotranspiration and the daily crop maps -
ET0_Penman_hourly (agrolib/meteo/meteo.cpp:550-609, helpers of agrolib/mathFunctions/physics.cpp) driven per cell as
Crit3DHourlyMeteoMaps::computeET0PMMap (agrolib/project/meteoMaps.cpp:238-271) drives it, the daily extremes of
Crit3DProject::updateDailyTemperatures (bin/CRITERIA3D/criteria3DProject.cpp:1994-2018), and Crit3DCrop::getDailyDegreeIncrease /
computeSimpleLAI (agrolib/crop/crop.cpp:161-224, development.cpp:117-154) driven as dailyUpdateCropMaps (:576-640) and
initializeCropFromDegreeDays (:524-573) drive them.  Run by hand where the reference tree is present; no test calls it:

    python tests/golden/make_crop_et0.py --reference <CRITERIA3D tree>

The driver below is this project's own text: float maps in plain arrays, one Crit3DCrop object per land unit with its public fields set
from the table, the map loops of the application restated around the reference's point functions, and a counter per arm.  It is compiled
with `g++ -O2 -ffunction-sections -fdata-sections -Wl,--gc-sections` together with the reference's agrolib/crop/{crop,development,root}.cpp,
soil/soil.cpp, meteo/meteo.cpp, mathFunctions/{physics,basicMath}.cpp and crit3dDate/crit3dDate.cpp WHERE THEY LIE into a scratch
directory, and only data is recorded: the DEM window, the land-unit index map and the crop table, the quantised inputs of the hourly
records, the list of operations (the calendar), the hand-set state maps, the five maps at the checkpoints and the arm table.

The calendar is a list of operations (OPS) replayed by the driver and, in the tests, by the product and by the restatement:
  latitude 44.5: degree-day map at doy 100 -> three 24-hour days (doy 100-102) -> hand-set degree days -> doy 300-340 at four hours a
  day (leaf fall starts at 305, the 30-day senescence ends at 335) -> doy 364, 1 (the reset), 2;
  latitude -35: hand-set degree days -> doy 119, 120 (leaf fall), 130, 181, 182 (the reset; no leaf fall any more)."""
import argparse
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "crop_et0.npz"
ROW0, COL0, NROWS, NCOLS = 8, 280, 24, 32             # the snow pin's window of ravone_dem_519x1208.npz (11.7 % flag cells)
CLEAR_SKY = 0.75                                      # CLEAR_SKY_TRANSMISSIVITY_DEFAULT
MAPS = ("degreeDays", "lai", "dailyTmin", "dailyTmax", "et0")
INPUT = ("airT", "relHum", "windInt", "globalRad", "transmissivity")
STEPS = (0.5, 1.0, 0.5, 4.0, 1.0 / 32)                # the inputs are int16 codes times these (exact in float32); code -32768: the flag
OP_HOUR, OP_DAY, OP_SET_STATE, OP_CHECKPOINT, OP_SET_DEGREE_DAYS, OP_LATITUDE = 1, 2, 3, 4, 5, 6
# speciesType (agrolib/crop/crop.h:14)
HERBACEOUS_ANNUAL, HERBACEOUS_PERENNIAL, HORTICULTURAL, GRASS, TREE, FALLOW, FALLOW_ANNUAL, BARESOIL = range(8)
UNIT_FIELDS = ("type", "isCrop", "sowingDoy", "plantCycle", "LAImin", "LAImax", "LAIgrass", "LAIcurve_a", "LAIcurve_b", "thermalThreshold",
               "upperThermalThreshold", "degreeDaysIncrease", "degreeDaysDecrease", "degreeDaysEmergence")
# synthetic land units (numbers in the range of a crop database): a winter annual whose cycle wraps the year end, a transplanted
# horticultural crop, a grass, a tree with undersown grass, bare soil, a unit without crop id, a summer annual, a tree without grass
UNITS = (
    (HERBACEOUS_ANNUAL, 1, 300, 200, 0.0, 5.0, 0.0, 4.0, -0.006, 0.0, 30.0, 1400, 1200, 120),
    (HORTICULTURAL, 1, 130, 115, 0.3, 4.0, 0.0, 5.0, -0.02, 10.0, 30.0, 600, 600, 0),
    (GRASS, 1, -9999, 365, 1.0, 4.0, 0.0, 4.8, -0.011, 2.0, 35.0, 1400, 100, -9999),
    (TREE, 1, -9999, 365, 0.0, 2.5, 0.5, 6.5, -0.015, 8.0, 35.0, 1200, 1200, -9999),
    (BARESOIL, 0, -9999, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0),
    (HERBACEOUS_ANNUAL, 0, -9999, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0),
    (HERBACEOUS_ANNUAL, 1, 90, 180, 0.0, 5.0, 0.0, 5.3, -0.014, 8.0, 30.0, 1000, 1200, 30),
    (TREE, 1, -9999, 365, 1.0, 4.0, 0.0, 4.1, -0.014, 0.0, 35.0, 2500, 1000, -9999),
)

DRIVER = r"""
// driver of the ET0 / crop pin: see make_crop_et0.py
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "crit3dDate.h"
#include "physics.h"
#include "meteo.h"
#include "crop.h"

double emissivityFromVaporPressure(double myVP);      // meteo.cpp:433, not in meteo.h

enum { A_ET0_NO_DEM, A_ET0_DEM_INT_ONLY, A_ET0_NO_RAD, A_ET0_NO_TRANS, A_ET0_NO_TEMP, A_ET0_NO_RH, A_ET0_NO_WIND, A_ET0_COMPUTED, A_ET0_TRANS_ABOVE_CLEAR,
       A_ET0_CLOUD_ZERO, A_ET0_CLOUD_BETWEEN, A_ET0_NETRAD_POS, A_ET0_NETRAD_NEG, A_ET0_POSITIVE, A_ET0_CLIPPED,
       A_T_NO_AIRT, A_T_FIRST_MIN, A_T_FIRST_MAX, A_T_MIN_LOWER, A_T_MIN_KEPT, A_T_MAX_HIGHER, A_T_MAX_KEPT,
       A_D_RESET, A_D_NO_DEM, A_D_DEM_ISEQUAL_ONLY, A_D_NO_UNIT, A_D_NOT_CROP, A_D_NO_EXTREMES, A_D_OUTSIDE_CYCLE, A_D_INSIDE_CYCLE, A_D_INSIDE_BY_WRAP,
       A_D_OUTSIDE_NEG_BRANCH, A_D_TMAX_CLIPPED, A_D_BELOW_THRESHOLD, A_D_FIRST_VALUE, A_D_ACCUMULATED,
       A_L_BEFORE_EMERGENCE, A_L_SOWN_RISING, A_L_SOWN_FALLING, A_L_PERENNIAL_RISING, A_L_PERENNIAL_FALLING, A_L_LAIMIN, A_L_TREE_NO_LEAF_FALL,
       A_L_TREE_SENESCENCE, A_L_TREE_AFTER_SENESCENCE, A_L_TREE_GRASS, A_L_FROM_DEGREE_DAY_MAP, A_L_DEGREE_DAY_MAP_FLAG, A_COUNT };
static const char* armNames[A_COUNT] = {
    "ET0: outside the DEM", "ET0: DEM cell by isEqual, not by int()", "ET0: no global radiation", "ET0: no transmissivity", "ET0: no air temperature",
    "ET0: no relative humidity", "ET0: no wind", "ET0: computed", "ET0: transmissivity above clear sky (min with 1)", "ET0: cloud factor clipped at 0",
    "ET0: cloud factor between", "ET0: net radiation > 0 (day)", "ET0: net radiation <= 0 (night)", "ET0: result > 0", "ET0: sum clipped at 0",
    "extremes: no air temperature", "extremes: first minimum of the day", "extremes: first maximum of the day", "extremes: new minimum", "extremes: minimum kept",
    "extremes: new maximum", "extremes: maximum kept",
    "day: reset (first doy) per cell", "day: outside the DEM", "day: DEM cell by isEqual, not by int()", "day: no land unit", "day: unit without crop (BARE or empty id)",
    "day: an extreme is missing", "day: sown crop outside its cycle (increase 0)", "day: sown crop inside its cycle", "day: inside the cycle across the year end",
    "day: outside the cycle, doy before sowing", "day: tmax clipped by the upper threshold", "day: mean below the thermal threshold (increase 0)",
    "day: first degree days (map held the flag)", "day: degree days accumulated",
    "LAI: sown crop before emergence", "LAI: sown crop rising", "LAI: sown crop falling", "LAI: perennial rising", "LAI: perennial falling", "LAI: LAImin (no degree days)",
    "LAI: tree outside leaf fall", "LAI: tree in the 30-day senescence", "LAI: tree after the senescence", "LAI: tree with LAIgrass > 0",
    "degree-day map: LAI from the map", "degree-day map: flag in the map" };
static long arms[A_COUNT];

static std::vector<float> readMap(FILE* f, size_t n) { std::vector<float> v(n); if (fread(v.data(), 4, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

static void laiArms(Crit3DCrop& crop, double dd, double latitude, int doy)
{
    if (crop.isSowingCrop()) {
        if (dd < crop.degreeDaysEmergence) arms[A_L_BEFORE_EMERGENCE]++;
        else if (dd - crop.degreeDaysEmergence <= crop.degreeDaysIncrease) arms[A_L_SOWN_RISING]++;
        else arms[A_L_SOWN_FALLING]++;
        return;
    }
    if (dd > 0) { if (dd <= crop.degreeDaysIncrease) arms[A_L_PERENNIAL_RISING]++; else arms[A_L_PERENNIAL_FALLING]++; }
    else arms[A_L_LAIMIN]++;
    if (crop.type == TREE) {
        const int start = latitude > 0 ? 305 : 120;
        const bool fall = latitude > 0 ? doy >= start : (doy >= start && doy < 182);
        if (!fall) arms[A_L_TREE_NO_LEAF_FALL]++;
        else if (doy - start > 30) arms[A_L_TREE_AFTER_SENESCENCE]++;
        else arms[A_L_TREE_SENESCENCE]++;
        if (crop.LAIgrass > 0) arms[A_L_TREE_GRASS]++;
    }
}

int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    int dims[4]; float fl[2];
    if (!in || !out || fread(dims, 4, 4, in) != 4 || fread(fl, 4, 2, in) != 2) return 2;
    const int nrows = dims[0], ncols = dims[1], nUnits = dims[2], nOps = dims[3];
    const float flag = fl[0], clearSkyIn = fl[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> dem = readMap(in, n);
    std::vector<int> unitIndex(n);
    if (fread(unitIndex.data(), 4, n, in) != n) return 2;
    std::vector<Crit3DCrop> cropList(nUnits);
    std::vector<int> isCrop(nUnits);
    for (int u = 0; u < nUnits; ++u) {
        int iv[4]; double dv[10];
        if (fread(iv, 4, 4, in) != 4 || fread(dv, 8, 10, in) != 10) return 2;
        Crit3DCrop& c = cropList[u];
        c.type = speciesType(iv[0]); isCrop[u] = iv[1]; c.sowingDoy = iv[2]; c.plantCycle = iv[3];
        c.LAImin = dv[0]; c.LAImax = dv[1]; c.LAIgrass = dv[2]; c.LAIcurve_a = dv[3]; c.LAIcurve_b = dv[4];
        c.thermalThreshold = dv[5]; c.upperThermalThreshold = dv[6]; c.degreeDaysIncrease = dv[7]; c.degreeDaysDecrease = dv[8]; c.degreeDaysEmergence = dv[9];
    }
    double latitude = 44.5;
    // initializeCropMaps: the flag everywhere
    std::vector<float> dd(n, flag), lai(n, flag), tmin(n, flag), tmax(n, flag), et0(n, flag);
    std::vector<float>* maps[5] = {&dd, &lai, &tmin, &tmax, &et0};
    for (int op = 0; op < nOps; ++op) {
        int code[3];
        if (fread(code, 4, 3, in) != 3) return 2;
        if (code[0] == 1) {                                                    // one hour: computeET0PMMap, updateDailyTemperatures
            std::vector<float> airT = readMap(in, n), rh = readMap(in, n), wind = readMap(in, n), glob = readMap(in, n), trans = readMap(in, n);
            for (size_t c = 0; c < n; ++c) {
                et0[c] = flag;
                float height = dem[c];
                if (int(height) != int(flag)) {
                    float clearSkyTransmissivity = clearSkyIn;
                    float globalRadiation = glob[c], transmissivity = trans[c], temperature = airT[c], relHumidity = rh[c], windSpeed = wind[c];
                    if (isEqual(globalRadiation, flag)) arms[A_ET0_NO_RAD]++;
                    if (isEqual(transmissivity, flag)) arms[A_ET0_NO_TRANS]++;
                    if (isEqual(temperature, flag)) arms[A_ET0_NO_TEMP]++;
                    if (isEqual(relHumidity, flag)) arms[A_ET0_NO_RH]++;
                    if (isEqual(windSpeed, flag)) arms[A_ET0_NO_WIND]++;
                    if (! isEqual(globalRadiation, flag) && ! isEqual(transmissivity, flag) && ! isEqual(temperature, flag)
                            && ! isEqual(relHumidity, flag) && ! isEqual(windSpeed, flag)) {
                        et0[c] = float(ET0_Penman_hourly(double(height), double(transmissivity / clearSkyTransmissivity),
                                          double(globalRadiation), double(temperature), double(relHumidity), double(windSpeed)));
                        arms[A_ET0_COMPUTED]++;
                        // the arms, from the same inputs
                        const double nt = double(transmissivity / clearSkyTransmissivity);
                        const double cf = 1.35 * MINVALUE(nt, 1) - 0.35;
                        if (nt > 1) arms[A_ET0_TRANS_ABOVE_CLEAR]++;
                        if (0 > cf) arms[A_ET0_CLOUD_ZERO]++; else if (!(nt > 1)) arms[A_ET0_CLOUD_BETWEEN]++;
                        const double es = saturationVaporPressure(temperature) / 1000., ea = relHumidity * es / 100.0;
                        const double lw = MAXVALUE(0, cf) * emissivityFromVaporPressure(ea) * (STEFAN_BOLTZMANN * 3600.) * pow(temperature + ZEROCELSIUS, 4);
                        if ((1 - ALBEDO_CROP_REFERENCE) * (3600 * double(globalRadiation)) - lw > 0) arms[A_ET0_NETRAD_POS]++; else arms[A_ET0_NETRAD_NEG]++;
                        if (et0[c] > 0) arms[A_ET0_POSITIVE]++; else arms[A_ET0_CLIPPED]++;
                    }
                } else { arms[A_ET0_NO_DEM]++; if (!isEqual(height, flag)) arms[A_ET0_DEM_INT_ONLY]++; }
            }
            for (size_t c = 0; c < n; ++c) {
                float t = airT[c];
                if (isEqual(t, flag)) { arms[A_T_NO_AIRT]++; continue; }
                float currentTmin = tmin[c];
                if (isEqual(currentTmin, flag)) arms[A_T_FIRST_MIN]++; else if (t < currentTmin) arms[A_T_MIN_LOWER]++; else arms[A_T_MIN_KEPT]++;
                tmin[c] = isEqual(currentTmin, flag) ? t : std::min(currentTmin, t);
                float currentTmax = tmax[c];
                if (isEqual(currentTmax, flag)) arms[A_T_FIRST_MAX]++; else if (currentTmax < t) arms[A_T_MAX_HIGHER]++; else arms[A_T_MAX_KEPT]++;
                tmax[c] = isEqual(currentTmax, flag) ? t : std::max(currentTmax, t);
            }
        } else if (code[0] == 2) {                                             // dailyUpdateCropMaps(date doy code[1]), current doy code[2]
            int firstDoy = 1;
            if (latitude < 0) firstDoy = 182;
            if (code[1] == firstDoy) { std::fill(lai.begin(), lai.end(), flag); std::fill(dd.begin(), dd.end(), flag); arms[A_D_RESET] += n; }
            int currentDoy = code[2];
            for (size_t c = 0; c < n; ++c) {
                float height = dem[c];
                if (isEqual(height, flag)) { arms[A_D_NO_DEM]++; continue; }
                if (int(height) == int(flag)) arms[A_D_DEM_ISEQUAL_ONLY]++;
                int index = unitIndex[c] < 0 ? NODATA : unitIndex[c];
                if (index == NODATA) { arms[A_D_NO_UNIT]++; continue; }
                if (!isCrop[index]) { arms[A_D_NOT_CROP]++; continue; }
                float tn = tmin[c], tx = tmax[c];
                if (isEqual(tn, flag) || isEqual(tx, flag)) { arms[A_D_NO_EXTREMES]++; continue; }
                Crit3DCrop& crop = cropList[index];
                double dailyDD = crop.getDailyDegreeIncrease(tn, tx, currentDoy);
                if (isEqual(dailyDD, NODATA)) continue;
                if (crop.isSowingCrop()) {
                    const int days = crop.getDaysFromTypicalSowing(currentDoy);
                    if (!crop.isInsideTypicalCycle(currentDoy)) { arms[A_D_OUTSIDE_CYCLE]++; if (days < 0) arms[A_D_OUTSIDE_NEG_BRANCH]++; }
                    else { arms[A_D_INSIDE_CYCLE]++; if (days < 0 || currentDoy - crop.sowingDoy >= 365) arms[A_D_INSIDE_BY_WRAP]++; }
                }
                if (!crop.isSowingCrop() || crop.isInsideTypicalCycle(currentDoy)) {
                    if (double(tx) > crop.upperThermalThreshold) arms[A_D_TMAX_CLIPPED]++;
                    if (dailyDD == 0) arms[A_D_BELOW_THRESHOLD]++;
                }
                if (isEqual(dd[c], flag)) { dd[c] = float(dailyDD); arms[A_D_FIRST_VALUE]++; }
                else { dd[c] += float(dailyDD); arms[A_D_ACCUMULATED]++; }
                lai[c] = crop.computeSimpleLAI(dd[c], latitude, currentDoy);
                laiArms(crop, dd[c], latitude, currentDoy);
            }
            std::fill(tmin.begin(), tmin.end(), flag); std::fill(tmax.begin(), tmax.end(), flag);
        } else if (code[0] == 3) {                                             // a hand-set state map (a resumed run)
            *maps[code[1]] = readMap(in, n);
        } else if (code[0] == 4) {
            for (auto* m : maps) fwrite(m->data(), 4, n, out);
        } else if (code[0] == 5) {                                             // initializeCropFromDegreeDays: a map of the DEM's header, current doy code[1]
            std::vector<float> map = readMap(in, n);
            for (auto* m : maps) std::fill(m->begin(), m->end(), flag);       // initializeCropMaps (the ET0 map: a fresh hour)
            for (size_t c = 0; c < n; ++c) {
                if (isEqual(dem[c], flag)) continue;
                int index = unitIndex[c] < 0 ? NODATA : unitIndex[c];
                if (index == NODATA || !isCrop[index]) continue;
                float currentDegreeDay = map[c];
                if (isEqual(currentDegreeDay, flag)) { arms[A_L_DEGREE_DAY_MAP_FLAG]++; continue; }
                dd[c] = currentDegreeDay;
                lai[c] = cropList[index].computeSimpleLAI(dd[c], latitude, code[1]);
                arms[A_L_FROM_DEGREE_DAY_MAP]++;
                laiArms(cropList[index], dd[c], latitude, code[1]);
            }
        } else if (code[0] == 6) {
            latitude = code[1] / 100.0;
        } else return 3;
    }
    fclose(out);
    printf("{");
    for (int a = 0; a < A_COUNT; ++a) printf("%s\"%s\": %ld", a ? ", " : "", armNames[a], arms[a]);
    printf("}\n");
    return 0;
}
"""


def decode_inputs(codes, flag):
    """int16 codes [H][5][rows][cols] -> float32 maps (code * step; -32768: the flag)"""
    steps = np.asarray(STEPS, np.float32).reshape(1, 5, 1, 1)
    return np.where(codes == -32768, np.float32(flag), codes.astype(np.float32) * steps).astype(np.float32)


def unit_map(dem, flag):
    """the synthetic land-unit index map: vertical stripes of four columns cycling through the units, a block without land use (-1)"""
    idx = (np.arange(NCOLS) // 4 % len(UNITS))[None, :].repeat(NROWS, 0).astype(np.int32)
    idx[12:, :] = np.roll(idx[12:, :], 4, axis=1)
    idx[2:4, 5:11] = -1
    idx[19, :] = -1
    return idx


def calendar(dem, flag, seed=20261017):
    """-> ops [nOps][3] int32, input codes [H][5][rows][cols] int16, hand-set maps [nSet][rows][cols] float32"""
    rng = np.random.default_rng(seed)
    shape = dem.shape
    valid = np.abs(dem.astype(np.float64) - float(flag)) >= 1e-5
    ops, codes, sets = [], [], []
    # a static exposure field, constant on blocks of eight columns, plus a sparse speckle: the compressed fixture stays small
    block = rng.integers(-3, 4, (NROWS, NCOLS // 8)).repeat(8, 1)

    def hour(doy, hod, south=False):
        h = len(codes)
        sun = max(0.0, np.sin(np.pi * (hod - 6) / 12.0))
        season = -np.cos(2 * np.pi * ((doy + (182 if south else 0)) % 365 - 15) / 365.0)          # -1 mid-winter .. 1 mid-summer
        base_t = 11.0 + 11.0 * season + 5.0 * sun - 2.0 * (hod < 6)
        speckle = np.where(rng.random(shape) < 0.05, rng.integers(-1, 2, shape), 0)
        c = np.zeros((5,) + shape, np.int64)
        c[0] = np.round(base_t / STEPS[0]) + block + speckle
        c[1] = np.clip(np.round(70 - 25 * sun) + 3 * block + speckle, 5, 100)
        c[2] = np.maximum(np.round((1.5 + 1.5 * sun) / STEPS[2]) + block + speckle, 0)
        rad = (350.0 + 350.0 * season) * sun
        c[3] = np.maximum(np.round(rad / STEPS[3]) + (block + speckle if sun > 0 else 0), 0)
        trans = 0.55 if (doy % 3) else 0.25
        c[4] = np.maximum(np.round(trans / STEPS[4]) + block // 2 + speckle, 1)
        # the arms of the cloud factor: above clear sky on one row, below 0.26 x clear sky (factor clipped at 0) on another
        c[4][6, :] = 28                                  # 0.875 > 0.75
        c[4][7, :] = 5                                   # 0.156 / 0.75 = 0.208 < 0.259
        c[1][8, :] = 100                                 # saturated air: at night the sum is negative and clips at 0
        c[0][9, 0:16] += 52                              # a hot block: tmax above the upper thermal thresholds in summer
        c[0][10, 0:16] -= 40                             # a cold block: means below the thermal thresholds
        # each input missing somewhere, some hours
        if h % 7 == 3: c[0][11, 8:24] = -32768
        if h % 7 == 4: c[1][12, 8:24] = -32768
        if h % 7 == 5: c[2][13, 8:24] = -32768
        if h % 7 == 6: c[3][14, 8:24] = -32768
        if h % 7 == 0: c[4][15, 8:24] = -32768
        c[0][16, 24:32] = -32768                         # a block that never sees an air temperature: no extremes, no degree days
        for k in range(5):
            c[k][~valid] = -32768
        codes.append(c.astype(np.int16))
        ops.append((OP_HOUR, h, 0))

    def day(doy):
        ops.append((OP_DAY, doy, doy))

    def checkpoint():
        ops.append((OP_CHECKPOINT, 0, 0))

    def set_state(which, values):
        sets.append(np.where(valid, values, flag).astype(np.float32))
        ops.append((OP_SET_STATE, MAPS.index(which), len(sets) - 1))

    q = lambda v: (np.round(np.asarray(v, np.float64) / 4.0) * 4.0)
    # northern hemisphere
    ops.append((OP_LATITUDE, 4450, 0))
    dd0 = q(150.0 + 40.0 * block + 600.0 * (np.arange(NCOLS) >= 16)[None, :])
    dd0[5, :] = flag
    dd0[20, :] = 0.0
    sets.append(np.where(valid, dd0, flag).astype(np.float32))
    ops.append((OP_SET_DEGREE_DAYS, 100, len(sets) - 1))
    checkpoint()
    for doy in (100, 101, 102):
        for hod in range(24):
            hour(doy, hod)
            if doy == 100 and hod in (0, 23):
                checkpoint()
        day(doy)
        checkpoint()
    # autumn: degree days of a whole season by hand (rising and falling parts of every curve), trees before / in / after the senescence
    dd1 = q(500.0 + 90.0 * (block + 3) + 1400.0 * (np.arange(NROWS) % 3)[:, None])
    set_state("degreeDays", dd1)
    for doy in range(300, 341):
        for hod in (3, 9, 14, 20):
            hour(doy, hod)
        if doy == 300:
            checkpoint()                                 # the extremes before the day closes
        day(doy)
        if doy in (300, 304, 305, 306, 320, 335, 336, 340):
            checkpoint()
    # the year end
    for doy in (364, 1, 2):
        for hod in (3, 9, 14, 20):
            hour(doy, hod)
        day(doy)
        checkpoint()
    # southern hemisphere: leaf fall from doy 120 to 181, the reset at 182
    ops.append((OP_LATITUDE, -3500, 0))
    set_state("degreeDays", dd1)
    for doy in (119, 120, 130, 181, 182):
        for hod in (3, 9, 14, 20):
            hour(doy, hod, south=True)
        day(doy)
        if doy != 181:
            checkpoint()
    return np.array(ops, np.int32), np.stack(codes), np.stack(sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    ref = Path(a.reference)
    d = np.load(HERE / "ravone_dem_519x1208.npz")
    flag = np.float32(d["nodata"])
    dem = d["dem"][ROW0:ROW0 + NROWS, COL0:COL0 + NCOLS].astype(np.float32)
    assert dem[1, 9] != flag
    dem[1, 9] = np.float32(-9999.5)                       # int(height) == int(flag) but not isEqual: no ET0, yet a cell of the daily update
    units = unit_map(dem, flag)
    ops, codes, sets = calendar(dem, flag)
    inputs = decode_inputs(codes, flag)
    assert len(codes) <= 400
    agro = ref / "agrolib"
    srcs = [agro / "crop" / "crop.cpp", agro / "crop" / "development.cpp", agro / "crop" / "root.cpp", agro / "soil" / "soil.cpp", agro / "meteo" / "meteo.cpp",
            agro / "mathFunctions" / "physics.cpp", agro / "mathFunctions" / "basicMath.cpp", agro / "crit3dDate" / "crit3dDate.cpp"]
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        inc = [f"-I{agro / sub}" for sub in ("mathFunctions", "meteo", "crit3dDate", "gis", "utilities", "crop", "soil")]
        cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"), *map(str, srcs),
               "-o", str(work / "crop_pin"), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        with open(work / "in.bin", "wb") as f:
            np.array([NROWS, NCOLS, len(UNITS), len(ops)], np.int32).tofile(f)
            np.array([flag, CLEAR_SKY], np.float32).tofile(f)
            dem.tofile(f)
            units.tofile(f)
            for u in UNITS:
                np.array(u[:4], np.int32).tofile(f)
                np.array(u[4:], np.float64).tofile(f)
            for op in ops:
                op.tofile(f)
                if op[0] == OP_HOUR:
                    inputs[op[1]].tofile(f)
                elif op[0] == OP_SET_STATE:
                    sets[op[2]].tofile(f)
                elif op[0] == OP_SET_DEGREE_DAYS:
                    sets[op[2]].tofile(f)
        r = subprocess.run([str(work / "crop_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True, capture_output=True, text=True)
        arms = json.loads(r.stdout)
        ncp = int((ops[:, 0] == OP_CHECKPOINT).sum())
        rec = np.fromfile(work / "out.bin", np.float32).reshape(ncp, 5, NROWS, NCOLS)
        # which pow of the models are calls of the library in this build
        dis = subprocess.run(["objdump", "-d", "--no-show-raw-insn", str(work / "crop_pin")], capture_output=True, text=True, check=True).stdout
        calls = {}
        for fn in ("ET0_Penman_hourly", "pressureFromAltitude", "getLAICriteria", "getLAISenescence"):
            body = re.search(r"<_Z\w*" + fn + r"\w*>:\n(.*?)\n\n", dis, re.S)
            calls[fn] = sorted(set(re.findall(r"call\s+\w+ <(\w+)@plt>", body.group(1)))) if body else None
        print("library calls:", calls)

    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    assert np.isfinite(rec).all(), "a checkpoint holds inf / NaN: change the forcing"
    empty = [k for k, v in arms.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"
    save = dict(dem=dem, flag=flag, clear_sky=np.float32(CLEAR_SKY), unit_index=units, unit_fields=np.array(UNIT_FIELDS), units=np.array(UNITS, np.float64),
                input_codes=codes, input_steps=np.array(STEPS, np.float32), input_names=np.array(INPUT), map_names=np.array(MAPS), ops=ops, set_maps=sets,
                maps=rec, window=np.array([ROW0, COL0, NROWS, NCOLS], np.int32), arm_names=np.array(list(arms)),
                arm_counts=np.array(list(arms.values()), np.int64), library_calls=np.array(json.dumps(calls)))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(codes)} hourly records, {ncp} checkpoints")
    assert OUT.stat().st_size <= (HERE / "snow_brooks.npz").stat().st_size
    return 0


if __name__ == "__main__":
    sys.exit(main())
