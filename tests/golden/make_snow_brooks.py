#!/usr/bin/env python3
"""Generate tests/golden/snow_brooks.npz: the compiled-reference pin of the hourly snow model (Crit3DSnow::computeSnowBrooksModel,
src/snow/snow.cpp, driven per cell as Crit3DProject::computeSnowModel / computeSnowPoint and Crit3DSnowMaps drive it).  Run by hand where
the reference tree is present; no test calls it:

    python tests/golden/make_snow_brooks.py --reference <CRITERIA3D tree>

The driver below is this project's own text: float maps in plain arrays, one Crit3DSnow object reused across the cells of a row-major
loop (the application's loop is `firstprivate(snowPoint)`), the reference's setters / getters and its computeSurfaceEnergy* /
computeInternalEnergy for the initial state.  It is compiled with plain `g++ -O2` together with the reference's src/snow/snow.cpp and
agrolib/meteo/meteo.cpp WHERE THEY LIE into a scratch directory (unused functions of meteo.cpp are dropped at link time), and only data
is recorded: the DEM window, the float32 inputs of 96 hours, the thirteen maps after the checkpoint hours, and the arm table.

Forcing (seeded): hours 1-24 a cold spell with snowfall (all-snow, mixed and rain cells), 25-48 a clear cold night and day, 49-60 rain
on snow, 61-96 a warm melt-out.  Some cells carry flag inputs, some a hand-set SWE with zero ice / liquid (the re-seeding branch), some a
hand-set surface temperature (the soil energy check), some more than 100 mm of surface water (free water: no snow model)."""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "snow_brooks.npz"
ROW0, COL0, NROWS, NCOLS = 8, 280, 24, 32             # window of ravone_dem_519x1208.npz (11.7 % flag cells)
HOURS = 96
CHECKPOINTS = (1, 24, 48, 72, 96)
CLEAR_SKY = 0.75
STATE = ("swe", "ice", "lwc", "internalEnergy", "surfaceEnergy", "surfaceTemp", "age")
OUTPUT = ("snowFall", "snowMelt", "deltaSWE", "sensibleHeat", "latentHeat", "liquid")
INPUT = ("airT", "prec", "relHum", "windInt", "globalRad", "beamRad", "transmissivity", "surfaceWater")

DRIVER = r"""
// driver of the snow pin: see make_snow_brooks.py
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "basicMath.h"
#include "meteo.h"
#include "snow.h"

static std::vector<float> readMap(FILE* f, size_t n) { std::vector<float> v(n); if (fread(v.data(), 4, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char** argv)
{
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    int dims[3]; float fl[2];
    if (!in || !out || fread(dims, 4, 3, in) != 3 || fread(fl, 4, 2, in) != 2) return 2;
    const int nrows = dims[0], ncols = dims[1], hours = dims[2];
    const float flag = fl[0]; const double clearSky = fl[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> dem = readMap(in, n), sweEdit = readMap(in, n), tsEdit = readMap(in, n);
    Crit3DSnow point;                                   // default parameters
    const double skin = point.snowParameters.skinThickness;
    std::vector<float> m[13];
    for (auto& v : m) v.assign(n, flag);
    // initializeSnowMaps + resetSnowModel: SWE 0 on the DEM's cells, surface 5.0, pack 3.4
    const double initPack = 3.4, initSurface = 5.0;
    for (size_t c = 0; c < n; ++c) {
        if (isEqual(dem[c], flag)) continue;
        const float initSWE = 0;
        m[0][c] = initSWE; m[1][c] = initSWE; m[2][c] = 0; m[6][c] = NODATA;
        m[5][c] = float(initSurface);
        m[4][c] = float(initSWE > 0 ? computeSurfaceEnergySnow(initSurface, skin) : computeSurfaceEnergySoil(initSurface, skin));
        m[3][c] = float(computeInternalEnergy(initPack, DEFAULT_BULK_DENSITY, initSWE / 1000.));
        for (int k = 7; k < 12; ++k) m[k][c] = 0;
    }
    for (auto& v : m) fwrite(v.data(), 4, n, out);      // record 0: the initial maps
    for (size_t c = 0; c < n; ++c) if (!isEqual(sweEdit[c], flag)) m[0][c] = sweEdit[c];     // a hand-edited SWE map, no reset
    for (size_t c = 0; c < n; ++c) if (!isEqual(tsEdit[c], flag)) m[5][c] = tsEdit[c];       // a resumed run: surface temperatures of another day
    for (int h = 0; h < hours; ++h) {
        std::vector<float> airT = readMap(in, n), prec = readMap(in, n), rh = readMap(in, n), wind = readMap(in, n), glob = readMap(in, n),
                           beam = readMap(in, n), trans = readMap(in, n), water = readMap(in, n);
        for (size_t c = 0; c < n; ++c) {
            if (isEqual(dem[c], flag)) { for (int k = 0; k < 12; ++k) m[k][c] = flag; m[12][c] = flag; continue; }
            point.setSnowWaterEquivalent(m[0][c]); point.setIceContent(m[1][c]); point.setLiquidWaterContent(m[2][c]);
            point.setInternalEnergy(m[3][c]); point.setSurfaceEnergy(m[4][c]); point.setSnowSurfaceTemp(m[5][c]); point.setAgeOfSnow(m[6][c]);
            double a = airT[c], p = prec[c], r = rh[c], w = wind[c], g = glob[c], b = beam[c], t = trans[c], sw = water[c];
            point.setSnowInputData(a, p, r, w, g, b, t, clearSky, sw);
            point.computeSnowBrooksModel();
            m[0][c] = float(point.getSnowWaterEquivalent()); m[1][c] = float(point.getIceContent()); m[2][c] = float(point.getLiquidWaterContent());
            m[3][c] = float(point.getInternalEnergy()); m[4][c] = float(point.getSurfaceEnergy()); m[5][c] = float(point.getSnowSurfaceTemp());
            m[6][c] = float(point.getAgeOfSnow());
            m[7][c] = float(point.getSnowFall()); m[8][c] = float(point.getSnowMelt()); m[9][c] = float(point.getDeltaSWE());
            m[10][c] = float(point.getSensibleHeat()); m[11][c] = float(point.getLatentHeat());
            // liquid water reaching the soil surface: the float expression of assignPrecipitation
            float pr = prec[c];
            if (isEqual(pr, flag)) { m[12][c] = flag; continue; }
            float liquid = pr;
            if (!isEqual(m[7][c], flag) && !isEqual(m[8][c], flag)) liquid = pr - m[7][c] + m[8][c];
            m[12][c] = liquid;
        }
        for (auto& v : m) fwrite(v.data(), 4, n, out);
    }
    fclose(out);
    printf("{\"snowWaterEquivalent_enum\": %d}\n", int(snowWaterEquivalent));
    return 0;
}
"""


def forcing(dem, flag, seed=20261016):
    """-> inputs [HOURS][8][nrows][ncols] float32, sweEdit, surfaceTempEdit [nrows][ncols] float32 (flag: no edit)"""
    rng = np.random.default_rng(seed)
    shape = dem.shape
    valid = dem != flag
    z = np.where(valid, dem, np.nan)
    dz = np.where(valid, z - np.nanmean(z), 0.0)
    cellT = rng.uniform(-1.5, 1.5, shape) - 0.0065 * dz * 4.0          # a static field: exposure and (exaggerated) lapse rate
    inp = np.zeros((HOURS, 8) + shape, np.float32)
    for h in range(HOURS):
        hod = h % 24
        sun = max(0.0, np.sin(np.pi * (hod - 6) / 12.0))
        if h < 24:      # cold spell with snowfall
            base, prec, trans, rad, wind, rh = 1.5 - 5.0 * h / 23.0, (2.0 if 2 <= h <= 20 else 0.0), 0.2, 150.0, 4.0, 95.0
        elif h < 48:    # clear cold night and day
            base, prec, trans, rad, wind, rh = -6.0 + 5.0 * sun - 2.0 * (hod < 6), 0.0, 0.72, 450.0, 1.0, 55.0
        elif h < 60:    # rain on snow
            base, prec, trans, rad, wind, rh = 4.0, 2.5, 0.15, 100.0, 5.0, 98.0
        else:           # warm melt-out
            base, prec, trans, rad, wind, rh = 7.0 + 7.0 * sun, 0.0, 0.6, 650.0, 3.0, 60.0
        # quantised (1/16 degC, 1/8 mm, 1 %, 1/4 m/s, 1 W m-2, 1/64): the float32 inputs stay small in the compressed fixture
        q = lambda v, step: np.round(np.asarray(v) / step) * step
        inp[h, 0] = q(base + cellT + rng.normal(0, 0.1, shape), 1 / 16)
        inp[h, 1] = q(prec * rng.uniform(0.6, 1.4, shape), 1 / 8) if prec else 0.0
        inp[h, 2] = q(np.clip(rh + rng.normal(0, 4, shape), 5, 100), 1)
        inp[h, 3] = q(np.maximum(wind * rng.uniform(0.0, 2.0, shape), 0.0), 1 / 4)
        g = q(rad * sun * rng.uniform(0.8, 1.0, shape), 1)
        inp[h, 4] = g
        inp[h, 5] = q(g * (0.7 if trans > 0.5 else 0.1), 1)
        inp[h, 6] = q(trans * rng.uniform(0.9, 1.1, shape), 1 / 64)
        inp[h, 7] = 0.0
    # flag inputs: a column without air temperature for three hours, a column without transmissivity, cells without precipitation or
    # radiation, hours with transmissivity above clear sky.  Humidity: the reference does not validate it - tDewFromRelHum answers
    # NODATA for a flag or 0, the vapour density computed from a dew point of -9999 degC puts -6e8 kJ m-2 of latent heat into the cell, its
    # surface temperature leaves the physical range in that hour and the float range (inf, then NaN) two hours later.  The pin has such
    # cells in its last two hours only, so every value compared is finite: the sign and payload of a NaN are the one thing the device
    # routines do not promise (sf3d_glibcmath.inc).
    inp[10:13, 0, :, 5] = flag
    inp[94:96, 2, 3, :] = flag
    inp[94:96, 2, 5, :] = 0.0
    inp[:, 6, :, 11] = flag
    inp[40:44, 6, 7, :] = 0.9
    inp[5:8, 1, 9, 20:30] = flag
    inp[70:73, 4, 10, 20:30] = flag
    inp[74:76, 5, 11, 20:30] = flag
    # surface water: free water (> 100 mm) on one row for the whole run, a shallow pond elsewhere, a negative value (clipped to 0)
    inp[:, 7, 13, :] = 150.0
    inp[20:60, 7, 15, 10:30] = 5.0
    inp[:, 7, 16, 0:8] = -3.0
    # calm and storm: the wind clamps of the aerodynamic resistance
    inp[:, 3, 17, :] = 0.0
    inp[:, 3, 18, :] = 14.0
    for k in range(8):
        inp[:, k][:, ~valid] = flag
    edit = np.full(shape, flag, np.float32)
    edit[20, 8:24] = 30.0          # hand-set SWE, ice and liquid stay 0: re-seeded in the first hour
    edit[21, 8:12] = 0.5           # below SNOW_MINIMUM_HEIGHT
    edit[~valid] = flag
    ts = np.full(shape, flag, np.float32)
    ts[22, 8:16] = -5.0            # snow-free soil far colder than its internal energy says: the soil energy check averages
    ts[22, 16:24] = 6.0            # ... warmer by more than 1000 kJ m-2 but within a factor of 2: it does not
    ts[~valid] = flag
    return inp, edit, ts


def arm_table(dem, flag, inp, rec):
    """how many (cell, hour) pairs reach each arm of the point model, judged from the inputs and the reference's own maps"""
    valid = dem != flag
    eq = lambda a, v=-9999.0: np.abs(a.astype(np.float64) - v) < 1e-5
    arms = {}
    def add(name, mask): arms[name] = arms.get(name, 0) + int(np.count_nonzero(mask & valid))
    for h in range(HOURS):
        before, after = rec[h], rec[h + 1]
        if h == 0:
            before = before.copy()
        swe0, ice0, lw0, ie0, se0, ts0, age0 = (before[k].astype(np.float64) for k in range(7))
        if h == 0:
            swe0 = np.where(eq(EDIT, flag), swe0, EDIT)
            ts0 = np.where(eq(TS_EDIT, flag), ts0, TS_EDIT)
        airT, prec, rh, wind, glob, beam, trans, water = (inp[h, k].astype(np.float64) for k in range(8))
        invalid = eq(airT) | eq(prec) | eq(glob) | eq(beam) | eq(swe0) | eq(ts0)
        freew = np.maximum(water, 0) > 100
        skip = invalid | freew
        add("free water (> 100 mm)", freew)
        add("invalid point", invalid & ~freew)
        run = ~skip
        add("computed", run)
        add("precipitation: all snow", run & (prec > 0) & (airT <= -0.5))
        add("precipitation: mixed", run & (prec > 0) & (airT > -0.5) & (airT < 2))
        add("precipitation: all rain", run & (prec > 0) & (airT >= 2))
        add("dew point: no humidity (flag or 0)", run & (eq(rh) | (rh == 0)))
        add("cloud cover from transmissivity", run & ~eq(trans))
        add("cloud cover default (flag)", run & eq(trans))
        add("transmissivity above clear sky", run & ~eq(trans) & (trans > CLEAR_SKY))
        add("previous SWE > 0", run & (swe0 > 0))
        add("re-seeding a hand-edited SWE", run & (swe0 > 0) & (ice0 <= 0) & (lw0 <= 0))
        seed = (swe0 > 0) & (ice0 <= 0) & (lw0 <= 0)
        ice0s, lw0s = np.where(seed, swe0, ice0), np.where(seed, swe0 * 0.05 / (1 - 0.05), lw0)
        ratio = np.divide(swe0, ice0s + lw0s, out=np.ones_like(swe0), where=(ice0s + lw0s) > 0)
        add("ice + liquid rescaled to SWE", run & (swe0 > 0) & ~(np.abs(ratio - 1) < 1e-5))
        add("no previous snow", run & (swe0 <= 0))
        est = ts0 * 1350 * 1.4 * 0.3
        with np.errstate(invalid='ignore'):
            far = np.abs(est - ie0) > 1000
        add("soil energy check: difference > 1000", run & (swe0 < 1e-5) & far)
        with np.errstate(invalid='ignore'):
            r2 = np.divide(ie0, est, out=np.ones_like(est), where=est != 0)
        add("soil energy check: energy averaged", run & (swe0 < 1e-5) & far & ((r2 < 0.5) | (r2 > 2)))
        add("resistance over snow (SWE > 1 mm)", run & (swe0 > 1))
        add("resistance over vegetation", run & (swe0 <= 1))
        add("wind below 0.05", run & (wind < 0.05))
        add("wind above 10", run & (wind > 10))
        add("albedo by age of snow", run & ~eq(age0) & (swe0 > 0))
        add("albedo of soil", run & (eq(age0) & ~((swe0 > 0) & (ice0 <= 0) & (lw0 <= 0)) | (swe0 <= 0)))
        lat = after[11].astype(np.float64)
        add("vapour flux x 0.4 (no snow)", run & (swe0 < 1e-5))
        add("evaporation limited branch (sublimation < 0)", run & (swe0 > 1e-5) & (lat < 0))
        add("condensation (sublimation >= 0)", run & (swe0 > 1e-5) & (lat >= 0))
        melt = after[8].astype(np.float64)
        add("melt", run & (melt > 0))
        ice1, lw1, swe1, ie1 = after[1].astype(np.float64), after[2].astype(np.float64), after[0].astype(np.float64), after[3].astype(np.float64)
        fall = np.where(eq(after[7]), 0, after[7].astype(np.float64))
        add("refreeze", run & (lw0 > 0) & (ts0 <= 0) & (melt == 0) & (lw1 < lw0) & (ice1 > ice0 + fall))
        add("internal energy > 0: pack gone", run & (ie1 > 1e-5))
        add("liquid capped by holding capacity", run & (ie1 <= 1e-5) & (ice1 > 0) & (np.abs(lw1 - (ice1 * (0.05 / 0.95)).astype(np.float32)) < 1e-6 * np.maximum(lw1, 1)))
        add("snow surface at 0 (internal energy ~ 0)", run & (swe1 > 0) & (np.abs(ie1) < 1e-5))
        age1 = after[6]
        add("age: new snow", run & (swe1 > 1e-5) & (age1 == 0))
        add("age: older", run & (swe1 > 1e-5) & (age1 > 0))
        add("age: no snow", run & (swe1 <= 1e-5))
    return arms


def main():
    global EDIT, TS_EDIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (src/snow, agrolib)")
    ap.add_argument("--keep", help="scratch directory to keep (default: a temporary one)")
    a = ap.parse_args()
    ref = Path(a.reference)
    d = np.load(HERE / "ravone_dem_519x1208.npz")
    flag = np.float32(d["nodata"])
    dem = d["dem"][ROW0:ROW0 + NROWS, COL0:COL0 + NCOLS].astype(np.float32)
    inp, EDIT, TS_EDIT = forcing(dem, flag)
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(a.keep or tmp)
        work.mkdir(parents=True, exist_ok=True)
        (work / "driver.cpp").write_text(DRIVER)
        inc = [f"-I{ref / 'agrolib' / sub}" for sub in ("mathFunctions", "meteo", "crit3dDate", "gis", "utilities")] + [f"-I{ref / 'src' / 'snow'}"]
        cmd = ["g++", "-O2", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", *inc, str(work / "driver.cpp"),
               str(ref / "src" / "snow" / "snow.cpp"), str(ref / "agrolib" / "meteo" / "meteo.cpp"), "-o", str(work / "snow_pin"), "-lm"]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        with open(work / "in.bin", "wb") as f:
            np.array([NROWS, NCOLS, HOURS], np.int32).tofile(f)
            np.array([flag, CLEAR_SKY], np.float32).tofile(f)
            dem.tofile(f)
            EDIT.tofile(f)
            TS_EDIT.tofile(f)
            inp.tofile(f)
        r = subprocess.run([str(work / "snow_pin"), str(work / "in.bin"), str(work / "out.bin")], check=True, capture_output=True, text=True)
        info = json.loads(r.stdout)
        rec = np.fromfile(work / "out.bin", np.float32).reshape(HOURS + 1, 13, NROWS, NCOLS)

    arms = arm_table(dem, flag, inp, rec)
    width = max(map(len, arms))
    for k, v in arms.items():
        print(f"  {k:<{width}} {v:>8}")
    valid = dem != flag
    nv = int(valid.sum())
    # not vacuous, by the reference alone
    snowy = max(int(((rec[h][0] > 0) & valid).sum()) for h in CHECKPOINTS)
    melting = max(int(((rec[h][8] > 0) & valid).sum()) for h in CHECKPOINTS)
    free = int(((rec[HOURS][0] == 0) & valid).sum())
    print(f"valid cells {nv}: SWE > 0 on {snowy}, melt > 0 on {melting}, snow-free at the end {free}")
    assert snowy * 4 >= nv and melting * 10 >= nv and free * 10 >= nv, "vacuous fixture"
    assert all(np.isfinite(rec[h]).all() for h in (0,) + CHECKPOINTS), "a checkpoint holds inf / NaN"
    empty = [k for k, v in arms.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"

    names = STATE + OUTPUT
    save = dict(dem=dem, flag=flag, clear_sky=np.float32(CLEAR_SKY), inputs=inp, swe_edit=EDIT, surface_temp_edit=TS_EDIT, input_names=np.array(INPUT), map_names=np.array(names),
                checkpoints=np.array(CHECKPOINTS, np.int32), initial=rec[0][:12], maps=np.stack([rec[h] for h in CHECKPOINTS]),
                window=np.array([ROW0, COL0, NROWS, NCOLS], np.int32), arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64),
                snow_water_equivalent_enum=np.int32(info["snowWaterEquivalent_enum"]),
                parameters=np.array([0.02, 0.2, 1, 0.05, 2, -0.5, 0.05]))      # initializeSnowParameters, in the order of snow.h
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, enum snowWaterEquivalent = {info['snowWaterEquivalent_enum']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
