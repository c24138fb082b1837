#!/usr/bin/env python3
"""Generate tests/golden/pond_day.npz: the compiled-reference pin of the day's ponds - Project3D::dailyUpdatePond
(src/project3D/project3D.cpp:1819-1843) called as a whole on a constructed Crit3DProject, over Project3D::computeCurrentPond (:1779-1816),
which is also called per cell for the value it returns.  Run by hand where the reference tree and a Qt 5 are present; no test calls it:

    python tests/golden/make_pond_day.py --reference <CRITERIA3D tree> --qt <prefix with include/qt, lib and bin/moc> [--objects DIR]

The driver below is this project's own text.  It constructs the reference's Crit3DProject, fills its public members (DEM, indexMap of the
surface layer, landUseMap, landUnitList with pond and idCrop, cropList with LAImax, laiMap, radiationMaps->slopeMap, processes.computeCrop,
isCriteria3DInitialized), sets up the reference solver (agrolib/soilFluxes3D) with one surface node per cell that has one and a pond of
its own on every node (setNodePond), and calls dailyUpdatePond().  The reference is compiled WHERE IT LIES - the closure
make_soil_cracking.py links.  Only data is recorded: the raster's maps and tables, computeCurrentPond of every cell and getNodePond of every
surface node afterwards, per case (computeCrop on and off).

The raster (7 x 37): flag cells in the index map, in the slope map and in the land use; land units that are crops, one that is BARE and one
without a crop; LAI flag cells; slopes from 0 to 80 degrees.  LAImax > 0 for every crop, so every compared value is finite.  The
restatement (criteria3d_amd/hour.py) must equal the pin bit for bit before the fixture is written."""
import argparse
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from tests.golden import make_soil_cracking as msc  # noqa: E402
from tests.golden import make_water_sinks as mw  # noqa: E402

OUT = HERE / "pond_day.npz"
SHAPE = (7, 37)
FLAG = -9999.0
SLOPE_FLAG = -32768.0          # radiationMaps->slopeMap carries a header of its own
CELL_SIZE = 4.0
# per land unit: id in the land use map, pond [m], idCrop ("" and BARE: not a crop), LAImax
UNITS = ((10, 0.01, "MAIZE", 4.5), (20, 0.004, "BARE", 0.0), (35, 0.02, "GRASS", 3.0), (40, 0.002, "", 0.0), (41, 0.03, "forest", 6.25))
INITIAL_POND = (0.0001, 0.0005, 0.002, 0.005)                 # [m] of the surface nodes before the call

DRIVER = r"""
// driver of the pond pin: see make_pond_day.py
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "gis.h"
#include "crop.h"
#include "landUnit.h"
#include "solarRadiation.h"
#include "soilFluxes3D.h"
#include "project3D.h"
#include "criteria3DProject.h"

template <class T> static void rd(FILE* f, T* p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int dims[5]; float flags[2]; double cellSize;
    rd(in, dims, 5); rd(in, flags, 2); rd(in, &cellSize, 1);
    const int nrows = dims[0], ncols = dims[1], nUnits = dims[2], ns = dims[3], computeCrop = dims[4];
    const float flag = flags[0], slopeFlag = flags[1];
    const size_t n = (size_t)nrows * ncols;
    std::vector<int> index(n), landUse(n); rd(in, index.data(), n); rd(in, landUse.data(), n);
    std::vector<float> slope(n), lai(n); rd(in, slope.data(), n); rd(in, lai.data(), n);
    std::vector<double> pond0(ns); rd(in, pond0.data(), ns);
    Crit3DProject p;
    p.landUnitList.resize(nUnits); p.cropList.resize(nUnits);
    for (int u = 0; u < nUnits; ++u) {
        int id, len; double pond, laiMax; char name[64] = {0};
        rd(in, &id, 1); rd(in, &pond, 1); rd(in, &laiMax, 1); rd(in, &len, 1); if (len > 0) rd(in, name, (size_t)len);
        p.landUnitList[u].id = id; p.landUnitList[u].pond = pond; p.landUnitList[u].idCrop = QString::fromLatin1(name, len);
        p.cropList[u].LAImax = laiMax;
    }
    using namespace soilFluxes3D;
    if (initializeSF3D(ns, ns, 8, true, false, false, heatFluxSaveMode_t::None) != SF3Derror_t::SF3Dok) return 5;
    setSurfaceProperties(0, 0.05);
    for (int i = 0; i < ns; ++i) {
        if (setNode(i, 0., 0., 100. + i, cellSize * cellSize, true, boundaryType_t::NoBoundary) != SF3Derror_t::SF3Dok) return 7;
        setNodeSurface(i, 0);
        if (setNodePond(i, pond0[i]) != SF3Derror_t::SF3Dok) return 8;
    }
    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = cellSize; header.flag = flag; header.llCorner.x = 0; header.llCorner.y = 0;
    gis::Crit3DRasterHeader slopeHeader = header;
    slopeHeader.flag = slopeFlag;
    p.DEM.initializeGrid(header);
    p.landUseMap.initializeGrid(header);
    p.laiMap.initializeGrid(header);
    p.indexMap.resize(1);
    p.indexMap[0].initializeGrid(header);
    p.radiationMaps = new Crit3DRadiationMaps();
    p.radiationMaps->slopeMap->initializeGrid(slopeHeader);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
        const size_t cell = (size_t)r * ncols + c;
        p.DEM.value[r][c] = 100.f;
        p.landUseMap.value[r][c] = landUse[cell] < 0 ? flag : float(landUse[cell]);
        p.laiMap.value[r][c] = lai[cell];
        p.indexMap[0].value[r][c] = index[cell] < 0 ? long(p.indexMap[0].header->flag) : long(index[cell]);
        p.radiationMaps->slopeMap->value[r][c] = slope[cell];
    }
    p.DEM.isLoaded = true; p.landUseMap.isLoaded = true; p.laiMap.isLoaded = true; p.radiationMaps->slopeMap->isLoaded = true;
    p.processes.computeCrop = computeCrop != 0;
    p.isCriteria3DInitialized = true;
    std::vector<float> cellPond(n);
    std::vector<int> unitIndex(n), isCrop(nUnits);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
        cellPond[(size_t)r * ncols + c] = p.computeCurrentPond(r, c);
        unitIndex[(size_t)r * ncols + c] = p.getLandUnitIndexRowCol(r, c);
    }
    for (int u = 0; u < nUnits; ++u) isCrop[u] = p.isCrop(u) ? 1 : 0;
    if (!p.dailyUpdatePond()) return 9;
    std::vector<double> pond(ns);
    for (int i = 0; i < ns; ++i) pond[i] = getNodePond(i);
    fwrite(cellPond.data(), 4, n, out); fwrite(unitIndex.data(), 4, n, out); fwrite(isCrop.data(), 4, nUnits, out); fwrite(pond.data(), 8, ns, out);
    fclose(out);
    return 0;
}
"""


def inputs(seed=20261021):
    rng = np.random.default_rng(seed)
    n = SHAPE[0] * SHAPE[1]
    index = np.full(SHAPE, -1, np.int32)
    has = rng.random(SHAPE) >= 0.08
    has.flat[0], has.flat[n - 1], has[3, 18] = False, True, False
    index[has] = np.arange(int(has.sum()), dtype=np.int32)
    ids = np.array([u[0] for u in UNITS], np.int32)
    land_use = ids[rng.integers(0, len(ids), SHAPE)].astype(np.int32)
    land_use[rng.random(SHAPE) < 0.06] = -1                              # the land use map's flag
    land_use[5, 5] = 99                                                 # an id of no land unit: getLandUnitListIndex answers NODATA
    slope = (np.round(rng.uniform(0.0, 80.0, SHAPE) * 4) / 4).astype(np.float32)
    slope[rng.random(SHAPE) < 0.12] = 0.0
    slope[rng.random(SHAPE) < 0.06] = SLOPE_FLAG
    slope[2, 2] = FLAG                                                  # -9999 is a slope like any other under this header
    lai = (np.round(rng.uniform(0.0, 6.0, SHAPE) * 16) / 16).astype(np.float32)
    lai[rng.random(SHAPE) < 0.1] = FLAG
    # the last lane: a crop on a steep slope with a LAI
    land_use.flat[n - 1], slope.flat[n - 1], lai.flat[n - 1] = 10, np.float32(63.5), np.float32(2.25)
    ns = int(has.sum())
    pond0 = np.array(INITIAL_POND)[np.arange(ns) % len(INITIAL_POND)]
    return index, land_use, slope, lai, pond0


def run_case(work, exe, index, land_use, slope, lai, pond0, compute_crop):
    n = index.size
    with open(work / "in.bin", "wb") as f:
        np.array([SHAPE[0], SHAPE[1], len(UNITS), len(pond0), int(compute_crop)], np.int32).tofile(f)
        np.array([FLAG, SLOPE_FLAG], np.float32).tofile(f)
        np.array([CELL_SIZE], np.float64).tofile(f)
        index.tofile(f); land_use.tofile(f); slope.tofile(f); lai.tofile(f); pond0.astype(np.float64).tofile(f)
        for uid, pond, crop, lai_max in UNITS:
            np.array([uid], np.int32).tofile(f)
            np.array([pond, lai_max], np.float64).tofile(f)
            np.array([len(crop)], np.int32).tofile(f)
            f.write(crop.encode("latin-1"))
    env = {**os.environ, "QT_QPA_PLATFORM": "offscreen", "LD_LIBRARY_PATH": os.pathsep.join(filter(None, [mw.QT_LIB[0], os.environ.get("LD_LIBRARY_PATH")]))}
    subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], check=True, env=env)
    with open(work / "out.bin", "rb") as f:
        cell_pond = np.fromfile(f, np.float32, n).reshape(SHAPE)
        unit_index = np.fromfile(f, np.int32, n).reshape(SHAPE)
        is_crop = np.fromfile(f, np.int32, len(UNITS))
        node_pond = np.fromfile(f, np.float64, len(pond0))
        assert f.read() == b""
    return cell_pond, unit_index, is_crop, node_pond


def main():
    from criteria3d_amd import hour
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree")
    ap.add_argument("--qt", required=True, help="prefix of a Qt 5 installation: <qt>/include/qt, <qt>/lib, <qt>/bin/moc")
    ap.add_argument("--objects", help="directory of the compiled reference objects (kept and reused; default: a temporary one)")
    a = ap.parse_args()
    ref, qt = Path(a.reference), Path(a.qt)
    runtime = Path(subprocess.run(["g++", "-print-file-name=libstdc++.so.6"], check=True, capture_output=True, text=True).stdout.strip()).resolve().parent
    mw.QT_LIB[0] = os.pathsep.join([str(runtime), str(qt / "lib")])
    index, land_use, slope, lai, pond0 = inputs()
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(tmp)
        objects = msc.compile_reference(ref, qt, Path(a.objects) if a.objects else work / "obj")
        (work / "driver.cpp").write_text(DRIVER)
        libs = [str(qt / "lib" / f"libQt5{mod[2:]}.so.5") for mod in mw.QT_MODULES]
        exe = work / "pond_pin"
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-fopenmp", "-w", *msc.include_dirs(ref, qt), str(work / "driver.cpp"), *map(str, objects), *libs,
               "-Wl,--unresolved-symbols=ignore-all", f"-Wl,-rpath-link,{qt / 'lib'}", "-o", str(exe)]
        print("linking", len(objects), "objects")
        subprocess.run(cmd, check=True)
        cases = [run_case(work, exe, index, land_use, slope, lai, pond0, cc) for cc in (True, False)]
    unit_index, is_crop = cases[0][1], cases[0][2]
    assert np.array_equal(unit_index, cases[1][1]) and np.array_equal(is_crop, cases[1][2])
    maximum_pond, lai_max = [u[1] for u in UNITS], [u[3] for u in UNITS]
    bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32)
    arms = {}
    for cc, (cell_pond, _, _, node_pond) in zip((True, False), cases):
        assert np.isfinite(cell_pond).all() and np.isfinite(node_pond).all(), "a compared value is inf / NaN"
        unit = np.where(unit_index == int(FLAG), -1, unit_index)
        want = hour.restate_pond(slope, unit, maximum_pond, lai_max, is_crop, cc, lai, SLOPE_FLAG, FLAG)
        assert np.array_equal(bits(want), bits(cell_pond)), f"computeCrop {cc}: the restatement differs from computeCurrentPond"
        # dailyUpdatePond: the surface node of a cell takes the value unless it is NODATA; the others keep theirs
        expect = pond0.copy()
        set_ = (index >= 0) & (cell_pond != np.float32(FLAG))
        expect[index[set_]] = cell_pond[set_].astype(np.float64)
        assert np.array_equal(expect, node_pond), f"computeCrop {cc}: the node ponds are not what the cell loop says"
        tag = "crop on" if cc else "crop off"
        crop_cell = (unit >= 0) & (np.asarray(is_crop)[np.where(unit >= 0, unit, 0)] != 0)
        computed = cell_pond != np.float32(FLAG)
        arms[f"{tag}: no surface node"] = int(np.count_nonzero(index < 0))
        arms[f"{tag}: slope at its flag"] = int(np.count_nonzero(slope == np.float32(SLOPE_FLAG)))
        arms[f"{tag}: no land unit"] = int(np.count_nonzero((unit < 0) & (slope != np.float32(SLOPE_FLAG))))
        arms[f"{tag}: slope 0"] = int(np.count_nonzero(computed & (slope == 0)))
        arms[f"{tag}: steeper than 60 degrees"] = int(np.count_nonzero(computed & (slope > 60)))
        arms[f"{tag}: crop cell with a LAI"] = int(np.count_nonzero(computed & crop_cell & (lai != np.float32(FLAG))))
        arms[f"{tag}: crop cell, LAI at the flag"] = int(np.count_nonzero(computed & crop_cell & (lai == np.float32(FLAG))))
        arms[f"{tag}: not a crop"] = int(np.count_nonzero(computed & ~crop_cell))
        arms[f"{tag}: node keeps its pond"] = int(np.count_nonzero(node_pond == pond0))
        arms[f"{tag}: node set"] = int(np.count_nonzero(node_pond != pond0))
    for k, v in arms.items():
        print(f"  {k:<40} {v:>5}")
    empty = [k for k, v in arms.items() if v == 0]
    assert not empty, f"arms never reached: {empty}"
    assert not np.array_equal(cases[0][0], cases[1][0])                  # computeCrop changes the day's ponds
    np.savez_compressed(OUT, flag=np.float32(FLAG), slope_flag=np.float32(SLOPE_FLAG), cell_size=np.float64(CELL_SIZE), index=index, land_use=land_use, slope=slope,
                        lai=lai, initial_pond=pond0, unit_ids=np.array([u[0] for u in UNITS], np.int32), maximum_pond=np.array(maximum_pond),
                        lai_max=np.array(lai_max), id_crop=np.array([u[2] for u in UNITS]), unit_index=unit_index, is_crop=is_crop,
                        compute_crop=np.array([1, 0], np.int32), cell_pond=np.stack([c[0] for c in cases]), node_pond=np.stack([c[3] for c in cases]),
                        arm_names=np.array(list(arms)), arm_counts=np.array(list(arms.values()), np.int64))
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
