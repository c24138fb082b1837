#!/usr/bin/env python3
"""Generate tests/golden/water_sinks.npz: the compiled-reference pin of the hourly water sinks - Project3D::initializeEvaporationCoefficient
(src/project3D/project3D.cpp:2331-2368), Project3D::assignEvaporation (:2377-2451) and Project3D::assignTranspiration (:2461-2610) called for
every cell as Crit3DProject::assignETreal does (bin/CRITERIA3D/criteria3DProject.cpp:796-911).  Run by hand where the reference tree and a
Qt 5 are present; no test calls it:

    python tests/golden/make_water_sinks.py --reference <CRITERIA3D tree> --qt <prefix with include/qt, lib and bin/moc> [--objects DIR]

The driver below is this project's own text.  It constructs the reference's Project3D, fills its public members (DEM, indexMap,
soilIndexMap, soilList, layerDepth, layerThickness, nrLayers, computationSoilDepth, hourlyMeteoMaps, waterSinkSource) from the tables
written here, sets up the reference solver (agrolib/soilFluxes3D) with one node per (layer, cell) and the per-node matric potentials, and
calls the three member functions; getCriteria3DVar inside them reads the compiled solver's getNodeWaterContent.  It is linked with the
reference compiled WHERE IT LIES: every translation unit of agrolib (but the file-format and GUI-only folders) and src/project3D by plain
g++ and moc into a scratch directory (--objects keeps / reuses it), with -Wl,--unresolved-symbols=ignore-all because a few units that
are not on the path of these functions (against Qt 5.9.7: utilities.cpp, formTimePeriod.cpp, and soilFluxes3D's gpusolver.cpp and
logFunctions.cpp) do not compile; no stand-in is written for them - a call into a missing symbol would crash the generator.  Only data is recorded.

The raster, land units, soils, layer grid and degree-day maps are those of the root pin (root_density.npz), extended by kcMax, fRAW and one
water-surplus-resistant unit, by water contents per horizon (HH, FC, WP, SAT) and van Genuchten parameters per horizon for the solver.
The node graph is catchment_model(32, 24, 14): the sinks depend on a node's water content only, so its geometry does not matter; the column
table leaves out the flag cells, a few surface nodes and a few nodes inside the root range.  One more case has nrLayers = 1.

The rain term cannot be pinned this way (assignPrecipitation lives in bin/CRITERIA3D): the generator adds it as snow.surface_sources
states it.  The arm table is counted by the restatement (criteria3d_amd/sinks.py) after it has equalled the driver's output bit for bit:
it says which arms the fixture's inputs reach."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from criteria3d_amd import catchment as cm, sinks  # noqa: E402

OUT = HERE / "water_sinks.npz"
COMPUTATION_DEPTH = 0.95
CELL_SIZE = 4.0                                       # the Ravone DEM's
SKIP = ("netcdfHandler", "gdalHandler", "shapeHandler", "shapeUtilities", "criteriaOutput", "importDataset", "inOutDataXML", "graphics", "soilWidget",
        "qcustomplot", "eispack")
QT_LIB = [""]                                         # <qt>/lib, where the driver finds the Qt libraries when it runs
QT_MODULES = ("QtCore", "QtGui", "QtWidgets", "QtSql", "QtXml", "QtCharts", "QtNetwork", "QtPrintSupport")
# per land unit of the root pin: kcMax, fRAW, isWaterSurplusResistant (idCrop == "RICE")
UNIT_EXTRA = ((1.1, 0.55, 0), (1.0, 0.4, 0), (0.9, 0.6, 0), (1.2, 0.7, 0), (1.15, 0.5, 0), (1.05, 0.45, 0), (1.2, 0.2, 1), (0.95, 0.65, 0))
# per soil and horizon of the root pin: van Genuchten alpha [kPa-1], n, he [kPa], thetaR, thetaS, kSat [cm d-1], l (a few USDA classes)
VG = (((0.036, 1.56, 2.0, 0.078, 0.43, 25.0, 0.5), (0.019, 1.31, 4.0, 0.095, 0.41, 6.2, 0.5), (0.008, 1.09, 8.0, 0.068, 0.38, 4.8, 0.5)),
      ((0.075, 1.89, 1.0, 0.065, 0.41, 106.0, 0.5), (0.02, 1.41, 3.0, 0.067, 0.45, 10.8, 0.5)),
      ((0.059, 1.48, 1.5, 0.1, 0.39, 31.4, 0.5), (0.01, 1.23, 6.0, 0.089, 0.43, 1.7, 0.5)),
      ((0.124, 2.28, 0.7, 0.057, 0.41, 350.0, 0.5),),
      ((0.016, 1.37, 5.0, 0.034, 0.46, 6.0, 0.5),))
GRAVITY = 9.80665
PSI = (-800.0, -150.0, -40.0, -12.0, -5.0, -2.0, -0.8, -0.3, -0.1, -0.02, 0.0, 0.05)      # matric potentials [m] of the soil nodes
SURFACE_WATER = (0.0, 0.0001, 0.0004, 0.002, 0.02)                                        # water level [m] of the surface nodes

DRIVER = r"""
// driver of the water-sink pin: see make_water_sinks.py
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "commonConstants.h"
#include "basicMath.h"
#include "gis.h"
#include "soil.h"
#include "crop.h"
#include "root.h"
#include "meteoMaps.h"
#include "soilFluxes3D.h"
#include "project3D.h"

template <class T> static void rd(FILE* f, T* p, size_t n) { if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int dims[9]; float flag; double cellSize, computationDepth;
    rd(in, dims, 9); rd(in, &flag, 1); rd(in, &cellSize, 1); rd(in, &computationDepth, 1);
    const int nrows = dims[0], ncols = dims[1], nUnits = dims[2], nSoils = dims[3], nl = dims[4], nHours = dims[5], N = dims[6], ns = dims[7], nlUsed = dims[8];
    const size_t n = (size_t)nrows * ncols;
    std::vector<float> dem(n); rd(in, dem.data(), n);
    std::vector<int> cropIndex(n), soilIndex(n); rd(in, cropIndex.data(), n); rd(in, soilIndex.data(), n);
    std::vector<double> layerDepth(nl), layerThickness(nl); rd(in, layerDepth.data(), nl); rd(in, layerThickness.data(), nl);
    std::vector<Crit3DCrop> cropList(nUnits);
    for (int u = 0; u < nUnits; ++u) {
        int iv[5]; double dv[6]; rd(in, iv, 5); rd(in, dv, 6);
        Crit3DCrop& c = cropList[u];
        c.roots.rootShape = rootDistributionType(iv[0]); c.roots.growth = rootGrowthType(iv[1]);
        c.type = iv[2] ? TREE : HERBACEOUS_ANNUAL;
        c.roots.degreeDaysRootGrowth = iv[3];
        c.idCrop = iv[4] ? "RICE" : "CROP";
        c.roots.shapeDeformation = dv[0]; c.roots.rootDepthMin = dv[1]; c.roots.rootDepthMax = dv[2]; c.degreeDaysEmergence = dv[3];
        c.kcMax = dv[4]; c.fRAW = dv[5];
        if (c.isWaterSurplusResistant() != (iv[4] != 0) || c.isRootStatic() != (iv[2] != 0)) return 4;
    }
    // the solver: water only
    using namespace soilFluxes3D;
    if (initializeSF3D(N, ns, 8, true, false, false, heatFluxSaveMode_t::None) != SF3Derror_t::SF3Dok) return 5;
    setHydraulicProperties(WRCModel::ModifiedVanGenuchten, meanType_t::Logarithmic, 4.0f);
    setSurfaceProperties(0, 0.05);
    Project3D p;
    p.soilList.resize(nSoils);
    for (int s = 0; s < nSoils; ++s) {
        double td; int nh; rd(in, &td, 1); rd(in, &nh, 1);
        soil::Crit3DSoil& so = p.soilList[s];
        so.totalDepth = td; so.nrHorizons = nh; so.horizon.resize(nh);
        for (int h = 0; h < nh; ++h) {
            double v[14]; rd(in, v, 14);
            soil::Crit3DHorizon& hz = so.horizon[h];
            hz.upperDepth = v[0]; hz.lowerDepth = v[1]; hz.coarseFragments = v[2];
            hz.waterContentHH = v[3]; hz.waterContentFC = v[4]; hz.waterContentWP = v[5]; hz.waterContentSAT = v[6];
            // setSoilProperties(soil, horizon, alpha, n, m, he, thetaR, thetaS, kSat, l, organicMatter, clay)
            if (setSoilProperties(s, h, v[7], v[8], 1. - 1. / v[8], v[9], v[10], v[11], v[12], v[13], 0.01, 0.2) != SF3Derror_t::SF3Dok) return 6;
        }
    }
    std::vector<int> col((size_t)nl * n); rd(in, col.data(), col.size());
    std::vector<double> z(N), psi(N); std::vector<int> nodeSoil(N), nodeHorizon(N);
    rd(in, z.data(), N); rd(in, psi.data(), N); rd(in, nodeSoil.data(), N); rd(in, nodeHorizon.data(), N);
    for (int i = 0; i < N; ++i) {
        const bool surf = i < ns;
        if (setNode(i, 0., 0., z[i], surf ? cellSize * cellSize : cellSize * cellSize * 0.1, surf, boundaryType_t::NoBoundary) != SF3Derror_t::SF3Dok) return 7;
        if (surf) setNodeSurface(i, 0); else setNodeSoil(i, nodeSoil[i], nodeHorizon[i]);
    }
    for (int i = 0; i < N; ++i) if (setNodeMatricPotential(i, psi[i]) != SF3Derror_t::SF3Dok) return 8;
    std::vector<double> vwc(N);
    for (int i = 0; i < N; ++i) vwc[i] = getCriteria3DVar(volumetricWaterContent, i);
    fwrite(vwc.data(), 8, N, out);

    // the members the three functions read
    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = cellSize; header.flag = flag; header.llCorner.x = 0; header.llCorner.y = 0;
    p.DEM.initializeGrid(header);
    p.soilIndexMap.initializeGrid(header);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
        p.DEM.value[r][c] = dem[(size_t)r * ncols + c];
        p.soilIndexMap.value[r][c] = soilIndex[(size_t)r * ncols + c] < 0 ? float(NODATA) : float(soilIndex[(size_t)r * ncols + c]);
    }
    p.DEM.isLoaded = true;
    p.nrLayers = nlUsed;
    p.layerDepth.assign(layerDepth.begin(), layerDepth.begin() + nlUsed); p.layerThickness.assign(layerThickness.begin(), layerThickness.begin() + nlUsed);
    p.computationSoilDepth = computationDepth;
    p.indexMap.resize(nlUsed);
    for (int l = 0; l < nlUsed; ++l) {
        p.indexMap[l].initializeGrid(header);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
            const int v = col[((size_t)l * nrows + r) * ncols + c];
            p.indexMap[l].value[r][c] = v < 0 ? long(p.indexMap[l].header->flag) : long(v);
        }
    }
    p.hourlyMeteoMaps = new Crit3DHourlyMeteoMaps(p.DEM);
    if (!p.initializeEvaporationCoefficient()) return 9;
    { int last = int(p.layerEvapCoeff.size()) - 1; fwrite(&last, 4, 1, out);
      std::vector<double> a(nl, 0.), b(nl, 0.);
      for (int l = 0; l <= last; ++l) { a[l] = p.evapCoeff[l]; b[l] = p.layerEvapCoeff[l]; }
      fwrite(a.data(), 8, nl, out); fwrite(b.data(), 8, nl, out); }
    { std::vector<int> hz((size_t)nSoils * nl);
      for (int s = 0; s < nSoils; ++s) for (int l = 0; l < nl; ++l) hz[(size_t)s * nl + l] = p.soilList[s].getHorizonIndex(layerDepth[l]);
      fwrite(hz.data(), 4, hz.size(), out); }

    std::vector<float> et0(n), lai(n), dd(n);
    std::vector<double> evap(n), transp(n);
    for (int k = 0; k < nHours; ++k) {
        rd(in, et0.data(), n); rd(in, lai.data(), n); rd(in, dd.data(), n);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) p.hourlyMeteoMaps->mapHourlyET0->value[r][c] = et0[(size_t)r * ncols + c];
        p.waterSinkSource.assign(N, 0.);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
            const size_t cell = (size_t)r * ncols + c;
            evap[cell] = transp[cell] = double(flag);
            // the cell loop of assignETreal (criteria3DProject.cpp:805-871)
            long surfaceIndex = p.indexMap.at(0).value[r][c];
            if (surfaceIndex == p.indexMap.at(0).header->flag) continue;
            if (isEqual(dem[cell], flag)) continue;                            // (the application's index map has no node outside the DEM)
            int soil = soilIndex[cell] < 0 ? int(NODATA) : soilIndex[cell];
            float currentLAI = 0;
            if (!isEqual(lai[cell], flag)) currentLAI = lai[cell];
            evap[cell] = p.assignEvaporation(r, c, currentLAI, soil);
            transp[cell] = 0;
            int crop = cropIndex[cell] < 0 ? int(NODATA) : cropIndex[cell];
            if (crop != NODATA && (int)cropList.size() > crop) {
                Crit3DCrop currentCrop = cropList[crop];
                if (currentLAI > 0) transp[cell] = p.assignTranspiration(r, c, currentCrop, currentLAI, dd[cell]);
            }
        }
        fwrite(p.waterSinkSource.data(), 8, N, out); fwrite(evap.data(), 8, n, out); fwrite(transp.data(), 8, n, out);
    }
    fclose(out);
    return 0;
}
"""


def compile_reference(ref: Path, qt: Path, obj: Path):
    """every translation unit the closure of Project3D needs, compiled where it lies; returns the object files that exist afterwards"""
    obj.mkdir(parents=True, exist_ok=True)
    agro = ref / "agrolib"
    dirs = [d for d in sorted(agro.iterdir()) if d.is_dir() and d.name not in SKIP]
    inc = [f"-I{d}" for d in sorted(agro.iterdir()) if d.is_dir()] + [f"-I{ref / 'src' / 'project3D'}", f"-I{agro / 'soilFluxes3D' / 'lineal'}"]
    qinc = [f"-I{qt / 'include' / 'qt'}"] + [f"-I{qt / 'include' / 'qt' / m}" for m in QT_MODULES]
    srcs = [f for d in dirs for f in sorted(d.glob("*.cpp"))] + [agro / "soilFluxes3D" / "lineal" / "linealiaLib.cpp",
                                                                  ref / "src" / "project3D" / "project3D.cpp", ref / "src" / "project3D" / "dialogWaterFluxesSettings.cpp"]
    for d in dirs + [ref / "src" / "project3D"]:
        for h in sorted(d.glob("*.h")):
            if "Q_OBJECT" in h.read_text(errors="replace"):
                moc = obj / f"moc_{d.name}_{h.stem}.cpp"
                if not moc.exists():
                    subprocess.run([str(qt / "bin" / "moc"), *inc, *qinc, str(h), "-o", str(moc)], check=False, capture_output=True)
                if moc.exists():
                    srcs.append(moc)

    def one(src):
        o = obj / f"{src.parent.name}_{src.stem}.o"
        if not o.exists():
            subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-fopenmp", "-w", "-c", str(src), *inc, *qinc, "-o", str(o)], check=False, capture_output=True)
        return o if o.exists() else None
    with ThreadPoolExecutor(8) as pool:
        done = list(pool.map(one, srcs))
    failed = [s.name for s, o in zip(srcs, done) if o is None]
    print(f"reference: {len(srcs) - len(failed)} of {len(srcs)} units compiled; not compiled: {failed}")
    return [o for o in done if o is not None]


def fixture_inputs(rp):
    """the tables and maps of the pin beyond the root pin's"""
    dem, flag = rp["dem"], np.float32(rp["flag"])
    rows, cols = dem.shape
    nl = len(rp["layer_depth"])
    valid = np.abs(dem.astype(np.float64) - float(flag)) >= 1e-5
    m = cm.catchment_model(cols, rows, nl)
    columns = np.asarray(m.meta["index"]).astype(np.int32).copy()          # [layer][row][col]
    columns[:, ~valid] = -1
    columns[0, 3, 10:13] = -1                                              # DEM cells without a surface node
    columns[4, 7, :] = -1                                                  # missing nodes inside the root range
    columns[2, :, 9] = -1
    columns[8, 16:20, 4:12] = -1
    soils = []
    for s, nh in enumerate(rp["soil_nr_horizons"]):
        hz = rp["soil_horizons"][s, :int(nh)]
        so = dict(totalDepth=float(rp["soil_total_depth"][s]), upperDepth=[float(v) for v in hz[:, 0]], lowerDepth=[float(v) for v in hz[:, 1]],
                  coarseFragments=[float(v) for v in hz[:, 2]], soilFraction=[1.0 - float(v) for v in hz[:, 2]], vg=[])
        for name in ("waterContentHH", "waterContentFC", "waterContentWP", "waterContentSAT"):
            so[name] = []
        for h in range(int(nh)):
            a, n_, he, tr, ts, ks, L = VG[s][h]
            fr = so["soilFraction"][h]
            so["vg"].append((a * GRAVITY, n_, he / GRAVITY, tr * fr, ts * fr, ks * 0.01 / 86400.0, L))      # as setCrit3DSoils converts (project3D.cpp:915-925)
            so["waterContentSAT"].append(ts * fr)
            so["waterContentFC"].append((tr + 0.55 * (ts - tr)) * fr)
            so["waterContentWP"].append((tr + 0.18 * (ts - tr)) * fr)
            so["waterContentHH"].append((tr + 0.04 * (ts - tr)) * fr)
        soils.append(so)
    hz_of = sinks.horizon_table(soils, rp["layer_depth"])
    # per node: soil and horizon of its cell and layer (horizon 0 where the layer lies below the soil), potential from a fixed pattern
    L, R, Cc = np.meshgrid(np.arange(nl), np.arange(rows), np.arange(cols), indexing="ij")
    si = np.where(rp["soil_index"] < 0, 0, rp["soil_index"])
    node_soil = np.broadcast_to(si[None], L.shape).ravel().astype(np.int32)
    node_hor = np.where(hz_of[node_soil, L.ravel()] < 0, 0, hz_of[node_soil, L.ravel()]).astype(np.int32)
    psi = np.array(PSI)[(R * 7 + Cc * 3 + L * 5) % len(PSI)].ravel()
    psi[:m.ns] = np.array(SURFACE_WATER)[(R[0] * 3 + Cc[0]) % len(SURFACE_WATER)].ravel()
    r, c = np.mgrid[0:rows, 0:cols]
    hours = []
    for k in range(6):
        et0 = (0.02 + 0.07 * ((r * 2 + c + k) % 9)).astype(np.float32)
        lai = (0.25 * ((r + 2 * c + 3 * k) % 17)).astype(np.float32)
        if k == 0:
            et0[:, 0:4] = 0.0                           # no evaporative demand
            lai[:, 28:] = flag                          # no LAI map value
        if k == 1:
            et0[:, :] = 0.004 + 0.002 * (c % 4)         # tiny demands: the residual falls below EPSILON after the surface term
            lai[:, 10:20] = 8.0                         # closed canopy
        if k == 2:
            et0[:] = np.float32(1.2)                    # a large demand: three iterations
            lai[:] = np.float32(0.3)
        if k == 5:
            et0[6, :] = flag
            lai[:, 0:3] = np.float32(0.000005)          # LAI > 0 and < EPSILON
        liquid = np.where((r + c + k) % 3 == 0, 0.0, 0.4 * ((r * 5 + c + k) % 7)).astype(np.float32)
        liquid[5, :] = flag
        dd = rp["degree_days"][k % len(rp["degree_days"])].copy()
        if k == 5:
            dd[9, :] = np.float32(-9999.0)
        hours.append(dict(et0=np.where(valid, et0, flag).astype(np.float32), lai=np.where(valid, lai, flag).astype(np.float32), dd=dd, liquid=liquid,
                          root=k % len(rp["degree_days"])))
    return m, columns, soils, node_soil, node_hor, psi, hours


def run_case(work, exe, rp, m, columns, soils, node_soil, node_hor, psi, hours, nl_used, computation_depth, units):
    dem, flag = rp["dem"], np.float32(rp["flag"])
    rows, cols = dem.shape
    nl = len(rp["layer_depth"])
    with open(work / "in.bin", "wb") as f:
        np.array([rows, cols, len(units), len(soils), nl, len(hours), m.n, m.ns, nl_used], np.int32).tofile(f)
        np.array([flag], np.float32).tofile(f)
        np.array([CELL_SIZE, computation_depth], np.float64).tofile(f)
        dem.tofile(f)
        rp["crop_index"].astype(np.int32).tofile(f)
        rp["soil_index"].astype(np.int32).tofile(f)
        rp["layer_depth"].tofile(f)
        rp["layer_thickness"].tofile(f)
        for u, (kc, fraw, rice) in zip(rp["units"], UNIT_EXTRA):
            np.array([u[0], u[1], u[2], u[3], rice], np.int32).tofile(f)
            np.array([u[4], u[5], u[6], u[7], kc, fraw], np.float64).tofile(f)
        for so in soils:
            np.array([so["totalDepth"]], np.float64).tofile(f)
            np.array([len(so["upperDepth"])], np.int32).tofile(f)
            for h in range(len(so["upperDepth"])):
                np.array([so["upperDepth"][h], so["lowerDepth"][h], so["coarseFragments"][h], so["waterContentHH"][h], so["waterContentFC"][h],
                          so["waterContentWP"][h], so["waterContentSAT"][h], *so["vg"][h]], np.float64).tofile(f)
        columns.astype(np.int32).tofile(f)
        m.z.astype(np.float64).tofile(f)
        psi.astype(np.float64).tofile(f)
        node_soil.tofile(f)
        node_hor.tofile(f)
        for h in hours:
            h["et0"].tofile(f); h["lai"].tofile(f); h["dd"].tofile(f)
    env = {**os.environ, "QT_QPA_PLATFORM": "offscreen", "LD_LIBRARY_PATH": os.pathsep.join(filter(None, [QT_LIB[0], os.environ.get("LD_LIBRARY_PATH")]))}
    subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], check=True, env=env)
    n = rows * cols
    with open(work / "out.bin", "rb") as f:
        vwc = np.fromfile(f, np.float64, m.n)
        last = int(np.fromfile(f, np.int32, 1)[0])
        ec, lec = np.fromfile(f, np.float64, nl), np.fromfile(f, np.float64, nl)
        hz = np.fromfile(f, np.int32, len(soils) * nl).reshape(len(soils), nl)
        res = []
        for _ in hours:
            res.append(dict(sinks_et=np.fromfile(f, np.float64, m.n), evaporation=np.fromfile(f, np.float64, n).reshape(rows, cols),
                            transpiration=np.fromfile(f, np.float64, n).reshape(rows, cols)))
        assert f.read() == b""
    return vwc, last, ec, lec, hz, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree")
    ap.add_argument("--qt", required=True, help="prefix of a Qt 5 installation: <qt>/include/qt, <qt>/lib, <qt>/bin/moc")
    ap.add_argument("--objects", help="directory of the compiled reference objects (kept and reused; default: a temporary one)")
    a = ap.parse_args()
    ref, qt = Path(a.reference), Path(a.qt)
    # the compiler's own C++ runtime first: a Qt prefix may ship an older libstdc++ that must not shadow it
    runtime = Path(subprocess.run(["g++", "-print-file-name=libstdc++.so.6"], check=True, capture_output=True, text=True).stdout.strip()).resolve().parent
    QT_LIB[0] = os.pathsep.join([str(runtime), str(qt / "lib")])
    z = np.load(HERE / "root_density.npz")
    rp = {k: z[k] for k in z.files}
    m, columns, soils, node_soil, node_hor, psi, hours = fixture_inputs(rp)
    units = [dict(kcMax=kc, fRAW=fr, isWaterSurplusResistant=rice) for kc, fr, rice in UNIT_EXTRA]
    flag = float(rp["flag"])
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(tmp)
        objects = compile_reference(ref, qt, Path(a.objects) if a.objects else work / "obj")
        (work / "driver.cpp").write_text(DRIVER)
        agro = ref / "agrolib"
        inc = [f"-I{d}" for d in sorted(agro.iterdir()) if d.is_dir()] + [f"-I{ref / 'src' / 'project3D'}", f"-I{agro / 'soilFluxes3D' / 'lineal'}"]
        qinc = [f"-I{qt / 'include' / 'qt'}"] + [f"-I{qt / 'include' / 'qt' / mod}" for mod in QT_MODULES]
        libs = [str(qt / "lib" / f"libQt5{mod[2:]}.so.5") for mod in QT_MODULES]
        exe = work / "sink_pin"
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-fopenmp", "-w", *inc, *qinc, str(work / "driver.cpp"), *map(str, objects), *libs, "-Wl,--unresolved-symbols=ignore-all",
               f"-Wl,-rpath-link,{qt / 'lib'}", "-o", str(exe)]
        print("linking", len(objects), "objects")
        subprocess.run(cmd, check=True)
        vwc, last, ec, lec, hz, res = run_case(work, exe, rp, m, columns, soils, node_soil, node_hor, psi, hours, len(rp["layer_depth"]), COMPUTATION_DEPTH, units)
        one_hours = hours[2:4]
        _, last1, _, _, _, res1 = run_case(work, exe, rp, m, columns, soils, node_soil, node_hor, psi, one_hours, 1, 0.0, units)

    # the restatement on the same inputs: the rain term, the arm table, and a first comparison
    arms = {}
    sinks_all = []
    for k, (h, want) in enumerate(zip(hours, res)):
        roots = dict(length=rp["length"][h["root"]], first=rp["first"][h["root"]], last=rp["last"][h["root"]], density=rp["density"][h["root"]])
        got = sinks.restate_sink_hour(rp["dem"], flag, CELL_SIZE, columns, vwc, rp["crop_index"], rp["soil_index"], units, soils, rp["layer_depth"], rp["layer_thickness"],
                                      COMPUTATION_DEPTH, h["et0"], h["lai"], h["dd"], h["liquid"], roots, m.n, arms)
        for name in ("sinks_et", "evaporation", "transpiration"):
            bad = got[name].view(np.uint64) != want[name].view(np.uint64)
            print(f"hour {k} {name}: restatement differs from the compiled reference in {int(bad.sum())} values")
            assert not bad.any(), (k, name)
        sinks_all.append(got["sinks"])                  # the reference's sinks (equal to the bit, asserted above) plus the rain term
    sinks1 = []
    for h, want in zip(one_hours, res1):
        roots = dict(length=rp["length"][h["root"]], first=rp["first"][h["root"]], last=rp["last"][h["root"]], density=rp["density"][h["root"]][:1])
        got = sinks.restate_sink_hour(rp["dem"], flag, CELL_SIZE, columns[:1], vwc, rp["crop_index"], rp["soil_index"], units, soils, rp["layer_depth"][:1],
                                      rp["layer_thickness"][:1], 0.0, h["et0"], h["lai"], h["dd"], h["liquid"], roots, m.n)
        for name in ("sinks_et", "evaporation", "transpiration"):
            assert np.array_equal(got[name].view(np.uint64), want[name].view(np.uint64)), ("one layer", name)
        assert np.all(want["transpiration"][want["transpiration"] != flag] == 0)
        sinks1.append(got["sinks"])
    width = max(map(len, arms))
    for k2, v in sorted(arms.items()):
        print(f"  {k2:<{width}} {v:>8}")
    missing = [a2 for a2 in REQUIRED_ARMS if arms.get(a2, 0) == 0]
    assert not missing, f"arms never reached: {missing}"
    save = dict(cell_size=np.float64(CELL_SIZE), computation_depth=np.float64(COMPUTATION_DEPTH), columns=columns, vwc=vwc, psi=psi, node_soil=node_soil,
                node_horizon=node_hor, unit_extra=np.array(UNIT_EXTRA, np.float64),
                soil_water=np.array([[[so[nm][h] if h < len(so["upperDepth"]) else -9999.0 for nm in ("waterContentHH", "waterContentFC", "waterContentWP", "waterContentSAT")]
                                      for h in range(3)] for so in soils]),
                soil_vg=np.array([[so["vg"][h] if h < len(so["vg"]) else (-9999.0,) * 7 for h in range(3)] for so in soils]),
                et0=np.stack([h["et0"] for h in hours]), lai=np.stack([h["lai"] for h in hours]), degree_days=np.stack([h["dd"] for h in hours]),
                liquid_water=np.stack([h["liquid"] for h in hours]), root_map=np.array([h["root"] for h in hours], np.int32),
                last_evap_layer=np.int32(last), evap_coeff=ec, layer_evap_coeff=lec, horizon=hz,
                sinks_et=np.stack([r["sinks_et"] for r in res]), sinks=np.stack(sinks_all), evaporation=np.stack([r["evaporation"] for r in res]),
                transpiration=np.stack([r["transpiration"] for r in res]),
                one_layer_hours=np.array([2, 3], np.int32), one_layer_last_evap_layer=np.int32(last1), one_layer_sinks_et=np.stack([r["sinks_et"] for r in res1]),
                one_layer_sinks=np.stack(sinks1), one_layer_evaporation=np.stack([r["evaporation"] for r in res1]),
                one_layer_transpiration=np.stack([r["transpiration"] for r in res1]),
                arm_names=np.array(sorted(arms)), arm_counts=np.array([arms[k2] for k2 in sorted(arms)], np.int64))
    for k2, v in save.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), f"{k2} holds inf / NaN"
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(hours)} hours")
    assert OUT.stat().st_size < 1 << 20
    return 0


REQUIRED_ARMS = (
    "evaporation: maxEvaporation < EPSILON", "evaporation: surface flow <= DBL_EPSILON", "evaporation: surface flow > DBL_EPSILON",
    "evaporation: residual < EPSILON", "evaporation: no soil", "evaporation: horizon NODATA", "evaporation: layerEvaporation <= EPSILON",
    "evaporation: layerEvaporation > EPSILON", "evaporation: loop ends after 1 iteration", "evaporation: loop ends after 2 iterations",
    "evaporation: loop ends after 3 iterations",
    "transpiration: no crop or LAI not positive (assignETreal)", "transpiration: LAI < EPSILON or degree days NODATA", "transpiration: no soil",
    "transpiration: maxTranspiration < EPSILON", "transpiration: root length <= 0", "transpiration: empty density row",
    "transpiration: a missing node inside the root range", "transpiration: horizon NODATA", "transpiration: no available water",
    "transpiration: water scarcity", "transpiration: water surplus", "transpiration: normal condition", "transpiration: redistribution off",
    "transpiration: redistribution limited by waterStress", "transpiration: redistribution limited by rootDensityWithoutStress",
    "transpiration: flow <= DBL_EPSILON")

if __name__ == "__main__":
    sys.exit(main())
