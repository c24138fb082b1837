#!/usr/bin/env python3
"""Generate tests/golden/soil_cracking.npz: the compiled-reference pin of the rain term of the hourly water sinks with soil cracking -
Crit3DProject::assignPrecipitation (bin/CRITERIA3D/criteria3DProject.cpp:914-968) called as a whole on a constructed Crit3DProject, over
Crit3DProject::computeSoilCracking (:978-1123), which is also called per cell for the value it returns.  Run by hand where the reference
tree and a Qt 5 are present; no test calls it:

    python tests/golden/make_soil_cracking.py --reference <CRITERIA3D tree> --qt <prefix with include/qt, lib and bin/moc> [--objects DIR]

The driver below is this project's own text.  It constructs the reference's Crit3DProject, fills its public members (DEM, indexMap,
soilIndexMap, soilList with texture, coarse fragments and organic matter, layerDepth, layerThickness, nrLayers, computationSoilDepth,
hourlyMeteoMaps->mapHourlyPrec, snowMaps' snowfall and snowmelt maps, processes.computeSnow, waterSinkSource), sets up the reference solver
(agrolib/soilFluxes3D) with one node per (layer, cell), per-node matric potentials and per-surface-node ponds (setNodePond), and runs per
hour the cell loop of assignETreal as make_water_sinks.py does (so that crack nodes already carry evaporation and transpiration
subtractions), then assignPrecipitation().  getCriteria3DVar inside reads the compiled solver's getters.  The reference is compiled WHERE
IT LIES, the closure of make_water_sinks.py plus bin/CRITERIA3D/criteria3DProject.cpp and geometry.cpp, src/snow, src/hydrall and
src/rothCplusplus; the link ignores unresolved symbols of units that are not on the path (see make_water_sinks.py).  Only data is recorded.

Recorded from the compiled reference: water content, maximum water content and pond of every node, getSoilLayerIndex(maxDepth) per soil,
and per hour the node sinks after the evaporation / transpiration loop, the node sinks after assignPrecipitation, actual evaporation and
transpiration, and computeSoilCracking's return value per cell.  Resting on the restatement (criteria3d_amd/sinks.py), after it equalled
all of the above bit for bit: maxDepth per soil and the crack-water map (locals of computeSoilCracking that no member exposes), and the
arm table.  The generator refuses to write a fixture with an empty arm.

The raster, land units, layer grid, degree days and node graph are the sink pin's; the soil list has two more soils (a thin fine horizon;
a gap between two fine horizons) on a band of cells without a crop.  One more case has nrLayers = 1 and computationSoilDepth = 0."""
import argparse
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from criteria3d_amd import sinks  # noqa: E402
from tests.golden import make_water_sinks as mw  # noqa: E402

OUT = HERE / "soil_cracking.npz"
COMPUTATION_DEPTH = mw.COMPUTATION_DEPTH
CELL_SIZE = mw.CELL_SIZE
# the two further soils: totalDepth, horizons (upperDepth, lowerDepth, coarseFragments), van Genuchten rows as make_water_sinks.VG
EXTRA_SOILS = ((0.8, ((0.0, 0.15, 0.0), (0.15, 0.8, 0.05)), ((0.008, 1.09, 8.0, 0.068, 0.38, 4.8, 0.5), (0.075, 1.89, 1.0, 0.065, 0.41, 106.0, 0.5))),
               (0.9, ((0.0, 0.3, 0.0), (0.35, 0.9, 0.02)), ((0.036, 1.56, 2.0, 0.078, 0.43, 25.0, 0.5), (0.019, 1.31, 4.0, 0.095, 0.41, 6.2, 0.5))))
# per soil and horizon: clay, silt [%], organicMatter [-] (coarse fragments are the horizon's)
TEXTURE = (((60.0, 30.0, 0.02), (55.0, 20.0, 0.01), (30.0, 30.0, 0.005)),      # fine down to 0.75 m: the crack ends at MAX_CRACKING_DEPTH
           ((48.0, 40.0, 0.02), (15.0, 25.0, 0.01)),                            # a second horizon ends the fine range at 0.4 m
           ((20.0, 40.0, 0.02), (60.0, 30.0, 0.01)),                            # first horizon not fine
           ((70.0, 20.0, 0.03),),                                               # fine, the soil ends at 0.29 m
           ((70.0, 20.0, 0.03),),                                               # 4 cm of soil
           ((65.0, 25.0, 0.02), (10.0, 20.0, 0.01)),                            # fine horizon too thin
           ((58.0, 36.0, 0.02), (52.0, 30.0, 0.01)))                            # fine with a gap at 0.3 - 0.35 m: horizon NODATA inside the range
POND = (0.0001, 0.0005, 0.002, 0.005)                                           # [m] of the surface nodes

DRIVER = r"""
// driver of the soil-cracking pin: see make_soil_cracking.py
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
#include "criteria3DProject.h"

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
    }
    using namespace soilFluxes3D;
    if (initializeSF3D(N, ns, 8, true, false, false, heatFluxSaveMode_t::None) != SF3Derror_t::SF3Dok) return 5;
    setHydraulicProperties(WRCModel::ModifiedVanGenuchten, meanType_t::Logarithmic, 4.0f);
    setSurfaceProperties(0, 0.05);
    Crit3DProject p;
    p.soilList.resize(nSoils);
    std::vector<double> crackDepth(nSoils);
    for (int s = 0; s < nSoils; ++s) {
        double td; int nh; rd(in, &td, 1); rd(in, &nh, 1); rd(in, &crackDepth[s], 1);
        soil::Crit3DSoil& so = p.soilList[s];
        so.totalDepth = td; so.nrHorizons = nh; so.horizon.resize(nh);
        for (int h = 0; h < nh; ++h) {
            double v[17]; rd(in, v, 17);
            soil::Crit3DHorizon& hz = so.horizon[h];
            hz.upperDepth = v[0]; hz.lowerDepth = v[1]; hz.coarseFragments = v[2];
            hz.waterContentHH = v[3]; hz.waterContentFC = v[4]; hz.waterContentWP = v[5]; hz.waterContentSAT = v[6];
            hz.texture.clay = v[14]; hz.texture.silt = v[15]; hz.organicMatter = v[16];
            if (setSoilProperties(s, h, v[7], v[8], 1. - 1. / v[8], v[9], v[10], v[11], v[12], v[13], 0.01, 0.2) != SF3Derror_t::SF3Dok) return 6;
        }
    }
    std::vector<int> col((size_t)nl * n); rd(in, col.data(), col.size());
    std::vector<double> z(N), psi(N), pond(ns); std::vector<int> nodeSoil(N), nodeHorizon(N);
    rd(in, z.data(), N); rd(in, psi.data(), N); rd(in, nodeSoil.data(), N); rd(in, nodeHorizon.data(), N); rd(in, pond.data(), ns);
    for (int i = 0; i < N; ++i) {
        const bool surf = i < ns;
        if (setNode(i, 0., 0., z[i], surf ? cellSize * cellSize : cellSize * cellSize * 0.1, surf, boundaryType_t::NoBoundary) != SF3Derror_t::SF3Dok) return 7;
        if (surf) setNodeSurface(i, 0); else setNodeSoil(i, nodeSoil[i], nodeHorizon[i]);
    }
    for (int i = 0; i < ns; ++i) if (setNodePond(i, pond[i]) != SF3Derror_t::SF3Dok) return 8;
    for (int i = 0; i < N; ++i) if (setNodeMatricPotential(i, psi[i]) != SF3Derror_t::SF3Dok) return 8;
    std::vector<double> var(N);
    for (int i = 0; i < N; ++i) var[i] = getCriteria3DVar(volumetricWaterContent, i);
    fwrite(var.data(), 8, N, out);
    for (int i = 0; i < N; ++i) var[i] = getCriteria3DVar(maxVolumetricWaterContent, i);
    fwrite(var.data(), 8, N, out);
    for (int i = 0; i < N; ++i) var[i] = getCriteria3DVar(surfacePond, i);
    fwrite(var.data(), 8, N, out);

    gis::Crit3DRasterHeader header;
    header.nrRows = nrows; header.nrCols = ncols; header.cellSize = cellSize; header.flag = flag; header.llCorner.x = 0; header.llCorner.y = 0;
    p.DEM.initializeGrid(header);
    p.soilIndexMap.initializeGrid(header);
    for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
        p.DEM.value[r][c] = dem[(size_t)r * ncols + c];
        p.soilIndexMap.value[r][c] = soilIndex[(size_t)r * ncols + c] < 0 ? flag : float(soilIndex[(size_t)r * ncols + c]);
    }
    p.DEM.isLoaded = true; p.soilIndexMap.isLoaded = true;
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
    { std::vector<int> last(nSoils);
      for (int s = 0; s < nSoils; ++s) last[s] = crackDepth[s] == NODATA ? int(NODATA) : p.getSoilLayerIndex(crackDepth[s]);
      fwrite(last.data(), 4, nSoils, out); }
    p.snowMaps.getSnowFallMap()->initializeGrid(header);
    p.snowMaps.getSnowMeltMap()->initializeGrid(header);

    std::vector<float> et0(n), lai(n), dd(n), prec(n), fall(n), melt(n), ret(n);
    std::vector<double> evap(n), transp(n);
    for (int k = 0; k < nHours; ++k) {
        int snow; rd(in, &snow, 1);
        rd(in, et0.data(), n); rd(in, lai.data(), n); rd(in, dd.data(), n); rd(in, prec.data(), n); rd(in, fall.data(), n); rd(in, melt.data(), n);
        p.processes.computeSnow = snow != 0;
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
            const size_t cell = (size_t)r * ncols + c;
            p.hourlyMeteoMaps->mapHourlyET0->value[r][c] = et0[cell];
            p.hourlyMeteoMaps->mapHourlyPrec->value[r][c] = prec[cell];
            p.snowMaps.getSnowFallMap()->value[r][c] = fall[cell];
            p.snowMaps.getSnowMeltMap()->value[r][c] = melt[cell];
        }
        // the value computeSoilCracking returns, cell by cell, on sinks of their own (the function reads none of them)
        p.waterSinkSource.assign(N, 0.);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
            const size_t cell = (size_t)r * ncols + c;
            ret[cell] = flag;
            if (p.indexMap.at(0).value[r][c] == p.indexMap.at(0).header->flag) continue;
            float liquidWater = prec[cell];
            if (!isEqual(prec[cell], flag) && snow && !isEqual(fall[cell], flag) && !isEqual(melt[cell], flag)) liquidWater = prec[cell] - fall[cell] + melt[cell];
            ret[cell] = liquidWater;
            if (!isEqual(prec[cell], flag) && liquidWater > 0) ret[cell] = p.computeSoilCracking(r, c, liquidWater);
        }
        // the hour: the cell loop of assignETreal (criteria3DProject.cpp:805-871), then assignPrecipitation as a whole
        p.waterSinkSource.assign(N, 0.);
        for (int r = 0; r < nrows; ++r) for (int c = 0; c < ncols; ++c) {
            const size_t cell = (size_t)r * ncols + c;
            evap[cell] = transp[cell] = double(flag);
            long surfaceIndex = p.indexMap.at(0).value[r][c];
            if (surfaceIndex == p.indexMap.at(0).header->flag) continue;
            if (isEqual(dem[cell], flag)) continue;
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
        p.assignPrecipitation();
        fwrite(p.waterSinkSource.data(), 8, N, out); fwrite(ret.data(), 4, n, out);
        fwrite(&p.totalPrecipitation, 8, 1, out);
    }
    fclose(out);
    return 0;
}
"""

EXTRA_UNITS = ("bin/CRITERIA3D/criteria3DProject.cpp", "bin/CRITERIA3D/geometry.cpp", "src/snow/snow.cpp", "src/snow/snowMaps.cpp", "src/hydrall/hydrall.cpp",
               "src/rothCplusplus/rothCplusplus.cpp")


def include_dirs(ref: Path, qt: Path):
    agro = ref / "agrolib"
    inc = [f"-I{d}" for d in sorted(agro.iterdir()) if d.is_dir()] + [f"-I{ref / 'src' / d}" for d in ("project3D", "snow", "hydrall", "rothCplusplus")]
    inc += [f"-I{agro / 'soilFluxes3D' / 'lineal'}", f"-I{ref / 'mapGraphics'}", f"-I{ref / 'bin' / 'CRITERIA3D'}"]
    return inc + [f"-I{qt / 'include' / 'qt'}"] + [f"-I{qt / 'include' / 'qt' / m}" for m in mw.QT_MODULES]


def compile_reference(ref: Path, qt: Path, obj: Path):
    """the closure of the sink pin and the units of Crit3DProject"""
    objects = mw.compile_reference(ref, qt, obj)
    for name in EXTRA_UNITS:
        src = ref / name
        o = obj / f"{src.parent.name}_{src.stem}.o"
        if not o.exists():
            subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-fopenmp", "-w", "-c", str(src), *include_dirs(ref, qt), "-o", str(o)], check=True)
        objects.append(o)
    return objects


def fixture_inputs(rp):
    """the sink pin's inputs, two more soils on a band of cells without a crop, a hole at layer 1, drier profiles, ponds and the rain hours"""
    m, columns, soils, _, _, psi, hours = mw.fixture_inputs(rp)
    vg_rows = [list(v) for v in mw.VG]
    for total, hz, vg in EXTRA_SOILS:
        so = dict(totalDepth=total, upperDepth=[h[0] for h in hz], lowerDepth=[h[1] for h in hz], coarseFragments=[h[2] for h in hz],
                  soilFraction=[1.0 - h[2] for h in hz], vg=[], waterContentHH=[], waterContentFC=[], waterContentWP=[], waterContentSAT=[])
        for h, (a, n_, he, tr, ts, ks, L) in enumerate(vg):
            fr = so["soilFraction"][h]
            so["vg"].append((a * mw.GRAVITY, n_, he / mw.GRAVITY, tr * fr, ts * fr, ks * 0.01 / 86400.0, L))
            so["waterContentSAT"].append(ts * fr)
            so["waterContentFC"].append((tr + 0.55 * (ts - tr)) * fr)
            so["waterContentWP"].append((tr + 0.18 * (ts - tr)) * fr)
            so["waterContentHH"].append((tr + 0.04 * (ts - tr)) * fr)
        soils.append(so)
        vg_rows.append(vg)
    crack_soils = [dict(totalDepth=so["totalDepth"], clay=[t[0] for t in tx], silt=[t[1] for t in tx], coarseFragments=list(so["coarseFragments"]),
                        organicMatter=[t[2] for t in tx]) for so, tx in zip(soils, TEXTURE)]
    dem = rp["dem"]
    rows, cols = dem.shape
    nl = len(rp["layer_depth"])
    soil_index, crop_index = rp["soil_index"].copy(), rp["crop_index"].copy()
    soil_index[0:12, 26:28], soil_index[0:12, 28:30] = 5, 6
    crop_index[0:12, 26:30] = -1
    columns[1, 11, 0:16] = -1                                               # a hole at layer 1
    hz_of = sinks.horizon_table(soils, rp["layer_depth"])
    L, R, Cc = np.meshgrid(np.arange(nl), np.arange(rows), np.arange(cols), indexing="ij")
    si = np.where(soil_index < 0, 0, soil_index)
    node_soil = np.broadcast_to(si[None], L.shape).ravel().astype(np.int32)
    node_hor = np.where(hz_of[node_soil, L.ravel()] < 0, 0, hz_of[node_soil, L.ravel()]).astype(np.int32)
    # a third of the cells dry in every layer, a third with dry and moist layers side by side, the others as the sink pin has them
    psi = psi.reshape(nl, rows, cols).copy()
    kind = (R + 2 * Cc) % 3
    dry = np.where(L % 2 == 1, -800.0, -150.0)
    mixed = np.array((-800.0, -0.3, -150.0, -2.0, -40.0))[(R + L) % 5]
    psi[1:] = np.where(kind[1:] == 0, dry[1:], np.where(kind[1:] == 1, mixed[1:], psi[1:]))
    psi = psi.ravel()
    pond = np.array(POND)[(R[0] * 5 + Cc[0]) % len(POND)].ravel()
    flag = np.float32(rp["flag"])
    r, c = np.mgrid[0:rows, 0:cols]
    out = []
    for k in range(4):
        h = hours[k]
        prec = (np.float32(0.4) * ((r * 5 + c + k) % 7).astype(np.float32), np.float32(5.0) + np.float32(6.0) * ((r + c) % 8).astype(np.float32),
                np.float32(1.0) + np.float32(1.1) * ((r * 3 + c) % 11).astype(np.float32), np.full((rows, cols), 60.0, np.float32))[k].astype(np.float32)
        prec[5, :] = flag
        fall, melt = np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.float32)
        snow = k in (1, 2)
        if snow:
            fall[(r + c) % 5 == 0] = np.float32(2.5)
            fall[(r * 2 + c) % 13 == 0] = np.float32(80.0)                   # more snowfall than precipitation: liquidWater <= 0
            melt[(r + 3 * c) % 4 == 0] = np.float32(0.7)
            fall[8, 0:10] = flag
            melt[9, 0:10] = flag
        liquid = prec.copy()
        if snow:
            both = (prec != flag) & (fall != flag) & (melt != flag)
            liquid[both] = (prec[both] - fall[both]) + melt[both]           # float arithmetic, left to right
        out.append(dict(et0=h["et0"], lai=h["lai"], dd=h["dd"], root=h["root"], snow=snow, prec=prec, fall=fall, melt=melt, liquid=liquid))
    return m, columns, soils, crack_soils, vg_rows, soil_index, crop_index, node_soil, node_hor, psi, pond, out


def run_case(work, exe, rp, m, columns, soils, crack_soils, soil_index, crop_index, node_soil, node_hor, psi, pond, hours, nl_used, computation_depth, max_depth):
    dem, flag = rp["dem"], np.float32(rp["flag"])
    rows, cols = dem.shape
    nl = len(rp["layer_depth"])
    with open(work / "in.bin", "wb") as f:
        np.array([rows, cols, len(mw.UNIT_EXTRA), len(soils), nl, len(hours), m.n, m.ns, nl_used], np.int32).tofile(f)
        np.array([flag], np.float32).tofile(f)
        np.array([CELL_SIZE, computation_depth], np.float64).tofile(f)
        dem.tofile(f)
        crop_index.astype(np.int32).tofile(f)
        soil_index.astype(np.int32).tofile(f)
        rp["layer_depth"].tofile(f)
        rp["layer_thickness"].tofile(f)
        for u, (kc, fraw, rice) in zip(rp["units"], mw.UNIT_EXTRA):
            np.array([u[0], u[1], u[2], u[3], rice], np.int32).tofile(f)
            np.array([u[4], u[5], u[6], u[7], kc, fraw], np.float64).tofile(f)
        for s, (so, cs) in enumerate(zip(soils, crack_soils)):
            np.array([so["totalDepth"]], np.float64).tofile(f)
            np.array([len(so["upperDepth"])], np.int32).tofile(f)
            np.array([max_depth[s]], np.float64).tofile(f)
            for h in range(len(so["upperDepth"])):
                np.array([so["upperDepth"][h], so["lowerDepth"][h], so["coarseFragments"][h], so["waterContentHH"][h], so["waterContentFC"][h],
                          so["waterContentWP"][h], so["waterContentSAT"][h], *so["vg"][h], cs["clay"][h], cs["silt"][h], cs["organicMatter"][h]], np.float64).tofile(f)
        columns.astype(np.int32).tofile(f)
        m.z.astype(np.float64).tofile(f)
        psi.astype(np.float64).tofile(f)
        node_soil.tofile(f)
        node_hor.tofile(f)
        pond.astype(np.float64).tofile(f)
        for h in hours:
            np.array([int(h["snow"])], np.int32).tofile(f)
            for name in ("et0", "lai", "dd", "prec", "fall", "melt"):
                h[name].astype(np.float32).tofile(f)
    env = {**os.environ, "QT_QPA_PLATFORM": "offscreen", "LD_LIBRARY_PATH": os.pathsep.join(filter(None, [mw.QT_LIB[0], os.environ.get("LD_LIBRARY_PATH")]))}
    subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], check=True, env=env)
    n = rows * cols
    with open(work / "out.bin", "rb") as f:
        vwc, max_vwc, pond_mm = (np.fromfile(f, np.float64, m.n) for _ in range(3))
        last_layer = np.fromfile(f, np.int32, len(soils))
        res = []
        for _ in hours:
            res.append(dict(sinks_et=np.fromfile(f, np.float64, m.n), evaporation=np.fromfile(f, np.float64, n).reshape(rows, cols),
                            transpiration=np.fromfile(f, np.float64, n).reshape(rows, cols), sinks=np.fromfile(f, np.float64, m.n),
                            prec_surface_water=np.fromfile(f, np.float32, n).reshape(rows, cols), total_precipitation=np.fromfile(f, np.float64, 1)[0]))
        assert f.read() == b""
    return vwc, max_vwc, pond_mm, last_layer, res


REQUIRED_ARMS = (
    "crack: no soil index", "crack: precipitation <= minimumPond", "crack: soilDepth <= 0.2 by totalDepth", "crack: soilDepth <= 0.2 by computationSoilDepth",
    "crack: first horizon not fine", "crack: fine horizon too thin", "crack: a second horizon ends the fine range", "crack: fine down to MAX_CRACKING_DEPTH",
    "crack: hole at layer 1", "crack: crackDepth == 0", "crack: a hole inside the range", "crack: horizon NODATA inside the range", "crack: avgVoidVolume <= 0.15",
    "crack: crackRatio inside (0, 1)", "crack: crackRatio clamped to 1", "crack: surfaceWater raised to minimumPond",
    "crack: storage capped in one layer and below the cap in another", "crack: rain used up before layer 1", "crack: residual left after layer 1",
    "crack: liquidWater <= 0", "crack: liquidWater at the flag", "crack: snowfall or snowmelt at the flag", "crack: liquidWater changed by snow",
    "crack: a filled layer already carries a subtraction")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree")
    ap.add_argument("--qt", required=True, help="prefix of a Qt 5 installation: <qt>/include/qt, <qt>/lib, <qt>/bin/moc")
    ap.add_argument("--objects", help="directory of the compiled reference objects (kept and reused; default: a temporary one)")
    a = ap.parse_args()
    ref, qt = Path(a.reference), Path(a.qt)
    runtime = Path(subprocess.run(["g++", "-print-file-name=libstdc++.so.6"], check=True, capture_output=True, text=True).stdout.strip()).resolve().parent
    mw.QT_LIB[0] = os.pathsep.join([str(runtime), str(qt / "lib")])
    z = np.load(HERE / "root_density.npz")
    rp = {k: z[k] for k in z.files}
    m, columns, soils, crack_soils, vg_rows, soil_index, crop_index, node_soil, node_hor, psi, pond, hours = fixture_inputs(rp)
    units = [dict(kcMax=kc, fRAW=fr, isWaterSurplusResistant=rice) for kc, fr, rice in mw.UNIT_EXTRA]
    flag = float(rp["flag"])
    nl = len(rp["layer_depth"])
    max_depth, last_layer_restated = sinks.crack_tables(soils, crack_soils, rp["layer_depth"], rp["layer_thickness"], COMPUTATION_DEPTH)
    max_depth1, last_layer1_restated = sinks.crack_tables(soils, crack_soils, rp["layer_depth"][:1], rp["layer_thickness"][:1], 0.0)
    with tempfile.TemporaryDirectory() as tmp:
        work = Path(tmp)
        objects = compile_reference(ref, qt, Path(a.objects) if a.objects else work / "obj")
        (work / "driver.cpp").write_text(DRIVER)
        libs = [str(qt / "lib" / f"libQt5{mod[2:]}.so.5") for mod in mw.QT_MODULES]
        exe = work / "crack_pin"
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-fopenmp", "-w", *include_dirs(ref, qt), str(work / "driver.cpp"), *map(str, objects), *libs,
               "-Wl,--unresolved-symbols=ignore-all", f"-Wl,-rpath-link,{qt / 'lib'}", "-o", str(exe)]
        print("linking", len(objects), "objects")
        subprocess.run(cmd, check=True)
        common = (rp, m, columns, soils, crack_soils, soil_index, crop_index, node_soil, node_hor, psi, pond)
        vwc, max_vwc, pond_mm, last_layer, res = run_case(work, exe, *common, hours, nl, COMPUTATION_DEPTH, max_depth)
        one_hours = hours[1:3]
        _, _, _, last_layer1, res1 = run_case(work, exe, *common, one_hours, 1, 0.0, max_depth1)
    assert np.array_equal(last_layer, last_layer_restated), (last_layer, last_layer_restated)
    assert np.array_equal(last_layer1, last_layer1_restated)

    arms = {}
    cracking = dict(crack_soils=crack_soils, max_vwc=max_vwc, pond=pond_mm)
    crack_water, crack_water1 = [], []

    def compare(tag, got, want):
        for name in ("sinks_et", "evaporation", "transpiration", "sinks"):
            bad = got[name].view(np.uint64) != want[name].view(np.uint64)
            print(f"{tag} {name}: restatement differs from the compiled reference in {int(bad.sum())} values")
            assert not bad.any(), (tag, name)
        bad = got["prec_surface_water"].view(np.uint32) != want["prec_surface_water"].view(np.uint32)
        print(f"{tag} prec_surface_water: restatement differs from the compiled reference in {int(bad.sum())} values")
        assert not bad.any(), tag

    for k, (h, want) in enumerate(zip(hours, res)):
        roots = dict(length=rp["length"][h["root"]], first=rp["first"][h["root"]], last=rp["last"][h["root"]], density=rp["density"][h["root"]])
        got = sinks.restate_sink_hour(rp["dem"], flag, CELL_SIZE, columns, vwc, crop_index, soil_index, units, soils, rp["layer_depth"], rp["layer_thickness"],
                                      COMPUTATION_DEPTH, h["et0"], h["lai"], h["dd"], h["liquid"], roots, m.n, arms, cracking)
        compare(f"hour {k}", got, want)
        crack_water.append(got["crack_water"])
        # the arms of assignPrecipitation's own lines (:939-953)
        computed = got["evaporation"] != flag
        fl = np.float32(flag)
        arms["crack: snowfall or snowmelt at the flag"] = arms.get("crack: snowfall or snowmelt at the flag", 0) + int(
            np.count_nonzero(computed & h["snow"] & (h["prec"] != fl) & ((h["fall"] == fl) | (h["melt"] == fl))))
        arms["crack: liquidWater changed by snow"] = arms.get("crack: liquidWater changed by snow", 0) + int(
            np.count_nonzero(computed & (h["prec"] != fl) & (h["liquid"] != h["prec"])))
    arms1 = {}
    for k, (h, want) in enumerate(zip(one_hours, res1)):
        roots = dict(length=rp["length"][h["root"]], first=rp["first"][h["root"]], last=rp["last"][h["root"]], density=rp["density"][h["root"]][:1])
        got = sinks.restate_sink_hour(rp["dem"], flag, CELL_SIZE, columns[:1], vwc, crop_index, soil_index, units, soils, rp["layer_depth"][:1],
                                      rp["layer_thickness"][:1], 0.0, h["et0"], h["lai"], h["dd"], h["liquid"], roots, m.n, arms1, cracking)
        compare(f"one layer, hour {k}", got, want)
        crack_water1.append(got["crack_water"])
    arms["crack: soilDepth <= 0.2 by computationSoilDepth"] = arms1.get("crack: soilDepth <= 0.2 by computationSoilDepth", 0)
    width = max(map(len, arms))
    for k2, v in sorted(arms.items()):
        if k2.startswith("crack"):
            print(f"  {k2:<{width}} {v:>8}")
    missing = [a2 for a2 in REQUIRED_ARMS if arms.get(a2, 0) == 0]
    assert not missing, f"arms never reached: {missing}"
    names = sorted(k2 for k2 in arms if k2.startswith("crack"))
    nh = max(len(so["upperDepth"]) for so in soils)
    pad = lambda rows_, width_: [list(r_) + [-9999.0] * (width_ - len(r_)) for r_ in rows_]
    save = dict(cell_size=np.float64(CELL_SIZE), computation_depth=np.float64(COMPUTATION_DEPTH), columns=columns, soil_index=soil_index.astype(np.int32),
                crop_index=crop_index.astype(np.int32), psi=psi, pond=pond, node_soil=node_soil, node_horizon=node_hor,
                vwc=vwc, max_vwc=max_vwc, pond_mm=pond_mm, unit_extra=np.array(mw.UNIT_EXTRA, np.float64),
                soil_nr_horizons=np.array([len(so["upperDepth"]) for so in soils], np.int32), soil_total_depth=np.array([so["totalDepth"] for so in soils]),
                soil_horizons=np.array([[[so["upperDepth"][h], so["lowerDepth"][h], so["coarseFragments"][h]] if h < len(so["upperDepth"]) else [-9999.0] * 3
                                         for h in range(nh)] for so in soils]),
                soil_water=np.array([[[so[nm][h] if h < len(so["upperDepth"]) else -9999.0 for nm in ("waterContentHH", "waterContentFC", "waterContentWP", "waterContentSAT")]
                                      for h in range(nh)] for so in soils]),
                soil_vg=np.array([[so["vg"][h] if h < len(so["vg"]) else (-9999.0,) * 7 for h in range(nh)] for so in soils]),
                soil_texture=np.array([pad([[cs["clay"][h], cs["silt"][h], cs["organicMatter"][h]] for h in range(len(cs["clay"]))], 3)
                                       + [[-9999.0] * 3] * (nh - len(cs["clay"])) for cs in crack_soils]),
                et0=np.stack([h["et0"] for h in hours]), lai=np.stack([h["lai"] for h in hours]), degree_days=np.stack([h["dd"] for h in hours]),
                root_map=np.array([h["root"] for h in hours], np.int32), snow=np.array([h["snow"] for h in hours], np.int32),
                precipitation=np.stack([h["prec"] for h in hours]), snow_fall=np.stack([h["fall"] for h in hours]), snow_melt=np.stack([h["melt"] for h in hours]),
                liquid_water=np.stack([h["liquid"] for h in hours]),
                crack_max_depth=max_depth, crack_last_layer=last_layer, one_layer_crack_max_depth=max_depth1, one_layer_crack_last_layer=last_layer1,
                sinks_et=np.stack([r["sinks_et"] for r in res]), sinks=np.stack([r["sinks"] for r in res]), evaporation=np.stack([r["evaporation"] for r in res]),
                transpiration=np.stack([r["transpiration"] for r in res]), prec_surface_water=np.stack([r["prec_surface_water"] for r in res]),
                crack_water=np.stack(crack_water), total_precipitation=np.array([r["total_precipitation"] for r in res]),
                one_layer_hours=np.array([1, 2], np.int32), one_layer_sinks=np.stack([r["sinks"] for r in res1]),
                one_layer_evaporation=np.stack([r["evaporation"] for r in res1]), one_layer_transpiration=np.stack([r["transpiration"] for r in res1]),
                one_layer_prec_surface_water=np.stack([r["prec_surface_water"] for r in res1]), one_layer_crack_water=np.stack(crack_water1),
                arm_names=np.array(names), arm_counts=np.array([arms[k2] for k2 in names], np.int64))
    for k2, v in save.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), f"{k2} holds inf / NaN"
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(hours)} hours")
    assert OUT.stat().st_size < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
