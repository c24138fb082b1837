/* part of sf3d_api.cpp (included at its end) - the C entry points of include/sf3d_maps.h: what the caller sets is kept here, on the host,
 * in its own (global) numbering; every map call hands the device the column table in the numbering of the model the device works on
 * (a strip-local model: local indices, other ranks' columns left out) and the geotechnics per soil class. */
#include "sf3d_maps.h"

namespace {

struct MapsHost {
    bool set = false;
    uint32_t nCells = 0, nLayers = 0;
    int32_t maxNode = -1;
    std::vector<int32_t> col;                  /* [nLayers][nCells] global */
    std::vector<double> thick;
    std::vector<double> slope;                 /* [2][nCells] */
    uint64_t colVer = 0, slopeVer = 0;
    std::vector<int32_t> colDev;               /* strip-local model: col in local numbering */
    uint64_t colDevVer = 0, colDevGen = 0;     /* (colVer, LM.gen) it was made from */
    uint64_t colDevVerDev = 0;                 /* its version for the device */
    std::vector<uint8_t> mine;                 /* strips: 1 on the cells this rank computes (mapsOwnedCells) */
    uint64_t mineColVer = 0, mineGen = 0;      /* (colVer, LM.gen) it was made from */
    struct Geo { uint16_t soil, horizon; double cohesion, tanFriction, bulkDensity; };
    std::vector<Geo> geo;
    std::vector<MapGeo> geoClass;
} MP;
uint64_t mapsVersion = 0;                      /* one counter for every version of MP: a value is never reused */

void mapsClear() { MP = MapsHost(); }

const double kMapEpsilon = 0.00001;            /* commonConstants.h:252 */
const double kMapDegToRad = 0.01745329252;     /* commonConstants.h:255 */

/* strips, the one ownership rule of every raster call: a rank computes the cells whose column it owns, and a column goes with its first
 * node in the column table */
bool mapsOwnsCell(size_t c)
{
    int32_t first = -1;
    for (uint32_t l = 0; l < MP.nLayers && first < 0; ++l) first = MP.col[l * MP.nCells + c];
    return first >= 0 && (size_t)first < LM.gpart.owner.size() && LM.gpart.owner[first] == distRank;
}

/* 1 on the cells of an n-cell raster that this rank computes; null (every cell) when the run is not distributed, no column table is set or
 * the raster is not the column table's */
const uint8_t* mapsOwnedCells(size_t n)
{
    if (!(LM.on && MP.set && MP.nCells == n && !LM.gpart.owner.empty())) return nullptr;
    if (MP.mineColVer != MP.colVer || MP.mineGen != LM.gen) {      /* (colVer is never 0 once set) */
        MP.mine.resize(n);
        for (size_t c = 0; c < n; ++c) MP.mine[c] = mapsOwnsCell(c);
        MP.mineColVer = MP.colVer; MP.mineGen = LM.gen;
    }
    return MP.mine.data();
}

/* the column table, the layer thickness and their version for the device, in the numbering of the model the device works on: a rank of a
 * strip-local model fills the cells whose column it owns (local indices there, -1 in every other column) */
void mapsDeviceInput(MapsInput& in)
{
    in.nCells = MP.nCells; in.nLayers = MP.nLayers; in.thick = MP.thick.data();
    if (!LM.on) { in.col = MP.col.data(); in.colVer = MP.colVer; return; }
    if (MP.colDevVer != MP.colVer || MP.colDevGen != LM.gen) {
        const size_t nc = MP.nCells;
        MP.colDev.assign(MP.col.size(), -1);
        for (size_t c = 0; c < nc; ++c) {
            if (!mapsOwnsCell(c)) continue;
            for (uint32_t l = 0; l < MP.nLayers; ++l) {
                const int32_t g = MP.col[l * nc + c];
                if (g >= 0) MP.colDev[l * nc + c] = LM.g2l[g];
            }
        }
        MP.colDevVer = MP.colVer; MP.colDevGen = LM.gen;
        MP.colDevVerDev = ++mapsVersion;
    }
    in.col = MP.colDev.data(); in.colVer = MP.colDevVerDev;
}

/* shared by the entry points of the five raster blocks */
sf3d_error_t rasterFail(const char* what, sf3d_error_t e) { if (e == SF3D_SOLVER_ERROR) fprintf(stderr, "sf3d: %s: %s\n", what, dev().last_error()); return e; }
bool rasterIsFlag(float v, float flag) { return std::fabs(static_cast<double>(v) - static_cast<double>(flag)) < 0.00001; }      /* isEqual(float, float) */
bool rasterShapeOk(uint32_t nrRows, uint32_t nrCols, const float* dem) { return nrRows != 0 && nrCols != 0 && dem && (uint64_t)nrRows * nrCols <= 0x7fffffffull; }
/* block `b` (SN, CR, RT) is initialised on the raster of nrRows x nrCols cells, so a block on that raster may read its maps on the device */
template <class Block> bool rasterFeeds(const Block& b, uint32_t nrRows, uint32_t nrCols) { return b.on && b.nRows == nrRows && b.nCols == nrCols; }

}  // namespace

extern "C" {

sf3d_error_t sf3d_set_output_columns(uint32_t nrCells, uint32_t nrLayers, const int32_t* nodeOfLayerCell, const double* layerThickness)
{
    NEED_INIT_E;
    if (nrCells == 0 || nrLayers == 0 || !nodeOfLayerCell || !layerThickness) return SF3D_PARAMETER_ERROR;
    const size_t n = (size_t)nrCells * nrLayers;
    int32_t mx = -1;
    for (size_t k = 0; k < n; ++k) {
        const int32_t v = nodeOfLayerCell[k];
        if (v < -1 || (v >= 0 && (uint32_t)v >= M.N)) return SF3D_INDEX_ERROR;
        if (v > mx) mx = v;
    }
    MP.col.assign(nodeOfLayerCell, nodeOfLayerCell + n);
    MP.thick.assign(layerThickness, layerThickness + nrLayers);
    MP.nCells = nrCells; MP.nLayers = nrLayers; MP.maxNode = mx;
    MP.colVer = ++mapsVersion;
    MP.set = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_set_horizon_geotechnics(uint16_t soilIndex, uint16_t horizonIndex, double effectiveCohesion, double frictionAngle, double bulkDensity)
{
    /* project3D.cpp:2645-2651: frictionAngle * DEG_TO_RAD, then tan */
    const double tanFriction = std::tan(frictionAngle * kMapDegToRad);
    for (auto& g : MP.geo)
        if (g.soil == soilIndex && g.horizon == horizonIndex) { g.cohesion = effectiveCohesion; g.tanFriction = tanFriction; g.bulkDensity = bulkDensity; return SF3D_OK; }
    MP.geo.push_back(MapsHost::Geo{soilIndex, horizonIndex, effectiveCohesion, tanFriction, bulkDensity});
    return SF3D_OK;
}

sf3d_error_t sf3d_set_cell_slopes(uint32_t nrCells, const float* slopeDegree, int increaseSlope)
{
    if (nrCells == 0 || !slopeDegree) return SF3D_PARAMETER_ERROR;
    MP.slope.resize((size_t)2 * nrCells);
    for (uint32_t c = 0; c < nrCells; ++c) {                 /* project3D.cpp:2638-2650 */
        double slopeDegreeD = double(slopeDegree[c]);
        if (increaseSlope) slopeDegreeD = std::min(slopeDegreeD * 1.5, 89.);
        const double slopeAngle = std::max(slopeDegreeD * kMapDegToRad, kMapEpsilon);
        MP.slope[c] = std::max(kMapEpsilon, std::tan(slopeAngle));
        MP.slope[(size_t)nrCells + c] = std::sin(2 * slopeAngle);
    }
    MP.slopeVer = ++mapsVersion;
    return SF3D_OK;
}

sf3d_error_t sf3d_compute_output_map(int variable, int layer, float flag, float* out)
{
    NEED_INIT_E;
    if (!MP.set) return SF3D_TOPOGRAPHY_ERROR;
    if (MP.maxNode >= 0 && (uint32_t)MP.maxNode >= M.N) return SF3D_TOPOGRAPHY_ERROR;
    const bool fos = variable == 12 || variable == 13;
    if (variable < 0 || variable > 16 || variable == 6 || variable == 7 || variable == 8 || !out) return SF3D_PARAMETER_ERROR;
    if (layer < -1 || (layer >= 0 && (uint32_t)layer >= MP.nLayers)) return SF3D_INDEX_ERROR;
    if (fos && (MP.slope.size() != (size_t)2 * MP.nCells || M.soils.empty())) return SF3D_MISSING_DATA_ERROR;     /* (nothing to compute from) */

    HostModel& D = deviceModel();
    MapsInput in;
    mapsDeviceInput(in);
    if (MP.slope.size() == (size_t)2 * MP.nCells) { in.slope = MP.slope.data(); in.slopeVer = MP.slopeVer; }
    /* geotechnics per soil class (the classes of sf3d_set_soil_properties, through the index table of sf3d_set_node_soil) */
    MP.geoClass.assign(M.soils.size(), MapGeo{0., 0., 0., 0.});
    for (const auto& g : MP.geo)
        if (g.soil < soil1D.size() && g.horizon < soil1D[g.soil].size() && soil1D[g.soil][g.horizon] < M.soils.size())
            MP.geoClass[soil1D[g.soil][g.horizon]] = MapGeo{g.cohesion, g.tanFriction, g.bulkDensity, 1.};
    in.geo = MP.geoClass.data(); in.nGeo = (uint32_t)MP.geoClass.size();

    int miss = 0;
    const sf3d_error_t e = dev().output_map(D, P, in, variable, layer, flag, out, &miss);
    if (e != SF3D_OK) { fprintf(stderr, "sf3d: output map: %s\n", dev().last_error()); return e; }
    return miss ? SF3D_MISSING_DATA_ERROR : SF3D_OK;
}

} /* extern "C" */
