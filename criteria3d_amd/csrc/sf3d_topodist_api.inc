/* part of sf3d_api.cpp (included after sf3d_meteo_api.inc, whose raster and call checks it uses) - the C entry points of
 * include/sf3d_topodist.h.  The host keeps which maps are held, bounds every walk before any device work (a point farther than
 * SF3D_TOPODIST_MAX_STEPS cell sizes from the farthest corner of the raster is refused) and decides whether the variable is a TD
 * variable; the walks, the look-ups and the interpolation live on the device (sf3d_topodist.inc). */
#include "sf3d_topodist.h"

static_assert(SF3D_TOPODIST_MAX_STEPS == TOPODIST_MAX_STEPS, "sf3d_topodist.h and sf3d_device.h disagree");

namespace {

struct TopoHost {
    std::vector<uint8_t> held;          /* per map of the last sf3d_topodist_compute: 1 held, 0 dropped */
} TD;

void topoHostClear() { TD = TopoHost(); }

/* needs no raster: checked first, as the caps are */
bool topoFinite(uint32_t n, const double* x, const double* y, const double* z)
{
    for (uint32_t k = 0; k < n; ++k)
        if (!std::isfinite(x[k]) || !std::isfinite(y[k]) || !std::isfinite(z[k])) return false;
    return true;
}

/* no cell centre farther than the cap in steps: the farthest corner bounds every cell centre (two steps of slack for the float
 * arithmetic of the walk) */
bool topoPointsOk(uint32_t n, const double* x, const double* y)
{
    const double x0 = MT.xll, y0 = MT.yll, x1 = MT.xll + MT.nCols * MT.cellSize, y1 = MT.yll + MT.nRows * MT.cellSize;
    for (uint32_t k = 0; k < n; ++k) {
        const double dx = std::max(std::fabs(x[k] - x0), std::fabs(x[k] - x1)), dy = std::max(std::fabs(y[k] - y0), std::fabs(y[k] - y1));
        if (!(std::sqrt(dx * dx + dy * dy) / MT.cellSize + 2. <= (double)SF3D_TOPODIST_MAX_STEPS)) return false;
    }
    return true;
}

/* every index is -1 or a held map */
bool topoIndicesOk(uint32_t n, const int32_t* mapIndex)
{
    for (uint32_t k = 0; mapIndex && k < n; ++k) {
        if (mapIndex[k] == -1) continue;
        if (mapIndex[k] < 0 || (size_t)mapIndex[k] >= TD.held.size() || !TD.held[(size_t)mapIndex[k]]) return false;
    }
    return true;
}

/* getUseTdVar, interpolation.cpp:1220-1234, among the block's variables */
bool topoVariable(int variable)
{
    return variable != SF3D_METEO_PRECIPITATION && variable != SF3D_METEO_GLOBAL_IRRADIANCE && variable != SF3D_METEO_ATM_TRANSMISSIVITY;
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_topodist_compute(uint32_t nPoints, const double* x, const double* y, const double* z)
{
    if (nPoints > SF3D_METEO_MAX_STATIONS || (nPoints > 0 && (!x || !y || !z)) || !topoFinite(nPoints, x, y, z)) return SF3D_PARAMETER_ERROR;
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!topoPointsOk(nPoints, x, y)) return SF3D_PARAMETER_ERROR;
    TD.held.clear();
    const sf3d_error_t e = rasterFail("topodist compute", dev().topo_compute(nPoints, x, y, z, mapsOwnedCells((size_t)MT.nRows * MT.nCols)));
    if (e != SF3D_OK) { (void)dev().topo_free(); return e; }
    TD.held.assign(nPoints, 1);
    return SF3D_OK;
}

uint64_t sf3d_topodist_bytes(void) { return MT.on ? (uint64_t)TD.held.size() * MT.nRows * MT.nCols * sizeof(float) : 0; }

sf3d_error_t sf3d_topodist_get_map(uint32_t index, uint32_t nrCells, float* map)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != MT.nRows * MT.nCols || index >= TD.held.size() || !TD.held[index]) return SF3D_PARAMETER_ERROR;
    return rasterFail("topodist get map", dev().topo_download(index, map));
}

sf3d_error_t sf3d_topodist_set_map(uint32_t index, uint32_t nrCells, const float* map)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != MT.nRows * MT.nCols || index >= TD.held.size()) return SF3D_PARAMETER_ERROR;
    const sf3d_error_t e = rasterFail("topodist set map", dev().topo_upload(index, map));
    if (e == SF3D_OK) TD.held[index] = 1;
    return e;
}

sf3d_error_t sf3d_topodist_drop_map(uint32_t index)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (index >= TD.held.size()) return SF3D_PARAMETER_ERROR;
    TD.held[index] = 0;
    return SF3D_OK;
}

sf3d_error_t sf3d_topodist_interpolate(int variable, int method, uint32_t nStations, const double* x, const double* y, const double* z, const float* value,
                                       const int32_t* mapIndex, float boundingBoxArea, const sf3d_meteo_settings_t* settings, int kh, float* out)
{
    if (kh < 0 || nStations > SF3D_METEO_MAX_STATIONS || (nStations > 0 && (!x || !y || !z)) || !topoFinite(nStations, x, y, z)) return SF3D_PARAMETER_ERROR;
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, settings, true, call);
    if (e != SF3D_OK) return e;
    if (!topoPointsOk(nStations, x, y) || !topoIndicesOk(nStations, mapIndex)) return SF3D_PARAMETER_ERROR;
    /* no map index handed in: no station carries a map */
    const std::vector<int32_t> none(mapIndex ? 0 : nStations, -1);
    TopoCall topo{z, mapIndex ? mapIndex : none.data(), (settings->useTopographicDistance && topoVariable(variable)) ? (int32_t)kh : 0};
    return rasterFail("topodist interpolate", dev().topo_interpolate(call, topo, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
}

sf3d_error_t sf3d_topodist_station_matrix(uint32_t nPoints, const double* x, const double* y, const double* z, const int32_t* mapIndex, float* matrix)
{
    if (nPoints > SF3D_METEO_MAX_STATIONS || (nPoints > 0 && (!x || !y || !z || !matrix)) || !topoFinite(nPoints, x, y, z)) return SF3D_PARAMETER_ERROR;
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!topoPointsOk(nPoints, x, y) || !topoIndicesOk(nPoints, mapIndex)) return SF3D_PARAMETER_ERROR;
    const std::vector<int32_t> none(mapIndex ? 0 : nPoints, -1);
    return rasterFail("topodist station matrix", dev().topo_matrix(nPoints, x, y, z, mapIndex ? mapIndex : none.data(), matrix));
}

double sf3d_topodist_kernel_ms(int which) { return dev().topo_kernel_ms(which); }

sf3d_error_t sf3d_topodist_clean(void)
{
    topoHostClear();
    (void)dev().topo_free();
    return SF3D_OK;
}

} /* extern "C" */
