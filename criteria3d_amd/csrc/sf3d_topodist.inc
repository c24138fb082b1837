/* part of sf3d_solver.hip (included there after sf3d_meteo.inc, whose raster, station table and methods it uses) - topographic distance
 * on the device: the maps of gis::topographicDistanceMap (agrolib/gis/gis.cpp:1650-1675), the distances of computeDistances under
 * getUseTD() (agrolib/interpolation/interpolation.cpp:208-256) in front of the unchanged methods of sf3d_meteo.inc, and the
 * topographic distances between the stations themselves for the caller's Kh search (topographicDistanceOptimize, :2297-2368).
 *
 * k_topodist_maps: one thread per cell, 256 per block, the station in blockIdx.y.  A thread walks the line between its cell centre and
 * the station in steps of one cell size and keeps the largest rise of the DEM above the lower of the two ends (gis::topographicDistance,
 * gis.cpp:1595-1647).  The lanes of a wave are neighbouring cells walking to the same station, so the samples of one step are
 * neighbours in the DEM, which is read from global memory (the Ravone DEM is 2.5 MB: it stays in L2).  No LDS, no atomics, no grid sync.
 * k_meteo_idw_td: k_meteo_idw with the station heights and map indices beside the station table in LDS; meteo_cell (sf3d_meteo.inc) is
 * the text both kernels run, with TopoDistance in the place of MeteoPlainDistance.
 * k_topodist_matrix: one thread per (seen from station j, station i).
 *
 * The bar is the compiled reference's bits (tests/golden/topodist.npz), so the types and the order are the reference's:
 *  - stepMeter = float(cellSize); a distance < stepMeter returns 0; nrStep = int(distance / stepMeter), a float quotient;
 *  - the walk starts at the lower end under the strict z1 < z2 (a tie starts from the station); dx, dy are float quotients by
 *    float(nrStep); x = x + dx, y = y + dy accumulate in float, step after step (a closed form rounds differently);
 *  - a sample is Crit3DRasterGrid::getValueFromXY (gis.cpp:533-546): the float promoted to double, times invCellSize, truncated by int()
 *    (not floor: a point up to one cell left of or below the grid reads column or row 0), the unsigned bounds test, the flag outside;
 *  - the map a station carries is read as computeDistances reads it: gis::isOutOfGridXY (gis.cpp:840-845) on the cell's FLOAT x, y, then
 *    gis::getRowColFromXY (:735-739) with floor - not the cell's own index: the float of a UTM coordinate can lie in the neighbouring
 *    cell when cells are small.  Where that row or column is outside the raster after all (the product rounds up to nrCols; the reference
 *    reads past its array there) the station counts as map-less;
 *  - distance += kh * topoDistance: an int times a float.
 * -ffp-contract=off, IEEE sqrtf and division, as the rest of the build.
 *
 * Every walk is bounded: the entry points refuse a point farther than TOPODIST_MAX_STEPS cell sizes from the farthest corner of the
 * raster before any device work, and the loop itself stops at TOPODIST_LOOP_CAP whatever it is handed.
 *
 * The per-cell text also compiles for the host (tests/topodist_host.cpp defines SF3D_METEO_HOST). */

#define TOPO_NODATA_F (-9999.f)

/* Crit3DRasterGrid::getValueFromXY, gis.cpp:533-546 */
SF3D_METEO_FN float topo_dem_at(const TopoGridDev& g, float x, float y)
{
    const int r = (int)(((double)y - g.yll) * g.invCellSize);
    const int row = (g.nRows - 1) - r;
    const int col = (int)(((double)x - g.xll) * g.invCellSize);
    if ((unsigned)row >= (unsigned)g.nRows || (unsigned)col >= (unsigned)g.nCols) return g.flag;
    return g.dem[(size_t)row * (size_t)g.nCols + (size_t)col];
}

/* gis::topographicDistance, gis.cpp:1595-1647 */
SF3D_METEO_FN float topo_walk(const TopoGridDev& g, float x1, float y1, float z1, float x2, float y2, float z2, float distance)
{
    const float stepMeter = (float)g.cellSize;
    if (distance < stepMeter) return 0.f;
    const int nrStep = (int)(distance / stepMeter);
    const bool fromFirst = z1 < z2;
    const float Xi = fromFirst ? x1 : x2, Yi = fromFirst ? y1 : y2, Zi = fromFirst ? z1 : z2;
    const float Xf = fromFirst ? x2 : x1, Yf = fromFirst ? y2 : y1;
    const float dx = (Xf - Xi) / (float)nrStep;
    const float dy = (Yf - Yi) / (float)nrStep;
    float x = Xi, y = Yi, maxDeltaZ = 0.f;
    const int last = nrStep < TOPODIST_LOOP_CAP ? nrStep : TOPODIST_LOOP_CAP;       /* never the smaller one after the entry points' check */
    for (int i = 1; i <= last; ++i) {
        x = x + dx;
        y = y + dy;
        const float demValue = topo_dem_at(g, x, y);
        if (!meteo_eqf(demValue, g.flag) && demValue > Zi) {
            const float rise = demValue - Zi;
            maxDeltaZ = (maxDeltaZ > rise) ? maxDeltaZ : rise;                      /* MAXVALUE */
        }
    }
    return maxDeltaZ;
}

/* one DEM cell of topographicDistanceMap, gis.cpp:1662-1668: the cell centre of Crit3DRasterGrid::getXY (:473-477) as floats */
SF3D_METEO_FN float topo_map_cell(const TopoGridDev& g, uint32_t c, float demValue, double px, double py, double pz)
{
    const int row = (int)(c / (uint32_t)g.nCols), col = (int)(c - (uint32_t)row * (uint32_t)g.nCols);
    const double gridX = g.xll + g.cellSize * ((double)col + 0.5);
    const double gridY = g.yll + g.cellSize * ((double)(g.nRows - row) - 0.5);
    const float distance = meteo_distance((float)gridX, (float)gridY, px, py);
    return topo_walk(g, (float)gridX, (float)gridY, demValue, (float)px, (float)py, (float)pz, distance);
}

/* topoDistance of computeDistances, interpolation.cpp:232-247, for the point (x, y, z) and a station at (sx, sy, sz) whose plain distance
 * is d.  map: the station's map on the DEM's header, null where it has none */
SF3D_METEO_FN float topo_distance(const TopoGridDev& g, const float* map, float x, float y, float z, float sx, float sy, float sz, float d)
{
    float topoDistance = TOPO_NODATA_F;
    if (map) {
        const double xd = x, yd = y;
        const bool out = (xd < g.xll) || (yd < g.yll) || (xd >= (g.xll + g.nCols * g.cellSize)) || (yd >= (g.yll + g.nRows * g.cellSize));    /* isOutOfGridXY */
        if (!out) {
            const int row = (g.nRows - 1) - (int)__builtin_floor((yd - g.yll) * g.invCellSize);                                                  /* getRowColFromXY */
            const int col = (int)__builtin_floor((xd - g.xll) * g.invCellSize);
            if ((unsigned)row < (unsigned)g.nRows && (unsigned)col < (unsigned)g.nCols) topoDistance = map[(size_t)row * (size_t)g.nCols + (size_t)col];
        }
    }
    if (meteo_eqf(topoDistance, TOPO_NODATA_F)) topoDistance = topo_walk(g, x, y, z, sx, sy, sz, d);
    return topoDistance;
}

/* the distance vector of computeDistances under getUseTD() for a TD variable: dist(i) for the methods of sf3d_meteo.inc */
struct TopoDistance {
    TopoGridDev g;
    const double* sx;
    const double* sy;
    const float* sz;                    /* float(point->z) */
    const int32_t* mapIndex;
    const float* maps;
    size_t nCells;
    float x, y, z;
    int32_t kh;
    SF3D_METEO_MEMBER float operator()(uint32_t i) const
    {
        float d = meteo_distance(x, y, sx[i], sy[i]);
        if (kh != 0) {
            const int32_t m = mapIndex[i];
            const float t = topo_distance(g, m >= 0 ? maps + (size_t)m * nCells : nullptr, x, y, z, (float)sx[i], (float)sy[i], sz[i], d);
            d += ((float)kh * t);
        }
        return d;
    }
};

/* one entry of the station matrix: the topoDistance computeDistances uses for station i at station j's (float x, float y, float z) */
SF3D_METEO_FN float topo_matrix_entry(const TopoGridDev& g, const float* maps, size_t nCells, const double* sx, const double* sy, const double* sz,
                                      const int32_t* mapIndex, uint32_t j, uint32_t i)
{
    const float x = (float)sx[j], y = (float)sy[j], z = (float)sz[j];
    const float d = meteo_distance(x, y, sx[i], sy[i]);
    const int32_t m = mapIndex[i];
    return topo_distance(g, m >= 0 ? maps + (size_t)m * nCells : nullptr, x, y, z, (float)sx[i], (float)sy[i], (float)sz[i], d);
}

#ifndef SF3D_METEO_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_topodist_maps(TopoMapsView v)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = blockIdx.y;
    if (c >= v.nCells || p >= v.nPoints) return;
    float result = v.g.flag;
    const float demValue = v.g.dem[c];
    if (!(v.mine && !v.mine[c]) && !meteo_eqf(demValue, v.g.flag)) result = topo_map_cell(v.g, c, demValue, v.sx[p], v.sy[p], v.sz[p]);
    v.maps[(size_t)p * v.nCells + c] = result;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_meteo_idw_td(TopoIdwView)
{
    const TopoIdwView& t = meteo_kernel_argument<TopoIdwView>();
    __shared__ double sx[METEO_MAX_STATIONS], sy[METEO_MAX_STATIONS];
    __shared__ float sv[METEO_MAX_STATIONS], sz[METEO_MAX_STATIONS];
    __shared__ int32_t sm[METEO_MAX_STATIONS];
    const MeteoView& v = t.m;
    const uint32_t nStations = v.nStations < METEO_MAX_STATIONS ? v.nStations : METEO_MAX_STATIONS;
    for (uint32_t k = threadIdx.x; k < nStations; k += blockDim.x) {
        sx[k] = v.sx[k]; sy[k] = v.sy[k]; sv[k] = v.sv[k]; sz[k] = (float)t.sz[k]; sm[k] = t.mapIndex[k];
    }
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    float result = v.flag;
    const float z = v.dem[c];
    if (!(v.mine && !v.mine[c]) && !meteo_eqf(z, v.flag)) {
        float x, y;
        meteo_cell_xy(v, c, x, y);
        TopoDistance dist;
        dist.g.dem = v.dem; dist.g.xll = v.xll; dist.g.yll = v.yll; dist.g.cellSize = v.cellSize; dist.g.invCellSize = t.invCellSize;
        dist.g.nRows = (int32_t)v.nRows; dist.g.nCols = (int32_t)v.nCols; dist.g.flag = v.flag;
        dist.sx = sx; dist.sy = sy; dist.sz = sz; dist.mapIndex = sm; dist.maps = t.maps; dist.nCells = v.nCells;
        dist.x = x; dist.y = y; dist.z = z; dist.kh = t.kh;
        result = meteo_cell(v, c, z, x, y, dist, sx, sy, sv, nStations);
    }
    v.out[c] = result;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_topodist_matrix(TopoMatrixView v)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.nPoints * v.nPoints) return;
    const uint32_t j = k / v.nPoints, i = k - j * v.nPoints;
    v.matrix[k] = topo_matrix_entry(v.g, v.maps, v.nCells, v.sx, v.sy, v.sz, v.mapIndex, j, i);
}

/* ---- host side: the maps and the point tables belong to the meteo block (MeteoCache) and go with meteo_free ---- */
static TopoGridDev topo_grid(const MeteoCache& K)
{
    TopoGridDev g{};
    g.dem = K.base; g.xll = K.xll; g.yll = K.yll; g.cellSize = K.cellSize; g.invCellSize = 1.0 / K.cellSize;
    g.nRows = (int32_t)K.nRows; g.nCols = (int32_t)K.nCols; g.flag = K.flag;
    return g;
}

/* x, y, z (doubles) and mapIndex (int32) of a call's points, each table at the cap */
static const size_t TOPO_TABLE_BYTES = (size_t)METEO_MAX_STATIONS * (3 * sizeof(double) + sizeof(int32_t));

sf3d_error_t DeviceSolver::topo_free()
{
    if (!impl_) return SF3D_OK;
    MeteoCache& K = impl_->meteo;
    raster_release({K.topoMaps, K.topoTables, K.topoMatrix});
    K.topoMaps = nullptr; K.topoTables = nullptr; K.topoMatrix = nullptr;
    K.topoPoints = 0; K.topoMatrixCap = 0;
    return SF3D_OK;
}

/* the point tables on the device; a null table is left as it is */
sf3d_error_t DeviceSolver::topo_tables(uint32_t n, const double* x, const double* y, const double* z, const int32_t* mapIndex,
                                       const double*& dx, const double*& dy, const double*& dz, const int32_t*& dm)
{
    MeteoCache& K = impl_->meteo;
    hipStream_t stream = impl_->stream;
    if (!K.topoTables) RASTER_TRY(hipMalloc((void**)&K.topoTables, TOPO_TABLE_BYTES));
    double* t = (double*)K.topoTables;
    dx = t; dy = t + METEO_MAX_STATIONS; dz = t + 2 * METEO_MAX_STATIONS; dm = (const int32_t*)(t + 3 * METEO_MAX_STATIONS);
    if (n && x) RASTER_TRY(hipMemcpyAsync((void*)dx, x, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if (n && y) RASTER_TRY(hipMemcpyAsync((void*)dy, y, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if (n && z) RASTER_TRY(hipMemcpyAsync((void*)dz, z, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if (n && mapIndex) RASTER_TRY(hipMemcpyAsync((void*)dm, mapIndex, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::topo_compute(uint32_t nPoints, const double* x, const double* y, const double* z, const uint8_t* mine)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    raster_release({K.topoMaps});
    K.topoMaps = nullptr; K.topoPoints = 0; K.topoMs[0] = 0.;
    if (nPoints == 0) return SF3D_OK;
    RASTER_TRY(hipMalloc((void**)&K.topoMaps, (size_t)nPoints * n * sizeof(float)));
    K.topoPoints = nPoints;
    TopoMapsView v{};
    const int32_t* unused = nullptr;
    sf3d_error_t e = topo_tables(nPoints, x, y, z, nullptr, v.sx, v.sy, v.sz, unused);
    if (e == SF3D_OK) e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.g = topo_grid(K);
    v.maps = K.topoMaps; v.nCells = K.nCells; v.nPoints = nPoints;
    return raster_launch(k_topodist_maps, n, v, K.topoMs[0], nPoints);
}

sf3d_error_t DeviceSolver::topo_download(uint32_t index, float* dst)
{
    const MeteoCache& K = impl_->meteo;
    return raster_download(dst, K.topoMaps + (size_t)index * K.nCells, (size_t)K.nCells * sizeof(float));
}

sf3d_error_t DeviceSolver::topo_upload(uint32_t index, const float* src)
{
    MeteoCache& K = impl_->meteo;
    return raster_upload(K.topoMaps + (size_t)index * K.nCells, src, (size_t)K.nCells * sizeof(float));
}

sf3d_error_t DeviceSolver::topo_interpolate(const MeteoCall& call, const TopoCall& topo, const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    TopoIdwView t{};
    sf3d_error_t e = meteo_view(call, mine, t.m);
    const double* unused[2] = {nullptr, nullptr};
    if (e == SF3D_OK) e = topo_tables(call.nStations, nullptr, nullptr, topo.z, topo.mapIndex, unused[0], unused[1], t.sz, t.mapIndex);
    if (e != SF3D_OK) return e;
    t.maps = K.topoMaps; t.invCellSize = 1.0 / K.cellSize; t.kh = topo.kh;
    e = raster_launch(k_meteo_idw_td, n, t, K.topoMs[1]);
    if (e == SF3D_OK) K.produced[call.var] = true;
    if (e != SF3D_OK || !out) return e;
    return raster_download(out, t.m.out, n * sizeof(float));
}

sf3d_error_t DeviceSolver::topo_matrix(uint32_t nPoints, const double* x, const double* y, const double* z, const int32_t* mapIndex, float* matrix)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    RASTER_TRY(hipSetDevice(I.device));
    K.topoMs[2] = 0.;
    if (nPoints == 0) return SF3D_OK;
    if (nPoints > K.topoMatrixCap) {
        raster_release({K.topoMatrix});
        K.topoMatrix = nullptr; K.topoMatrixCap = 0;
        RASTER_TRY(hipMalloc((void**)&K.topoMatrix, (size_t)nPoints * nPoints * sizeof(float)));
        K.topoMatrixCap = nPoints;
    }
    TopoMatrixView v{};
    const sf3d_error_t e = topo_tables(nPoints, x, y, z, mapIndex, v.sx, v.sy, v.sz, v.mapIndex);
    if (e != SF3D_OK) return e;
    v.g = topo_grid(K);
    v.maps = K.topoMaps; v.matrix = K.topoMatrix; v.nCells = K.nCells; v.nPoints = nPoints;
    const sf3d_error_t el = raster_launch(k_topodist_matrix, (size_t)nPoints * nPoints, v, K.topoMs[2]);
    if (el != SF3D_OK) return el;
    return raster_download(matrix, K.topoMatrix, (size_t)nPoints * nPoints * sizeof(float));
}

double DeviceSolver::topo_kernel_ms(int which) const { return (impl_ && which >= 0 && which < 3) ? impl_->meteo.topoMs[which] : 0.; }
#endif
