/* part of sf3d_solver.hip (included there after sf3d_glocal.inc; it uses the elevation fit of sf3d_localdetrend.inc, the proxies' fit,
 * detrending, compaction and retrend of sf3d_localproxies.inc and the methods of sf3d_meteo.inc) - air and dew-point temperature with
 * MULTIPLE DETRENDING AND NOTHING ELSE on the device: what Project::interpolationDemMain (agrolib/project/project.cpp:3531-3561) does
 * with useMultipleDetrending set and neither local nor glocal detrending, topographic distance and lapse-rate codes off:
 *   1. preInterpolation -> multipleDetrendingMain (agrolib/interpolation/interpolation.cpp:2444-2499, 1832-1859), ONCE over all the call's
 *      stations in call order: multipleDetrendingElevationFitting(.., isWeighted = true) (:1862-1953) with every regressionWeight NODATA,
 *      which is weight 1, and no minimum of points (:1885 is off); detrendingElevation (:1956-1972) over EVERY point, those without a
 *      height included: the function of -9999 is subtracted from their value; multipleDetrendingOtherProxiesFitting (:1975-2171), whose
 *      two prunings erase stations from the interpolated list itself (:2038-2069), without the rule of :2140; detrendingOtherProxies
 *      (:2173-2236), which erases more;
 *   2. interpolationRaster (agrolib/project/interpolationCmd.cpp:354-395) per DEM cell, at the float (x, y) of
 *      getUtmXYFromRowColSinglePrecision's header overload - half a metre inside the cell's north-west corner, not its centre (md_cell_xy):
 *      getProxyValuesXY (:2620-2647) through Crit3DRasterGrid::getValueFromXY at that point (md_cell_at), interpolate()
 *      (:2502-2560) over what 1 left with the neighbour search of the meteo block (radius NODATA: no local radius), retrend through
 *      getMultipleDetrendingValues (:1298-1313, :2563-2617): a cell that lacks a value of a significant proxy KEEPS its interpolated
 *      value and gets retrend 0; a cell whose interpolate() gives -9999 stores -9999 and the call still succeeds;
 *   3. computeResiduals (agrolib/interpolation/spatialControl.cpp:102-160) and interpolationOutputPoints (project.cpp:2892-2937):
 *      interpolate() at a float (x, y) with the point's own proxy values, over the same kept list.
 *
 * k_multidetrend_fit: ONE wave64 - step 1.  The shape of k_localdetrend and k_glocal_areas: the list in LDS in call order (LdList), lane
 * k runs the Marquardt fit from first guess k, every lane walks the results in the order of k; the proxies' fit is lp_others with unit
 * weights and minPointsLocal 0 in the set-up.  It calls ld_elevation (which detrends the whole list where the height is significant) and
 * lp_others (which prunes, fits, detrends and compacts) - THE LIST-ORDER RULE of sf3d_localdetrend.inc holds: no atomics, tree reductions
 * or shuffles in any value.  The kept stations go to global memory compacted, in call order: x, y, the detrended value, and their count
 * in the call's record.
 * k_multidetrend_cells: one thread per DEM cell, as k_meteo_idw - step 2.  It is launched behind the fit on the same stream; the block
 * reads the kept count from the record and stages the kept stations into LDS (x, y doubles, value float: 20 KiB, k_meteo_idw's table).
 * k_multidetrend_points: one thread per point - step 3: the same text with x, y and the proxy values from the call's arrays.
 *
 * Every loop is bounded: list lengths <= METEO_MAX_STATIONS (the entry point refuses longer lists, the kernels clamp), a fit ends after
 * 1 001 iterations, the proxies' after 101, the neighbour search is the meteo block's.
 * The texts also compile for the host (tests/multidetrend_host.cpp defines SF3D_METEO_HOST): one lane, the same text. */

/* step 1 over the call's stations; the record, the per-station outcome and the kept list go to global memory */
SF3D_METEO_FN void md_fit(const MultiDetrendFitView& v, const LdList& L, LpCtx& X)
{
    const uint32_t lane = ld_lane();
    const uint32_t all = v.nStations < METEO_MAX_STATIONS ? v.nStations : METEO_MAX_STATIONS;
    /* the list: every point in call order, unit weights (regressionWeight NODATA, :1901-1903) */
    for (uint32_t i = lane; i < all; i += LD_LANES) {
        L.idx[i] = (uint16_t)i; L.d[i] = 0.f; L.h[i] = v.sh[i]; L.val[i] = v.sv[i]; L.w[i] = 1.f;
        X.member[i] = (uint8_t)(LP_FIT | LP_INTERP);
        v.detrended[i] = (float)LD_NODATA; v.keptBit[i] = 0;
    }
    ld_sync();
    double par[LD_MAX_PARAMETERS];
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = LD_NODATA;
    double R2 = LD_NODATA;
    bool significant = false;
    X.mask = 0;
    uint32_t n = all;
    /* the elevationPos arm of multipleDetrendingMain (:1845): the fit, and detrendingElevation over every entry where it is significant */
    if (v.p.heightSlot >= 0) significant = ld_elevation(v.s, L, n, par, R2);
    if (!significant) {
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = LD_NODATA;
    }
    /* the prunings carry over: what lp_others leaves is the list the cells and the points interpolate over */
    if (X.nOthers > 0) n = lp_others(v.s, v.p, L, X, n);
    ld_sync();
    for (uint32_t i = lane; i < n; i += LD_LANES) {
        const uint32_t at = L.idx[i];
        v.detrended[at] = L.val[i]; v.keptBit[at] = 1;
        v.keptX[i] = v.sx[at]; v.keptY[i] = v.sy[at]; v.keptValue[i] = L.val[i];
    }
    if (lane == 0) {
        MultiDetrendRecord& o = *v.record;
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = par[j];
        o.r2 = (float)R2; o.significant = significant ? 1 : 0; o.fitted = all; o.kept = n; o.mask = X.mask; o.reserved = 0;
        for (uint32_t p = 0; p < METEO_MAX_PROXIES; ++p) { o.line[p][0] = LD_NODATA; o.line[p][1] = LD_NODATA; }
        uint32_t j = 0;
        for (uint32_t r = 0; r < X.nOthers; ++r) {
            if (!((X.mask >> r) & 1u)) continue;
            o.line[j][0] = X.vec[LP_P * LP_NP + 2 * j]; o.line[j][1] = X.vec[LP_P * LP_NP + 2 * j + 1];
            ++j;
        }
    }
}

/* the methods of interpolate() (interpolation.cpp:2511-2528) at the float (x, y) over the kept stations, with shepardSearchNeighbour:
 * modifiedShepardIdw gets the radius NODATA, there is no local radius on this path */
SF3D_METEO_FN float md_methods(const LdSetup& s, const double* kx, const double* ky, const float* kv, uint32_t n, float x, float y)
{
    const MeteoPlainDistance dist{kx, ky, x, y};
    if (s.method == METEO_IDW) return meteo_idw(dist, kv, n);
    /* computeShepardInitialRadius(area, nrPoints, SHEPARD_AVG_NRPOINTS) with the kept list's size (interpolation.cpp:812-813) */
    const float radius0 = __builtin_sqrtf(((float)8u * s.area) / ((float)3.1415926535898 * (float)n));
    return meteo_shepard(dist, kx, ky, kv, n, x, y, radius0, s.method == METEO_SHEPARD_MODIFIED);
}

/* gis::getUtmXYFromRowColSinglePrecision(header, row, col, ..) (agrolib/gis/gis.cpp:799-804), which interpolationRaster calls: as its
 * parentheses stand it is NOT the cell's centre but the cell's west edge + 0.5 m and its north edge - 0.5 m, rounded to float.  The other
 * blocks' loops take the centre (getUtmXYFromRowCol); this one does not */
SF3D_METEO_FN void md_cell_xy(const MeteoView& v, uint32_t c, float& x, float& y)
{
    const int row = (int)(c / v.nCols), col = (int)(c - (uint32_t)row * v.nCols);
    x = (float)(v.xll + v.cellSize * (col) + 0.5);
    y = (float)(v.yll + v.cellSize * ((int)v.nRows - row) - 0.5);
}

/* the cell Crit3DRasterGrid::getValueFromXY (gis.cpp:533-546) reads at (x, y), which getProxyValuesXY hands it: int() of the offsets times
 * invCellSize; -1: outside the raster, the grid's flag.  With the rounding of md_cell_xy it need not be the cell the loop stands on */
SF3D_METEO_FN int32_t md_cell_at(const MeteoView& v, float x, float y)
{
    const double invCellSize = 1.0 / v.cellSize;
    const int r = (int)(((double)y - v.yll) * invCellSize);
    const int row = ((int)v.nRows - 1) - r;
    const int col = (int)(((double)x - v.xll) * invCellSize);
    if ((unsigned)row >= v.nRows || (unsigned)col >= v.nCols) return -1;
    return row * (int32_t)v.nCols + col;
}

/* step 2 for DEM cell c: a cell that lacks a significant proxy keeps its value, lp_retrend gives it 0 */
SF3D_METEO_FN float md_cell(const MultiDetrendCellsView& v, const double* kx, const double* ky, const float* kv, uint32_t n, uint32_t c)
{
    float x, y;
    md_cell_xy(v.m, c, x, y);
    float result = md_methods(v.s, kx, ky, kv, n, x, y);
    if (meteo_eqf(result, (float)LD_NODATA)) return (float)LD_NODATA;
    if (v.s.useDetrending) {
        const MultiDetrendRecord& R = *v.record;
        double par[LD_MAX_PARAMETERS];
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = R.parameters[j];
        /* getProxyValuesXY at (x, y); outside every raster each active proxy is NODATA: retrend 0 */
        const int32_t at = md_cell_at(v.m, x, y);
        result += (at >= 0) ? lp_retrend(v.m, v.s, v.p, (uint32_t)v.p.nOthers, R.mask, &R.line[0][0], (uint32_t)at, v.m.dem[at], R.significant != 0, par) : 0.f;
    }
    return result;
}

/* retrend (:1298-1313) through getMultipleDetrendingValues (:2563-2617) with the proxy values of point i of the call's arrays: lp_retrend's
 * arithmetic with another source of the values (a function of its own: lp_retrend reads rasters, and the kernels that share it keep their
 * registers) */
SF3D_METEO_FN float md_point_retrend(const MultiDetrendPointsView& v, const MultiDetrendRecord& R, uint32_t i, double* par)
{
    const uint32_t nOthers = (uint32_t)v.p.nOthers < LP_MAX_OTHERS ? (uint32_t)v.p.nOthers : LP_MAX_OTHERS;
    const bool significant = R.significant != 0;
    double retrendValue = 0.;
    bool complete = true;
    double zh = 0;
    if (significant) {
        zh = (double)v.pv[(size_t)v.p.heightSlot * v.nPoints + i];
        complete = zh != LD_NODATA;
    }
    for (uint32_t r = 0; r < nOthers; ++r)
        if (((R.mask >> r) & 1u) && (double)v.pv[(size_t)v.p.slot[r] * v.nPoints + i] == LD_NODATA) complete = false;
    if (complete && (significant || R.mask != 0)) {
        double sumOfFunctions = 0.0;
        if (significant) sumOfFunctions += ld_height_function(v.s, zh, par);
        int j = 0;
        for (uint32_t r = 0; r < nOthers; ++r) {
            if (!((R.mask >> r) & 1u)) continue;
            sumOfFunctions += R.line[j][0] * (double)v.pv[(size_t)v.p.slot[r] * v.nPoints + i] + R.line[j][1];
            ++j;
        }
        retrendValue = (float)sumOfFunctions;
    }
    return (float)retrendValue;
}

/* step 3 for point i of the call */
SF3D_METEO_FN float md_point(const MultiDetrendPointsView& v, const double* kx, const double* ky, const float* kv, uint32_t n, uint32_t i)
{
    float result = md_methods(v.s, kx, ky, kv, n, v.px[i], v.py[i]);
    if (meteo_eqf(result, (float)LD_NODATA)) return (float)LD_NODATA;
    if (v.s.useDetrending) {
        const MultiDetrendRecord& R = *v.record;
        double par[LD_MAX_PARAMETERS];
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = R.parameters[j];
        result += md_point_retrend(v, R, i, par);
    }
    return result;
}

#ifndef SF3D_METEO_HOST
__global__ void __launch_bounds__(64) k_multidetrend_fit(MultiDetrendFitView)
{
    const MultiDetrendFitView& v = meteo_kernel_argument<MultiDetrendFitView>();
    __shared__ double heightsAndWeights[METEO_MAX_STATIONS];
    __shared__ double fit[LD_MAX_FIRST_GUESS * LD_FIT_STRIDE];
    __shared__ double work[LP_WORK_DOUBLES];
    __shared__ float places[METEO_MAX_STATIONS], values[METEO_MAX_STATIONS];
    __shared__ uint16_t indices[METEO_MAX_STATIONS];
    __shared__ uint8_t members[METEO_MAX_STATIONS];
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    LdList L;
    L.idx = indices; L.d = places; L.val = values;
    L.h = (float*)heightsAndWeights; L.w = L.h + METEO_MAX_STATIONS; L.wt = heightsAndWeights;
    L.lanes = nullptr; L.fit = fit;                                             /* no selection here: its lane maxima have no room */
    LpCtx X;
    X.rows = v.rows; X.member = members; X.vec = work; X.mat = fit;
    X.nOthers = (uint32_t)v.p.nOthers < LP_MAX_OTHERS ? (uint32_t)v.p.nOthers : LP_MAX_OTHERS; X.mask = 0;
    md_fit(v, L, X);
}

/* the kept stations of the fit into the block's LDS; their count is read here, on the device */
#define MD_STAGE(view)                                                                                                       \
    __shared__ double kx[METEO_MAX_STATIONS], ky[METEO_MAX_STATIONS];                                                        \
    __shared__ float kv[METEO_MAX_STATIONS];                                                                                 \
    const uint32_t kept = (view).record->kept < METEO_MAX_STATIONS ? (view).record->kept : METEO_MAX_STATIONS;               \
    for (uint32_t k = threadIdx.x; k < kept; k += blockDim.x) { kx[k] = (view).keptX[k]; ky[k] = (view).keptY[k]; kv[k] = (view).keptValue[k]; } \
    __syncthreads()

__global__ void __launch_bounds__(SF3D_BLOCK) k_multidetrend_cells(MultiDetrendCellsView)
{
    const MultiDetrendCellsView& v = meteo_kernel_argument<MultiDetrendCellsView>();
    const MeteoView& m = v.m;
    MD_STAGE(v);
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m.nCells) return;
    float result = m.flag;
    const float z = m.dem[c];
    if (!(m.mine && !m.mine[c]) && !meteo_eqf(z, m.flag)) {
        result = md_cell(v, kx, ky, kv, kept, c);
    }
    m.out[c] = result;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_multidetrend_points(MultiDetrendPointsView)
{
    const MultiDetrendPointsView& v = meteo_kernel_argument<MultiDetrendPointsView>();
    MD_STAGE(v);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.nPoints) return;
    v.out[i] = md_point(v, kx, ky, kv, kept, i);
}

/* ---- host side: one block of fixed size, allocated by the first call and freed with the meteo block's raster (meteo_free): the call's
 * tables and what k_multidetrend_fit leaves; the points of a call of sf3d_multidetrend_points in a buffer that grows ---- */
enum : size_t {
    MD_OFF_TABLE = 0,
    MD_OFF_KEPT_X = MD_OFF_TABLE + (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double),
    MD_OFF_KEPT_Y = MD_OFF_KEPT_X + (size_t)METEO_MAX_STATIONS * sizeof(double),
    MD_OFF_RECORD = MD_OFF_KEPT_Y + (size_t)METEO_MAX_STATIONS * sizeof(double),
    MD_OFF_HEIGHTS = MD_OFF_RECORD + sizeof(MultiDetrendRecord),
    MD_OFF_ROWS = MD_OFF_HEIGHTS + (size_t)METEO_MAX_STATIONS * sizeof(float),
    MD_OFF_DETRENDED = MD_OFF_ROWS + (size_t)LP_MAX_OTHERS * METEO_MAX_STATIONS * sizeof(float),
    MD_OFF_KEPT_VALUE = MD_OFF_DETRENDED + (size_t)METEO_MAX_STATIONS * sizeof(float),
    MD_OFF_KEPT_BIT = MD_OFF_KEPT_VALUE + (size_t)METEO_MAX_STATIONS * sizeof(float),
    MD_BLOCK_BYTES = MD_OFF_KEPT_BIT + (size_t)METEO_MAX_STATIONS
};
static_assert(sizeof(MultiDetrendRecord) % 8 == 0 && MD_OFF_RECORD % 8 == 0, "the record's doubles are aligned");

sf3d_error_t DeviceSolver::multidetrend_free()
{
    if (!impl_) return SF3D_OK;
    MeteoCache& K = impl_->meteo;
    raster_release({K.multiBlock, K.multiPoints});
    K.multiBlock = nullptr; K.multiPoints = nullptr; K.multiPointsCap = 0; K.multiStations = 0; K.multiDone = false;
    K.multiMs[0] = K.multiMs[1] = K.multiMs[2] = 0.;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::multidetrend_interpolate(const MeteoCall& call, const MultiDetrendCall& g, const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    MultiDetrendCellsView c{};
    sf3d_error_t e = meteo_view(call, mine, c.m);
    if (e != SF3D_OK) return e;
    K.multiDone = false;
    K.produced[call.var] = false;                                               /* the slot is overwritten; it counts again once the call is whole */
    if (!K.multiBlock) RASTER_TRY(hipMalloc((void**)&K.multiBlock, MD_BLOCK_BYTES));
    char* B = K.multiBlock;
    double* table = (double*)(B + MD_OFF_TABLE);
    float* heights = (float*)(B + MD_OFF_HEIGHTS);
    float* rows = (float*)(B + MD_OFF_ROWS);
    RASTER_TRY(hipMemcpyAsync(table, g.table, (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice, I.stream));
    if (call.nStations) {
        RASTER_TRY(hipMemcpyAsync(heights, g.height, call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
        for (int r = 0; r < g.proxies.nOthers; ++r)
            RASTER_TRY(hipMemcpyAsync(rows + (size_t)r * METEO_MAX_STATIONS, g.rows[r], call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
    }

    MultiDetrendFitView f{};
    f.s = g.setup;
    f.s.table = table;
    f.s.method = call.method; f.s.useDetrending = call.useDetrending;
    f.p = g.proxies;
    f.sx = c.m.sx; f.sy = c.m.sy; f.sv = c.m.sv; f.sh = heights; f.rows = rows;
    f.record = (MultiDetrendRecord*)(B + MD_OFF_RECORD);
    f.detrended = (float*)(B + MD_OFF_DETRENDED);
    f.keptBit = (uint8_t*)(B + MD_OFF_KEPT_BIT);
    f.keptX = (double*)(B + MD_OFF_KEPT_X); f.keptY = (double*)(B + MD_OFF_KEPT_Y);
    f.keptValue = (float*)(B + MD_OFF_KEPT_VALUE);
    f.nStations = call.nStations;
    c.s = f.s; c.p = f.p;
    c.record = f.record; c.keptX = f.keptX; c.keptY = f.keptY; c.keptValue = f.keptValue;

    /* the fit, and the cells behind it on the same stream: no host round trip in between */
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (I.timing) {
        for (int k = 0; k < 3; ++k) RASTER_TRY(hipEventCreate(&ev[k]));
        RASTER_TRY(hipEventRecord(ev[0], I.stream));
    }
    hipLaunchKernelGGL(k_multidetrend_fit, dim3(1), dim3(64), 0, I.stream, f);
    RASTER_TRY(hipGetLastError());
    if (I.timing) RASTER_TRY(hipEventRecord(ev[1], I.stream));
    hipLaunchKernelGGL(k_multidetrend_cells, dim3((uint32_t)((n + SF3D_BLOCK - 1) / SF3D_BLOCK)), dim3(SF3D_BLOCK), 0, I.stream, c);
    RASTER_TRY(hipGetLastError());
    if (I.timing) RASTER_TRY(hipEventRecord(ev[2], I.stream));
    RASTER_TRY(hipStreamSynchronize(I.stream));
    K.multiMs[0] = K.multiMs[1] = 0.;
    if (I.timing) {
        float t[2] = {0.f, 0.f};
        RASTER_TRY(hipEventElapsedTime(&t[0], ev[0], ev[1]));
        RASTER_TRY(hipEventElapsedTime(&t[1], ev[1], ev[2]));
        for (int k = 0; k < 3; ++k) (void)hipEventDestroy(ev[k]);
        K.multiMs[0] = t[0]; K.multiMs[1] = t[1];
    }
    K.multiSetup = f.s; K.multiProxies = f.p; K.multiStations = call.nStations;
    K.multiDone = true;
    K.produced[call.var] = true;
    if (!out) return SF3D_OK;
    return raster_download(out, c.m.out, n * sizeof(float));
}

bool DeviceSolver::multidetrend_done() const { return impl_ && impl_->meteo.base && impl_->meteo.multiBlock && impl_->meteo.multiDone; }

sf3d_error_t DeviceSolver::multidetrend_points(uint32_t nPoints, uint32_t nProxies, const float* x, const float* y, const float* proxyValues, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    if (nPoints == 0) return SF3D_OK;
    RASTER_TRY(hipSetDevice(I.device));
    const size_t floats = (size_t)(3 + nProxies) * nPoints;
    if (floats > K.multiPointsCap) {
        raster_release({K.multiPoints});
        K.multiPoints = nullptr; K.multiPointsCap = 0;
        RASTER_TRY(hipMalloc((void**)&K.multiPoints, floats * sizeof(float)));
        K.multiPointsCap = floats;
    }
    float* px = (float*)K.multiPoints;
    float* py = px + nPoints;
    float* po = py + nPoints;
    float* pv = po + nPoints;
    RASTER_TRY(hipMemcpyAsync(px, x, (size_t)nPoints * sizeof(float), hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(py, y, (size_t)nPoints * sizeof(float), hipMemcpyHostToDevice, I.stream));
    if (nProxies) RASTER_TRY(hipMemcpyAsync(pv, proxyValues, (size_t)nProxies * nPoints * sizeof(float), hipMemcpyHostToDevice, I.stream));
    char* B = K.multiBlock;
    MultiDetrendPointsView v{};
    v.s = K.multiSetup; v.p = K.multiProxies;
    v.record = (const MultiDetrendRecord*)(B + MD_OFF_RECORD);
    v.keptX = (const double*)(B + MD_OFF_KEPT_X); v.keptY = (const double*)(B + MD_OFF_KEPT_Y);
    v.keptValue = (const float*)(B + MD_OFF_KEPT_VALUE);
    v.px = px; v.py = py; v.pv = pv; v.out = po;
    v.nPoints = nPoints; v.nProxies = nProxies;
    const sf3d_error_t e = raster_launch(k_multidetrend_points, (size_t)nPoints, v, K.multiMs[2]);
    if (e != SF3D_OK) return e;
    return raster_download(out, po, (size_t)nPoints * sizeof(float));
}

sf3d_error_t DeviceSolver::multidetrend_records(MultiDetrendRecord* record, float* detrended, uint8_t* kept, LocalProxiesSetup* proxies)
{
    const MeteoCache& K = impl_->meteo;
    sf3d_error_t e = SF3D_OK;
    if (record) e = raster_download(record, K.multiBlock + MD_OFF_RECORD, sizeof(MultiDetrendRecord));
    if (e == SF3D_OK && detrended && K.multiStations) e = raster_download(detrended, K.multiBlock + MD_OFF_DETRENDED, (size_t)K.multiStations * sizeof(float));
    if (e == SF3D_OK && kept && K.multiStations) e = raster_download(kept, K.multiBlock + MD_OFF_KEPT_BIT, K.multiStations);
    if (proxies) *proxies = K.multiProxies;
    return e;
}

uint64_t DeviceSolver::multidetrend_bytes() const
{
    if (!impl_) return 0;
    const MeteoCache& K = impl_->meteo;
    return (K.multiBlock ? (uint64_t)MD_BLOCK_BYTES : 0) + (uint64_t)K.multiPointsCap * sizeof(float);
}

double DeviceSolver::multidetrend_kernel_ms(int which) const { return (impl_ && which >= 0 && which < 3) ? impl_->meteo.multiMs[which] : 0.; }
#endif
