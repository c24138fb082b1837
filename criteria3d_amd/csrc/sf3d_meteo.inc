/* part of sf3d_solver.hip (included there after the root maps) - the hourly meteo maps from station data: what the library function
 * interpolate() (agrolib/interpolation/interpolation.cpp:2502-2560) does for every DEM cell in the application's default non-local set-up,
 * on the device.  k_meteo_idw: one thread per cell, the station table (x, y as doubles, the value as float) staged once per block into
 * LDS - every lane reads the same station at the same time, a broadcast.
 *   inverseDistanceWeighted (:1031-1051)   one pass over the stations;
 *   shepardIdw (:871-945), modifiedShepardIdw (:948-1028) over shepardSearchNeighbour (:806-868): pass one counts the stations inside the
 *       initial radius, pass two fills a ten-slot list kept in registers (constant indices after full unrolling: no scratch) - the
 *       neighbourhood in INPUT order when it holds 5 to 10 stations, else the 5 nearest of all stations / the 10 nearest of the
 *       neighbourhood by insertion with the strict < of sortPointsByDistance (:121-159) - then the 10 x 10 direction terms and the sums, all
 *       in the order of that list;
 *   retrend (:1288-1351), single detrending, and the tail of interpolate().
 * The methods take the distance vector of computeDistances as a template argument (MeteoPlainDistance here, TopoDistance in
 * sf3d_topodist.inc) and meteo_cell is interpolate() for one cell: k_meteo_idw and k_meteo_idw_td run the same text.
 * The bar is the compiled reference's bits (tests/golden/meteo_idw.npz): the reference's types at every step (float distances, float
 * S = 1 / d, float products of two distances, double sums) in its order, -ffp-contract=off, IEEE sqrtf and float / double division (the
 * compiler's default for HIP: no fast-math flag, no approximate-division flag in the build).  No exp, log, pow or atan2; no atomics, no
 * grid sync, nothing of the solver.
 *
 * Kept from the reference on purpose:
 *  - interpolate() hands (radius, x, y) to modifiedShepardIdw's (radius, y, x) (:2527 against :949): its direction terms pair the cell's
 *    y with the stations' x;
 *  - a station at distance 0 is left out of every list (> 0, !isEqual(d, 0), > EPSILON), it does not set the cell;
 *  - result += retrend() adds 0.f for a variable that is not detrended (-0 becomes +0). */

#define METEO_NODATA (-9999)
#define METEO_EPSILON 0.00001
#define METEO_LIST 10                         /* SHEPARD_MAX_NRPOINTS */
#define METEO_MIN 5                           /* SHEPARD_MIN_NRPOINTS */

/* the per-cell text also compiles for the host (tests/topodist_host.cpp defines SF3D_METEO_HOST and the qualifier) */
#ifndef SF3D_METEO_FN
#define SF3D_METEO_FN __device__ __forceinline__
#define SF3D_METEO_MEMBER __device__ __forceinline__     /* a member function: the host build cannot say `static` there */
#endif

SF3D_METEO_FN bool meteo_eqf(float a, float b) { return __builtin_fabs((double)a - (double)b) < METEO_EPSILON; }      /* isEqual(float, float), basicMath.h:25 */

/* gis::computeDistance(x, y, float(utm.x), float(utm.y)), gis.cpp:685-691 */
SF3D_METEO_FN float meteo_distance(float x, float y, double sx, double sy)
{
    const float dx = (float)sx - x;
    const float dy = (float)sy - y;
    return __builtin_sqrtf(dx * dx + dy * dy);
}

/* the distance vector of computeDistances (interpolation.cpp:208-256), one station at a time: dist(i).  This one is the plain distance
 * of k_meteo_idw; sf3d_topodist.inc has the one with topographic distance.  The methods below take either. */
struct MeteoPlainDistance {
    const double* sx;
    const double* sy;
    float x, y;
    SF3D_METEO_MEMBER float operator()(uint32_t i) const { return meteo_distance(x, y, sx[i], sy[i]); }
};

/* inverseDistanceWeighted, interpolation.cpp:1031-1051 */
template <class Dist> SF3D_METEO_FN float meteo_idw(const Dist& dist, const float* sv, uint32_t n)
{
    double sum = 0, sumWeights = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float d = dist(i);
        if ((double)d > METEO_EPSILON) {
            const double dist_km = (double)d / 10000.;
            const double weight = 1.0 / (dist_km * dist_km * dist_km);
            sumWeights += weight;
            sum += (double)sv[i] * weight;
        }
    }
    return (sumWeights > 0.0) ? (float)(sum / sumWeights) : (float)METEO_NODATA;
}

/* shepardSearchNeighbour, then shepardIdw (modified == false) or modifiedShepardIdw with radius == NODATA on entry.  sx, sy, sv: the
 * station table (pointers here; sf3d_localdetrend.inc hands in a cell's selected list, indexed the same way) */
template <class Dist, class Coord, class Value> SF3D_METEO_FN float meteo_shepard(const Dist& dist, Coord sx, Coord sy, Value sv, uint32_t nStations, float x, float y, float radius0, bool modified)
{
    float ld[METEO_LIST];
    uint32_t li[METEO_LIST];
#pragma unroll
    for (int s = 0; s < METEO_LIST; ++s) { ld[s] = __builtin_inff(); li[s] = 0; }
    uint32_t inside = 0;
    for (uint32_t i = 0; i < nStations; ++i) {
        const float d = dist(i);
        inside += (d <= radius0 && d > 0) ? 1u : 0u;
    }
    const bool few = inside < METEO_MIN;
    const bool sorted = few || inside > METEO_LIST;
    const int keep = few ? METEO_MIN : METEO_LIST;
    int n = 0;
    for (uint32_t i = 0; i < nStations; ++i) {
        const float d = dist(i);
        const bool in = d <= radius0 && d > 0;
        if (sorted) {
            /* sortPointsByDistance: ! isEqual(d, 0) (d is never near NODATA); of all stations (few) or of the neighbourhood */
            if ((few || in) && !(__builtin_fabs((double)d) < METEO_EPSILON)) {
                float nd = d;
                uint32_t ni = i;
                bool shifting = false;
#pragma unroll
                for (int s = 0; s < METEO_LIST; ++s) {
                    const bool sw = s < keep && (shifting || nd < ld[s]);
                    const float td = ld[s];
                    const uint32_t ti = li[s];
                    ld[s] = sw ? nd : td; li[s] = sw ? ni : ti;
                    nd = sw ? td : nd; ni = sw ? ti : ni;
                    shifting = shifting || sw;
                }
                n = (n < keep) ? n + 1 : n;
            }
        } else if (in) {
#pragma unroll
            for (int s = 0; s < METEO_LIST; ++s)
                if (s == n) { ld[s] = d; li[s] = i; }
            ++n;
        }
    }
    float radius = radius0;
    if (sorted) {
        radius = (float)METEO_NODATA;
#pragma unroll
        for (int s = 0; s < METEO_LIST; ++s)
            if (s == n - 1) radius = ld[s] + (float)METEO_EPSILON;
    }
    if (modified && n == 0) return (float)METEO_NODATA;

    double S[METEO_LIST], dxs[METEO_LIST], dys[METEO_LIST];
    float val[METEO_LIST];
    /* modifiedShepardIdw is declared (radius, y, x) and called with (radius, x, y) */
    const double X = modified ? (double)y : (double)x, Y = modified ? (double)x : (double)y;
    double weightSum = 0;
    const double radius_3 = radius / 3., radius_27_4 = 6.75 / radius;
#pragma unroll
    for (int s = 0; s < METEO_LIST; ++s) {
        S[s] = 0; dxs[s] = 0; dys[s] = 0; val[s] = 0;
        if (s < n) {
            const float d = ld[s];
            dxs[s] = X - sx[li[s]]; dys[s] = Y - sy[li[s]]; val[s] = sv[li[s]];
            if (modified) {
                if ((double)d > METEO_EPSILON && d <= radius) {
                    S[s] = (radius - d) / (radius * d);                     /* float arithmetic */
                    weightSum += S[s];
                }
            } else if ((double)d > METEO_EPSILON) {
                if ((double)d <= radius_3) S[s] = 1.f / d;                  /* 1 / float: a float quotient */
                else if (d <= radius) {
                    const double tmp = (d / radius) - 1.f;                  /* float too */
                    S[s] = radius_27_4 * tmp * tmp;
                } else S[s] = 0;
                weightSum += S[s];
            }
        }
    }
    if (weightSum == 0) return (float)METEO_NODATA;
    const double invWeightSum = 1.0 / weightSum;

    double weight[METEO_LIST];
    double weightSum2 = 0;
#pragma unroll
    for (int i = 0; i < METEO_LIST; ++i) {
        weight[i] = 0;
        if (i < n) {
            double t = 0;
            if (!modified || !(S[i] == 0.0 || ld[i] <= 0)) {
#pragma unroll
                for (int j = 0; j < METEO_LIST; ++j) {
                    if (j < n && j != i && (!modified || !(S[j] == 0.0 || ld[j] <= 0))) {
                        const double cosine = (dxs[i] * dxs[j] + dys[i] * dys[j]) / (ld[i] * ld[j]);       /* the float product of the two distances */
                        t += S[j] * (1 - cosine);
                    }
                }
                if (modified) t *= invWeightSum; else t /= weightSum;
            }
            weight[i] = S[i] * S[i] * (1 + t);
            weightSum2 += weight[i];
        }
    }
    const double invWeightSumFinal = 1.0 / weightSum2;
    double result = 0;
#pragma unroll
    for (int i = 0; i < METEO_LIST; ++i)
        if (i < n) result += (modified ? weight[i] * invWeightSumFinal : weight[i] / weightSum2) * val[i];
    return (float)result;
}

/* gis::getUtmXYFromRowCol, gis.cpp:806-810, then the float x, y of interpolate() */
SF3D_METEO_FN void meteo_cell_xy(const MeteoView& v, uint32_t c, float& x, float& y)
{
    const int row = (int)(c / v.nCols), col = (int)(c - (uint32_t)row * v.nCols);
    const double xd = v.xll + v.cellSize * (col + 0.5);
    const double yd = v.yll + v.cellSize * ((int)v.nRows - row - 0.5);
    x = (float)xd; y = (float)yd;
}

/* interpolate() (interpolation.cpp:2502-2560) on DEM cell c of height z at the float (x, y), with the distances `dist` */
template <class Dist> SF3D_METEO_FN float meteo_cell(const MeteoView& v, uint32_t c, float z, float x, float y, const Dist& dist,
                                                      const double* sx, const double* sy, const float* sv, uint32_t nStations)
{
    const float flag = v.flag;
    float result;
    if (v.var == METEO_PRECIPITATION && v.allZero) result = 0.f;
    else {
        if (v.method == METEO_IDW) result = meteo_idw(dist, sv, nStations);
        else result = meteo_shepard(dist, sx, sy, sv, nStations, x, y, v.radius0, v.method == METEO_SHEPARD_MODIFIED);
        if (meteo_eqf(result, (float)METEO_NODATA)) result = (float)METEO_NODATA;
        else {
            if (v.useDetrending) {
                float add = 0.f;                                        /* retrend of a variable that is not detrended */
                if (v.detrendingVar) {
                    double retrendValue = 0.;
#pragma unroll
                    for (int p = 0; p < METEO_MAX_PROXIES; ++p) {
                        if (p < (int)v.nProxies && v.proxy[p].active) {
                            const float f = v.proxyMap[p] ? v.proxyMap[p][c] : z;
                            const double myProxyValue = (f != flag) ? (double)f : (double)METEO_NODATA;           /* getProxyValuesXY */
                            if (myProxyValue != METEO_NODATA) {
                                const float proxySlope = v.proxy[p].slope;
                                if (v.proxy[p].isHeight) {
                                    if (v.proxy[p].inversion) {
                                        const float LR_H0 = v.proxy[p].lapseRateH0, LR_H1 = v.proxy[p].lapseRateH1, LR_Below = v.proxy[p].inversionLapseRate;
                                        if (myProxyValue <= LR_H1) {
                                            const double a = myProxyValue - LR_H0;
                                            retrendValue += ((a > 0) ? a : 0) * LR_Below;
                                        } else retrendValue += ((LR_H1 - LR_H0) * LR_Below) + (myProxyValue - LR_H1) * proxySlope;   /* a float product first */
                                    } else retrendValue += ((myProxyValue > 0) ? myProxyValue : 0) * proxySlope;
                                } else retrendValue += myProxyValue * proxySlope;
                            }
                        }
                    }
                    add = (float)retrendValue;
                }
                result += add;
            }
            /* the switch of interpolate(), with the comparisons of std::min / std::max */
            if (v.var == METEO_PRECIPITATION) result = (result < v.rainfallThreshold) ? 0.f : result;
            else if (v.var == METEO_AIR_REL_HUMIDITY) {
                const float m = (100.f < result) ? 100.f : result;
                result = (0.f < m) ? m : 0.f;
            } else if (v.var == METEO_WIND_SCALAR_INTENSITY || v.var == METEO_GLOBAL_IRRADIANCE || v.var == METEO_ATM_TRANSMISSIVITY)
                result = (result < 0.f) ? 0.f : result;
        }
    }
    return result;
}

#ifndef SF3D_METEO_HOST
/* The first argument of the running kernel, read where it lies in the kernel argument segment.  meteo_cell takes the view by reference;
 * a reference to the by-value parameter makes the compiler copy the whole struct at the kernel's entry - every proxy held in scalar
 * registers across the neighbour search, 40 of them spilled - while a reference into the segment loads each field where it is used,
 * as the kernel did when this text stood in its body. */
template <class View> __device__ __forceinline__ const View& meteo_kernel_argument()
{
    return *(const View*)__builtin_amdgcn_kernarg_segment_ptr();
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_meteo_idw(MeteoView)
{
    const MeteoView& v = meteo_kernel_argument<MeteoView>();
    __shared__ double sx[METEO_MAX_STATIONS], sy[METEO_MAX_STATIONS];
    __shared__ float sv[METEO_MAX_STATIONS];
    const uint32_t nStations = v.nStations < METEO_MAX_STATIONS ? v.nStations : METEO_MAX_STATIONS;
    for (uint32_t k = threadIdx.x; k < nStations; k += blockDim.x) { sx[k] = v.sx[k]; sy[k] = v.sy[k]; sv[k] = v.sv[k]; }
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    float result = v.flag;
    const float z = v.dem[c];
    if (!(v.mine && !v.mine[c]) && !meteo_eqf(z, v.flag)) {
        float x, y;
        meteo_cell_xy(v, c, x, y);
        result = meteo_cell(v, c, z, x, y, MeteoPlainDistance{sx, sy, x, y}, sx, sy, sv, nStations);
    }
    v.out[c] = result;
}

/* ---- host side: the DEM, the proxy rasters and one float map per variable in one block; calls go through the shared raster path at the
 * end of sf3d_maps.inc. */
sf3d_error_t DeviceSolver::meteo_free()
{
    if (!impl_) return SF3D_OK;
    raster_unbind(FEED_METEO);
    raster_release({impl_->meteo.base, impl_->meteo.stations, impl_->meteo.topoMaps, impl_->meteo.topoTables, impl_->meteo.topoMatrix,
                    impl_->meteo.localFit, impl_->meteo.localTables, impl_->meteo.proxiesFit, impl_->meteo.proxiesTables,
                    impl_->meteo.glocalBlock, impl_->meteo.glocalTables, impl_->meteo.multiBlock,
                    impl_->meteo.multiPoints});       /* the topographic distance maps, the local detrending's outcome, the macro areas and the one fit go with their raster */
    impl_->meteo = MeteoCache();
    return SF3D_OK;
}

/* maps of the block: the DEM, nProxies proxy rasters (a NULL one has none: its slot is unused), METEO_VARIABLES outputs */
sf3d_error_t DeviceSolver::meteo_alloc(uint32_t nRows, uint32_t nCols, const float* dem, float flag, double xll, double yll, double cellSize,
                                       uint32_t nProxies, const float* const* proxyMaps)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    meteo_free();
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = (size_t)nRows * nCols;
    RASTER_TRY(hipMalloc((void**)&K.base, (1 + (size_t)nProxies + METEO_VARIABLES) * n * sizeof(float)));
    RASTER_TRY(hipMalloc((void**)&K.stations, (size_t)METEO_MAX_STATIONS * (2 * sizeof(double) + sizeof(float))));
    K.nCells = (uint32_t)n; K.nRows = nRows; K.nCols = nCols; K.nProxies = nProxies; K.xll = xll; K.yll = yll; K.cellSize = cellSize; K.flag = flag;
    RASTER_TRY(hipMemcpyAsync(K.base, dem, n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    for (uint32_t p = 0; p < nProxies; ++p) {
        K.hasMap[p] = proxyMaps[p] != nullptr;
        if (proxyMaps[p]) RASTER_TRY(hipMemcpyAsync(K.base + (1 + (size_t)p) * n, proxyMaps[p], n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    }
    /* before the first call of a variable its map holds the flag */
    const std::vector<float> empty((size_t)METEO_VARIABLES * n, flag);
    return raster_upload(K.base + (1 + (size_t)nProxies) * n, empty.data(), empty.size() * sizeof(float));
}

/* the station table of a call on the device and the view of its launch: what k_meteo_idw and k_meteo_idw_td (sf3d_topodist.inc) share */
sf3d_error_t DeviceSolver::meteo_view(const MeteoCall& call, const uint8_t* mine, MeteoView& v)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    double* dsx = (double*)K.stations;
    double* dsy = dsx + METEO_MAX_STATIONS;
    float* dsv = (float*)(dsy + METEO_MAX_STATIONS);
    if (call.nStations) {
        RASTER_TRY(hipMemcpyAsync(dsx, call.x, call.nStations * sizeof(double), hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipMemcpyAsync(dsy, call.y, call.nStations * sizeof(double), hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipMemcpyAsync(dsv, call.value, call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
    }
    v = MeteoView{};
    const sf3d_error_t e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.dem = K.base;
    for (uint32_t p = 0; p < METEO_MAX_PROXIES; ++p) {
        v.proxyMap[p] = (p < K.nProxies && K.hasMap[p]) ? K.base + (1 + (size_t)p) * n : nullptr;
        v.proxy[p] = call.proxy[p];
    }
    v.sx = dsx; v.sy = dsy; v.sv = dsv;
    v.out = K.base + (1 + (size_t)K.nProxies + (size_t)call.var) * n;
    v.xll = K.xll; v.yll = K.yll; v.cellSize = K.cellSize;
    v.nCells = K.nCells; v.nRows = K.nRows; v.nCols = K.nCols; v.nStations = call.nStations; v.nProxies = call.nProxies;
    v.var = call.var; v.method = call.method; v.allZero = call.allZero; v.useDetrending = call.useDetrending; v.detrendingVar = call.detrendingVar;
    v.flag = K.flag; v.radius0 = call.radius0; v.rainfallThreshold = call.rainfallThreshold;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::meteo_interpolate(const MeteoCall& call, const uint8_t* mine, float* out)
{
    MeteoCache& K = impl_->meteo;
    const size_t n = K.nCells;
    MeteoView v;
    sf3d_error_t e = meteo_view(call, mine, v);
    if (e != SF3D_OK) return e;
    e = raster_launch(k_meteo_idw, n, v, K.lastMs);
    if (e == SF3D_OK) K.produced[call.var] = true;
    if (e != SF3D_OK || !out) return e;
    return raster_download(out, v.out, n * sizeof(float));
}

sf3d_error_t DeviceSolver::meteo_download(int var, float* dst)
{
    const MeteoCache& K = impl_->meteo;
    return raster_download(dst, K.base + (1 + (size_t)K.nProxies + (size_t)var) * K.nCells, (size_t)K.nCells * sizeof(float));
}

/* a map of the caller's in the place of an interpolation */
sf3d_error_t DeviceSolver::meteo_upload(int var, const float* src)
{
    MeteoCache& K = impl_->meteo;
    const sf3d_error_t e = raster_upload(K.base + (1 + (size_t)K.nProxies + (size_t)var) * K.nCells, src, (size_t)K.nCells * sizeof(float));
    if (e == SF3D_OK) K.produced[var] = true;
    return e;
}

/* what the radiation block reads of this one: the map of a variable, safe once meteo_produced says the block is on the caller's raster
 * and an interpolation of the variable has run (until then the map holds the flag) */
bool DeviceSolver::meteo_produced(int var, uint32_t nRows, uint32_t nCols) const
{
    return impl_ && impl_->meteo.base && var >= 0 && var < METEO_VARIABLES && impl_->meteo.nRows == nRows && impl_->meteo.nCols == nCols && impl_->meteo.produced[var];
}
static const float* meteo_map(const MeteoCache& K, int var) { return K.base + (1 + (size_t)K.nProxies + (size_t)var) * K.nCells; }

double DeviceSolver::meteo_kernel_ms() const { return impl_ ? impl_->meteo.lastMs : 0.; }
#endif
