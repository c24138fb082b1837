/* part of sf3d_solver.hip (included there after the crop maps) - the two calls Project3D::assignTranspiration makes for every crop cell,
 * every hour (src/project3D/project3D.cpp:2487-2498), on the device:
 *   k_root_cell    Crit3DCrop::computeRootLength3D (agrolib/crop/crop.cpp:651-691) over root::getRootLengthDD (agrolib/crop/root.cpp:139-170):
 *                  root length and depth of every cell, and the cell's key into the density table;
 *   k_root_table   root::computeRootDensity3D (root.cpp:505-633) over cardioidDistribution / cylindricalDistribution (root.cpp:255-364), once,
 *                  at initialisation, for every key that can occur: one thread per (land unit, soil, number of rooted atoms);
 *   k_root_gather  the density maps: every cell reads the vector of its key.
 * The density vector of a cell depends on its land unit, its soil and numberOfRootedLayers = round(min(currentRootLength, totalDepth) / 0.01)
 * only (root.cpp:535-553: the atom clamp is a function of the three), so the reference's per-cell, per-hour recomputation is the same few
 * thousand vectors over and over; here they are computed once.  No atomics, no reduction, no per-thread arrays: the thin-layer density
 * is evaluated twice (one pass for rootDensitySum, one for the binning) instead of being stored.
 *
 * The bar is the compiled reference's bits (tests/golden/root_density.npz): the same double operations in the same order
 * (-ffp-contract=off), rootDensitySum added over the atoms and rootDensitySumSubset over the layers as the reference adds them.  In the
 * object code of the pin build (g++ -O2) std::exp is a call of the library's (fexp here), log(9.), log(1 / 0.99 - 1), log(0.2) and
 * log(0.05) are folded constants (the literals below), round is the C one; atan2 is evaluated on the host (lunette[] depends on two
 * integers only) with the C library and uploaded as a triangular table.
 *
 * Kept from the reference on purpose:
 *  - cylindricalDistribution normalises the lower half of its 2 m values only;
 *  - PI is 3.1415926535898 (commonConstants.h:249);
 *  - the early returns leave zeros in the density and NODATA in firstRootLayer / lastRootLayer (Crit3DRoot::clear);
 *  - a GAMMA_DISTRIBUTION unit becomes a cardioid (root.cpp:530-533).
 * The per-cell and per-row text compiles for the host too (tests/root_host.cpp defines SF3D_ROOT_HOST). */

#ifndef SF3D_ROOT_HOST
#define SF3D_ROOT_FN __device__ __forceinline__
#endif

#define ROOT_NODATA (-9999)
#define ROOT_EPSILON 0.00001
#define ROOT_CYLINDER 0                       /* rootDistributionType, agrolib/crop/root.h:11: the other two are the cardioid here */
#define ROOT_LINEAR 0                         /* rootGrowthType, root.h:14 */
#define ROOT_LOGISTIC 2
#define ROOT_INI_LOG 2.1972245773362196       /* log(9.) */
#define ROOT_FIL_LOG (-4.595119850134584)     /* log(1 / 0.99 - 1) */
#define ROOT_LOG_02 (-1.6094379124341003)     /* log(0.2) */
#define ROOT_LOG_005 (-2.995732273553991)     /* log(0.05) */

/* root::getRootLengthDD, root.cpp:139-170 */
SF3D_ROOT_FN double root_length_dd(const RootUnitDev& u, double actualRootDepthMax, double currentDD)
{
    if (currentDD <= 1) return 0.;
    const double maxRootLength = actualRootDepthMax - u.rootDepthMin;
    if (currentDD > u.degreeDaysRootGrowth) return maxRootLength;
    double currentRootLength = ROOT_NODATA;
    if (u.growth == ROOT_LINEAR)
        currentRootLength = maxRootLength * (currentDD / u.degreeDaysRootGrowth);
    else if (u.growth == ROOT_LOGISTIC) {
        const double iniLog = ROOT_INI_LOG, filLog = ROOT_FIL_LOG;
        const double k = -(iniLog - filLog) / (u.degreeDaysEmergence - u.degreeDaysRootGrowth);
        const double b = -(filLog + k * u.degreeDaysRootGrowth);
        const double logMax = actualRootDepthMax / (1 + fexp(-b - k * u.degreeDaysRootGrowth));
        const double logMin = actualRootDepthMax / (1 + fexp(-b));
        const double deformationFactor = (logMax - logMin) / maxRootLength;
        currentRootLength = 1.0 / deformationFactor * (actualRootDepthMax / (1.0 + fexp(-b - k * currentDD)) - logMin);
    }
    return currentRootLength;
}

/* one cell of k_root_cell; units: the unit table (v.nUnits entries) */
SF3D_ROOT_FN void root_cell(const RootView& v, const RootUnitDev* units, uint32_t c)
{
    const float flag = v.flag;
    double length = (double)flag, depth = (double)flag;
    int32_t first = (int32_t)flag, last = (int32_t)flag, key = -1;
    const int32_t ci = v.cropIndex[c], si = v.soilIndex[c];
    const float ddF = v.dd[c];
    bool cell = !(v.mine && !v.mine[c]) && !snow_eqf(v.dem[c], flag) && ci >= 0 && ci < (int32_t)v.nUnits && si >= 0 && si < (int32_t)v.nSoils
                && !snow_eqf(ddF, flag) && !snow_eq((double)ddF, (double)ROOT_NODATA);
    int32_t row0 = -1;
    if (cell) { row0 = v.pairRow[(uint32_t)ci * v.nSoils + (uint32_t)si]; cell = row0 >= 0; }
    if (cell) {
        const RootUnitDev& u = units[ci];
        const double totalSoilDepth = v.soilDepth[si];
        double currentDegreeDays = ddF;
        /* computeRootLength3D, crop.cpp:651-691 */
        const double actualRootDepthMax = snow_eq(totalSoilDepth, (double)ROOT_NODATA) ? u.rootDepthMax : ((totalSoilDepth < u.rootDepthMax) ? totalSoilDepth : u.rootDepthMax);
        if (u.isRootStatic) length = actualRootDepthMax - u.rootDepthMin;
        else if (currentDegreeDays <= 0) length = 0.0;
        else if (currentDegreeDays > u.degreeDaysRootGrowth) length = actualRootDepthMax - u.rootDepthMin;
        else {
            currentDegreeDays = (currentDegreeDays < 1.0) ? 1.0 : currentDegreeDays;                       /* std::max(., 1.0) */
            length = root_length_dd(u, actualRootDepthMax, currentDegreeDays);
        }
        depth = u.rootDepthMin + length;
        /* the key: the pair's row of numberOfRootedLayers (root.cpp:540); row 0 also serves currentRootLength <= 0 */
        int32_t n = 0;
        if (length > 0) {
            const double r = round(((totalSoilDepth < length) ? totalSoilDepth : length) / 0.01);          /* std::min(length, totalDepth) */
            const int32_t maxN = v.soilMaxN[si];
            n = (r >= (double)maxN) ? maxN : ((r > 0) ? (int32_t)r : 0);
        }
        key = row0 + n;
        first = v.rowLayers[2 * (size_t)key];
        last = v.rowLayers[2 * (size_t)key + 1];
    }
    v.length[c] = length; v.depth[c] = depth;
    v.first[c] = first; v.last[c] = last; v.key[c] = key;
}

/* one row of the density table: computeRootDensity3D on a fresh Crit3DRoot whose currentRootLength rounds to rowN rooted atoms */
SF3D_ROOT_FN void root_table_row(const RootTableView& t, uint32_t r)
{
    const RootUnitDev u = t.units[t.rowUnit[r]];
    const uint32_t s = (uint32_t)t.rowSoil[r];
    const int n = t.rowN[r];
    const uint32_t nl = t.nrLayers;
    const size_t stride = t.nRows;
    double* dens = t.table + r;                                       /* dens[l * stride] */
    for (uint32_t l = 0; l < nl; ++l) dens[l * stride] = 0.0;
    int32_t first = ROOT_NODATA, last = ROOT_NODATA;
    const double totalDepth = t.soilDepth[s];
    const int nrAtoms = (int)(totalDepth * 100) + 1;
    const int top = (int)round(u.rootDepthMin / 0.01);
    int m = n;
    if (top + m > nrAtoms) m = nrAtoms - top;
    /* m <= 0 after the clamp: the reference hands a negative count on as unsigned; here the row stays empty (DESIGN.md 16) */
    if (nl > 1 && n > 0 && top >= 0 && m > 0 && (uint32_t)m <= t.lunetteMax) {
        const bool cylinder = u.rootShape == ROOT_CYLINDER;
        const double dm = (double)(uint32_t)m;
        /* cardioidDistribution, root.cpp:255-318 */
        const double shapeFactor = (u.shapeDeformation < 1.0) ? 1.0 : ((2.0 < u.shapeDeformation) ? 2.0 : u.shapeDeformation);     /* std::clamp */
        const double* lunette = t.lunette + (size_t)(m - 1) * m / 2;
        const double liMin = -ROOT_LOG_02 / dm, liMax = -ROOT_LOG_005 / dm;
        const double k = liMin + (liMax - liMin) * (shapeFactor - 1);
        /* cylindricalDistribution, root.cpp:321-364 */
        const double cylinder0 = 1. / (double)(2u * (uint32_t)m);
        const double deltaDeformation = u.shapeDeformation - 1;
        /* pass 1: rootDensitySum over i = 0 .. 2 m - 1 */
        double sum = 0.;
        if (cylinder) {
            double deformation = u.shapeDeformation;
            for (int i = 0; i < m; ++i) { const double c = cylinder0 * deformation; deformation -= deltaDeformation / dm; sum += c; }
            for (int i = m; i < 2 * m; ++i) { deformation -= deltaDeformation / dm; const double c = cylinder0 * deformation; sum += c; }
        } else {
            for (int i = 0; i < 2 * m; ++i) {
                const int j = (i < m) ? i : 2 * m - 1 - i;
                const double lunetteDensity = (j == 0) ? lunette[0] : lunette[j] - lunette[j - 1];
                sum += lunetteDensity * fexp(-k * (i + 0.5));
            }
        }
        /* pass 2: the thin layers top .. top + m - 1 in order, binned into the layers (root.cpp:566-586; the atoms above and below hold 0) */
        const double maxLayerDepth = t.layerDepth[nl - 1] + t.layerThickness[nl - 1] * 0.5;
        double rootDensitySum = 0.;
        double deformation = u.shapeDeformation;
        for (int i = 0; i < m; ++i) {
            double pair[2];
            for (int h = 0; h < 2; ++h) {
                const int i2 = 2 * i + h;
                if (cylinder) {
                    if (i2 < m) { pair[h] = cylinder0 * deformation; deformation -= deltaDeformation / dm; }
                    else { deformation -= deltaDeformation / dm; pair[h] = cylinder0 * deformation / sum; }
                } else {
                    const int j = (i2 < m) ? i2 : 2 * m - 1 - i2;
                    const double lunetteDensity = (j == 0) ? lunette[0] : lunette[j] - lunette[j - 1];
                    pair[h] = lunetteDensity * fexp(-k * (i2 + 0.5)) / sum;
                }
            }
            const double thin = pair[0] + pair[1];
            const int atom = top + i;
            const double currentDepth = (double)atom * 0.01;
            if (!(currentDepth <= maxLayerDepth && atom < nrAtoms)) break;
            for (uint32_t l = 0; l < nl; ++l) {
                const double upperDepth = t.layerDepth[l] - t.layerThickness[l] * 0.5;
                const double lowerDepth = t.layerDepth[l] + t.layerThickness[l] * 0.5;
                if (currentDepth >= upperDepth && currentDepth <= lowerDepth) {
                    dens[l * stride] += thin;
                    rootDensitySum += thin;
                    break;
                }
            }
        }
        if (!(rootDensitySum <= ROOT_EPSILON)) {
            double rootDensitySumSubset = 0.;
            for (uint32_t l = 0; l < nl; ++l) {
                const double fraction = t.layerFrac[(size_t)s * nl + l];
                if (fraction >= 0) {
                    const double d = dens[l * stride] * fraction;
                    dens[l * stride] = d;
                    rootDensitySumSubset += d;
                }
            }
            if (rootDensitySumSubset > ROOT_EPSILON && fabs(rootDensitySumSubset - rootDensitySum) > ROOT_EPSILON) {
                const double ratio = rootDensitySum / rootDensitySumSubset;
                for (uint32_t l = 0; l < nl; ++l) dens[l * stride] *= ratio;
            }
            for (uint32_t l = 0; l < nl; ++l)
                if (dens[l * stride] > ROOT_EPSILON) {
                    if (first == ROOT_NODATA) first = (int32_t)l;
                    last = (int32_t)l;
                }
        }
    }
    t.rowLayers[2 * (size_t)r] = first;
    t.rowLayers[2 * (size_t)r + 1] = last;
}

/* the density maps of layers layer0 .. layer0 + layerCount - 1: out[k][cell] = table[layer0 + k][key[cell]], the flag where the cell has no key */
SF3D_ROOT_FN void root_gather_cell(const RootView& v, uint32_t c)
{
    const int32_t key = v.key[c];
    const bool has = key >= 0 && (uint32_t)key < v.nRows;
    const double flag = (double)v.flag;
    for (uint32_t k = 0; k < v.layerCount; ++k)
        v.out[(size_t)k * v.nCells + c] = has ? v.table[(size_t)(v.layer0 + k) * v.nRows + (uint32_t)key] : flag;
}

#ifndef SF3D_ROOT_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_root_cell(RootView v)
{
    __shared__ RootUnitDev units[CROP_MAX_UNITS];
    {   /* the unit table: consecutive words from memory into LDS, read from there (every lane its own unit) */
        const uint32_t* src = reinterpret_cast<const uint32_t*>(v.units);
        uint32_t* dst = reinterpret_cast<uint32_t*>(units);
        const uint32_t words = v.nUnits * (uint32_t)(sizeof(RootUnitDev) / 4);
        for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) dst[k] = src[k];
    }
    fm_init();
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    root_cell(v, units, c);
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_root_table(RootTableView t)
{
    fm_init();
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= t.nRows) return;
    root_table_row(t, r);
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_root_gather(RootView v)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    root_gather_cell(v, c);
}

/* ---- host side: the per-cell block, one block of tables and the gathered density maps; calls go through the shared raster path at the end
 * of sf3d_maps.inc. */
enum { ROOT_T_UNITS = 0, ROOT_T_SOIL_DEPTH, ROOT_T_LAYER_DEPTH, ROOT_T_LAYER_THICKNESS, ROOT_T_LAYER_FRAC, ROOT_T_LUNETTE, ROOT_T_TABLE, ROOT_T_SOIL_MAXN,
       ROOT_T_PAIR_ROW, ROOT_T_ROW_UNIT, ROOT_T_ROW_SOIL, ROOT_T_ROW_N, ROOT_T_ROW_LAYERS, ROOT_T_END };

sf3d_error_t DeviceSolver::root_free()
{
    if (!impl_) return SF3D_OK;
    raster_release({impl_->root.cells, impl_->root.tables, impl_->root.out});
    impl_->root = RootCache();
    return SF3D_OK;
}

static void root_view(RootView& v, const RootCache& K, float flag)
{
    const auto map = [&K](int k) { return raster_cell_map(K.cells, K.nCells, k); };
    v.length = (double*)map(ROOT_MAP_LENGTH); v.depth = (double*)map(ROOT_MAP_DEPTH);
    v.dem = (const float*)map(ROOT_MAP_DEM); v.dd = (const float*)map(ROOT_MAP_DD);
    v.cropIndex = (const int32_t*)map(ROOT_MAP_CROP); v.soilIndex = (const int32_t*)map(ROOT_MAP_SOIL);
    v.first = (int32_t*)map(ROOT_MAP_FIRST); v.last = (int32_t*)map(ROOT_MAP_LAST); v.key = (int32_t*)map(ROOT_MAP_KEY);
    v.units = (const RootUnitDev*)(K.tables + K.off[ROOT_T_UNITS]);
    v.soilDepth = (const double*)(K.tables + K.off[ROOT_T_SOIL_DEPTH]);
    v.soilMaxN = (const int32_t*)(K.tables + K.off[ROOT_T_SOIL_MAXN]);
    v.pairRow = (const int32_t*)(K.tables + K.off[ROOT_T_PAIR_ROW]);
    v.rowLayers = (const int32_t*)(K.tables + K.off[ROOT_T_ROW_LAYERS]);
    v.table = (const double*)(K.tables + K.off[ROOT_T_TABLE]);
    v.out = K.out;
    v.nCells = K.nCells; v.nUnits = K.nUnits; v.nSoils = K.nSoils; v.nRows = K.nRows; v.nrLayers = K.nrLayers; v.layer0 = 0; v.layerCount = 0;
    v.flag = flag;
}

sf3d_error_t DeviceSolver::root_alloc(const RootSetup& S)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    root_free();
    Impl& I = *impl_;
    RootCache& K = I.root;
    const size_t n = S.nCells, nl = S.nrLayers, rows = S.nRows;
    const size_t lunetteCount = (size_t)S.lunetteMax * (S.lunetteMax + 1) / 2;
    /* the tables: the 8-byte ones first */
    const size_t bytes[ROOT_T_END] = {
        (size_t)CROP_MAX_UNITS * sizeof(RootUnitDev), S.nSoils * sizeof(double), nl * sizeof(double), nl * sizeof(double), S.nSoils * nl * sizeof(double),
        (lunetteCount ? lunetteCount : 1) * sizeof(double), rows * nl * sizeof(double), S.nSoils * sizeof(int32_t), (size_t)S.nUnits * S.nSoils * sizeof(int32_t),
        rows * sizeof(int32_t), rows * sizeof(int32_t), rows * sizeof(int32_t), 2 * rows * sizeof(int32_t)};
    const void* src[ROOT_T_END] = {S.units, S.soilDepth, S.layerDepth, S.layerThickness, S.layerFrac, S.lunette, nullptr, S.soilMaxN, S.pairRow, S.rowUnit, S.rowSoil,
                                   S.rowN, nullptr};
    const size_t srcBytes[ROOT_T_END] = {S.nUnits * sizeof(RootUnitDev), bytes[1], bytes[2], bytes[3], bytes[4], lunetteCount * sizeof(double), 0, bytes[7], bytes[8],
                                         bytes[9], bytes[10], bytes[11], 0};
    RASTER_TRY(hipMalloc((void**)&K.cells, (size_t)ROOT_MAP_WORDS * n * 4));
    K.nCells = S.nCells; K.nUnits = S.nUnits; K.nSoils = S.nSoils; K.nRows = S.nRows; K.nrLayers = S.nrLayers; K.lunetteMax = S.lunetteMax;
    e = raster_tables(K.tables, K.off, ROOT_T_END, bytes, src, srcBytes);
    if (e != SF3D_OK) return e;
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, ROOT_MAP_DEM), S.dem, n * 4, hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, ROOT_MAP_CROP), S.cropIndex, n * 4, hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, ROOT_MAP_SOIL), S.soilIndex, n * 4, hipMemcpyHostToDevice, I.stream));
    /* before the first compute every output holds the flag: the degree days are the flag everywhere and k_root_cell runs once below */
    {
        const std::vector<float> empty(n, S.flag);
        RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, ROOT_MAP_DD), empty.data(), n * 4, hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipStreamSynchronize(I.stream));
    }
    if (rows) {
        RootTableView t{};
        t.units = (const RootUnitDev*)(K.tables + K.off[ROOT_T_UNITS]);
        t.soilDepth = (const double*)(K.tables + K.off[ROOT_T_SOIL_DEPTH]);
        t.layerDepth = (const double*)(K.tables + K.off[ROOT_T_LAYER_DEPTH]);
        t.layerThickness = (const double*)(K.tables + K.off[ROOT_T_LAYER_THICKNESS]);
        t.layerFrac = (const double*)(K.tables + K.off[ROOT_T_LAYER_FRAC]);
        t.lunette = (const double*)(K.tables + K.off[ROOT_T_LUNETTE]);
        t.rowUnit = (const int32_t*)(K.tables + K.off[ROOT_T_ROW_UNIT]);
        t.rowSoil = (const int32_t*)(K.tables + K.off[ROOT_T_ROW_SOIL]);
        t.rowN = (const int32_t*)(K.tables + K.off[ROOT_T_ROW_N]);
        t.table = (double*)(K.tables + K.off[ROOT_T_TABLE]);
        t.rowLayers = (int32_t*)(K.tables + K.off[ROOT_T_ROW_LAYERS]);
        t.nRows = S.nRows; t.nrLayers = S.nrLayers; t.lunetteMax = S.lunetteMax;
        e = raster_launch(k_root_table, rows, t, K.lastMs[1]);
        if (e != SF3D_OK) return e;
    }
    RootView v{};
    root_view(v, K, S.flag);
    e = raster_launch(k_root_cell, n, v, K.lastMs[0]);
    K.lastMs[0] = 0.;
    return e;
}

sf3d_error_t DeviceSolver::root_compute(const float* dd, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    RootCache& K = I.root;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    if (dd) RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, ROOT_MAP_DD), dd, n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    RootView v{};
    sf3d_error_t e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    root_view(v, K, flag);
    if (!dd) v.dd = crop_degree_days(I.crop);                                   /* degreeDaysMap of the crop block */
    e = raster_launch(k_root_cell, n, v, K.lastMs[0]);
    if (e == SF3D_OK) K.computed = true;
    return e;
}

sf3d_error_t DeviceSolver::root_download(int map, void* dst)
{
    const RootCache& K = impl_->root;
    return raster_download(dst, raster_cell_map(K.cells, K.nCells, map), (size_t)K.nCells * (map < 2 ? 8 : 4));
}

/* layer < 0: every layer, [layer][cell] */
sf3d_error_t DeviceSolver::root_density(int layer, double* dst, float flag)
{
    Impl& I = *impl_;
    RootCache& K = I.root;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    if (!K.out) RASTER_TRY(hipMalloc((void**)&K.out, (size_t)K.nrLayers * n * sizeof(double)));
    RootView v{};
    root_view(v, K, flag);
    v.layer0 = layer < 0 ? 0 : (uint32_t)layer;
    v.layerCount = layer < 0 ? K.nrLayers : 1;
    const sf3d_error_t e = raster_launch(k_root_gather, n, v, K.lastMs[2]);
    return e != SF3D_OK ? e : raster_download(dst, K.out, (size_t)v.layerCount * n * sizeof(double));
}

/* what the sink block asks before it reads this block's maps and its density table */
bool DeviceSolver::root_computed(uint32_t nCells, uint32_t nrLayers) const
{
    return impl_ && impl_->root.cells && impl_->root.computed && impl_->root.nCells == nCells && impl_->root.nrLayers == nrLayers;
}

/* which: 0 k_root_cell, 1 k_root_table, 2 k_root_gather */
double DeviceSolver::root_kernel_ms(int which) const { return (impl_ && which >= 0 && which < 3) ? impl_->root.lastMs[which] : 0.; }
uint32_t DeviceSolver::root_table_rows() const { return impl_ ? impl_->root.nRows : 0; }
#endif
