/* part of sf3d_solver.hip (included there after sf3d_localproxies.inc, whose lists, Marquardt runs, proxy fit, detrending, retrend and
 * wave primitives it uses) - air and dew-point temperature with GLOCAL detrending on the device: what
 * Project::interpolationDemGlocalDetrending (agrolib/project/project.cpp:3267-3384) does with useMultipleDetrending and glocal set, local
 * detrending, topographic distance and lapse-rate codes off:
 *   1. glocalDetrendingFitting (agrolib/interpolation/interpolation.cpp:2239-2294), per macro area over the area's stations that have a
 *      point this hour, in the area's order: multipleDetrendingElevationFitting(..., isWeighted = false) (:1862-1953: proxyValidity, no
 *      minimum of points) over the UNWEIGHTED bestFittingMarquardt_nDimension (agrolib/mathFunctions/furtherMathFunctions.cpp:1433-1529)
 *      with computeR2adjusted (:1175) and computeRMSE (:1324); detrendingElevation; multipleDetrendingOtherProxiesFitting (:1975-2171)
 *      with regression weights 1 and without the rule of :2140;
 *   2. macroAreaDetrending (:1759-1829): the subset rebuilt from ALL the area's points - the prunings of 1 do not carry over - and
 *      detrended with the area's parameters: detrendingElevation, then detrendingOtherProxies, which may erase stations;
 *   3. the cell loop (project.cpp:3343-3379), per (area, cell, weight): getSignificantProxyValuesXY (:2650-2677), interpolate() over
 *      the area's kept stations with the neighbour search of the meteo block, retrend through getMultipleDetrendingValues, and the blend.
 * THE SERIAL ORDER: the reference's area loop is an OpenMP loop, its order is not defined; here the areas are visited in index order,
 * which is what the loop does on one thread.  A cell's value depends on that order (a later area overwrites with NODATA, float sums).
 *
 * k_glocal_areas: one wave64 per macro area, four areas per 256-thread block - steps 1 and 2.  The area's list lies in LDS in the area's
 * order (LdList); the call's point table stays in global memory and is read through the list's point index.  Lane k runs the Marquardt
 * fit from first guess k and every lane walks the results in the order of k, as k_localdetrend does; the proxies' fit is
 * sf3d_localproxies.inc's (lp_others) with unit weights and minPointsLocal 0 in the set-up, which switches the rule of :2140 off.  THE
 * LIST-ORDER RULE of sf3d_localdetrend.inc holds: no atomics, tree reductions or shuffles in any value.
 * The unweighted fittingMarquardt_nDimension (furtherMathFunctions.cpp:2125-2283) is the weighted one (ld_marquardt) with every weight 1:
 * error * error * 1 * 1, P[i] * (1 * P[j]) and P[i] * 1 * (y - firstEst) are the unweighted terms to the bit, the pivots (max(.,
 * EPSILON)), the clamps ((new > max) && (lambda < 1000)) and the newSSE == NODATA exit are the same text in the reference: it stands
 * once.  What differs is the choice among the first guesses (gl_fit): a guess whose result leaves [min, max] is skipped; the scores are
 * computeR2adjusted and computeRMSE; the double-inversion rule (par[0] + par[2]) < maxZ gates the replacement, not the first acceptance,
 * and keeps its last value across skipped guesses; the refit after bestR2 < 0 runs only where some guess was scored.
 *
 * k_glocal_cells: one thread per DEM cell, as k_meteo_idw - step 3.  The host turned the area-major cell lists into a cell-major table
 * (per cell its (area, weight) pairs, ascending area index) when the areas were set; the thread walks its pairs in that order.  The
 * methods are sf3d_meteo.inc's (meteo_idw, meteo_shepard with its ten-slot list), called over the area's kept stations in global memory.
 * An interpolate() that gives NODATA raises a flag word through a plain store of 1: the entry point then fails as the reference does.
 *
 * Kept from the reference on purpose:
 *  - a cell whose significant proxy value is missing for area a is SET to NODATA there: what earlier areas added is lost, a later area
 *    starts again from NODATA;
 *  - raster += interpolatedValue * weight is a double product (exact: two floats) added to the float cell in double and rounded once;
 *    the first assignment rounds the product alone; the weights are not normalised;
 *  - the grid starts at the header's flag and is tested against NODATA.
 *
 * Every loop is bounded: list lengths <= METEO_MAX_STATIONS, a fit ends after 1 001 iterations, the proxies' after 101, the pair walk at
 * the cell's row of the table, the neighbour search is the meteo block's.
 * The per-area and per-cell texts also compile for the host (tests/glocal_host.cpp defines SF3D_METEO_HOST): one lane, the same text. */

#define GL_SKIPPED (-1.0)                   /* in the RMSE slot of a fit's record: the guess left its range (an RMSE is never negative) */

/* computeR2adjusted and computeRMSE (furtherMathFunctions.cpp:1175-1194, 1324-1340) of the fit `par` over the elevation points */
template <int F> SF3D_METEO_FN void gl_scores(double* par, const LdList& L, uint32_t n, uint32_t nrData, double& R2, double& RMSE)
{
    double meanObs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (L.h[i] == (float)LD_NODATA) continue;
        meanObs += (double)L.val[i];
    }
    meanObs /= (double)nrData;
    double RSS = 0, TSS = 0, sumResiduals = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf == (float)LD_NODATA) continue;
        const double y = L.val[i];
        const double ySim = ld_func<F>((double)hf, par);
        RSS += (y - ySim) * (y - ySim);
        TSS += (y - meanObs) * (y - meanObs);
        sumResiduals += (y - ySim) * (y - ySim);
    }
    R2 = 1 - RSS / TSS;
    RMSE = __builtin_sqrt(sumResiduals / (double)nrData);
}

/* the unweighted bestFittingMarquardt_nDimension (furtherMathFunctions.cpp:1433-1529), then the significance rule and detrendingElevation
 * (interpolation.cpp:1937-1972).  The list's weights are 1.  Returns whether the height proxy is significant; par: the area's parameters */
template <int F, int NP> SF3D_METEO_FN bool gl_fit(const LdSetup& s, const LdList& L, uint32_t n, uint32_t nrData, double* par, double& bestR2)
{
    const double* pmin = s.table;
    const double* pmax = s.table + LD_MAX_PARAMETERS;
    const double* pdelta = s.table + 2 * LD_MAX_PARAMETERS;
    const double* guess = s.table + 3 * LD_MAX_PARAMETERS;
    const uint32_t nGuess = (uint32_t)s.nFirstGuess < LD_MAX_FIRST_GUESS ? (uint32_t)s.nFirstGuess : LD_MAX_FIRST_GUESS;
    for (uint32_t k = ld_lane(); k < nGuess; k += LD_LANES) {
        double p[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) p[j] = guess[k * LD_MAX_PARAMETERS + j];
        ld_marquardt<F, NP>(p, pmin, pmax, pdelta, L, n);
        bool rangeFlag = true;
#pragma unroll
        for (int j = 0; j < NP; ++j) rangeFlag = rangeFlag && !(p[j] < pmin[j] || p[j] > pmax[j]);
        double R2 = 0, RMSE = GL_SKIPPED;
        if (rangeFlag) gl_scores<F>(p, L, n, nrData, R2, RMSE);
#pragma unroll
        for (int j = 0; j < NP; ++j) L.fit[k * LD_FIT_STRIDE + j] = p[j];
        L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS] = R2;
        L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS + 1] = RMSE;
    }
    ld_sync();
    /* the highest station of the fit */
    double maxZ = LD_NODATA;
    bool first = true;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf == (float)LD_NODATA) continue;
        if (first || (double)hf > maxZ) maxZ = hf;
        first = false;
    }
    /* the choice, in the order of k */
    bestR2 = LD_NODATA;
    double bestRMSE = LD_NODATA;
    bool scored = false;                                                    /* RMSEindex != NODATA */
    uint32_t RMSEindex = 0;
    bool isValid = true;
#pragma unroll
    for (int j = 0; j < NP; ++j) par[j] = 0;
    for (uint32_t k = 0; k < nGuess; ++k) {
        const double R2 = L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS], RMSE = L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS + 1];
        if (RMSE == GL_SKIPPED) continue;
        if (ld_eqd(bestRMSE, LD_NODATA) || RMSE < bestRMSE) { bestRMSE = RMSE; RMSEindex = k; scored = true; }
        if (NP > 4) isValid = (L.fit[k * LD_FIT_STRIDE] + L.fit[k * LD_FIT_STRIDE + 2]) < maxZ;      /* double inversion only */
        if (ld_eqd(bestR2, LD_NODATA) || (R2 > (bestR2 + LD_DELTA_R2) && isValid)) {
#pragma unroll
            for (int j = 0; j < NP; ++j) par[j] = L.fit[k * LD_FIT_STRIDE + j];
            bestR2 = R2;
        }
    }
    if (bestR2 < 0 && scored) {
#pragma unroll
        for (int j = 0; j < NP; ++j) par[j] = guess[RMSEindex * LD_MAX_PARAMETERS + j];
        ld_marquardt<F, NP>(par, pmin, pmax, pdelta, L, n);
    }
    bool nodataOrZero = false;
#pragma unroll
    for (int j = 0; j < NP; ++j) nodataOrZero = nodataOrZero || ld_eqd(par[j], LD_NODATA) || ld_eqd(par[j], 0);
    const bool significant = !ld_eqd(bestR2, LD_NODATA) || !nodataOrZero;
    ld_sync();
    return significant;
}

/* detrendingElevation (interpolation.cpp:1956-1972) over the list with a copy of the parameters, as the reference takes one */
SF3D_METEO_FN void gl_detrend_elevation(const LdSetup& s, const LdList& L, uint32_t n, const double* par)
{
    double q[LD_MAX_PARAMETERS];
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) q[j] = par[j];
    for (uint32_t i = ld_lane(); i < n; i += LD_LANES) {
        const float detrendValue = (float)ld_height_function(s, (double)L.h[i], q);
        L.val[i] -= detrendValue;
    }
    ld_sync();
}

/* the area's stations that have a point this hour, in the area's order: the subset of glocalDetrendingFitting and of macroAreaDetrending
 * (the entry point refuses a repeated point index, so the two are one list).  L.d holds the entry's place in the area's station list */
SF3D_METEO_FN uint32_t gl_fill(const GlocalAreasView& v, uint32_t begin, uint32_t end, const LdList& L, uint8_t* member)
{
    uint32_t n = 0;
    for (uint32_t base = begin; base < end; base += LD_LANES) {
        const uint32_t l = base + ld_lane();
        const int32_t point = (l < end) ? v.listPoint[l] : -1;
        const bool in = point >= 0 && point < METEO_MAX_STATIONS;
        const uint64_t mask = ld_ballot(in);
        if (in) {
            const uint32_t at = n + ld_below(mask);
            L.idx[at] = (uint16_t)point; L.d[at] = (float)(l - begin); L.h[at] = v.sh[point]; L.val[at] = v.sv[point]; L.w[at] = 1.f;
            member[at] = (uint8_t)(LP_FIT | LP_INTERP);
        }
        n += (uint32_t)__builtin_popcountll(mask);
    }
    ld_sync();
    return n;
}

/* steps 1 and 2 for macro area a; the record, the per-entry outcome and the kept list go to global memory */
SF3D_METEO_FN void gl_area(const GlocalAreasView& v, uint32_t a, const LdList& L, LpCtx& X)
{
    const uint32_t lane = ld_lane();
    const uint32_t begin = v.stationOffset[a];
    const uint32_t all = v.stationOffset[a + 1] - begin;
    const uint32_t end = begin + (all < METEO_MAX_STATIONS ? all : METEO_MAX_STATIONS);
    for (uint32_t l = begin + lane; l < end; l += LD_LANES) { v.detrended[l] = (float)LD_NODATA; v.keptBit[l] = 0; }

    /* 1. the fits */
    uint32_t n = gl_fill(v, begin, end, L, X.member);
    const uint32_t fitted = n;
    double par[LD_MAX_PARAMETERS];
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = LD_NODATA;
    double R2 = LD_NODATA;
    bool significant = false;
    X.mask = 0;
    if (n > 0) {
        if (v.p.heightSlot >= 0) {
            uint32_t nrData = 0;
            for (uint32_t i = 0; i < n; ++i) nrData += (L.h[i] != (float)LD_NODATA) ? 1u : 0u;
            /* proxyValidity of the height over the elevation points; no minimum of points without local detrending (:1885) */
            if (lp_validity(L, X.member, v.sh, n, v.s.stdDevThreshold)) {
                if (v.s.function == LD_PIECEWISE_TWO) significant = gl_fit<LD_PIECEWISE_TWO, 4>(v.s, L, n, nrData, par, R2);
                else if (v.s.function == LD_PIECEWISE_THREE) significant = gl_fit<LD_PIECEWISE_THREE, 5>(v.s, L, n, nrData, par, R2);
                else significant = gl_fit<LD_PIECEWISE_THREE_FREE, 6>(v.s, L, n, nrData, par, R2);
                if (significant) gl_detrend_elevation(v.s, L, n, par);
                else {
#pragma unroll
                    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = LD_NODATA;
                }
            }
        }
        if (X.nOthers > 0) (void)lp_others(v.s, v.p, L, X, n);                 /* leaves X.mask and the lines in vec[LP_P]; its list is spent */
        ld_sync();

        /* 2. the subset again, from all the area's points, detrended with what 1 left */
        n = gl_fill(v, begin, end, L, X.member);
        if (significant) gl_detrend_elevation(v.s, L, n, par);
        if (X.mask != 0) lp_detrend(L, X, n);
        for (uint32_t i = lane; i < n; i += LD_LANES) {
            if (!(X.member[i] & LP_INTERP)) continue;
            const uint32_t l = begin + (uint32_t)L.d[i];
            v.detrended[l] = L.val[i]; v.keptBit[l] = 1;
        }
        ld_sync();
        n = lp_compact(L, X.member, n);
        for (uint32_t i = lane; i < n; i += LD_LANES) { v.keptPoint[begin + i] = L.idx[i]; v.keptValue[begin + i] = L.val[i]; }
    }
    if (lane == 0) {
        GlocalAreaDev& o = v.area[a];
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = par[j];
        o.r2 = (float)R2; o.significant = significant ? 1 : 0; o.fitted = fitted; o.kept = n; o.mask = X.mask; o.reserved = 0;
        for (uint32_t p = 0; p < METEO_MAX_PROXIES; ++p) { o.line[p][0] = LD_NODATA; o.line[p][1] = LD_NODATA; o.proxySignificant[p] = 0; }
        uint32_t j = 0;
        for (uint32_t r = 0; r < X.nOthers; ++r) {
            if (!((X.mask >> r) & 1u)) continue;
            o.line[j][0] = X.vec[LP_P * LP_NP + 2 * j]; o.line[j][1] = X.vec[LP_P * LP_NP + 2 * j + 1];
            o.proxySignificant[v.p.slot[r]] = 1;
            ++j;
        }
    }
}

/* the distances of computeDistances from the cell to an area's kept stations, and the stations as the methods index them */
struct GlDistance {
    const double* sx;
    const double* sy;
    const uint16_t* point;
    float x, y;
    SF3D_METEO_MEMBER float operator()(uint32_t i) const { return meteo_distance(x, y, sx[point[i]], sy[point[i]]); }
};

/* step 3 for DEM cell c of height z at the float (x, y): the cell's value after every area that covers it, from `start` (the
 * initialised grid's flag) */
SF3D_METEO_FN float gl_cell(const GlocalCellsView& v, uint32_t c, float z, float x, float y, float start)
{
    const MeteoView& m = v.m;
    float cell = start;
    const uint32_t first = v.pairOffset[c];
    const uint32_t last = v.pairOffset[c + 1] < v.nPairs ? v.pairOffset[c + 1] : v.nPairs;
    for (uint32_t k = first; k < last; ++k) {
        const GlocalAreaDev& A = v.area[v.pairArea[k]];
        const float weight = v.pairWeight[k];
        const bool significant = A.significant != 0;
        const uint32_t mask = A.mask;
        /* getSignificantProxyValuesXY */
        bool complete = true;
        if (significant && lp_cell_proxy(m, c, z, v.p.heightSlot) == LD_NODATA) complete = false;
        for (uint32_t r = 0; r < (uint32_t)v.p.nOthers; ++r)
            if (((mask >> r) & 1u) && lp_cell_proxy(m, c, z, v.p.slot[r]) == LD_NODATA) complete = false;
        if (!complete) { cell = (float)LD_NODATA; continue; }
        /* interpolate() over the area's kept stations */
        const uint32_t begin = v.stationOffset[v.pairArea[k]];
        const uint32_t n = A.kept < METEO_MAX_STATIONS ? A.kept : METEO_MAX_STATIONS;
        const uint16_t* point = v.keptPoint + begin;
        const float* value = v.keptValue + begin;
        const GlDistance dist{m.sx, m.sy, point, x, y};
        float result;
        if (v.s.method == METEO_IDW) result = meteo_idw(dist, value, n);
        else {
            /* computeShepardInitialRadius(area, nrPoints, SHEPARD_AVG_NRPOINTS) with the subset's size (interpolation.cpp:812-813) */
            const float radius0 = __builtin_sqrtf(((float)8u * v.s.area) / ((float)3.1415926535898 * (float)n));
            result = meteo_shepard(dist, LdCoord{m.sx, point}, LdCoord{m.sy, point}, value, n, x, y, radius0, v.s.method == METEO_SHEPARD_MODIFIED);
        }
        if (meteo_eqf(result, (float)LD_NODATA)) {
            result = (float)LD_NODATA;
            *v.failed = 1u;                                                     /* isOk = false */
        } else if (v.s.useDetrending) {
            double par[LD_MAX_PARAMETERS];
#pragma unroll
            for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = A.parameters[j];
            result += lp_retrend(m, v.s, v.p, (uint32_t)v.p.nOthers, mask, &A.line[0][0], c, z, significant, par);
        }
        const double interpolatedValue = result;
        if (meteo_eqf(cell, (float)LD_NODATA)) cell = (float)(interpolatedValue * weight);
        else cell = (float)(cell + interpolatedValue * weight);
    }
    return cell;
}

#ifndef SF3D_METEO_HOST
#define GL_AREAS_PER_BLOCK (SF3D_BLOCK / 64)

__global__ void __launch_bounds__(SF3D_BLOCK) k_glocal_areas(GlocalAreasView)
{
    const GlocalAreasView& v = meteo_kernel_argument<GlocalAreasView>();
    __shared__ double heightsAndWeights[GL_AREAS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ double fit[GL_AREAS_PER_BLOCK][LD_MAX_FIRST_GUESS * LD_FIT_STRIDE];
    __shared__ double work[GL_AREAS_PER_BLOCK][LP_WORK_DOUBLES];
    __shared__ float places[GL_AREAS_PER_BLOCK][METEO_MAX_STATIONS], values[GL_AREAS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ uint16_t indices[GL_AREAS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ uint8_t members[GL_AREAS_PER_BLOCK][METEO_MAX_STATIONS];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t a = blockIdx.x * GL_AREAS_PER_BLOCK + wave;
    if (a >= v.nAreas) return;
    LdList L;
    L.idx = indices[wave]; L.d = places[wave]; L.val = values[wave];
    L.h = (float*)heightsAndWeights[wave]; L.w = L.h + METEO_MAX_STATIONS; L.wt = heightsAndWeights[wave];
    L.lanes = nullptr; L.fit = fit[wave];                                      /* no selection here: its lane maxima have no room */
    LpCtx X;
    X.rows = v.rows; X.member = members[wave]; X.vec = work[wave]; X.mat = fit[wave];
    X.nOthers = (uint32_t)v.p.nOthers < LP_MAX_OTHERS ? (uint32_t)v.p.nOthers : LP_MAX_OTHERS; X.mask = 0;
    gl_area(v, a, L, X);
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_glocal_cells(GlocalCellsView)
{
    const GlocalCellsView& v = meteo_kernel_argument<GlocalCellsView>();
    const MeteoView& m = v.m;
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m.nCells) return;
    float result = m.flag;
    const float z = m.dem[c];
    if (!(m.mine && !m.mine[c]) && !meteo_eqf(z, m.flag)) {
        float x, y;
        meteo_cell_xy(m, c, x, y);
        result = gl_cell(v, c, z, x, y, m.flag);
    }
    m.out[c] = result;
}

/* ---- host side: the areas' tables and what k_glocal_areas records lie in one block that goes with the meteo block's raster
 * (meteo_free); the call's tables (the fit table, the height row, the other proxies' rows) in another ---- */
enum { GL_T_STATION_OFFSET = 0, GL_T_PAIR_OFFSET, GL_T_PAIR_AREA, GL_T_PAIR_WEIGHT, GL_T_AREA, GL_T_LIST_POINT, GL_T_DETRENDED, GL_T_KEPT_VALUE, GL_T_KEPT_POINT,
       GL_T_KEPT_BIT, GL_T_FAILED, GL_TABLES };
static_assert(GL_TABLES == sizeof(((MeteoCache*)nullptr)->glocalOff) / sizeof(size_t), "MeteoCache::glocalOff holds an offset per table");
static const size_t GL_CALL_BYTES = (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double) + (size_t)(1 + LP_MAX_OTHERS) * METEO_MAX_STATIONS * sizeof(float);

sf3d_error_t DeviceSolver::glocal_free()
{
    if (!impl_) return SF3D_OK;
    MeteoCache& K = impl_->meteo;
    raster_release({K.glocalBlock, K.glocalTables});
    K.glocalBlock = nullptr; K.glocalTables = nullptr; K.glocalBytes = 0; K.glocalAreas = 0; K.glocalList = 0; K.glocalPairs = 0; K.glocalDone = false;
    K.glocalMs[0] = K.glocalMs[1] = 0.;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::glocal_set(const GlocalStatic& g)
{
    glocal_free();
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    RASTER_TRY(hipSetDevice(I.device));
    const size_t n = K.nCells;
    size_t bytes[GL_TABLES], given[GL_TABLES];
    const void* src[GL_TABLES] = {nullptr};
    bytes[GL_T_STATION_OFFSET] = ((size_t)g.nAreas + 1) * sizeof(uint32_t); src[GL_T_STATION_OFFSET] = g.stationOffset;
    bytes[GL_T_PAIR_OFFSET] = (n + 1) * sizeof(uint32_t); src[GL_T_PAIR_OFFSET] = g.pairOffset;
    bytes[GL_T_PAIR_AREA] = (size_t)g.nPairs * sizeof(uint32_t); src[GL_T_PAIR_AREA] = g.pairArea;
    bytes[GL_T_PAIR_WEIGHT] = (size_t)g.nPairs * sizeof(float); src[GL_T_PAIR_WEIGHT] = g.pairWeight;
    bytes[GL_T_AREA] = (size_t)g.nAreas * sizeof(GlocalAreaDev);
    bytes[GL_T_LIST_POINT] = (size_t)g.nList * sizeof(int32_t);
    bytes[GL_T_DETRENDED] = bytes[GL_T_KEPT_VALUE] = (size_t)g.nList * sizeof(float);
    bytes[GL_T_KEPT_POINT] = (size_t)g.nList * sizeof(uint16_t);
    bytes[GL_T_KEPT_BIT] = (size_t)g.nList;
    bytes[GL_T_FAILED] = sizeof(uint32_t);
    for (int k = 0; k < GL_TABLES; ++k) given[k] = src[k] ? bytes[k] : 0;
    const sf3d_error_t e = raster_tables(K.glocalBlock, K.glocalOff, GL_TABLES, bytes, src, given);
    if (e != SF3D_OK) return e;
    RASTER_TRY(hipStreamSynchronize(I.stream));
    K.glocalBytes = K.glocalOff[GL_TABLES - 1] + 8;
    K.glocalAreas = g.nAreas; K.glocalList = g.nList; K.glocalPairs = g.nPairs;
    return SF3D_OK;
}

bool DeviceSolver::glocal_areas_set() const { return impl_ && impl_->meteo.base && impl_->meteo.glocalBlock; }

sf3d_error_t DeviceSolver::glocal_interpolate(const MeteoCall& call, const GlocalCall& g, const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    GlocalCellsView c{};
    sf3d_error_t e = meteo_view(call, mine, c.m);
    if (e != SF3D_OK) return e;
    K.glocalDone = false;
    K.produced[call.var] = false;                                               /* the slot is overwritten; it counts again once the call is whole */
    if (!K.glocalTables) RASTER_TRY(hipMalloc((void**)&K.glocalTables, GL_CALL_BYTES));
    double* table = (double*)K.glocalTables;
    float* heights = (float*)(table + LOCALDETREND_TABLE_DOUBLES);
    float* rows = heights + METEO_MAX_STATIONS;
    char* B = K.glocalBlock;
    uint32_t* failed = (uint32_t*)(B + K.glocalOff[GL_T_FAILED]);
    RASTER_TRY(hipMemcpyAsync(table, g.table, (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice, I.stream));
    if (call.nStations) {
        RASTER_TRY(hipMemcpyAsync(heights, g.height, call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
        for (int r = 0; r < g.proxies.nOthers; ++r)
            RASTER_TRY(hipMemcpyAsync(rows + (size_t)r * METEO_MAX_STATIONS, g.rows[r], call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
    }
    if (K.glocalList) RASTER_TRY(hipMemcpyAsync(B + K.glocalOff[GL_T_LIST_POINT], g.listPoint, (size_t)K.glocalList * sizeof(int32_t), hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemsetAsync(failed, 0, sizeof(uint32_t), I.stream));

    GlocalAreasView a{};
    a.s = g.setup;
    a.s.table = table;
    a.s.method = call.method; a.s.useDetrending = call.useDetrending;
    a.p = g.proxies;
    a.stationOffset = (const uint32_t*)(B + K.glocalOff[GL_T_STATION_OFFSET]);
    a.listPoint = (const int32_t*)(B + K.glocalOff[GL_T_LIST_POINT]);
    a.sv = c.m.sv; a.sh = heights; a.rows = rows;
    a.area = (GlocalAreaDev*)(B + K.glocalOff[GL_T_AREA]);
    a.detrended = (float*)(B + K.glocalOff[GL_T_DETRENDED]);
    a.keptBit = (uint8_t*)(B + K.glocalOff[GL_T_KEPT_BIT]);
    a.keptPoint = (uint16_t*)(B + K.glocalOff[GL_T_KEPT_POINT]);
    a.keptValue = (float*)(B + K.glocalOff[GL_T_KEPT_VALUE]);
    a.nAreas = K.glocalAreas;
    K.glocalProxies = g.proxies;
    e = raster_launch(k_glocal_areas, (size_t)K.glocalAreas * 64, a, K.glocalMs[0]);
    if (e != SF3D_OK) return e;

    c.s = a.s; c.p = a.p;
    c.pairOffset = (const uint32_t*)(B + K.glocalOff[GL_T_PAIR_OFFSET]);
    c.pairArea = (const uint32_t*)(B + K.glocalOff[GL_T_PAIR_AREA]);
    c.pairWeight = (const float*)(B + K.glocalOff[GL_T_PAIR_WEIGHT]);
    c.stationOffset = a.stationOffset;
    c.area = a.area; c.keptPoint = a.keptPoint; c.keptValue = a.keptValue;
    c.failed = failed;
    c.nPairs = K.glocalPairs;
    e = raster_launch(k_glocal_cells, n, c, K.glocalMs[1]);
    if (e != SF3D_OK) return e;
    K.glocalDone = true;                                                        /* the areas' records are this call's, whatever the cells did */
    uint32_t flag = 0;
    e = raster_download(&flag, failed, sizeof(uint32_t));
    if (e != SF3D_OK) return e;
    if (flag) return SF3D_MISSING_DATA_ERROR;                                  /* isOk == false: the slot does not count as produced */
    K.produced[call.var] = true;
    if (!out) return SF3D_OK;
    return raster_download(out, c.m.out, n * sizeof(float));
}

bool DeviceSolver::glocal_done() const { return glocal_areas_set() && impl_->meteo.glocalDone; }

sf3d_error_t DeviceSolver::glocal_records(GlocalAreaDev* area, float* detrended, uint8_t* kept, LocalProxiesSetup* proxies)
{
    const MeteoCache& K = impl_->meteo;
    sf3d_error_t e = SF3D_OK;
    if (area && K.glocalAreas) e = raster_download(area, K.glocalBlock + K.glocalOff[GL_T_AREA], (size_t)K.glocalAreas * sizeof(GlocalAreaDev));
    if (e == SF3D_OK && detrended && K.glocalList) e = raster_download(detrended, K.glocalBlock + K.glocalOff[GL_T_DETRENDED], (size_t)K.glocalList * sizeof(float));
    if (e == SF3D_OK && kept && K.glocalList) e = raster_download(kept, K.glocalBlock + K.glocalOff[GL_T_KEPT_BIT], K.glocalList);
    if (proxies) *proxies = K.glocalProxies;
    return e;
}

uint64_t DeviceSolver::glocal_bytes() const
{
    if (!impl_) return 0;
    const MeteoCache& K = impl_->meteo;
    return (K.glocalBlock ? (uint64_t)K.glocalBytes : 0) + (K.glocalTables ? (uint64_t)GL_CALL_BYTES : 0);
}

double DeviceSolver::glocal_kernel_ms(int which) const { return (impl_ && which >= 0 && which < 2) ? impl_->meteo.glocalMs[which] : 0.; }
#endif
