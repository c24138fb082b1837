/* part of sf3d_solver.hip (included there after sf3d_localdetrend.inc, whose selection, elevation fit, methods and wave primitives it
 * uses) - local detrending with every active proxy, not only the height: what the cell loop of
 * Project::interpolationDemLocalDetrending (agrolib/project/project.cpp:3226-3254) does for one DEM cell with the height and up to
 * LP_MAX_OTHERS other active proxies:
 *   getProxyValuesXY (agrolib/interpolation/interpolation.cpp:2620-2647)            the cell's value of every active proxy;
 *   localSelection, multipleDetrendingElevationFitting, detrendingElevation          the text of sf3d_localdetrend.inc (ld_select,
 *                                                                                    ld_elevation), skipped where the height is not active;
 *   multipleDetrendingOtherProxiesFitting (:1975-2171)                               proxyValidity twice, the two prunings, the minimum of
 *                                                                                    fit points, setFittingParameters_otherProxies (:1680-1728),
 *   bestFittingMarquardt_nDimension(&functionSum, ...) -> fittingMarquardt_nDimension (agrolib/mathFunctions/furtherMathFunctions.cpp:1535-1580,
 *                                                                                    1740-1947) of functionLinear_intercept per proxy: ONE run;
 *   detrendingOtherProxies (:2173-2236); interpolate() over what is left of the list (ld_methods); retrend through
 *   getMultipleDetrendingValues (:1298-1313, :2563-2617).
 *
 * k_localdetrend_proxies keeps the mapping of k_localdetrend: one wave64 per cell, four cells per 256-thread block, the station table
 * staged once per block, THE LIST-ORDER RULE for every sum.  On top of it:
 *  - the stations' values of the other proxies lie in LDS, a row of METEO_MAX_STATIONS floats per proxy shared by the block's cells and
 *    read through the list's station index: nothing is copied per cell;
 *  - THE TWO LISTS.  The reference prunes the interpolated list (myPoints) and the fit list (othersPoints, a copy taken after the
 *    elevation detrending) by different rules; the fit list contains the interpolated one and both keep the selection's order.  The
 *    kernel holds one list and two membership bits per entry (LP_FIT, LP_INTERP); the interpolated list is compacted in place with
 *    ballots, order kept, only when the fit is over;
 *  - the fit is one Marquardt run, so the parallelism is in the normal matrix: with NP <= 14 parameters the upper triangle of a and g are
 *    NP (NP + 1) / 2 + NP <= 119 independent sequential sums over the fit points.  A lane owns the entries lane, lane + 64: it runs the
 *    points in list order and forms the two derivatives it needs at each point by replaying the walk of the parameter vector up to its
 *    columns.  The matrix goes to LDS (the room of the elevation fit's records, spent by then); lane 0 scales the diagonal, eliminates,
 *    substitutes back and clamps, in the reference's order; every lane alike forms the two SSE sums;
 *  - the parameter vectors live in LDS (p, p + delta, (p + delta) - delta, delta, the range, lambda, the change, the new parameters):
 *    they are indexed by run-time columns, which registers cannot be without scratch.
 *
 * Kept from the reference on purpose:
 *  - the pivots are taken raw, with no max(., EPSILON): a zero pivot gives inf / NaN, a NaN diffSSE ends the loop with the parameters as
 *    the walk left them;
 *  - parameters[i][k] += delta; ...; -= delta walks across all proxies in turn: the columns that follow see (p + d) - d of those before,
 *    within the iteration and - where the step is refused - into the next;
 *  - the second validity pass judges every active proxy again over the pruned fit list: a proxy that failed the first pass may pass now,
 *    and the stations whose value of it is NODATA were never pruned: their -9999 enters the fit as a predictor, and detrendingOtherProxies
 *    erases them from the interpolated list;
 *  - a station leaves the interpolated list when all its significant proxy values are 0 (atLeastOneProxy); it stays in the fit;
 *  - if the cell's value of ANY significant proxy is NODATA the whole retrend is 0, the elevation part included.
 * The one arm the reference leaves undefined (the elevation function in the function list without its parameters, which needs a fitted
 * R2 within 1e-5 of -9999) is treated as unreachable: here the height is then simply not significant, functions and parameters stay aligned.
 *
 * Every loop is bounded: the ring cap of sf3d_localdetrend.inc, LP_MAX_ITERATIONS + 1 iterations, list lengths <= METEO_MAX_STATIONS.
 * The per-cell text also compiles for the host (tests/localproxies_host.cpp): one lane, the same text. */

#define LP_MAX_OTHERS LOCALPROXIES_MAX_OTHERS
#define LP_NP (2 * LP_MAX_OTHERS)               /* functionLinear_intercept: slope, intercept */
#define LP_MAX_ITERATIONS 100                   /* maxIterationsNr, interpolation.cpp:2165 */
#define LP_FIT_EPSILON 0.005                    /* myEpsilon */
#define LP_RATIO_DELTA 1000                     /* setFittingParameters_otherProxies */
#define LP_FIT 1u                               /* the entry is in othersPoints */
#define LP_INTERP 2u                            /* the entry is in myPoints */
enum { LP_P = 0, LP_BUMPED, LP_WALKED, LP_DELTA, LP_MIN, LP_MAX, LP_LAMBDA, LP_CHANGE, LP_FRESH, LP_VECTORS };
#define LP_WORK_DOUBLES (LP_VECTORS * LP_NP)
#define LP_MATRIX_DOUBLES (LP_NP * LP_NP + LP_NP)
static_assert(LP_MATRIX_DOUBLES <= LD_MAX_FIRST_GUESS * LD_FIT_STRIDE, "the normal matrix takes the room of the elevation fit's records");

typedef LocalProxiesSetup LpSetup;

/* what the other-proxy steps of a cell work on */
struct LpCtx {
    const float* rows;                  /* [LP_MAX_OTHERS][METEO_MAX_STATIONS]: the stations' values of other proxy r */
    uint8_t* member;                    /* per list entry: LP_FIT | LP_INTERP */
    double* vec;                        /* LP_VECTORS vectors of LP_NP */
    double* mat;                        /* a[LP_NP][LP_NP], then g[LP_NP] */
    uint32_t nOthers;
    uint32_t mask;                      /* bit r: other proxy r is significant */
};

/* the cell's value of the proxy in `slot`, getProxyValuesXY: the raster's value, the DEM's where the slot has no raster */
SF3D_METEO_FN double lp_cell_proxy(const MeteoView& m, uint32_t c, float z, int slot)
{
    const float* map = m.proxyMap[slot];
    const float f = map ? map[c] : z;
    return (f != m.flag) ? (double)f : (double)LD_NODATA;
}

/* proxyValidity (interpolation.cpp:1418-1457) of one other proxy over the fit list */
SF3D_METEO_FN bool lp_validity(const LdList& L, const uint8_t* member, const float* row, uint32_t n, float threshold)
{
    uint32_t nr = 0;
    double sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(member[i] & LP_FIT)) continue;
        const float v = row[L.idx[i]];
        if (v != (float)LD_NODATA) { ++nr; sum += v; }
    }
    if (nr < LD_MIN_NR) return false;
    const double avg = sum / (double)nr;
    sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(member[i] & LP_FIT)) continue;
        const float v = row[L.idx[i]];
        if (v != (float)LD_NODATA) sum += (v - avg) * (v - avg);
    }
    const double stdDev = __builtin_sqrt(sum / (double)(nr - 1));
    if (threshold != (float)LD_NODATA) return stdDev > threshold;
    return true;
}

/* a validity pass over every active other proxy: a lane judges a proxy; the mask of those that pass */
SF3D_METEO_FN uint32_t lp_validity_pass(const LpSetup& ps, const LdList& L, const LpCtx& X, uint32_t n)
{
    uint32_t mask = 0;
    for (uint32_t base = 0; base < X.nOthers; base += LD_LANES) {
        const uint32_t r = base + ld_lane();
        const bool ok = r < X.nOthers && lp_validity(L, X.member, X.rows + (size_t)r * METEO_MAX_STATIONS, n, ps.stdDevThreshold[r]);
        mask |= (uint32_t)(ld_ballot(ok) << base);
    }
    return mask;
}

/* parameter j as the forward difference of column c sees it (c < 0: the vector `base` as it is): the columns before c were walked,
 * c itself is raised, those after it are untouched */
SF3D_METEO_FN double lp_par(const LpCtx& X, const double* base, int c, int j)
{
    if (c < 0) return base[j];
    if (j < c) return X.vec[LP_WALKED * LP_NP + j];
    if (j == c) return X.vec[LP_BUMPED * LP_NP + j];
    return X.vec[LP_P * LP_NP + j];
}

/* functionSum of functionLinear_intercept (furtherMathFunctions.cpp:181-201) over the significant proxies of station `at` */
SF3D_METEO_FN double lp_sum(const LpCtx& X, uint32_t at, const double* base, int c)
{
    double result = 0.0;
    int j = 0;
    for (uint32_t r = 0; r < X.nOthers; ++r) {
        if (!((X.mask >> r) & 1u)) continue;
        const double x = (double)X.rows[(size_t)r * METEO_MAX_STATIONS + at];
        const double slope = lp_par(X, base, c, j), intercept = lp_par(X, base, c, j + 1);
        result += slope * x + intercept;
        j += 2;
    }
    return result;
}

/* normGeneric_nDimension with weights (furtherMathFunctions.cpp:2774-2788) over the fit list */
SF3D_METEO_FN double lp_sse(const LdList& L, const LpCtx& X, uint32_t n, const double* par)
{
    double norm = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(X.member[i] & LP_FIT)) continue;
        const double w = L.w[i];
        const double error = (double)L.val[i] - lp_sum(X, L.idx[i], par, -1);
        norm += error * error * w * w;
    }
    return norm;
}

/* fittingMarquardt_nDimension with weights (furtherMathFunctions.cpp:1740-1947) of NP = 2 x (significant proxies) parameters over the
 * fit list; the parameters are left in vec[LP_P] */
SF3D_METEO_FN void lp_marquardt(const LdList& L, const LpCtx& X, uint32_t n, int NP)
{
    const uint32_t lane = ld_lane();
    double* p = X.vec + LP_P * LP_NP;
    double* bumped = X.vec + LP_BUMPED * LP_NP;
    double* walked = X.vec + LP_WALKED * LP_NP;
    const double* delta = X.vec + LP_DELTA * LP_NP;
    const double* pmin = X.vec + LP_MIN * LP_NP;
    const double* pmax = X.vec + LP_MAX * LP_NP;
    double* lambda = X.vec + LP_LAMBDA * LP_NP;
    double* change = X.vec + LP_CHANGE * LP_NP;
    double* fresh = X.vec + LP_FRESH * LP_NP;
    double* a = X.mat;
    double* g = X.mat + LP_NP * LP_NP;
    const uint32_t nTriangle = (uint32_t)(NP * (NP + 1) / 2), nEntries = nTriangle + (uint32_t)NP;

    double mySSE = lp_sse(L, X, n, p);
    int iterationNr = 0;
    double diffSSE;
    do {
        for (uint32_t j = lane; j < (uint32_t)NP; j += LD_LANES) {
            bumped[j] = p[j] + delta[j];
            walked[j] = bumped[j] - delta[j];
        }
        ld_sync();
        /* a[i][j] (j >= i) and g[i]: a lane's entries, each a sequential sum over the fit points in list order */
        for (uint32_t e = lane; e < nEntries; e += LD_LANES) {
            int i = 0, j = -1;
            if (e < nTriangle) {
                uint32_t rem = e;
                while (rem >= (uint32_t)(NP - i)) { rem -= (uint32_t)(NP - i); ++i; }
                j = i + (int)rem;
            } else i = (int)(e - nTriangle);
            double acc = 0;
            for (uint32_t k = 0; k < n; ++k) {
                if (!(X.member[k] & LP_FIT)) continue;
                const uint32_t at = L.idx[k];
                const double w = L.w[k];
                const double firstEst = lp_sum(X, at, p, -1);
                const double Pi = (lp_sum(X, at, p, i) - firstEst) / delta[i];
                if (j >= 0) {
                    const double Pj = (j == i) ? Pi : (lp_sum(X, at, p, j) - firstEst) / delta[j];
                    acc += (Pi * (w * Pj));
                } else acc += Pi * w * ((double)L.val[k] - firstEst);
            }
            if (j >= 0) { a[i * LP_NP + j] = acc; a[j * LP_NP + i] = acc; }         /* a[j][i] = a[i][j], :1860 */
            else g[i] = acc;
        }
        ld_sync();
        if (lane == 0) {
            for (int j = 0; j < NP; ++j) p[j] = walked[j];                          /* what the walk left in the vector */
            for (int k = 0; k < NP; ++k) a[k * LP_NP + k] += lambda[k] * a[k * LP_NP + k];
            for (int j = 0; j < NP - 1; ++j) {
                const double pivot = a[j * LP_NP + j];
                for (int i = j + 1; i < NP; ++i) {
                    const double mult = a[i * LP_NP + j] / pivot;
                    for (int k = j + 1; k < NP; ++k) a[i * LP_NP + k] -= mult * a[j * LP_NP + k];
                    g[i] -= mult * g[j];
                }
            }
            change[NP - 1] = g[NP - 1] / a[(NP - 1) * LP_NP + NP - 1];
            for (int i = NP - 2; i >= 0; --i) {
                double top = g[i];
                for (int k = i + 1; k < NP; ++k) top -= a[i * LP_NP + k] * change[k];
                change[i] = top / a[i * LP_NP + i];
            }
            for (int j = 0; j < NP; ++j) {
                double f = p[j] + change[j];
                double l = lambda[j];
                if ((f > pmax[j]) && (l < 1000)) {
                    f = pmax[j];
                    if (l < 1000) l *= 10;                                          /* VFACTOR */
                }
                if (f < pmin[j]) {
                    f = pmin[j];
                    if (l < 1000) l *= 10;
                }
                fresh[j] = f; lambda[j] = l;
            }
        }
        ld_sync();
        const double newSSE = lp_sse(L, X, n, fresh);
        if (newSSE == LD_NODATA) return;
        diffSSE = mySSE - newSSE;
        ld_sync();
        if (diffSSE > 0) {
            mySSE = newSSE;
            for (uint32_t j = lane; j < (uint32_t)NP; j += LD_LANES) { p[j] = fresh[j]; lambda[j] /= 10; }
        } else {
            for (uint32_t j = lane; j < (uint32_t)NP; j += LD_LANES) lambda[j] *= 10;
        }
        ld_sync();
        iterationNr++;
    } while (__builtin_fabs(diffSSE) > LP_FIT_EPSILON && iterationNr <= LP_MAX_ITERATIONS);
}

/* the interpolated list compacted in place, order kept: 64 entries at a time, read, then written at or before where they lay */
SF3D_METEO_FN uint32_t lp_compact(const LdList& L, const uint8_t* member, uint32_t n)
{
    uint32_t kept = 0;
    for (uint32_t base = 0; base < n; base += LD_LANES) {
        const uint32_t i = base + ld_lane();
        const bool keep = i < n && (member[i] & LP_INTERP);
        const uint16_t idx = keep ? L.idx[i] : (uint16_t)0;
        const float d = keep ? L.d[i] : 0.f, val = keep ? L.val[i] : 0.f;
        const uint64_t mask = ld_ballot(keep);
        ld_sync();
        if (keep) {
            const uint32_t at = kept + ld_below(mask);
            L.idx[at] = idx; L.d[at] = d; L.val[at] = val;
        }
        kept += (uint32_t)__builtin_popcountll(mask);
        ld_sync();
    }
    return kept;
}

/* detrendingOtherProxies (interpolation.cpp:2173-2236) with the lines of vec[LP_P] over the entries that are in the interpolated list: a
 * station with an incomplete significant proxy (X.mask) leaves it.  k_glocal_areas (sf3d_glocal.inc) runs the same text */
SF3D_METEO_FN void lp_detrend(const LdList& L, const LpCtx& X, uint32_t n)
{
    for (uint32_t i = ld_lane(); i < n; i += LD_LANES) {
        if (!(X.member[i] & LP_INTERP)) continue;
        const uint32_t at = L.idx[i];
        bool proxyComplete = true;
        for (uint32_t r = 0; r < X.nOthers; ++r)
            if (((X.mask >> r) & 1u) && meteo_eqf(X.rows[(size_t)r * METEO_MAX_STATIONS + at], (float)LD_NODATA)) proxyComplete = false;
        if (proxyComplete) {
            const float detrendValue = (float)lp_sum(X, at, X.vec + LP_P * LP_NP, -1);
            L.val[i] -= detrendValue;
        } else X.member[i] = (uint8_t)(X.member[i] & ~LP_INTERP);
    }
    ld_sync();
}

/* multipleDetrendingOtherProxiesFitting and detrendingOtherProxies over the selected list of n entries (their values detrended by the
 * elevation already).  Returns the length of the interpolated list, compacted; X.mask: the significant proxies; their slope and
 * intercept are left in vec[LP_P], two per significant proxy in slot order */
SF3D_METEO_FN uint32_t lp_others(const LdSetup& s, const LpSetup& ps, const LdList& L, LpCtx& X, uint32_t n)
{
    const uint32_t lane = ld_lane();
    X.mask = 0;
    for (uint32_t i = lane; i < n; i += LD_LANES) X.member[i] = (uint8_t)(LP_FIT | LP_INTERP);
    ld_sync();
    /* proxy spatial variability, first pass: over the whole list */
    uint32_t first = lp_validity_pass(ps, L, X, n);
    if (first == 0) return n;                                                       /* the list untouched */
    /* the two prunings, :2033-2093 */
    for (uint32_t i = lane; i < n; i += LD_LANES) {
        const uint32_t at = L.idx[i];
        bool nodataClose = false, nodataExact = false, atLeastOneProxy = false;
        for (uint32_t r = 0; r < X.nOthers; ++r) {
            if (!((first >> r) & 1u)) continue;
            const float v = X.rows[(size_t)r * METEO_MAX_STATIONS + at];
            nodataClose = nodataClose || meteo_eqf(v, (float)LD_NODATA);
            nodataExact = nodataExact || v == (float)LD_NODATA;
            atLeastOneProxy = atLeastOneProxy || !meteo_eqf(v, 0.f);
        }
        X.member[i] = (uint8_t)((nodataExact ? 0u : LP_FIT) | ((nodataClose || !atLeastOneProxy) ? 0u : LP_INTERP));
    }
    ld_sync();
    /* second pass: every active proxy again, over the pruned fit list */
    uint32_t second = lp_validity_pass(ps, L, X, n);
    uint32_t nFit = 0;
    for (uint32_t base = 0; base < n; base += LD_LANES) {
        const uint32_t i = base + lane;
        nFit += (uint32_t)__builtin_popcountll(ld_ballot(i < n && (X.member[i] & LP_FIT)));
    }
    /* too few fit points: no other proxy is significant, the prunings stay (:2140-2150) */
    if (second != 0 && (int)nFit < s.minPointsLocal) second = 0;
    if (second != 0) {
        X.mask = second;
        const int NP = 2 * __builtin_popcount(second);
        /* setFittingParameters_otherProxies, and parametersDelta = max(delta, EPSILON) of bestFittingMarquardt_nDimension */
        for (uint32_t j = lane; j < (uint32_t)NP; j += LD_LANES) {
            uint32_t r = 0, seen = 0;
            for (; r < X.nOthers; ++r) {
                if (!((second >> r) & 1u)) continue;
                if (seen == j / 2) break;
                ++seen;
            }
            const double min_ = ps.range[r][j & 1u], max_ = ps.range[r][2 + (j & 1u)];
            X.vec[LP_MIN * LP_NP + j] = min_;
            X.vec[LP_MAX * LP_NP + j] = max_;
            X.vec[LP_DELTA * LP_NP + j] = ld_max((max_ - min_) / LP_RATIO_DELTA, LD_EPSILON);
            X.vec[LP_P * LP_NP + j] = (max_ + min_) / 2;
            X.vec[LP_LAMBDA * LP_NP + j] = 0.01;
        }
        ld_sync();
        lp_marquardt(L, X, n, NP);
        ld_sync();
        lp_detrend(L, X, n);
    }
    return lp_compact(L, X.member, n);
}

/* the per-cell outcome beside that of the elevation (LdOutcome) */
struct LpOutcome {
    uint32_t interpolated;              /* the length of the interpolated list */
    uint32_t mask;                      /* bit r: other proxy r is significant; its slope and intercept are in vec[LP_P] */
};

/* retrend (:1298-1313) through getMultipleDetrendingValues (:2563-2617) on cell c: the height first (significant: with par), then the
 * significant proxies (mask) in slot order, slope and intercept of each in `lines`; a NODATA among the cell's values of them: 0.
 * k_glocal_cells (sf3d_glocal.inc) runs the same text */
SF3D_METEO_FN float lp_retrend(const MeteoView& m, const LdSetup& s, const LpSetup& ps, uint32_t nOthers, uint32_t mask, const double* lines, uint32_t c, float z,
                               bool significant, double* par)
{
    double retrendValue = 0.;
    bool complete = true;
    double zh = 0;
    if (significant) {
        zh = lp_cell_proxy(m, c, z, ps.heightSlot);
        complete = zh != LD_NODATA;
    }
    for (uint32_t r = 0; r < nOthers; ++r)
        if (((mask >> r) & 1u) && lp_cell_proxy(m, c, z, ps.slot[r]) == LD_NODATA) complete = false;
    if (complete && (significant || mask != 0)) {
        double sumOfFunctions = 0.0;
        if (significant) sumOfFunctions += ld_height_function(s, zh, par);
        int j = 0;
        for (uint32_t r = 0; r < nOthers; ++r) {
            if (!((mask >> r) & 1u)) continue;
            sumOfFunctions += lines[j] * lp_cell_proxy(m, c, z, ps.slot[r]) + lines[j + 1];
            j += 2;
        }
        retrendValue = (float)sumOfFunctions;
    }
    return (float)retrendValue;
}

/* one DEM cell c of height z at the float (x, y): the map value */
SF3D_METEO_FN float lp_cell(const MeteoView& m, const LdSetup& s, const LpSetup& ps, const LdStations& st, const LdList& L, LpCtx& X, uint32_t c, float z, float x,
                            float y, LdOutcome& o, LpOutcome& po)
{
    float radius;
    const uint32_t n = ld_select(s, st, L, x, y, radius);
    o.count = n; o.radius = radius; o.significant = 0; o.r2 = (float)LD_NODATA;
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = LD_NODATA;

    double par[LD_MAX_PARAMETERS];
    bool significant = false;
    if (ps.heightSlot >= 0) {                                                       /* the elevationPos arm of multipleDetrendingMain, :1845 */
        double R2;
        significant = ld_elevation(s, L, n, par, R2);
        o.r2 = (float)R2;
        if (significant) {
            o.significant = 1;
#pragma unroll
            for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = par[j];
        }
    }
    X.mask = 0;
    const uint32_t nInterpolated = (X.nOthers > 0) ? lp_others(s, ps, L, X, n) : n;
    po.interpolated = nInterpolated; po.mask = X.mask;

    /* interpolate() over what is left of the list; modifiedShepardIdw still takes the localRadius of the selection */
    float result = ld_methods(s, st, L, nInterpolated, radius, x, y);
    if (meteo_eqf(result, (float)LD_NODATA)) return (float)LD_NODATA;
    if (s.useDetrending) result += lp_retrend(m, s, ps, X.nOthers, X.mask, X.vec + LP_P * LP_NP, c, z, significant, par);
    return result;
}

#ifndef SF3D_METEO_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_localdetrend_proxies(LocalProxiesView)
{
    const LocalProxiesView& v = meteo_kernel_argument<LocalProxiesView>();
    __shared__ double sx[METEO_MAX_STATIONS], sy[METEO_MAX_STATIONS];
    __shared__ float sh[METEO_MAX_STATIONS], sv[METEO_MAX_STATIONS];
    __shared__ double heightsAndWeights[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ double fit[LD_CELLS_PER_BLOCK][LD_MAX_FIRST_GUESS * LD_FIT_STRIDE];
    __shared__ double work[LD_CELLS_PER_BLOCK][LP_WORK_DOUBLES];
    __shared__ float distances[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS], values[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ float rows[LP_MAX_OTHERS * METEO_MAX_STATIONS];
    __shared__ float lanes[LD_CELLS_PER_BLOCK][64];
    __shared__ uint16_t indices[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ uint8_t members[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    const MeteoView& m = v.d.m;
    const LpSetup& ps = v.p;
    const uint32_t nStations = m.nStations < METEO_MAX_STATIONS ? m.nStations : METEO_MAX_STATIONS;
    const uint32_t nOthers = (uint32_t)ps.nOthers < LP_MAX_OTHERS ? (uint32_t)ps.nOthers : LP_MAX_OTHERS;
    for (uint32_t k = threadIdx.x; k < nStations; k += blockDim.x) {
        sx[k] = m.sx[k]; sy[k] = m.sy[k]; sv[k] = m.sv[k]; sh[k] = v.d.sh[k];
        for (uint32_t r = 0; r < nOthers; ++r) rows[r * METEO_MAX_STATIONS + k] = v.rows[(size_t)r * METEO_MAX_STATIONS + k];
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * LD_CELLS_PER_BLOCK + wave;
    if (c >= m.nCells) return;
    float result = m.flag;
    LdOutcome o;
    o.count = 0; o.radius = (float)LD_NODATA; o.significant = 0; o.r2 = (float)LD_NODATA;
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = LD_NODATA;
    LpOutcome po;
    po.interpolated = 0; po.mask = 0;
    const float z = m.dem[c];
    if (!(m.mine && !m.mine[c]) && !meteo_eqf(z, m.flag)) {
        float x, y;
        meteo_cell_xy(m, c, x, y);
        LdList L;
        L.idx = indices[wave]; L.d = distances[wave]; L.val = values[wave];
        L.h = (float*)heightsAndWeights[wave]; L.w = L.h + METEO_MAX_STATIONS; L.wt = heightsAndWeights[wave];
        L.lanes = lanes[wave]; L.fit = fit[wave];
        LpCtx X;
        X.rows = rows; X.member = members[wave]; X.vec = work[wave]; X.mat = fit[wave]; X.nOthers = nOthers; X.mask = 0;
        result = lp_cell(m, v.d.s, ps, LdStations{sx, sy, sh, sv, nStations}, L, X, c, z, x, y, o, po);
    }
    if (ld_lane() == 0) {
        m.out[c] = result;
        v.d.count[c] = o.count; v.d.radius[c] = o.radius; v.d.significant[c] = (uint8_t)o.significant; v.d.r2[c] = o.r2;
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) v.d.parameters[(size_t)c * LD_MAX_PARAMETERS + j] = o.parameters[j];
        v.interpolated[c] = po.interpolated;
        /* per proxy slot: significance, slope, intercept; -9999 where the slot is not a significant other proxy */
        for (uint32_t p = 0; p < METEO_MAX_PROXIES; ++p) {
            v.proxySignificant[(size_t)c * METEO_MAX_PROXIES + p] = 0;
            v.proxyLine[((size_t)c * METEO_MAX_PROXIES + p) * 2] = LD_NODATA;
            v.proxyLine[((size_t)c * METEO_MAX_PROXIES + p) * 2 + 1] = LD_NODATA;
        }
        uint32_t j = 0;
        for (uint32_t r = 0; r < nOthers; ++r) {
            if (!((po.mask >> r) & 1u)) continue;
            const size_t at = (size_t)c * METEO_MAX_PROXIES + (uint32_t)ps.slot[r];
            v.proxySignificant[at] = 1;
            v.proxyLine[at * 2] = work[wave][LP_P * LP_NP + j];
            v.proxyLine[at * 2 + 1] = work[wave][LP_P * LP_NP + j + 1];
            j += 2;
        }
    }
}

/* ---- host side: the elevation's per-cell outcome goes where k_localdetrend leaves its own (MeteoCache::localFit: the getters of
 * sf3d_localdetrend.h keep their meaning after a call of either kind); the block's own: the interpolated count and the proxies' lines ---- */
static const size_t LP_CELL_BYTES = METEO_MAX_PROXIES * (2 * sizeof(double) + sizeof(uint8_t)) + sizeof(uint32_t);
static const size_t LP_TABLE_BYTES = (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double) + (size_t)(1 + LP_MAX_OTHERS) * METEO_MAX_STATIONS * sizeof(float);

sf3d_error_t DeviceSolver::localproxies_free()
{
    if (!impl_) return SF3D_OK;
    MeteoCache& K = impl_->meteo;
    raster_release({K.proxiesFit, K.proxiesTables});
    K.proxiesFit = nullptr; K.proxiesTables = nullptr; K.proxiesDone = false; K.proxiesMs = 0.;
    return SF3D_OK;
}

bool DeviceSolver::meteo_has_map(uint32_t proxy) const { return impl_ && impl_->meteo.base && proxy < impl_->meteo.nProxies && impl_->meteo.hasMap[proxy]; }

sf3d_error_t DeviceSolver::localproxies_interpolate(const MeteoCall& call, const LocalProxiesCall& local, const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    LocalProxiesView v{};
    sf3d_error_t e = meteo_view(call, mine, v.d.m);
    if (e != SF3D_OK) return e;
    K.localDone = false; K.proxiesDone = false;
    if (!K.localFit) RASTER_TRY(hipMalloc((void**)&K.localFit, n * LD_CELL_BYTES));
    if (!K.proxiesFit) RASTER_TRY(hipMalloc((void**)&K.proxiesFit, n * LP_CELL_BYTES));
    if (!K.proxiesTables) RASTER_TRY(hipMalloc((void**)&K.proxiesTables, LP_TABLE_BYTES));
    double* table = (double*)K.proxiesTables;
    float* heights = (float*)(table + LOCALDETREND_TABLE_DOUBLES);
    float* rows = heights + METEO_MAX_STATIONS;
    RASTER_TRY(hipMemcpyAsync(table, local.table, (size_t)LOCALDETREND_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice, I.stream));
    if (call.nStations) {
        RASTER_TRY(hipMemcpyAsync(heights, local.height, call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
        for (int r = 0; r < local.proxies.nOthers; ++r)
            RASTER_TRY(hipMemcpyAsync(rows + (size_t)r * METEO_MAX_STATIONS, local.rows[r], call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
    }
    v.d.sh = heights;
    v.d.parameters = (double*)K.localFit;
    v.d.count = (uint32_t*)(v.d.parameters + n * LD_MAX_PARAMETERS);
    v.d.radius = (float*)(v.d.count + n);
    v.d.r2 = v.d.radius + n;
    v.d.significant = (uint8_t*)(v.d.r2 + n);
    v.d.s = local.setup;
    v.d.s.table = table;
    v.d.s.method = call.method; v.d.s.useDetrending = call.useDetrending;
    v.p = local.proxies;
    v.rows = rows;
    v.proxyLine = (double*)K.proxiesFit;
    v.interpolated = (uint32_t*)(v.proxyLine + n * METEO_MAX_PROXIES * 2);
    v.proxySignificant = (uint8_t*)(v.interpolated + n);
    e = raster_launch(k_localdetrend_proxies, n * 64, v, K.proxiesMs);
    if (e != SF3D_OK) return e;
    K.produced[call.var] = true;
    K.localDone = true; K.proxiesDone = true;
    if (!out) return SF3D_OK;
    return raster_download(out, v.d.m.out, n * sizeof(float));
}

bool DeviceSolver::localproxies_done() const { return localdetrend_done() && impl_->meteo.proxiesFit && impl_->meteo.proxiesDone; }

sf3d_error_t DeviceSolver::localproxies_interpolated(uint32_t* count)
{
    const MeteoCache& K = impl_->meteo;
    const size_t n = K.nCells;
    return count ? raster_download(count, (const double*)K.proxiesFit + n * METEO_MAX_PROXIES * 2, n * sizeof(uint32_t)) : SF3D_OK;
}

sf3d_error_t DeviceSolver::localproxies_fit(uint8_t* significant, double* lines)
{
    const MeteoCache& K = impl_->meteo;
    const size_t n = K.nCells;
    const double* dl = (const double*)K.proxiesFit;
    sf3d_error_t e = SF3D_OK;
    if (lines) e = raster_download(lines, dl, n * METEO_MAX_PROXIES * 2 * sizeof(double));
    if (e == SF3D_OK && significant) e = raster_download(significant, (const uint32_t*)(dl + n * METEO_MAX_PROXIES * 2) + n, n * METEO_MAX_PROXIES);
    return e;
}

uint64_t DeviceSolver::localproxies_bytes() const
{
    if (!impl_) return 0;
    const MeteoCache& K = impl_->meteo;
    return (K.proxiesFit ? (uint64_t)K.nCells * LP_CELL_BYTES : 0) + (K.proxiesTables ? (uint64_t)LP_TABLE_BYTES : 0);
}

double DeviceSolver::localproxies_kernel_ms() const { return impl_ ? impl_->meteo.proxiesMs : 0.; }
#endif
