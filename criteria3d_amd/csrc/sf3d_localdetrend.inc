/* part of sf3d_solver.hip (included there after sf3d_topodist.inc; it uses the raster, the station table and the methods of
 * sf3d_meteo.inc) - air and dew-point temperature with local detrending on the device: what the cell loop of
 * Project::interpolationDemLocalDetrending (agrolib/project/project.cpp:3226-3254) does for one DEM cell with the height proxy as the only
 * active proxy:
 *   localSelection (agrolib/interpolation/interpolation.cpp:1087-1170)             the stations around the cell, ring by ring;
 *   multipleDetrendingMain -> multipleDetrendingElevationFitting (:1832-1953)       proxyValidity (:1418-1457), then
 *   bestFittingMarquardt_nDimension -> fittingMarquardt_nDimension, weighted        (agrolib/mathFunctions/furtherMathFunctions.cpp:1360-1427,
 *                                                                                   1954-2118) over the caller's first guesses, with
 *   computeWeighted_R2 / computeWeighted_RMSE (:1245-1322) and lapseRatePiecewise_two / _three / _three_free (:115-179);
 *   detrendingElevation (interpolation.cpp:1956-1972); interpolate() (:2502-2560) over the selected stations - inverseDistanceWeighted,
 *   shepardIdw, or modifiedShepardIdw with radius = getLocalRadius() (:961-965: no neighbour search, every selected station);
 *   retrend in its multiple-detrending form (:1298-1313).
 *
 * k_localdetrend: one wave64 per cell, four cells per 256-thread block.  A thread per cell cannot hold a selected list of up to 1 024
 * stations, and the Marquardt runs from the different first guesses do not depend on one another, so
 *  - the block's station table (x, y doubles; height, value floats) is staged once into LDS, as k_meteo_idw does;
 *  - the wave compacts its cell's selected list into LDS with ballots, ring after ring and 64 stations at a time in input order, which is
 *    the (ring, input index) order of the reference's push_back: per station its index, distance, height, value and regression weight;
 *  - lane k runs the Marquardt fit from first guess k (at most 31) against broadcast LDS reads, and leaves its parameters, R2 and RMSE in
 *    LDS; every lane then walks the 31 results in the order of k, as bestFittingMarquardt_nDimension does, so the choice is the wave's
 *    without a broadcast; the fit from firstGuessCombinations[RMSEindex] after bestR2 < 0 is run by every lane alike;
 *  - in the O(n^2) direction terms of modifiedShepardIdw lane i owns t[i] and runs j in list order; weight[i] goes to LDS (over the
 *    heights and regression weights, which are spent by then) and every lane forms the two sums over i in list order.
 * THE LIST-ORDER RULE: every sum the reference forms sequentially is formed sequentially in the same order by one lane (or by every lane
 * alike).  No tree, shuffle or atomic reduction enters a value.  The one wave-wide combination is the largest selected distance, a
 * maximum of floats (exact in any order), taken from 64 per-lane maxima through LDS.
 * P[k][j] of fittingMarquardt_nDimension is not stored: a[i][j] and g[i] are separate accumulators over the data points, so a point's
 * derivatives are formed when the point is visited and the order of every sum is kept.
 *
 * Kept from the reference on purpose:
 *  - lapseRatePiecewise_three and _three_free write par[2] = max(10, par[2]) into the vector they are handed: the fitted parameters, the
 *    perturbed vector of the forward differences and newParameters all carry it;
 *  - parameters[k] += delta; ...; parameters[k] -= delta leaves (p + d) - d in the vector, iteration after iteration;
 *  - a station at distance 0 is never selected (r0 < d) unless every station is (N <= minPoints);
 *  - the weighted R2 of equal station values divides by a total deviation of 0: -inf (bestR2 < 0: the fit is repeated from the RMSE
 *    index) or, where the residuals are 0 too, NaN, which compares false everywhere: the fit of the first guess stays;
 *  - interpolate() hands (radius, x, y) to modifiedShepardIdw's (radius, y, x), as sf3d_meteo.inc notes.
 * Numerics are those of sf3d_meteo.inc: the reference's types at every step, -ffp-contract=off, IEEE division and square root.
 *
 * Every loop is bounded: the ring loop ends where no station lies beyond the ring (stations are finite: the entry point refuses others)
 * and at LD_RING_CAP rings whatever it is handed; a fit ends after 1 001 iterations.
 *
 * The per-cell text also compiles for the host (tests/localdetrend_host.cpp defines SF3D_METEO_HOST): one lane, the same text. */

#define LD_NODATA (-9999)
#define LD_EPSILON 0.00001
#define LD_MAX_PARAMETERS LOCALDETREND_MAX_PARAMETERS
#define LD_MAX_FIRST_GUESS LOCALDETREND_MAX_FIRST_GUESS
#define LD_FIT_STRIDE (LD_MAX_PARAMETERS + 2)        /* a fit's record in LDS: the parameters, R2, RMSE */
#define LD_RING_CAP 131072
#define LD_MAX_ITERATIONS 1000               /* maxIterationsNr, interpolation.cpp:1929 */
#define LD_FIT_EPSILON 0.002                 /* myEpsilon */
#define LD_DELTA_R2 0.005                    /* deltaR2 */
#define LD_MIN_NR 5                          /* proxyValidity */
enum { LD_PIECEWISE_TWO = 0, LD_PIECEWISE_THREE_FREE = 1, LD_PIECEWISE_THREE = 2 };     /* TFittingFunction, interpolationConstants.h:41 */

/* the wave, or the host's single lane */
#ifdef SF3D_METEO_HOST
#define LD_LANES 1u
SF3D_METEO_FN uint32_t ld_lane() { return 0; }
SF3D_METEO_FN uint64_t ld_ballot(bool p) { return p ? 1ull : 0ull; }
SF3D_METEO_FN uint32_t ld_below(uint64_t) { return 0; }
SF3D_METEO_FN void ld_sync() {}
#else
#define LD_LANES 64u
SF3D_METEO_FN uint32_t ld_lane() { return threadIdx.x & 63u; }
SF3D_METEO_FN uint64_t ld_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
/* the set bits of a ballot below this lane */
SF3D_METEO_FN uint32_t ld_below(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }
/* what the wave's lanes wrote to LDS is visible to its other lanes */
SF3D_METEO_FN void ld_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

/* the station table of the call */
struct LdStations {
    const double* sx;
    const double* sy;
    const float* sh;                    /* getProxyValue(elevationPos) */
    const float* sv;
    uint32_t n;
};

/* a cell's selected list, in (ring, input index) order, and the wave's working room */
struct LdList {
    uint16_t* idx;
    float* d;                           /* the distance from the cell */
    float* h;
    float* w;                           /* regressionWeight, 1 where it is NODATA (interpolation.cpp:1901-1903) */
    float* val;                         /* the station's value, detrended in place */
    double* wt;                         /* weight[i] of modifiedShepardIdw: the room of h and w */
    float* lanes;                       /* LD_LANES floats */
    double* fit;                        /* LD_MAX_FIRST_GUESS x LD_FIT_STRIDE */
};

typedef LocalDetrendSetup LdSetup;         /* what the call fixes for every cell (sf3d_device.h) */

/* the per-cell outcome beside the map value */
struct LdOutcome {
    uint32_t count;
    float radius;
    int32_t significant;
    float r2;
    double parameters[LD_MAX_PARAMETERS];
};

SF3D_METEO_FN bool ld_eqd(double a, double b) { return __builtin_fabs(a - b) < LD_EPSILON; }       /* isEqual(double, double), basicMath.h:28 */
SF3D_METEO_FN double ld_max(double a, double b) { return (a < b) ? b : a; }                         /* std::max */

/* lapseRatePiecewise_two (F 0), _three_free (1), _three (2), furtherMathFunctions.cpp:115-179 */
template <int F> SF3D_METEO_FN double ld_func(double x, double* par)
{
    if (F == LD_PIECEWISE_TWO) {
        if (x < par[0]) return par[2] * (x - par[0]) + par[1];
        return par[3] * (x - par[0]) + par[1];
    }
    par[2] = (10 > par[2]) ? 10 : par[2];                                   /* MAXVALUE(10, par[2]), written back */
    const double xb = par[2] + par[0];
    const double upper = (F == LD_PIECEWISE_THREE) ? par[4] : par[LD_MAX_PARAMETERS - 1];
    if (x < par[0]) return par[4] * x - par[0] * par[4] + par[1];
    if (x > xb) return upper * x - upper * par[0] - upper * par[2] + par[3] * par[2] + par[1];
    return par[3] * x - par[3] * par[0] + par[1];
}

/* fittingMarquardt_nDimension with weights, furtherMathFunctions.cpp:1954-2118, over the elevation points of the list (a station whose
 * height is NODATA is not one: interpolation.cpp:1874) */
template <int F, int NP> SF3D_METEO_FN void ld_marquardt(double* par, const double* pmin, const double* pmax, const double* pdelta, const LdList& L, uint32_t n)
{
    double lambda[NP], change[NP], fresh[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) { lambda[j] = 0.01; change[j] = 0; fresh[j] = 0; }
    double mySSE = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf == (float)LD_NODATA) continue;
        const double w = L.w[i];
        const double error = (double)L.val[i] - ld_func<F>((double)hf, par);
        mySSE += error * error * w * w;
    }
    int iterationNr = 0;
    double diffSSE;
    do {
        double g[NP], a[NP][NP], q[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            g[i] = 0; q[i] = par[i];
#pragma unroll
            for (int j = 0; j < NP; ++j) a[i][j] = 0;
        }
        for (uint32_t k = 0; k < n; ++k) {
            const float hf = L.h[k];
            if (hf == (float)LD_NODATA) continue;
            const double x = hf, y = L.val[k], w = L.w[k];
            const double firstEst = ld_func<F>(x, par);
            /* the forward differences: parameters[p] += delta, every point, parameters[p] -= delta - the same walk of the vector at
             * every point, so the point sees what the reference's P[p][k] saw */
            double P[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) q[p] = par[p];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                q[p] += pdelta[p];
                P[p] = (ld_func<F>(x, q) - firstEst) / pdelta[p];
                q[p] -= pdelta[p];
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) {
#pragma unroll
                for (int j = i; j < NP; ++j) a[i][j] += (P[i] * (w * P[j]));
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) g[i] += P[i] * w * (y - firstEst);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) par[p] = q[p];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            a[k][k] += lambda[k] * a[k][k];
#pragma unroll
            for (int j = k + 1; j < NP; ++j) a[j][k] = a[k][j];
        }
#pragma unroll
        for (int j = 0; j < NP - 1; ++j) {
            const double pivot = ld_max(a[j][j], LD_EPSILON);
#pragma unroll
            for (int i = j + 1; i < NP; ++i) {
                const double mult = a[i][j] / pivot;
#pragma unroll
                for (int k = j + 1; k < NP; ++k) a[i][k] -= mult * a[j][k];
                g[i] -= mult * g[j];
            }
        }
        change[NP - 1] = g[NP - 1] / ld_max(a[NP - 1][NP - 1], LD_EPSILON);
#pragma unroll
        for (int i = NP - 2; i >= 0; --i) {
            double top = g[i];
#pragma unroll
            for (int k = i + 1; k < NP; ++k) top -= a[i][k] * change[k];
            change[i] = top / ld_max(a[i][i], LD_EPSILON);
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            fresh[j] = par[j] + change[j];
            if ((fresh[j] > pmax[j]) && (lambda[j] < 1000)) {
                fresh[j] = pmax[j];
                if (lambda[j] < 1000) lambda[j] *= 10;                     /* VFACTOR */
            }
            if (fresh[j] < pmin[j]) {
                fresh[j] = pmin[j];
                if (lambda[j] < 1000) lambda[j] *= 10;
            }
        }
        double newSSE = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const float hf = L.h[i];
            if (hf == (float)LD_NODATA) continue;
            const double w = L.w[i];
            const double error = (double)L.val[i] - ld_func<F>((double)hf, fresh);
            newSSE += error * error * w * w;
        }
        if (newSSE == LD_NODATA) return;
        diffSSE = mySSE - newSSE;
        if (diffSSE > 0) {
            mySSE = newSSE;
#pragma unroll
            for (int j = 0; j < NP; ++j) { par[j] = fresh[j]; lambda[j] /= 10; }
        } else {
#pragma unroll
            for (int j = 0; j < NP; ++j) lambda[j] *= 10;
        }
        iterationNr++;
    } while (__builtin_fabs(diffSSE) > LD_FIT_EPSILON && iterationNr <= LD_MAX_ITERATIONS);
}

/* computeWeighted_R2 and computeWeighted_RMSE (furtherMathFunctions.cpp:1245-1322) of the fit `par` over the elevation points */
template <int F> SF3D_METEO_FN void ld_scores(double* par, const LdList& L, uint32_t n, uint32_t nrData, double& R2, double& RMSE)
{
    double mean = 0, sumWeights = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf == (float)LD_NODATA) continue;
        const double w = L.w[i];
        mean += (double)L.val[i] * w;
        sumWeights += w;
    }
    mean /= sumWeights;
    double residuals = 0, total = 0, rmseSum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf == (float)LD_NODATA) continue;
        const double w = L.w[i], y = L.val[i];
        const double ySim = ld_func<F>((double)hf, par);
        const double weightedResidual = w * (y - ySim);
        residuals += weightedResidual * weightedResidual;
        const double deviation = w * (y - mean);
        total += deviation * deviation;
        rmseSum += w * (y - ySim) * (y - ySim);
    }
    R2 = 1.0 - (residuals / total);
    RMSE = __builtin_sqrt(rmseSum / (sumWeights * (double)nrData));
}

/* bestFittingMarquardt_nDimension with weights (furtherMathFunctions.cpp:1360-1427), then the significance rule and
 * detrendingElevation (interpolation.cpp:1937-1972).  Returns whether the height proxy is significant; par: the cell's parameters */
template <int F, int NP> SF3D_METEO_FN bool ld_fit(const LdSetup& s, const LdList& L, uint32_t n, uint32_t nrData, double* par, double& bestR2)
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
        double R2, RMSE;
        ld_scores<F>(p, L, n, nrData, R2, RMSE);
#pragma unroll
        for (int j = 0; j < NP; ++j) L.fit[k * LD_FIT_STRIDE + j] = p[j];
        L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS] = R2;
        L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS + 1] = RMSE;
    }
    ld_sync();
    /* the choice, in the order of k */
    bestR2 = LD_NODATA;
    double bestRMSE = LD_NODATA;
    uint32_t RMSEindex = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) par[j] = 0;
    for (uint32_t k = 0; k < nGuess; ++k) {
        const double R2 = L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS], RMSE = L.fit[k * LD_FIT_STRIDE + LD_MAX_PARAMETERS + 1];
        if (ld_eqd(bestRMSE, LD_NODATA) || RMSE < bestRMSE) { bestRMSE = RMSE; RMSEindex = k; }
        if (ld_eqd(bestR2, LD_NODATA) || R2 > (bestR2 + LD_DELTA_R2)) {
#pragma unroll
            for (int j = 0; j < NP; ++j) par[j] = L.fit[k * LD_FIT_STRIDE + j];
            bestR2 = R2;
        }
    }
    if (bestR2 < 0) {
#pragma unroll
        for (int j = 0; j < NP; ++j) par[j] = guess[RMSEindex * LD_MAX_PARAMETERS + j];
        ld_marquardt<F, NP>(par, pmin, pmax, pdelta, L, n);
    }
    /* ! isEqual(R2, NODATA) || ! isVectorNodataOrZero(parameters) */
    bool nodataOrZero = false;
#pragma unroll
    for (int j = 0; j < NP; ++j) nodataOrZero = nodataOrZero || ld_eqd(par[j], LD_NODATA) || ld_eqd(par[j], 0);
    const bool significant = !ld_eqd(bestR2, LD_NODATA) || !nodataOrZero;
    if (significant) {
        ld_sync();
        for (uint32_t i = ld_lane(); i < n; i += LD_LANES) {
            const float detrendValue = (float)ld_func<F>((double)L.h[i], par);
            L.val[i] -= detrendValue;
        }
    }
    ld_sync();
    return significant;
}

/* the selected list's x, y and values, indexed as meteo_shepard indexes the station table */
struct LdCoord {
    const double* table;
    const uint16_t* idx;
    SF3D_METEO_MEMBER double operator[](uint32_t i) const { return table[idx[i]]; }
};
struct LdListDistance {
    const float* d;
    SF3D_METEO_MEMBER float operator()(uint32_t i) const { return d[i]; }
};

/* modifiedShepardIdw with the radius handed in (interpolation.cpp:948-1028, the arm of :961-965) over the whole list.  x, y: the cell's
 * float coordinates as interpolate() passes them: the function's own x is the cell's y */
SF3D_METEO_FN float ld_shepard_modified(const LdStations& st, const LdList& L, uint32_t n, float radius, float x, float y)
{
    if (n == 0) return (float)LD_NODATA;
    double weightSum = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const float d = L.d[i];
        if ((double)d > LD_EPSILON && d <= radius) weightSum += (double)((radius - d) / (radius * d));
    }
    if (weightSum == 0.0) return (float)LD_NODATA;
    const double invWeightSum = 1.0 / weightSum;
    const double X = (double)y, Y = (double)x;
    ld_sync();                                                               /* the heights and weights are spent: their room takes weight[i] */
    for (uint32_t i = ld_lane(); i < n; i += LD_LANES) {
        const float di = L.d[i];
        const double si = ((double)di > LD_EPSILON && di <= radius) ? (double)((radius - di) / (radius * di)) : 0.0;
        double t = 0.0;
        if (!(si == 0.0 || di <= 0.0)) {
            const double xi = st.sx[L.idx[i]], yi = st.sy[L.idx[i]];
            for (uint32_t j = 0; j < n; ++j) {
                const float dj = L.d[j];
                const double sj = ((double)dj > LD_EPSILON && dj <= radius) ? (double)((radius - dj) / (radius * dj)) : 0.0;
                if (i == j || sj == 0.0 || dj <= 0.0) continue;
                const double xj = st.sx[L.idx[j]], yj = st.sy[L.idx[j]];
                const double cosine = ((X - xi) * (X - xj) + (Y - yi) * (Y - yj)) / (di * dj);          /* the float product of the two distances */
                t += sj * (1.0 - cosine);
            }
            t *= invWeightSum;
        }
        L.wt[i] = si * si * (1.0 + t);
    }
    ld_sync();
    weightSum = 0.0;
    for (uint32_t i = 0; i < n; ++i) weightSum += L.wt[i];
    const double invWeightSumFinal = 1.0 / weightSum;
    double result = 0.0;
    for (uint32_t i = 0; i < n; ++i) result += (L.wt[i] * invWeightSumFinal) * (double)L.val[i];
    return (float)result;
}

/* localSelection (interpolation.cpp:1087-1170) for the cell at the float (x, y): fills the list, returns its length; radius: localRadius */
SF3D_METEO_FN uint32_t ld_select(const LdSetup& s, const LdStations& st, const LdList& L, float x, float y, float& radius)
{
    const uint32_t lane = ld_lane();
    if (st.n <= s.minPoints) {
        for (uint32_t i = lane; i < st.n; i += LD_LANES) {
            L.idx[i] = (uint16_t)i; L.d[i] = meteo_distance(x, y, st.sx[i], st.sy[i]); L.h[i] = st.sh[i]; L.val[i] = st.sv[i]; L.w[i] = 1.f;
        }
        radius = s.radiusAll;
        ld_sync();
        return st.n;
    }
    uint32_t nrValid = 0;
    float maxDistance = 0.f, stepRadius = 7500.f, r0 = 0.f, r1 = stepRadius;
    bool beyondLastPoint = false;
    for (uint32_t ring = 0; nrValid < s.minPoints && !beyondLastPoint && ring < LD_RING_CAP; ++ring) {
        bool anyBeyond = false;
        for (uint32_t base = 0; base < st.n; base += LD_LANES) {
            const uint32_t i = base + lane;
            const bool in = i < st.n;
            const float d = in ? meteo_distance(x, y, st.sx[i], st.sy[i]) : 0.f;
            const bool selected = in && !meteo_eqf(d, (float)LD_NODATA) && d > r0 && d <= r1;
            const uint64_t mask = ld_ballot(selected);
            if (selected) {
                const uint32_t at = nrValid + ld_below(mask);
                L.idx[at] = (uint16_t)i; L.d[at] = d; L.h[at] = st.sh[i]; L.val[at] = st.sv[i]; L.w[at] = 1.f;
                if (d > maxDistance) maxDistance = d;
            }
            nrValid += (uint32_t)__builtin_popcountll(mask);
            anyBeyond = anyBeyond || (ld_ballot(in && d > r1) != 0);
        }
        beyondLastPoint = !anyBeyond;
        if (nrValid > s.minPointsStep) stepRadius = 1000.f;
        r0 = r1;
        r1 += stepRadius;
    }
    /* the largest of the lanes' maxima: a maximum of floats, the same in any order */
    L.lanes[lane] = maxDistance;
    ld_sync();
    for (uint32_t k = 0; k < LD_LANES; ++k) maxDistance = (L.lanes[k] > maxDistance) ? L.lanes[k] : maxDistance;
    if (!meteo_eqf(maxDistance, 0.f)) {
        for (uint32_t i = lane; i < nrValid; i += LD_LANES) {
            const float w = 1.f - L.d[i] / maxDistance;
            L.w[i] = (w > (float)LD_EPSILON) ? w : (float)LD_EPSILON;        /* MAXVALUE */
        }
    }
    radius = maxDistance;
    ld_sync();
    return nrValid;
}

/* multipleDetrendingElevationFitting (interpolation.cpp:1862-1953) and detrendingElevation over the list: proxyValidity (:1418-1457) and
 * the minimum of elevation points (:1885), then the fit.  Returns whether the height proxy is significant; par: the cell's parameters,
 * NODATA where it is not; R2: NODATA where no fit ran.  k_localdetrend_proxies (sf3d_localproxies.inc) runs the same text */
SF3D_METEO_FN bool ld_elevation(const LdSetup& s, const LdList& L, uint32_t n, double* par, double& R2)
{
    uint32_t nrData = 0;
    double sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float hf = L.h[i];
        if (hf != (float)LD_NODATA) { ++nrData; sum += hf; }
    }
    bool valid = nrData >= LD_MIN_NR;
    if (valid) {
        const double avg = sum / (double)nrData;
        sum = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const float hf = L.h[i];
            if (hf != (float)LD_NODATA) sum += (hf - avg) * (hf - avg);
        }
        const double stdDev = __builtin_sqrt(sum / (double)(nrData - 1));
        if (s.stdDevThreshold != (float)LD_NODATA) valid = stdDev > s.stdDevThreshold;
    }
    valid = valid && nrData >= (uint32_t)s.minPointsLocal;

#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) par[j] = LD_NODATA;
    R2 = LD_NODATA;
    bool significant = false;
    if (valid) {
        if (s.function == LD_PIECEWISE_TWO) significant = ld_fit<LD_PIECEWISE_TWO, 4>(s, L, n, nrData, par, R2);
        else if (s.function == LD_PIECEWISE_THREE) significant = ld_fit<LD_PIECEWISE_THREE, 5>(s, L, n, nrData, par, R2);
        else significant = ld_fit<LD_PIECEWISE_THREE_FREE, 6>(s, L, n, nrData, par, R2);
    }
    return significant;
}

/* the methods of interpolate() (interpolation.cpp:2511-2528) over a list of n stations; radius: localRadius */
SF3D_METEO_FN float ld_methods(const LdSetup& s, const LdStations& st, const LdList& L, uint32_t n, float radius, float x, float y)
{
    if (s.method == METEO_IDW) return meteo_idw(LdListDistance{L.d}, L.val, n);
    if (s.method == METEO_SHEPARD) {
        /* computeShepardInitialRadius(area, nrPoints, SHEPARD_AVG_NRPOINTS) with the list's size (interpolation.cpp:812-813) */
        const float radius0 = __builtin_sqrtf(((float)8u * s.area) / ((float)3.1415926535898 * (float)n));
        return meteo_shepard(LdListDistance{L.d}, LdCoord{st.sx, L.idx}, LdCoord{st.sy, L.idx}, (const float*)L.val, n, x, y, radius0, false);
    }
    return ld_shepard_modified(st, L, n, radius, x, y);
}

/* the elevation function of the call at the height z */
SF3D_METEO_FN double ld_height_function(const LdSetup& s, double z, double* par)
{
    if (s.function == LD_PIECEWISE_TWO) return ld_func<LD_PIECEWISE_TWO>(z, par);
    if (s.function == LD_PIECEWISE_THREE) return ld_func<LD_PIECEWISE_THREE>(z, par);
    return ld_func<LD_PIECEWISE_THREE_FREE>(z, par);
}

/* one DEM cell of height z at the float (x, y): the map value; `o`: what the getters return of the cell */
SF3D_METEO_FN float ld_cell(const LdSetup& s, const LdStations& st, const LdList& L, float z, float x, float y, LdOutcome& o)
{
    float radius;
    const uint32_t n = ld_select(s, st, L, x, y, radius);
    o.count = n; o.radius = radius; o.significant = 0;
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = LD_NODATA;

    double par[LD_MAX_PARAMETERS];
    double R2;
    const bool significant = ld_elevation(s, L, n, par, R2);
    o.r2 = (float)R2;
    if (significant) {
        o.significant = 1;
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = par[j];
    }

    /* interpolate() over the list */
    float result = ld_methods(s, st, L, n, radius, x, y);
    if (meteo_eqf(result, (float)LD_NODATA)) return (float)LD_NODATA;
    if (s.useDetrending) {
        /* retrend, interpolation.cpp:1298-1313: float(functionSum(...)) of the cell's height with the cell's parameters */
        double retrendValue = 0.;
        if (significant) {
            double sumOfFunctions = 0.0;
            sumOfFunctions += ld_height_function(s, (double)z, par);
            retrendValue = (float)sumOfFunctions;
        }
        result += (float)retrendValue;
    }
    return result;
}

#ifndef SF3D_METEO_HOST
#define LD_CELLS_PER_BLOCK (SF3D_BLOCK / 64)

__global__ void __launch_bounds__(SF3D_BLOCK) k_localdetrend(LocalDetrendView)
{
    const LocalDetrendView& v = meteo_kernel_argument<LocalDetrendView>();
    __shared__ double sx[METEO_MAX_STATIONS], sy[METEO_MAX_STATIONS];
    __shared__ float sh[METEO_MAX_STATIONS], sv[METEO_MAX_STATIONS];
    __shared__ double heightsAndWeights[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ double fit[LD_CELLS_PER_BLOCK][LD_MAX_FIRST_GUESS * LD_FIT_STRIDE];
    __shared__ float distances[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS], values[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    __shared__ float lanes[LD_CELLS_PER_BLOCK][64];
    __shared__ uint16_t indices[LD_CELLS_PER_BLOCK][METEO_MAX_STATIONS];
    const MeteoView& m = v.m;
    const uint32_t nStations = m.nStations < METEO_MAX_STATIONS ? m.nStations : METEO_MAX_STATIONS;
    for (uint32_t k = threadIdx.x; k < nStations; k += blockDim.x) { sx[k] = m.sx[k]; sy[k] = m.sy[k]; sv[k] = m.sv[k]; sh[k] = v.sh[k]; }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * LD_CELLS_PER_BLOCK + wave;
    if (c >= m.nCells) return;
    float result = m.flag;
    LdOutcome o;
    o.count = 0; o.radius = (float)LD_NODATA; o.significant = 0; o.r2 = (float)LD_NODATA;
#pragma unroll
    for (int j = 0; j < LD_MAX_PARAMETERS; ++j) o.parameters[j] = LD_NODATA;
    const float z = m.dem[c];
    if (!(m.mine && !m.mine[c]) && !meteo_eqf(z, m.flag)) {
        float x, y;
        meteo_cell_xy(m, c, x, y);
        LdList L;
        L.idx = indices[wave]; L.d = distances[wave]; L.val = values[wave];
        L.h = (float*)heightsAndWeights[wave]; L.w = L.h + METEO_MAX_STATIONS; L.wt = heightsAndWeights[wave];
        L.lanes = lanes[wave]; L.fit = fit[wave];
        result = ld_cell(v.s, LdStations{sx, sy, sh, sv, nStations}, L, z, x, y, o);
    }
    if (ld_lane() == 0) {
        m.out[c] = result;
        v.count[c] = o.count; v.radius[c] = o.radius; v.significant[c] = (uint8_t)o.significant; v.r2[c] = o.r2;
#pragma unroll
        for (int j = 0; j < LD_MAX_PARAMETERS; ++j) v.parameters[(size_t)c * LD_MAX_PARAMETERS + j] = o.parameters[j];
    }
}

/* ---- host side: the per-cell outcome of the last call belongs to the meteo block (MeteoCache) and goes with meteo_free ---- */
static const size_t LD_CELL_BYTES = LD_MAX_PARAMETERS * sizeof(double) + sizeof(uint32_t) + 2 * sizeof(float) + sizeof(uint8_t);
static const size_t LD_TABLE_BYTES = (size_t)(3 + LD_MAX_FIRST_GUESS) * LD_MAX_PARAMETERS * sizeof(double) + (size_t)METEO_MAX_STATIONS * sizeof(float);

sf3d_error_t DeviceSolver::localdetrend_free()
{
    if (!impl_) return SF3D_OK;
    MeteoCache& K = impl_->meteo;
    raster_release({K.localFit, K.localTables});
    K.localFit = nullptr; K.localTables = nullptr; K.localDone = false; K.localMs = 0.;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::localdetrend_interpolate(const MeteoCall& call, const LocalDetrendCall& local, const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    LocalDetrendView v{};
    sf3d_error_t e = meteo_view(call, mine, v.m);
    if (e != SF3D_OK) return e;
    K.localDone = false; K.proxiesDone = false;             /* the outcome of a call of sf3d_localproxies.inc is overwritten */
    if (!K.localFit) RASTER_TRY(hipMalloc((void**)&K.localFit, n * LD_CELL_BYTES));
    if (!K.localTables) RASTER_TRY(hipMalloc((void**)&K.localTables, LD_TABLE_BYTES));
    double* table = (double*)K.localTables;
    float* heights = (float*)(table + (size_t)(3 + LD_MAX_FIRST_GUESS) * LD_MAX_PARAMETERS);
    RASTER_TRY(hipMemcpyAsync(table, local.table, (size_t)(3 + LD_MAX_FIRST_GUESS) * LD_MAX_PARAMETERS * sizeof(double), hipMemcpyHostToDevice, I.stream));
    if (call.nStations) RASTER_TRY(hipMemcpyAsync(heights, local.height, call.nStations * sizeof(float), hipMemcpyHostToDevice, I.stream));
    v.sh = heights;
    v.parameters = (double*)K.localFit;
    v.count = (uint32_t*)(v.parameters + n * LD_MAX_PARAMETERS);
    v.radius = (float*)(v.count + n);
    v.r2 = v.radius + n;
    v.significant = (uint8_t*)(v.r2 + n);
    v.s = local.setup;
    v.s.table = table;
    v.s.method = call.method; v.s.useDetrending = call.useDetrending;
    e = raster_launch(k_localdetrend, n * 64, v, K.localMs);
    if (e != SF3D_OK) return e;
    K.produced[call.var] = true;
    K.localDone = true;
    if (!out) return SF3D_OK;
    return raster_download(out, v.m.out, n * sizeof(float));
}

bool DeviceSolver::localdetrend_done() const { return impl_ && impl_->meteo.base && impl_->meteo.localFit && impl_->meteo.localDone; }

sf3d_error_t DeviceSolver::localdetrend_fit(uint8_t* significant, float* r2, double* parameters)
{
    const MeteoCache& K = impl_->meteo;
    const size_t n = K.nCells;
    const double* dp = (const double*)K.localFit;
    const float* dr2 = (const float*)((const uint32_t*)(dp + n * LD_MAX_PARAMETERS) + n) + n;
    sf3d_error_t e = SF3D_OK;
    if (parameters) e = raster_download(parameters, dp, n * LD_MAX_PARAMETERS * sizeof(double));
    if (e == SF3D_OK && r2) e = raster_download(r2, dr2, n * sizeof(float));
    if (e == SF3D_OK && significant) e = raster_download(significant, dr2 + n, n);
    return e;
}

sf3d_error_t DeviceSolver::localdetrend_selection(uint32_t* count, float* radius)
{
    const MeteoCache& K = impl_->meteo;
    const size_t n = K.nCells;
    const uint32_t* dc = (const uint32_t*)((const double*)K.localFit + n * LD_MAX_PARAMETERS);
    sf3d_error_t e = SF3D_OK;
    if (count) e = raster_download(count, dc, n * sizeof(uint32_t));
    if (e == SF3D_OK && radius) e = raster_download(radius, dc + n, n * sizeof(float));
    return e;
}

uint64_t DeviceSolver::localdetrend_bytes() const
{
    if (!impl_) return 0;
    const MeteoCache& K = impl_->meteo;
    return (K.localFit ? (uint64_t)K.nCells * LD_CELL_BYTES : 0) + (K.localTables ? (uint64_t)LD_TABLE_BYTES : 0);
}

double DeviceSolver::localdetrend_kernel_ms() const { return impl_ ? impl_->meteo.localMs : 0.; }
#endif
