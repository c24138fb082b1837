/* part of sf3d_solver.hip (included there, in this order: physics, control, phases, host_build, host_step) - device helpers: non-temporal streams, table-driven log / pow glue, Math::computeMean, the Soil:: functions of soilPhysics.cpp */
/* ======================================================================================= */
/* device helpers                                                                           */
/* ======================================================================================= */

/* Streaming accesses that do not allocate in the caches: the coefficient slabs (80 B/node, read exactly
 * once per sweep by exactly one wave), the static link geometry and the per-link flow sums would
 * otherwise evict x, b and z from L2 / the 256 MiB Infinity Cache between two sweeps.  `NT is a kernel
 * template parameter chosen per launch from DevView::ntStream (a run-time select of the two forms is
 * merged by the compiler into one plain load): off when a rank's whole working set fits the Infinity Cache. */
typedef double sf3d_v2 __attribute__((ext_vector_type(2)));
template <bool NT> __device__ __forceinline__ sf3d_d2 load_coeff(const sf3d_d2* p)
{
    sf3d_v2 t;
    if (NT) t = __builtin_nontemporal_load(reinterpret_cast<const sf3d_v2*>(p));
    else t = *reinterpret_cast<const sf3d_v2*>(p);
    sf3d_d2 r; r.x = t.x; r.y = t.y; return r;
}
template <bool NT> __device__ __forceinline__ void store_coeff(sf3d_d2* p, double x, double y)
{
    sf3d_v2 t; t.x = x; t.y = y;
    if (NT) __builtin_nontemporal_store(t, reinterpret_cast<sf3d_v2*>(p));
    else *reinterpret_cast<sf3d_v2*>(p) = t;
}
typedef float sf3d_fv2 __attribute__((ext_vector_type(2)));
template <bool NT> __device__ __forceinline__ sf3d_f2 load_f2(const sf3d_f2* p)
{
    sf3d_fv2 t;
    if (NT) t = __builtin_nontemporal_load(reinterpret_cast<const sf3d_fv2*>(p));
    else t = *reinterpret_cast<const sf3d_fv2*>(p);
    sf3d_f2 r; r.x = t.x; r.y = t.y; return r;
}
template <bool NT> __device__ __forceinline__ void store_f2(sf3d_f2* p, float x, float y)
{
    sf3d_fv2 t; t.x = x; t.y = y;
    if (NT) __builtin_nontemporal_store(t, reinterpret_cast<sf3d_fv2*>(p));
    else *reinterpret_cast<sf3d_fv2*>(p) = t;
}
template <bool NT, class T> __device__ __forceinline__ T load_stream(const T* p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}
template <bool NT, class T> __device__ __forceinline__ void store_stream(T* p, T x)
{
    if (NT) __builtin_nontemporal_store(x, p); else *p = x;
}

/* std::max / std::min semantics (NaN handling included) */
__device__ __forceinline__ double dmax(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double dmin(double a, double b) { return (b < a) ? b : a; }

/* ---- log / pow / exp / cbrt of the kernels ---------------------------------------------------------------------------------------------
 * Two sets, chosen at compile time (SF3D_LIBM_GLIBC, default 1):
 *  1  sf3d_glibcmath.inc - the operations of the reference build's C library (glibc 2.35: the FMA variants of log / exp / pow, the generic
 *     cbrt) one for one, so every elementary function of the time step returns the bits the reference's libm call returns
 *     (tests/test_glibcmath.py: host build == libm on > 10^8 arguments; tests/test_gpu_fastmath.py: device == host build).  Config 5's
 *     air-entry kink amplifies a last-ulp difference of these functions to 7.7e-4 (DESIGN.md 2); with this set nothing is left to amplify.
 *  0  sf3d_fastmath.inc - the 0.50-0.51-ulp table routines of rounds 1-4 (closer to the true value than the library, hence NOT the
 *     library's bits in 0.1 % of the calls); kept as the build the oracle's fast-math twin is a twin of (-DSF3D_LIBM_GLIBC=0).
 * Both are table designs of the same size (128 pieces of log, 128 of 2^(j/128)); the tables sit in LDS: 64 lanes with 64 different
 * pieces would cost ~64 texture-addresser cycles per vector-memory gather.  Every kernel that evaluates flog() / ppow() / fexp() calls
 * fm_init() first.  -DSF3D_FAST_LOG=0 / -DSF3D_FAST_POW=0 (set 0 only) restore the device library's calls. */
#ifndef SF3D_LIBM_GLIBC
#define SF3D_LIBM_GLIBC 1
#endif
#if SF3D_LIBM_GLIBC
#define SF3D_GL_FN __device__ __forceinline__
#define SF3D_GL_TABLE __device__ const
struct FmLds { double linvc[128], llogc[128], pinvc[128], plogc[128], ptail[128]; uint64_t etail[128], esbits[128]; };
__device__ __forceinline__ FmLds& fm_lds() { __shared__ FmLds t; return t; }
#define SF3D_GL_LOG_LOOKUP(i, vInvc, vLogc) const double vInvc = fm_lds().linvc[i], vLogc = fm_lds().llogc[i]
#define SF3D_GL_POWLOG_LOOKUP(i, vInvc, vLogc, vTail) const double vInvc = fm_lds().pinvc[i], vLogc = fm_lds().plogc[i], vTail = fm_lds().ptail[i]
#define SF3D_GL_EXP_LOOKUP(i, vTail, vSbits) const uint64_t vTail = fm_lds().etail[i], vSbits = fm_lds().esbits[i]
#include "sf3d_glibcmath.inc"
__device__ __forceinline__ void fm_init()
{
    FmLds& t = fm_lds();
    for (uint32_t k = threadIdx.x; k < 128; k += blockDim.x) {
        t.linvc[k] = sf3d_gl_log_table[k].invc; t.llogc[k] = sf3d_gl_log_table[k].logc;
        t.pinvc[k] = sf3d_gl_powlog_table[k].invc; t.plogc[k] = sf3d_gl_powlog_table[k].logc; t.ptail[k] = sf3d_gl_powlog_table[k].logctail;
        t.etail[k] = sf3d_gl_exp_table[k].tail; t.esbits[k] = sf3d_gl_exp_table[k].sbits;
    }
    __syncthreads();
}
__device__ __forceinline__ double flog(double x) { return sf3d_gl_log(x); }
__device__ __forceinline__ double fexp(double x) { return sf3d_gl_exp(x); }
__device__ __forceinline__ double ppow(double x, double y) { return sf3d_gl_pow(x, y); }
__device__ __forceinline__ double pcbrt(double x) { return sf3d_gl_cbrt(x); }
/* Mualem's tortuosity factor Se^L is a pow call in the reference (soilPhysics.cpp:213) - also for L = 0.5, where the library's pow and
 * a correctly rounded square root differ in the last bit now and then */
__device__ __forceinline__ double tortuosity(double Se, double L) { return sf3d_gl_pow(Se, L); }
#else
#ifndef SF3D_FAST_LOG
#define SF3D_FAST_LOG 1
#endif
#ifndef SF3D_FAST_POW
#define SF3D_FAST_POW 1
#endif
#define SF3D_FM_FN __device__ __forceinline__
#define SF3D_FM_TABLE __device__ const
struct FmLds { double invc[128], lhi[128], llo[128], ehi[128], elo[128]; };
__device__ __forceinline__ FmLds& fm_lds() { __shared__ FmLds t; return t; }
#define SF3D_FM_LOOKUP(i, e) struct sf3d_flog_entry e; { const FmLds& t_ = fm_lds(); e.invc = t_.invc[i]; e.logc_hi = t_.lhi[i]; e.logc_lo = t_.llo[i]; }
#define SF3D_FM_EXP_LOOKUP(j, e) struct sf3d_fexp_entry e; { const FmLds& t_ = fm_lds(); e.hi = t_.ehi[j]; e.lo = t_.elo[j]; }
#include "sf3d_fastmath.inc"
__device__ __forceinline__ void fm_init()
{
#if SF3D_FAST_LOG || SF3D_FAST_POW
    FmLds& t = fm_lds();
    for (uint32_t k = threadIdx.x; k < 128; k += blockDim.x) {
        t.invc[k] = sf3d_flog_table[k].invc; t.lhi[k] = sf3d_flog_table[k].logc_hi; t.llo[k] = sf3d_flog_table[k].logc_lo;
        t.ehi[k] = sf3d_fexp_table[k].hi; t.elo[k] = sf3d_fexp_table[k].lo;
    }
    __syncthreads();
#endif
}
__device__ __forceinline__ double flog(double x)
{
#if SF3D_FAST_LOG
    return sf3d_flog(x);
#else
    return log(x);
#endif
}
__device__ __forceinline__ double fexp(double x)
{
#if SF3D_FAST_POW
    return sf3d_fexp(x);
#else
    return exp(x);
#endif
}
extern "C" __device__ double __ocml_powr_f64(double, double);
__device__ __forceinline__ double ppow(double x, double y)
{
#if SF3D_FAST_POW
    return sf3d_fpow(x, y);
#else
    return __ocml_powr_f64(x, y);
#endif
}
/* cbrt of Manning's Hs^(2/3) (water.cpp:389-390, 468-469): the table routine too - 0.504 ulp (glibc's cbrt, the reference's: 2.85 ulp;
 * the device library's: 1 ulp) and the same bits in the host build of the text (tests, the fast-math twin of the oracle) */
__device__ __forceinline__ double pcbrt(double x)
{
#if SF3D_FAST_POW
    return sf3d_fcbrt(x);
#else
    return cbrt(x);
#endif
}
/* Mualem tortuosity Se^L: L = 0.5 in every soil table of the application -> correctly rounded sqrt */
__device__ __forceinline__ double tortuosity(double Se, double L) { return (L == 0.5) ? sqrt(Se) : ppow(Se, L); }
#endif

/* the coefficient matrix of the computeStep in progress */
__device__ __forceinline__ sf3d_d2* cur_A2(const DevView& v) { return v.A2x[v.ctrl->aBuf]; }      /* aBuf < Ctrl::aRing (k_step_begin) */

__device__ __forceinline__ int free_buffer3(int cur, int hold, int best)
{
    for (int b = 0; b < SF3D_POOL; ++b)
        if (b != cur && b != hold && b != best) return b;
    return 0;   /* unreachable: at most three of five buffers are in use */
}
__device__ __forceinline__ int free_buffer(const Ctrl* c) { return free_buffer3(c->cur, c->hold, c->best); }

/* the two free buffers of the pool of five (paired sweep: x' and x'') */
__device__ __forceinline__ void free_buffers2(const Ctrl* c, int& f1, int& f2)
{
    uint32_t used = (1u << c->cur) | (1u << c->hold);
    if (c->best >= 0) used |= 1u << c->best;
    uint32_t fr = ~used & ((1u << SF3D_POOL) - 1u);      /* at least two bits: three of five buffers are in use at most */
    f1 = __builtin_ctz(fr); fr &= fr - 1u;
    f2 = __builtin_ctz(fr);
}

/* fixed-shape block reductions (256 threads = 4 waves of 64) */
__device__ __forceinline__ double block_sum(double v)
{
    __shared__ double sm[SF3D_BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__device__ __forceinline__ double block_max(double v)
{
    __shared__ double sm[SF3D_BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) v = dmax(v, __shfl_down(v, off, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    return dmax(dmax(sm[0], sm[1]), dmax(sm[2], sm[3]));
}
/* ---- the norm of a Jacobi sweep as a DOUBLE-DOUBLE sum ------------------------------------------------------------------------------
 * JacobiWaterCPU's norm (water.cpp:592-600) is a sum of N non-negative terms, and solveLinearSystem compares it with the tolerance
 * (cpusolver.cpp:672-703).  The kernels that can produce an iteration - k_sweep, the paired passes, k_sweep_bnd, one GPU or N strips -
 * add the same terms in different associations (lanes, waves, blocks, patches, ranks); summed in plain doubles their norms agree to
 * rounding only and a decision could differ at a tie of that size (round 3's review: "an empirical, not a structural, property").
 * Carried as an unevaluated pair (hi, lo) with an error-free TwoSum per addition, every association gives the true sum to ~2^-100
 * relative, so the ONE rounding at the end (hi + lo) gives the same double whatever the launch form or the number of ranks - up to the
 * ~1e-9 of the cases in which the true sum lies within 2^-100 of a rounding boundary.  (-ffp-contract=off and no fast-math: the
 * compiler keeps the TwoSum.)  Cost: five more additions per node in kernels whose VALU is 13-24 % busy. */
__device__ __forceinline__ void dd_add(double& hi, double& lo, double x)
{
    const double s = hi + x, bb = s - hi;
    lo += (hi - (s - bb)) + (x - bb);
    hi = s;
}
__device__ __forceinline__ void dd_merge(double& hi, double& lo, double h2, double l2)
{
    const double s = hi + h2, bb = s - hi;
    lo += ((hi - (s - bb)) + (h2 - bb)) + l2;
    hi = s;
}
__device__ __forceinline__ void wave_sum_dd(double& hi, double& lo)         /* result in lane 0 */
{
    for (int off = 32; off > 0; off >>= 1) { const double h2 = __shfl_down(hi, off, 64), l2 = __shfl_down(lo, off, 64); dd_merge(hi, lo, h2, l2); }
}
__device__ __forceinline__ void block_sum_dd(double& hi, double& lo)        /* 256 threads; result in every thread */
{
    __shared__ double smh[SF3D_BLOCK / 64], sml[SF3D_BLOCK / 64];
    wave_sum_dd(hi, lo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { smh[wave] = hi; sml[wave] = lo; }
    __syncthreads();
    hi = smh[0]; lo = sml[0];
    for (int w = 1; w < SF3D_BLOCK / 64; ++w) dd_merge(hi, lo, smh[w], sml[w]);
}
/* one block reduces nb pairs of partials */
__device__ __forceinline__ void reduce_partials_sum_dd(const double* ph, const double* pl, uint32_t nb, double& hi, double& lo)
{
    hi = 0.; lo = 0.;
    for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK) dd_merge(hi, lo, ph[k], pl[k]);
    block_sum_dd(hi, lo);
}

/* one block reduces nb partials in a fixed order */
__device__ __forceinline__ double reduce_partials_sum(const double* p, uint32_t nb)
{
    double s = 0.;
    for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK) s += p[k];
    return block_sum(s);
}
__device__ __forceinline__ double reduce_partials_max(const double* p, uint32_t nb)
{
    double s = 0.;
    for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK) s = dmax(s, p[k]);
    return block_max(s);
}

/* a / b for the link arithmetic (conductivities, distances, logarithms of conductivity ratios: finite operands of ordinary
 * magnitude).  The compiler's IEEE sequence is 17 instructions - operand scaling, reciprocal seed, two Newton steps, quotient,
 * residual, re-scaling, special-case fix-up - and there are thirty divisions per soil row; this one keeps the seed, the Newton
 * steps and the residual correction (8 instructions, the same <= 1 ulp) and hands everything whose result is not a finite number
 * (b = 0, denormal or infinite operands, nan) to the full sequence, so that the special cases keep the reference's answers - the
 * logarithmic mean of two conductivities one ulp apart really divides by log(1) = 0.
 * OFF by default (-DSF3D_FAST_DIV=1 turns it on): measured at C4, k_assemble 303-305 us with it against 300 us without - the kernel's
 * time is not in its VALU instruction count (DESIGN.md 4), so the exactly rounded quotients stay. */
#ifndef SF3D_FAST_DIV
#define SF3D_FAST_DIV 0
#endif
__device__ __forceinline__ double qdiv(double a, double b)
{
#if SF3D_FAST_DIV
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
    double q = a * r;
    q = __builtin_fma(__builtin_fma(-b, q, a), r, q);
    if (__builtin_expect(!(fabs(q) < __builtin_inf()), 0)) q = a / b;
    return q;
#else
    return a / b;
#endif
}

/* ---- Math::computeMean (otherFunctions.cpp:7-36) ---- */
/* the logarithm is the table-driven one: every kernel that evaluates a mean has called fm_init() */
__device__ __forceinline__ double mean_of(double v1, double v2, uint32_t type)
{
    if (type == SF3D_MEAN_ARITHMETIC) return (v1 + v2) * 0.5;
    if (type == SF3D_MEAN_GEOMETRIC) { const int sign = (v1 > 0) - (v1 < 0); return sign * sqrt(v1 * v2); }
    return (v1 == v2) ? v1 : qdiv(v1 - v2, flog(qdiv(v1, v2)));
}

/* ---- Soil:: (soilPhysics.cpp) ---- */
__device__ __forceinline__ double se_from_psi(const SoilDev& s, double psi, uint32_t wrc)   /* :91-115 */
{
    if (wrc == SF3D_WRC_VAN_GENUCHTEN) return ppow(1.0 + ppow(s.alpha * psi, s.n), -s.m);
    if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) {
        if (psi <= s.he) return 1.0;
        return ppow(1.0 + ppow(s.alpha * psi, s.n), -s.m) * s.invSc;
    }
    return NODATA_D;
}
__device__ __forceinline__ double node_se(const SoilDev& s, double H, double z, uint32_t wrc)  /* :68-83 */
{
    if (H >= z) return 1.;
    return se_from_psi(s, fabs(H - z), wrc);
}
__device__ __forceinline__ double mualem_k(const SoilDev& s, double Se, uint32_t wrc)          /* :181-214 */
{
    if (Se >= 1.0) return s.Ksat;
    double temp;
    if (wrc == SF3D_WRC_VAN_GENUCHTEN) {
        const double sePow = ppow(Se, s.invM);
        temp = 1.0 - ppow(1.0 - sePow, s.m);
    } else if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) {
        const double seScPow = ppow(Se * s.Sc, s.invM);
        const double tNum = 1.0 - ppow(1.0 - seScPow, s.m);
        temp = tNum / s.mualemDen;
    } else return NODATA_D;
    return s.Ksat * tortuosity(Se, s.L) * (temp * temp);
}
__device__ __forceinline__ double dtheta_dh(const SoilDev& s, double H, double Ho, double z, uint32_t wrc)   /* :224-279 */
{
    const double psiCurr = fabs(dmin(0.0, H - z));
    const double psiPrev = fabs(dmin(0.0, Ho - z));
    if (wrc == SF3D_WRC_VAN_GENUCHTEN) { if (psiCurr == 0.0 && psiPrev == 0.0) return 0.0; }
    else if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) { if (psiCurr <= s.he && psiPrev <= s.he) return 0.0; }
    double dSe;
    if (fabs(psiCurr - psiPrev) < 1e-12) {
        const double xx = s.alpha * psiCurr;
        const double onePlus = 1. + ppow(xx, s.n);
        const double t1 = ppow(onePlus, -(s.m + 1.));
        const double t2 = ppow(xx, s.n - 1.);
        dSe = s.alpha * s.n * s.m * t1 * t2;
        if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) dSe *= s.invSc;
    } else {
        const double a = se_from_psi(s, psiCurr, wrc), c = se_from_psi(s, psiPrev, wrc);
        dSe = fabs((a - c) / (H - Ho));
    }
    return dSe * (s.thetaS - s.thetaR);
}

