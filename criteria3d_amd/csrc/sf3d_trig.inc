/*
 * sf3d_trig.inc - the trigonometry of the radiation block (sf3d_rad.inc), in the dual host / device style of sf3d_glibcmath.inc: the same
 * text compiles for the device (inside sf3d_solver.hip) and for the host (tests/trig_host.c, tests/rad_host.cpp), every operation is
 * written out, and the translation units that include it are compiled with -ffp-contract=off, so the two builds give the same bits
 * (tests/test_gpu_rad.py) - the operations are IEEE + - x / sqrt, integer conversions and bit moves only, no table but powf's.
 *
 * Two kinds of routine:
 *
 *  FAITHFUL, not the C library's: sf3d_tr_sin, sf3d_tr_cos, sf3d_tr_tan, sf3d_tr_acos (double).  glibc's double sin / cos / tan / acos
 *    are the IBM Accurate Mathematical Library's table designs with multi-stage fall-backs and cannot be restated operation by operation;
 *    these are the classic Sun fdlibm algorithms (k_sin.c, k_cos.c, k_tan.c, e_acos.c, and the Cody-Waite medium path of e_rem_pio2.c:
 *    pi/2 in three 33-bit pieces with the next piece added when the leading bits cancel): error below one ulp, so never more than one ulp
 *    from libm (tests/test_trig_host.py, 10^7 arguments per function, with the measured share of arguments that differ at all).
 *    Argument reduction holds for |x| < 2^20 pi/2; the radiation block stays below 7 rad and the tests below 200.  Beyond that range the
 *    result is finite but not accurate, inf and nan give nan.
 *
 *  THE LIBRARY'S BITS: sf3d_tr_acosf and sf3d_tr_powf.  The reference's solPos.cpp passes floats to acos() and pow(), which in C++ are the
 *    float overloads: its object code calls acosf (zenith, sunset hour angle, azimuth, incidence) and powf (Kasten's air mass).  glibc 2.35's
 *    acosf is fdlibm's float routine in float arithmetic (sysdeps/ieee754/flt-32/e_acosf.c) and its powf Szabolcs Nagy's table design in
 *    double arithmetic rounded to float once (e_powf.c; data: sf3d_trig_tables.h, read from the library by scripts/gen_trig_tables.py).
 *    Both are restated operation by operation and held against libm bit for bit.  powf: the ordinary path only - x a positive normal
 *    float, y finite and non-zero, |y log2 x| < 126 - anything else returns nan; the multiply-adds are fused where the library's x86-64
 *    FMA build fuses them (a different choice moves the double result by 2^-53 before it is rounded to 24 bits).
 *
 * Include with SF3D_TR_FN defined as the function qualifiers (`__device__ __forceinline__` / `static inline`) and SF3D_TR_TABLE as the
 * storage qualifiers of powf's tables (`__device__ const` / `static const`).
 */
#include <stdint.h>

#include "sf3d_trig_tables.h"

SF3D_TR_FN double sf3d_tr_from_bits(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
SF3D_TR_FN uint64_t sf3d_tr_bits(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
SF3D_TR_FN float sf3d_tr_from_bitsf(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
SF3D_TR_FN uint32_t sf3d_tr_bitsf(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
SF3D_TR_FN uint32_t sf3d_tr_hi(double d) { return (uint32_t)(sf3d_tr_bits(d) >> 32); }
SF3D_TR_FN double sf3d_tr_clear_lo(double d) { return sf3d_tr_from_bits(sf3d_tr_bits(d) & 0xffffffff00000000ull); }

/* ---- x = n pi/2 + (y0 + y1), |y0 + y1| <= pi/4 (e_rem_pio2.c, the path for |x| < 2^20 pi/2) ------------------------------------------- */
struct sf3d_tr_reduced { double y0, y1; int n; };
SF3D_TR_FN struct sf3d_tr_reduced sf3d_tr_rem_pio2(double x)
{
    const double invpio2 = 6.36619772367581382433e-01;         /* 53 bits of 2/pi */
    const double pio2_1 = 1.57079632673412561417e+00;          /* first 33 bits of pi/2 */
    const double pio2_1t = 6.07710050650619224932e-11;         /* pi/2 - pio2_1 */
    const double pio2_2 = 6.07710050630396597660e-11;          /* second 33 bits */
    const double pio2_2t = 2.02226624879595063154e-21;         /* pi/2 - (pio2_1 + pio2_2) */
    const double pio2_3 = 2.02226624871116645580e-21;          /* third 33 bits */
    const double pio2_3t = 8.47842766036889956997e-32;         /* pi/2 - (pio2_1 + pio2_2 + pio2_3) */
    struct sf3d_tr_reduced o;
    const uint32_t hx = sf3d_tr_hi(x);
    const int32_t j = (int32_t)((hx & 0x7fffffffu) >> 20);
    const double t = __builtin_fabs(x);
    const int n = (int)(t * invpio2 + 0.5);
    const double fn = (double)n;
    double r = t - fn * pio2_1;                                 /* exact: fn has at most 20 bits */
    double w = fn * pio2_1t;
    double y0 = r - w;
    int32_t i = j - (int32_t)((sf3d_tr_hi(y0) >> 20) & 0x7ffu);
    if (i > 16) {                                               /* the leading bits cancelled: second piece, good to 118 bits */
        double tt = r;
        w = fn * pio2_2;
        r = tt - w;
        w = fn * pio2_2t - ((tt - r) - w);
        y0 = r - w;
        i = j - (int32_t)((sf3d_tr_hi(y0) >> 20) & 0x7ffu);
        if (i > 49) {                                           /* third piece, 151 bits: covers every double */
            tt = r;
            w = fn * pio2_3;
            r = tt - w;
            w = fn * pio2_3t - ((tt - r) - w);
            y0 = r - w;
        }
    }
    const double y1 = (r - y0) - w;
    if (hx >> 31) { o.y0 = -y0; o.y1 = -y1; o.n = -n; }
    else { o.y0 = y0; o.y1 = y1; o.n = n; }
    return o;
}

/* ---- sin and cos on [-pi/4, pi/4] of x + y, y the tail of x (k_sin.c, k_cos.c) -------------------------------------------------------- */
SF3D_TR_FN double sf3d_tr_ksin(double x, double y, int iy)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x;
    const double v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

SF3D_TR_FN double sf3d_tr_kcos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const uint32_t ix = sf3d_tr_hi(x) & 0x7fffffffu;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3fd33333u) return 1.0 - (0.5 * z - (z * r - x * y));                    /* |x| < 0.3 */
    const double qx = (ix > 0x3fe90000u) ? 0.28125 : sf3d_tr_from_bits((uint64_t)(ix - 0x00200000u) << 32);      /* about x / 4 */
    const double hz = 0.5 * z - qx;
    const double a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}

/* ---- tan on [-pi/4, pi/4] of x + y; iy = 1: tan, iy = -1: -1 / tan (k_tan.c) ------------------------------------------------------------ */
SF3D_TR_FN double sf3d_tr_ktan(double x, double y, int iy)
{
    const double T0 = 3.33333333333334091986e-01, T1 = 1.33333333333201242699e-01, T2 = 5.39682539762260521377e-02,
                 T3 = 2.18694882948595424599e-02, T4 = 8.86323982359930005737e-03, T5 = 3.59207910759131235356e-03,
                 T6 = 1.45620945432529025516e-03, T7 = 5.88041240820264096874e-04, T8 = 2.46463134818469906812e-04,
                 T9 = 7.81794442939557092300e-05, T10 = 7.14072491382608190305e-05, T11 = -1.85586374855275456654e-05,
                 T12 = 2.59073051863633712884e-05;
    const double pio4 = 7.85398163397448278999e-01, pio4lo = 3.06161699786838301793e-17;
    const uint32_t hx = sf3d_tr_hi(x);
    const uint32_t ix = hx & 0x7fffffffu;
    const int big = ix >= 0x3fe59428u;                          /* |x| >= 0.6744: tan(x) from tan(pi/4 - x) */
    if (big) {
        if (hx >> 31) { x = -x; y = -y; }
        const double z0 = pio4 - x;
        const double w0 = pio4lo - y;
        x = z0 + w0;
        y = 0.0;
    }
    double z = x * x;
    double w = z * z;
    double r = T1 + w * (T3 + w * (T5 + w * (T7 + w * (T9 + w * T11))));
    double v = z * (T2 + w * (T4 + w * (T6 + w * (T8 + w * (T10 + w * T12)))));
    double s = z * x;
    r = y + z * (s * (r + v) + y);
    r += T0 * s;
    w = x + r;
    if (big) {
        v = (double)iy;
        return (double)(1 - (int)((hx >> 30) & 2u)) * (v - 2.0 * (x - (w * w / (w + v) - r)));
    }
    if (iy == 1) return w;
    /* -1 / (x + r) with the error of the quotient compensated */
    z = sf3d_tr_clear_lo(w);
    v = r - (z - x);
    const double a = -1.0 / w;
    const double t = sf3d_tr_clear_lo(a);
    s = 1.0 + t * z;
    return t + a * (s + t * v);
}

SF3D_TR_FN double sf3d_tr_sin(double x)
{
    const uint32_t ix = sf3d_tr_hi(x) & 0x7fffffffu;
    if (ix < 0x3e400000u) return x;                            /* |x| < 2^-27 (and -0 stays -0) */
    if (ix <= 0x3fe921fbu) return sf3d_tr_ksin(x, 0.0, 0);
    if (ix >= 0x7ff00000u) return x - x;
    const struct sf3d_tr_reduced q = sf3d_tr_rem_pio2(x);
    switch (q.n & 3) {
        case 0: return sf3d_tr_ksin(q.y0, q.y1, 1);
        case 1: return sf3d_tr_kcos(q.y0, q.y1);
        case 2: return -sf3d_tr_ksin(q.y0, q.y1, 1);
        default: return -sf3d_tr_kcos(q.y0, q.y1);
    }
}

SF3D_TR_FN double sf3d_tr_cos(double x)
{
    const uint32_t ix = sf3d_tr_hi(x) & 0x7fffffffu;
    if (ix <= 0x3fe921fbu) return sf3d_tr_kcos(x, 0.0);
    if (ix >= 0x7ff00000u) return x - x;
    const struct sf3d_tr_reduced q = sf3d_tr_rem_pio2(x);
    switch (q.n & 3) {
        case 0: return sf3d_tr_kcos(q.y0, q.y1);
        case 1: return -sf3d_tr_ksin(q.y0, q.y1, 1);
        case 2: return -sf3d_tr_kcos(q.y0, q.y1);
        default: return sf3d_tr_ksin(q.y0, q.y1, 1);
    }
}

SF3D_TR_FN double sf3d_tr_tan(double x)
{
    const uint32_t ix = sf3d_tr_hi(x) & 0x7fffffffu;
    if (ix < 0x3e300000u) return x;                            /* |x| < 2^-28 */
    if (ix <= 0x3fe921fbu) return sf3d_tr_ktan(x, 0.0, 1);
    if (ix >= 0x7ff00000u) return x - x;
    const struct sf3d_tr_reduced q = sf3d_tr_rem_pio2(x);
    return sf3d_tr_ktan(q.y0, q.y1, 1 - ((q.n & 1) << 1));
}

/* ---- acos (e_acos.c): a rational approximation of (asin(x) - x) / x^3 on [0, 0.5], the half-angle identity above ---------------------- */
SF3D_TR_FN double sf3d_tr_acos(double x)
{
    const double pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const uint32_t hx = sf3d_tr_hi(x);
    const uint32_t ix = hx & 0x7fffffffu;
    if (ix >= 0x3ff00000u) {                                   /* |x| >= 1 */
        if (x == 1.0) return 0.0;
        if (x == -1.0) return pi + 2.0 * pio2_lo;
        return (x - x) / (x - x);
    }
    if (ix < 0x3fe00000u) {                                    /* |x| < 0.5 */
        if (ix <= 0x3c600000u) return pio2_hi + pio2_lo;
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx >> 31) {                                            /* x < -0.5 */
        const double z = (1.0 + x) * 0.5;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double s = __builtin_sqrt(z);
        const double r = p / q;
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;                          /* x > 0.5 */
    const double s = __builtin_sqrt(z);
    const double df = sf3d_tr_clear_lo(s);
    const double c = (z - df * df) / (s + df);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    const double w = r * s + c;
    return 2.0 * (df + w);
}

/* ---- acosf: the library's bits (e_acosf.c of glibc 2.35; every operation rounds to float) ------------------------------------------------ */
SF3D_TR_FN float sf3d_tr_acosf(float x)
{
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const float pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f, pS4 = 7.9153501429e-04f,
                pS5 = 3.4793309169e-05f;
    const float qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    const uint32_t hx = sf3d_tr_bitsf(x);
    const uint32_t ix = hx & 0x7fffffffu;
    if (ix == 0x3f800000u) return (hx >> 31) ? pi + 2.0f * pio2_lo : 0.0f;
    if (ix > 0x3f800000u) return (x - x) / (x - x);
    if (ix < 0x3f000000u) {                                    /* |x| < 0.5 */
        if (ix <= 0x32800000u) return pio2_hi + pio2_lo;
        const float z = x * x;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = 1.0f + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx >> 31) {                                            /* x < -0.5 */
        const float z = (1.0f + x) * 0.5f;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = 1.0f + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float s = __builtin_sqrtf(z);
        const float r = p / q;
        const float w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    const float z = (1.0f - x) * 0.5f;                         /* x > 0.5 */
    const float s = __builtin_sqrtf(z);
    const float df = sf3d_tr_from_bitsf(sf3d_tr_bitsf(s) & 0xfffff000u);
    const float c = (z - df * df) / (s + df);
    const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const float q = 1.0f + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const float r = p / q;
    const float w = r * s + c;
    return 2.0f * (df + w);
}

/* ---- powf: the library's bits on its ordinary path (e_powf.c of glibc 2.35, the FMA build) ----------------------------------------------- */
struct sf3d_tr_log2_entry { double invc, logc; };
SF3D_TR_TABLE struct sf3d_tr_log2_entry sf3d_tr_powf_log2_table[16] = SF3D_TR_POWF_LOG2_TABLE;
SF3D_TR_TABLE uint64_t sf3d_tr_exp2f_table[32] = SF3D_TR_EXP2F_TABLE;

SF3D_TR_FN float sf3d_tr_powf(float x, float y)
{
    const double A[5] = SF3D_TR_POWF_LOG2_A;
    const double C[3] = SF3D_TR_EXP2F_C;
    const uint32_t ix = sf3d_tr_bitsf(x), iy = sf3d_tr_bitsf(y);
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u || 2u * iy - 1u >= 2u * 0x7f800000u - 1u) return __builtin_nanf("");
    /* log2 x = k + log2 c + log2(z / c), z in [0x1.66p-1, 0x1.66p0) */
    const uint32_t tmp = ix - 0x3f330000u;
    const uint32_t i = (tmp >> 19) & 15u;
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int32_t k = (int32_t)top >> 23;                       /* arithmetic shift */
    const double invc = sf3d_tr_powf_log2_table[i].invc, logc = sf3d_tr_powf_log2_table[i].logc;
    const double z = (double)sf3d_tr_from_bitsf(iz);
    const double r = __builtin_fma(z, invc, -1.0);
    const double y0 = logc + (double)k;
    const double r2 = r * r;
    double yy = __builtin_fma(A[0], r, A[1]);
    const double p = __builtin_fma(A[2], r, A[3]);
    const double r4 = r2 * r2;
    double q = __builtin_fma(A[4], r, y0);
    q = __builtin_fma(p, r2, q);
    yy = __builtin_fma(yy, r4, q);
    const double ylogx = (double)y * yy;
    if (!(__builtin_fabs(ylogx) < 126.0)) return __builtin_nanf("");
    /* 2^ylogx = 2^(k/32) 2^r, k = round(32 ylogx) from the low bits of ylogx + 0x1.8p52 / 32 */
    const double shift = 0x1.8p+52 / 32;
    double kd = ylogx + shift;
    const uint64_t ki = sf3d_tr_bits(kd);
    kd -= shift;
    const double rr = ylogx - kd;
    uint64_t t = sf3d_tr_exp2f_table[ki & 31u];
    t += ki << (52 - 5);
    const double s = sf3d_tr_from_bits(t);
    const double zz = __builtin_fma(C[0], rr, C[1]);
    const double rr2 = rr * rr;
    double e = __builtin_fma(C[2], rr, 1.0);
    e = __builtin_fma(zz, rr2, e);
    e = e * s;
    return (float)e;
}
