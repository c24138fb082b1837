/* host build of criteria3d_amd/csrc/sf3d_trig.inc (same text as the device compiles) for tests/test_trig_host.py and tests/test_gpu_rad.py:
 * the routines next to the C library's own, the distance between the two in ulps, and counters of the arguments on which they differ */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#define SF3D_TR_FN static inline
#define SF3D_TR_TABLE static const
#include "sf3d_trig.inc"

/* doubles as ordered integers: neighbours differ by one, -0 and +0 coincide */
static int64_t ordered(double d)
{
    int64_t i;
    memcpy(&i, &d, 8);
    return i < 0 ? (int64_t)0x8000000000000000ull - i : i;
}

static double ours(int which, double x)
{
    switch (which) {
        case 0: return sf3d_tr_sin(x);
        case 1: return sf3d_tr_cos(x);
        case 2: return sf3d_tr_tan(x);
        default: return sf3d_tr_acos(x);
    }
}
static double libm(int which, double x)
{
    switch (which) {
        case 0: return sin(x);
        case 1: return cos(x);
        case 2: return tan(x);
        default: return acos(x);
    }
}

/* which: 0 sin, 1 cos, 2 tan, 3 acos */
void tr_eval(int which, const double* x, double* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = ours(which, x[i]); }
void tr_eval_acosf(const float* x, float* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sf3d_tr_acosf(x[i]); }
void tr_eval_powf(const float* x, const float* e, float* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sf3d_tr_powf(x[i], e[i]); }

/* out[0]: the largest distance from libm in ulps, out[1]: the number of arguments that differ at all, out[2]: the argument of out[0];
 * a nan equals a nan */
void tr_compare(int which, const double* x, size_t n, double* out)
{
    int64_t worst = 0;
    size_t differ = 0;
    double at = 0;
    for (size_t i = 0; i < n; ++i) {
        const double a = ours(which, x[i]), b = libm(which, x[i]);
        if (a != a && b != b) continue;
        if (a != a || b != b) { worst = INT64_MAX; at = x[i]; ++differ; continue; }
        int64_t d = ordered(a) - ordered(b);
        if (d < 0) d = -d;
        if (d) ++differ;
        if (d > worst) { worst = d; at = x[i]; }
    }
    out[0] = (double)worst; out[1] = (double)differ; out[2] = at;
}

static int samef(float a, float b) { return (a != a && b != b) || memcmp(&a, &b, 4) == 0; }

/* number of arguments on which sf3d_tr_acosf and acosf differ; first[0] receives the first of them */
size_t tr_count_diff_acosf(const float* x, size_t n, float* first)
{
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (!samef(sf3d_tr_acosf(x[i]), acosf(x[i]))) { if (!bad) first[0] = x[i]; ++bad; }
    return bad;
}
size_t tr_count_diff_powf(const float* x, const float* e, size_t n, float* first)
{
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i)
        if (!samef(sf3d_tr_powf(x[i], e[i]), powf(x[i], e[i]))) { if (!bad) { first[0] = x[i]; first[1] = e[i]; } ++bad; }
    return bad;
}
