/* shared by every host program that reads an input file (tests/<block>_host.cpp for snow, crop, root, sink, rad, transmissivity, hour,
 * topodist, localdetrend and localproxies): binary input and output, and the elementary functions of the kernels' text on a CPU.
 *
 * Every array a program hands to the kernels' text is a std::vector of exactly the size the text may index (one heap block per map or
 * table), so that the address sanitizer sees a read one element past its end. */
#ifndef SF3D_TESTS_HOST_IO_H
#define SF3D_TESTS_HOST_IO_H
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sf3d_device.h"

#define SF3D_GL_FN static inline
#define SF3D_GL_TABLE static const
#include "sf3d_glibcmath.inc"

/* what sf3d_physics.inc gives the device: std::max / std::min semantics, the C library's exp / log / pow; no tables to stage */
static inline double dmax(double a, double b) { return (a < b) ? b : a; }
static inline double dmin(double a, double b) { return (b < a) ? b : a; }
static inline double flog(double x) { return sf3d_gl_log(x); }
static inline double fexp(double x) { return sf3d_gl_exp(x); }
static inline double ppow(double x, double y) { return sf3d_gl_pow(x, y); }

template <class T> static std::vector<T> readv(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "host program: short input\n"); exit(2); }
    return v;
}

template <class T> static T read1(FILE* f) { return readv<T>(f, 1)[0]; }

template <class T> static void writev(FILE* f, const std::vector<T>& v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "host program: short output\n"); exit(3); }
}

#endif
