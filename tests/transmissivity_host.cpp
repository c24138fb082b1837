/* host build of the station transmissivity kernel's evaluation and summation text (criteria3d_amd/csrc/sf3d_transmissivity.inc over
 * sf3d_rad.inc with sf3d_trig.inc and sf3d_rad_setup.inc: the text the device compiles) for tests/test_transmissivity_host.py, so that
 * the pin is checked on a CPU before any device runs the kernel, and so that the device's evaluations can be held against the same
 * text bit for bit.  One CPU thread does what the kernel's lanes do, slot by slot, then what lane 0 does.
 *
 *   transmissivity_host <input> <output> [repeat]
 * input : int32 nRows, nCols; float flag; double xll, yll, cellSize; float map dem; int32 nCases; per case:
 *         int32 realSky, realSkyAlgorithm, shadowing, linkeMode, albedoMode, tiltMode, timeZone, isUTC; float linke, linkeMonthly[12],
 *         albedo, tilt, aspect, clearSky; int32 year, month, day, hour, minute, second, mode (0 points, 1 window), width, step, nPoints;
 *         double stations[nPoints][5] (x, y, z, lat, lon); mode 0: float measured[nPoints][width].
 * output: per case int32 status[nPoints] (0; 1: the window is refused), the results (mode 0: float[nPoints], mode 1: int32[nPoints]),
 *         uint8 written[nPoints][slots], float elevationRefr[nPoints][slots], double global[nPoints][slots]; slots = width, or 24 in mode 1.
 * repeat: evaluate every case that many times and print the seconds of all but the reading and writing (scripts/transmissivity_timing.py). */
#include <chrono>

#include "host_io.h"

#define SF3D_RAD_HOST
#define SF3D_RAD_FN static inline
#define SF3D_TR_FN static inline
#define SF3D_TR_TABLE static const
#define rad_exp(x) sf3d_gl_exp(x)
#define rad_pow(x, y) sf3d_gl_pow(x, y)
#include "sf3d_rad.inc"
#include "sf3d_rad_setup.inc"
#include "sf3d_transmissivity.inc"

struct Case {
    std::vector<int32_t> si, call;
    std::vector<float> sf, measured;
    std::vector<double> stations;
    /* results */
    std::vector<int32_t> status, steps;
    std::vector<float> result, elev;
    std::vector<uint8_t> written;
    std::vector<double> global;
};

static void hourOf(const Case& c, int hour, int minute, long offset, RadHourDev& h, uint8_t& ok)
{
    h = RadHourDev{};
    const int month = c.call[1];
    ok = radsHour(c.call[0], month, c.call[2], hour, minute, (int)offset, c.si[6], c.si[7] != 0, h) ? 1 : 0;
    if (c.si[3] == 2) h.linke = c.sf[1 + month - 1];
    else h.linke = (c.si[3] == 0) ? c.sf[0] : -9999.f;
    h.albedo = (c.si[4] == 0) ? c.sf[13] : -9999.f;
    h.clearSky = c.sf[16];
    h.realSky = c.si[0] != 0; h.realSkyAlgorithm = c.si[1]; h.shadowing = c.si[2] != 0;
}

static void run(const RadGridDev& g, Case& c)
{
    const int mode = c.call[6], width = c.call[7], step = c.call[8], nPoints = c.call[9];
    const int slots = mode == TR_MODE_WINDOW ? TR_WINDOW_SLOTS : width;
    std::vector<RadHourDev> hours((size_t)slots);
    std::vector<uint8_t> ok((size_t)slots);
    const int hh = c.call[3], mi = c.call[4], ss = c.call[5];
    if (mode == TR_MODE_WINDOW) {
        hourOf(c, 12, 0, c.si[7] ? -(long)c.si[6] * 3600 : 0, hours[0], ok[0]);
        hourOf(c, hh, mi, ss, hours[1], ok[1]);
        for (int k = 1; k <= (TR_WINDOW_SLOTS - 2) / 2; ++k) {
            hourOf(c, hh, mi, ss - (long)k * step, hours[2 * k], ok[2 * k]);
            hourOf(c, hh, mi, ss + (long)k * step, hours[2 * k + 1], ok[2 * k + 1]);
        }
    } else
        for (int i = 0; i < width; ++i) hourOf(c, hh, mi, ss + (long)(i - (width - 1) / 2) * step, hours[i], ok[i]);
    const size_t nE = (size_t)nPoints * slots;
    c.status.assign(nPoints, 0); c.steps.assign(nPoints, 0); c.result.assign(nPoints, -9999.f);
    c.written.assign(nE, 0); c.elev.assign(nE, -9999.f); c.global.assign(nE, -9999.);
    for (int p = 0; p < nPoints; ++p) {
        const double* in = &c.stations[(size_t)p * 5];
        TrPointDev pt{};
        pt.x = in[0]; pt.y = in[1]; pt.z = in[2];
        pt.cell = radsCellAt(in[2], float(in[3]), float(in[4]), 0.f, 180.f);
        const bool out = (in[0] < g.xll) || (in[1] < g.yll) || (in[0] >= (g.xll + g.nCols * g.cellSize)) || (in[1] >= (g.yll + g.nRows * g.cellSize));
        pt.inGrid = out ? 0 : 1;
        uint8_t* w = &c.written[(size_t)p * slots];
        float* e = &c.elev[(size_t)p * slots];
        double* gl = &c.global[(size_t)p * slots];
        const float* row = mode == TR_MODE_POINTS ? &c.measured[(size_t)p * width] : nullptr;
        if (mode == TR_MODE_WINDOW && (!pt.cell.ok || !ok[0])) { c.status[p] = 1; continue; }
        const bool go = mode == TR_MODE_WINDOW || tr_point_go(row, width);
        for (int s = 0; s < slots; ++s) {           /* a lane per slot */
            if (!go || (mode == TR_MODE_POINTS && s != (width - 1) / 2 && tr_eq(row[s], TR_NODATA_F))) continue;
            bool written;
            tr_evaluate(g, hours[s], ok[s] != 0, pt, written, e[s], gl[s]);
            w[s] = written ? 1 : 0;
        }
        if (mode == TR_MODE_POINTS) c.result[p] = go ? tr_sum_points(row, w, gl, width, c.sf[16]) : TR_NODATA_F;
        else c.steps[p] = tr_scan_window(w, e, gl);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    const std::vector<int32_t> dims = readv<int32_t>(in, 2);
    const float flag = read1<float>(in);
    const std::vector<double> geo = readv<double>(in, 3);
    const size_t n = (size_t)dims[0] * dims[1];
    const std::vector<float> dem = readv<float>(in, n);
    RadGridDev g{};
    g.dem = dem.data(); g.xll = geo[0]; g.yll = geo[1]; g.cellSize = geo[2]; g.invCellSize = 1.0 / geo[2];
    g.nRows = dims[0]; g.nCols = dims[1]; g.flag = flag; g.demMax = -9999.f;
    auto isFlag = [](float v, float f) { return std::fabs((double)v - (double)f) < 0.00001; };
    bool first = true;
    for (size_t c = 0; c < n; ++c)
        if (!isFlag(dem[c], flag) && !isFlag(dem[c], -9999.f)) { if (first || dem[c] > g.demMax) g.demMax = dem[c]; first = false; }
    const int nCases = read1<int32_t>(in);
    std::vector<Case> cases((size_t)nCases);
    for (Case& c : cases) {
        c.si = readv<int32_t>(in, 8);
        c.sf = readv<float>(in, 17);
        c.call = readv<int32_t>(in, 10);
        const int mode = c.call[6], width = c.call[7], nPoints = c.call[9];
        if (nPoints < 0 || (mode == TR_MODE_POINTS && (width < 1 || width > TR_MAX_WIDTH || width % 2 != 1))) return 2;
        c.stations = readv<double>(in, (size_t)nPoints * 5);
        if (mode == TR_MODE_POINTS) c.measured = readv<float>(in, (size_t)nPoints * width);
    }
    fclose(in);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < repeat; ++r)
        for (Case& c : cases) run(g, c);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (argc > 3) printf("%.9f\n", seconds);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (const Case& c : cases) {
        writev(out, c.status);
        if (c.call[6] == TR_MODE_POINTS) writev(out, c.result);
        else writev(out, c.steps);
        writev(out, c.written); writev(out, c.elev); writev(out, c.global);
    }
    return fclose(out) == 0 ? 0 : 3;
}
