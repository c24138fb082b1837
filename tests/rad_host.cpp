/* host build of the radiation block's point function (criteria3d_amd/csrc/sf3d_rad.inc with sf3d_trig.inc and sf3d_rad_setup.inc: the text
 * the device compiles) for tests/test_rad_point_host.py: runs rad_point over every cell of a raster for a list of hours and writes the
 * five maps after each, so that the pin is checked on a CPU before any device runs the kernel; the same program is built once with
 * -fsanitize=address,undefined.
 *
 *   rad_host <input> <output>
 * input : int32 nRows, nCols; float flag; double xll, yll, cellSize; float maps dem, lat, lon, slope, aspect; int32 nCases; per case:
 *         int32 realSky, realSkyAlgorithm, shadowing, linkeMode, albedoMode, tiltMode, timeZone, isUTC; float linke, linkeMonthly[12],
 *         albedo, tilt, aspect, clearSky; int32 year, month, day, hour, minute, second, keep; float map transmissivity.
 *         keep = 0: the five maps start at the flag (a fresh sf3d_rad_initialize); 1: they are the previous case's.
 * output: per case int32 status (0, or 1: S_solpos refuses the date) and the five maps. */
#include "host_io.h"

#define SF3D_RAD_HOST
#define SF3D_RAD_FN static inline
#define SF3D_TR_FN static inline
#define SF3D_TR_TABLE static const
#define rad_exp(x) sf3d_gl_exp(x)
#define rad_pow(x, y) sf3d_gl_pow(x, y)
#include "sf3d_rad.inc"
#include "sf3d_rad_setup.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 2);
    const float flag = read1<float>(in);
    const std::vector<double> geo = readv<double>(in, 3);
    const int nRows = dims[0], nCols = dims[1];
    const size_t n = (size_t)nRows * nCols;
    const std::vector<float> dem = readv<float>(in, n), lat = readv<float>(in, n), lon = readv<float>(in, n), slope = readv<float>(in, n), aspect = readv<float>(in, n);
    RadGridDev g{};
    g.dem = dem.data(); g.xll = geo[0]; g.yll = geo[1]; g.cellSize = geo[2]; g.invCellSize = 1.0 / geo[2];
    g.nRows = nRows; g.nCols = nCols; g.flag = flag; g.demMax = -9999.f;
    auto isFlag = [](float v, float f) { return std::fabs((double)v - (double)f) < 0.00001; };
    bool first = true;
    for (size_t c = 0; c < n; ++c)
        if (!isFlag(dem[c], flag) && !isFlag(dem[c], -9999.f)) { if (first || dem[c] > g.demMax) g.demMax = dem[c]; first = false; }
    const int nCases = read1<int32_t>(in);
    std::vector<float> maps[5];
    for (int k = 0; k < nCases; ++k) {
        const std::vector<int32_t> si = readv<int32_t>(in, 8);
        const std::vector<float> sf = readv<float>(in, 17);
        const std::vector<int32_t> when = readv<int32_t>(in, 7);
        const std::vector<float> trans = readv<float>(in, n);
        if (!when[6]) for (auto& m : maps) m.assign(n, flag);
        RadHourDev h{};
        int32_t status = radsHour(when[0], when[1], when[2], when[3], when[4], when[5], si[6], si[7] != 0, h) ? 0 : 1;
        if (!status) {
            if (si[3] == 2) h.linke = sf[1 + when[1] - 1];
            else h.linke = (si[3] == 0) ? sf[0] : -9999.f;
            h.albedo = (si[4] == 0) ? sf[13] : -9999.f;
            h.clearSky = sf[16];
            h.realSky = si[0] != 0; h.realSkyAlgorithm = si[1]; h.shadowing = si[2] != 0;
            const bool fixed = si[5] == 1;
            for (size_t c = 0; c < n; ++c) {
                if (isFlag(dem[c], flag)) continue;
                const RadCellDev cell = radsCell(dem[c], lat[c], lon[c], fixed ? sf[14] : slope[c], fixed ? sf[15] : aspect[c]);
                float o[5];
                if (!rad_point(g, h, cell, (int)(c / nCols), (int)(c % nCols), trans[c], o)) continue;
                for (int m = 0; m < 5; ++m) maps[m][c] = o[m];
            }
        }
        writev(out, std::vector<int32_t>{status});
        for (auto& m : maps) writev(out, m);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
