/* host build of the per-cell text of k_snow_hour (criteria3d_amd/csrc/sf3d_snow.inc with sf3d_glibcmath.inc: the text the device compiles)
 * for tests/test_snow_host.py and tests/test_gpu_snow.py: loops snow_cell over a raster for a list of hours, the state carried from hour
 * to hour, so that the pin is checked on a CPU before any device runs the kernel; the same program is built once with
 * -fsanitize=address,undefined.
 *
 *   snow_host <input> <output>
 * input : int32 nCells, nHours; float flag; double parameters[7] (SnowParamsDev without clearSky); float dem[nCells]; float state[7][nCells];
 *         per hour: double clearSky; int32 hasSurfaceWater; float in[7][nCells] (air temperature, precipitation, relative humidity, wind,
 *         global radiation, beam radiation, transmissivity); float surfaceWater[nCells] if hasSurfaceWater.
 * output: per hour float maps[13][nCells]: the seven state maps, then the six outputs. */
#include "host_io.h"

#define SF3D_SNOW_HOST
#define SF3D_SNOW_FN static inline
#include "sf3d_snow.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 2);
    const size_t n = (size_t)dims[0], nHours = (size_t)dims[1];
    const float flag = read1<float>(in);
    const std::vector<double> par = readv<double>(in, 7);
    const std::vector<float> dem = readv<float>(in, n);
    std::vector<float> st[7], o[6];
    for (int k = 0; k < 7; ++k) st[k] = readv<float>(in, n);
    for (int k = 0; k < 6; ++k) o[k].assign(n, flag);
    for (size_t h = 0; h < nHours; ++h) {
        const double clearSky = read1<double>(in);
        const bool water = read1<int32_t>(in) != 0;
        std::vector<float> met[8];
        for (int k = 0; k < 7 + (water ? 1 : 0); ++k) met[k] = readv<float>(in, n);
        SnowView v{};
        for (int k = 0; k < 7; ++k) v.st[k] = st[k].data();
        for (int k = 0; k < 6; ++k) v.out[k] = o[k].data();
        for (int k = 0; k < 7; ++k) v.in[k] = met[k].data();
        v.in[7] = water ? met[7].data() : nullptr;
        v.dem = dem.data(); v.mine = nullptr; v.nCells = (uint32_t)n; v.flag = flag;
        v.p = SnowParamsDev{par[0], par[1], par[2], par[3], par[4], par[5], par[6], clearSky};
        for (uint32_t c = 0; c < v.nCells; ++c) snow_cell(v, c);
        for (int k = 0; k < 7; ++k) writev(out, st[k]);
        for (int k = 0; k < 6; ++k) writev(out, o[k]);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
