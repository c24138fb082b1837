/* host build of the per-cell text of k_et0_hour and k_crop_day (criteria3d_amd/csrc/sf3d_crop.inc with sf3d_glibcmath.inc: the text the
 * device compiles) for tests/test_crop_host.py and tests/test_gpu_crop.py: replays a list of operations as tests/crop_cases.py replay does
 * on a backend and writes the five maps at every checkpoint; the same program is built once with -fsanitize=address,undefined.
 *
 *   crop_host <input> <output>
 * input : int32 nCells, nUnits, nOps; float flag, clearSky; float dem[nCells]; int32 unitIndex[nCells]; CropUnitDev units[nUnits];
 *         per operation int32 code, a, b and then
 *           1 hour              float in[5][nCells] (air temperature, relative humidity, wind, global radiation, transmissivity)
 *           2 day               a = dateDoy, b = currentDoy
 *           3 set state         a = map (0 degree days, 1 LAI, 2 daily minimum, 3 daily maximum); float map[nCells]
 *           4 checkpoint        the five maps are written
 *           5 set degree days   a = currentDoy; float map[nCells] (sf3d_crop_set_degree_days: the map, then the day with dateDoy = -1)
 *           6 latitude          a = 1: the four state maps stay (ET0 starts at the flag), 0: all five start at the flag; double latitude
 * output: per checkpoint float maps[5][nCells]: degree days, LAI, daily minimum, daily maximum, ET0. */
#include "host_io.h"

#define SF3D_SNOW_HOST
#define SF3D_SNOW_FN static inline
#include "sf3d_snow.inc"
#define SF3D_CROP_HOST
#define SF3D_CROP_FN static inline
#include "sf3d_crop.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 3);
    const size_t n = (size_t)dims[0], nUnits = (size_t)dims[1], nOps = (size_t)dims[2];
    const std::vector<float> fl = readv<float>(in, 2);
    const float flag = fl[0], clearSky = fl[1];
    const std::vector<float> dem = readv<float>(in, n);
    const std::vector<int32_t> index = readv<int32_t>(in, n);
    const std::vector<CropUnitDev> units = readv<CropUnitDev>(in, nUnits);
    std::vector<float> st[4], et0(n, flag);
    for (int k = 0; k < 4; ++k) st[k].assign(n, flag);
    double latitude = 0.;
    CropView v{};
    const auto view = [&]() {
        for (int k = 0; k < 4; ++k) v.st[k] = st[k].data();
        v.et0 = et0.data(); v.dem = dem.data(); v.index = index.data(); v.units = units.data(); v.mine = nullptr;
        v.nCells = (uint32_t)n; v.nUnits = (uint32_t)nUnits; v.flag = flag; v.clearSky = clearSky; v.latitude = latitude;
    };
    const auto day = [&](int dateDoy, int currentDoy) {
        view();
        v.dateDoy = dateDoy; v.currentDoy = currentDoy;
        for (uint32_t c = 0; c < v.nCells; ++c) crop_day_cell(v, units.data(), c);
    };
    for (size_t op = 0; op < nOps; ++op) {
        const std::vector<int32_t> o = readv<int32_t>(in, 3);
        switch (o[0]) {
            case 1: {
                std::vector<float> met[5];
                for (int k = 0; k < 5; ++k) met[k] = readv<float>(in, n);
                view();
                for (int k = 0; k < 5; ++k) v.in[k] = met[k].data();
                for (uint32_t c = 0; c < v.nCells; ++c) crop_et0_cell(v, c);
                for (int k = 0; k < 5; ++k) v.in[k] = nullptr;
                break;
            }
            case 2: day(o[1], o[2]); break;
            case 3:
                if (o[1] < 0 || o[1] > 3) { fprintf(stderr, "crop_host: state map %d\n", o[1]); return 2; }
                st[o[1]] = readv<float>(in, n);
                break;
            case 4:
                for (int k = 0; k < 4; ++k) writev(out, st[k]);
                writev(out, et0);
                break;
            case 5: st[0] = readv<float>(in, n); day(-1, o[1]); break;
            case 6:
                latitude = read1<double>(in);
                if (!o[1]) for (int k = 0; k < 4; ++k) st[k].assign(n, flag);
                et0.assign(n, flag);
                break;
            default: fprintf(stderr, "crop_host: operation %d\n", o[0]); return 2;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
