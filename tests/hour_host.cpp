/* host build of the per-cell text of k_hour_relhum and k_hour_pond (criteria3d_amd/csrc/sf3d_hour.inc with sf3d_glibcmath.inc: the text the
 * device compiles) for tests/test_hour_host.py: the pins are checked on a CPU before any device runs the kernels, and the same program is
 * built once with -fsanitize=address,undefined.
 *
 *   hour_host <input> <output>
 * input : int32 nPairs, nCells; float flag; float dewT[nPairs], airT[nPairs]; float mapAirT[nCells], mapDewT[nCells];
 *         int32 nPond, nUnits, computeCrop; float slopeFlag, laiFlag; float slopeDegree[nPond]; int32 unit[nPond]; float lai[nPond];
 *         per unit double maximumPond, laiMax; int32 isCrop[nUnits].
 * output: float relHum[nPairs] (relHumFromTdew), float map[nCells] (the map loop's rule), float pond[nPond] (-9999: skipped). */
#include "host_io.h"

#define SF3D_HOUR_HOST
#define SF3D_HOUR_FN static inline
#define hour_exp(x) sf3d_gl_exp(x)
#define hour_pow(x, y) sf3d_gl_pow(x, y)
#include "sf3d_hour.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 2);
    const float flag = read1<float>(in);
    const size_t nPairs = (size_t)dims[0], nCells = (size_t)dims[1];
    const std::vector<float> dewT = readv<float>(in, nPairs), airT = readv<float>(in, nPairs), mapAirT = readv<float>(in, nCells), mapDewT = readv<float>(in, nCells);
    std::vector<float> rh(nPairs), map(nCells);
    for (size_t k = 0; k < nPairs; ++k) rh[k] = hour_relhum_from_tdew(dewT[k], airT[k]);
    for (size_t c = 0; c < nCells; ++c) map[c] = hour_relhum_cell(mapAirT[c], mapDewT[c], flag);

    const std::vector<int32_t> pd = readv<int32_t>(in, 3);
    const std::vector<float> pf = readv<float>(in, 2);
    const size_t nPond = (size_t)pd[0], nUnits = (size_t)pd[1];
    const bool computeCrop = pd[2] != 0;
    const float slopeFlag = pf[0], laiFlag = pf[1];
    const std::vector<float> slope = readv<float>(in, nPond);
    const std::vector<int32_t> unit = readv<int32_t>(in, nPond);
    const std::vector<float> lai = readv<float>(in, nPond);
    const std::vector<double> table = readv<double>(in, 2 * nUnits);
    const std::vector<int32_t> isCrop = readv<int32_t>(in, nUnits);
    std::vector<float> pond(nPond, HOUR_NODATA);
    for (size_t c = 0; c < nPond; ++c) {
        const int32_t u = unit[c];
        if (hour_eqf(slope[c], slopeFlag) || u < 0 || (size_t)u >= nUnits) continue;          /* what sf3d_hour_set_ponds marks with unit -1 */
        const double tanSlope = std::tan(slope[c] * 0.01745329252);                           /* the host's, as in sf3d_hour_api.inc */
        pond[c] = hour_pond_cell(tanSlope, table[2 * (size_t)u], table[2 * (size_t)u + 1], computeCrop && isCrop[u], lai[c], laiFlag);
    }
    writev(out, rh); writev(out, map); writev(out, pond);
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
