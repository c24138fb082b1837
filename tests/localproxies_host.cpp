/* host build of the per-cell text of k_localdetrend_proxies (criteria3d_amd/csrc/sf3d_meteo.inc, sf3d_localdetrend.inc and
 * sf3d_localproxies.inc: the text the device compiles, here with one lane) behind the checks and the set-up of
 * sf3d_localproxies_interpolate (sf3d_localdetrend_setup.inc; a case they refuse ends the program with status 2) for
 * tests/test_localproxies_host.py: the pin is checked on a CPU before any device runs the kernel, and the same program is built once with
 * -fsanitize=address,undefined.
 *
 *   localproxies_host <input> <output>
 * input : int32 nRows, nCols, nCases; float flag; double xll, yll, cellSize; float dem[nCells]; float maps[8][nCells] (slot 0 unused:
 *         the height's values are the DEM's);
 *         per case: int32 var, method, function, nParameters, nFirstGuess, minPointsLocalDetrending, useDetrending, nStations;
 *                   int32 active[8] (slot 0: the height); float stdDevThreshold (the height's), area; float threshold[8];
 *                   double range[8][4] (min slope, min intercept, max slope, max intercept); double table[(3 + 31) * 6];
 *                   double x[nStations], y[nStations]; float proxyValues[8][nStations]; float value[nStations].
 * output: per case float map[nCells]; uint32 count[nCells], interpolated[nCells]; float radius[nCells]; int32 significant[nCells];
 *         float r2[nCells]; double parameters[nCells][6]; int32 proxySignificant[nCells][8]; double slope[nCells][8], intercept[nCells][8]. */
#include "host_io.h"
#include "sf3d_localdetrend_setup.inc"

#define SF3D_METEO_HOST
#define SF3D_METEO_FN static inline
#define SF3D_METEO_MEMBER inline
#include "sf3d_meteo.inc"
#include "sf3d_localdetrend.inc"
#include "sf3d_localproxies.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 3);
    const float flag = read1<float>(in);
    const std::vector<double> geo = readv<double>(in, 3);
    const uint32_t nRows = (uint32_t)dims[0], nCols = (uint32_t)dims[1];
    const int nCases = dims[2];
    const size_t n = (size_t)nRows * nCols;
    const int S = METEO_MAX_PROXIES;
    const std::vector<float> dem = readv<float>(in, n);
    const std::vector<float> maps = readv<float>(in, S * n);

    MeteoView v{};
    v.dem = dem.data();
    for (int p = 1; p < S; ++p) v.proxyMap[p] = maps.data() + (size_t)p * n;
    v.xll = geo[0]; v.yll = geo[1]; v.cellSize = geo[2];
    v.nCells = (uint32_t)n; v.nRows = nRows; v.nCols = nCols; v.flag = flag; v.nProxies = (uint32_t)S;

    for (int k = 0; k < nCases; ++k) {
        const std::vector<int32_t> iv = readv<int32_t>(in, 8);
        const std::vector<int32_t> active = readv<int32_t>(in, S);
        const std::vector<float> fv = readv<float>(in, 2);
        const std::vector<float> threshold = readv<float>(in, S);
        const std::vector<double> range = readv<double>(in, S * 4);
        const std::vector<double> table = readv<double>(in, LOCALDETREND_TABLE_DOUBLES);
        const uint32_t m = (uint32_t)iv[7];
        const std::vector<double> sx = readv<double>(in, m), sy = readv<double>(in, m);
        const std::vector<float> pv = readv<float>(in, (size_t)S * m), sv = readv<float>(in, m);
        if (m > METEO_MAX_STATIONS || iv[4] < 1 || iv[4] > LOCALDETREND_MAX_FIRST_GUESS) return 2;

        LocalDetrendSetup s{};
        s.table = table.data();
        s.method = iv[1]; s.useDetrending = iv[6];
        localNumbers(iv[2], iv[4], iv[5], fv[0], m, fv[1], s);

        /* the proxies of the call as the entry point takes them (slot 0 is the height), through its check and lay-out */
        sf3d_meteo_settings_t settings{};
        sf3d_localproxies_others_t others{};
        settings.nProxies = S;
        for (int p = 0; p < S; ++p) {
            settings.proxy[p].active = active[p]; settings.proxy[p].isHeight = p == 0;
            others.proxy[p].stdDevThreshold = threshold[p];
            for (int t = 0; t < 2; ++t) { others.proxy[p].min[t] = range[(size_t)p * 4 + t]; others.proxy[p].max[t] = range[(size_t)p * 4 + 2 + t]; }
        }
        LocalProxiesSetup ps{};
        const float* row[LP_MAX_OTHERS] = {nullptr};
        const float* height = nullptr;
        if (!proxiesCallOk(m, (uint32_t)S, pv.data(), &settings, &others, ps, row, &height)) { fprintf(stderr, "localproxies_host: case %d is refused\n", k); return 2; }
        std::vector<float> rows((size_t)LP_MAX_OTHERS * METEO_MAX_STATIONS, 0.f);          /* the kernel's: METEO_MAX_STATIONS a row */
        for (int r = 0; r < ps.nOthers; ++r)
            for (uint32_t i = 0; i < m; ++i) rows[(size_t)r * METEO_MAX_STATIONS + i] = row[r][i];
        const std::vector<float> sh = height ? std::vector<float>(height, height + m) : std::vector<float>(m, 0.f);      /* zeros where the height is not active */

        /* the wave's room */
        std::vector<uint16_t> idx(m + 1);
        std::vector<uint8_t> member(m + 1);
        std::vector<float> d(m + 1), val(m + 1), lanes(LD_LANES);
        std::vector<double> wt(m + 1), fit((size_t)LD_MAX_FIRST_GUESS * LD_FIT_STRIDE), work(LP_WORK_DOUBLES);
        float* h = reinterpret_cast<float*>(wt.data());                /* as in the kernel: weight[i] takes the room of the heights and weights */
        LdList L{idx.data(), d.data(), h, h + (m + 1), val.data(), wt.data(), lanes.data(), fit.data()};
        const LdStations st{sx.data(), sy.data(), sh.data(), sv.data(), m};

        std::vector<float> map(n, flag), radius(n, (float)LD_NODATA), r2(n, (float)LD_NODATA);
        std::vector<uint32_t> count(n, 0), interpolated(n, 0);
        std::vector<int32_t> significant(n, 0), proxySignificant(n * S, 0);
        std::vector<double> parameters(n * LD_MAX_PARAMETERS, (double)LD_NODATA), slope(n * S, (double)LD_NODATA), intercept(n * S, (double)LD_NODATA);
        for (uint32_t c = 0; c < n; ++c) {
            const float z = dem[c];
            if (meteo_eqf(z, flag)) continue;
            float x, y;
            meteo_cell_xy(v, c, x, y);
            LdOutcome o;
            LpOutcome po;
            LpCtx X{rows.data(), member.data(), work.data(), fit.data(), (uint32_t)ps.nOthers, 0u};
            map[c] = lp_cell(v, s, ps, st, L, X, c, z, x, y, o, po);
            count[c] = o.count; interpolated[c] = po.interpolated; radius[c] = o.radius; significant[c] = o.significant; r2[c] = o.r2;
            for (int j = 0; j < LD_MAX_PARAMETERS; ++j) parameters[(size_t)c * LD_MAX_PARAMETERS + j] = o.parameters[j];
            int j = 0;
            for (int r = 0; r < ps.nOthers; ++r) {
                if (!((po.mask >> r) & 1u)) continue;
                const size_t at = (size_t)c * S + ps.slot[r];
                proxySignificant[at] = 1; slope[at] = work[LP_P * LP_NP + j]; intercept[at] = work[LP_P * LP_NP + j + 1];
                j += 2;
            }
        }
        writev(out, map); writev(out, count); writev(out, interpolated); writev(out, radius); writev(out, significant); writev(out, r2); writev(out, parameters);
        writev(out, proxySignificant); writev(out, slope); writev(out, intercept);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
