/* host build of the per-area and per-cell text of k_glocal_areas and k_glocal_cells (criteria3d_amd/csrc/sf3d_meteo.inc,
 * sf3d_localdetrend.inc, sf3d_localproxies.inc and sf3d_glocal.inc: the text the device compiles, here with one lane) behind the checks and
 * the set-up of sf3d_glocal_set_areas and sf3d_glocal_interpolate (sf3d_localdetrend_setup.inc, sf3d_glocal_setup.inc) for
 * tests/test_glocal_host.py: the pin is checked on a CPU before any device runs the kernels, every refusal of the two entry points is
 * exercised here, and the same program is built once with -fsanitize=address,undefined.
 *
 *   glocal_host <input> <output>
 *   glocal_host shape <rows> <cols>     status 0: sf3d_glocal_set_areas takes one area of one cell on a raster of that shape, 1: it refuses
 * input : int32 nRows, nCols, nCases; float flag; double xll, yll, cellSize; float dem[nCells]; float maps[8][nCells] (slot 0 unused:
 *         the height's values are the DEM's);
 *         int32 nAreas (-1: sf3d_glocal_set_areas was never called, the two counts are 0 and no array follows), nAreaCells, nList;
 *         uint32 cellOffset[nAreas + 1]; float cell[nAreaCells], weight[nAreaCells];
 *         uint32 stationOffset[nAreas + 1]; int32 stationIndex[nList];
 *         per case: int32 var, method, function, nParameters, nFirstGuess, minPointsLocalDetrending, useDetrending, nStations;
 *                   int32 useMultipleDetrending, useLocalDetrending, nProxies; int32 active[8] (slot 0: the height);
 *                   float stdDevThreshold (the height's), area; float threshold[8]; double range[8][4]; double table[(3 + 31) * 6];
 *                   int32 pointIndex[nStations]; double x[nStations], y[nStations]; float proxyValues[8][nStations]; float value[nStations].
 * output: int32 areasOk (0: sf3d_glocal_set_areas refuses them, nothing follows; 1 also where it was never called: every case is then refused);
 *         per case int32 status (0: a map; 1: an interpolate() gave NODATA; 2: sf3d_glocal_interpolate refuses the call, nothing follows
 *         of the case); float map[nCells]; int32 significant[nAreas]; float r2[nAreas]; double parameters[nAreas][6];
 *         int32 proxySignificant[nAreas][8]; double slope[nAreas][8], intercept[nAreas][8]; uint32 fitted[nAreas], kept[nAreas];
 *         float detrended[nList]; int32 stationKept[nList]. */
#include <string>

#include "host_io.h"
#include "sf3d_localdetrend_setup.inc"
#include "sf3d_glocal_setup.inc"

#define SF3D_METEO_HOST
#define SF3D_METEO_FN static inline
#define SF3D_METEO_MEMBER inline
#include "sf3d_meteo.inc"
#include "sf3d_localdetrend.inc"
#include "sf3d_localproxies.inc"
#include "sf3d_glocal.inc"

int main(int argc, char** argv)
{
    if (argc == 4 && std::string(argv[1]) == "shape") {
        const uint32_t offset[2] = {0, 1}, none[2] = {0, 0};
        const float cell = 0.f, weight = 1.f;
        GlocalAreasHost A;
        return glocalAreasOk((uint32_t)atol(argv[2]), (uint32_t)atol(argv[3]), 1, offset, &cell, &weight, none, nullptr, A) ? 0 : 1;
    }
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
    const std::vector<int32_t> adims = readv<int32_t>(in, 3);
    const bool areasSet = adims[0] >= 0;
    const uint32_t nAreas = areasSet ? (uint32_t)adims[0] : 0u, nAreaCells = (uint32_t)adims[1], nList = (uint32_t)adims[2];
    const std::vector<uint32_t> cellOffset = readv<uint32_t>(in, areasSet ? (size_t)nAreas + 1 : 0);
    const std::vector<float> cell = readv<float>(in, nAreaCells), weight = readv<float>(in, nAreaCells);
    const std::vector<uint32_t> stationOffset = readv<uint32_t>(in, areasSet ? (size_t)nAreas + 1 : 0);
    const std::vector<int32_t> stationIndex = readv<int32_t>(in, nList);

    GlocalAreasHost A;
    const bool areasOk = !areasSet || glocalAreasOk(nRows, nCols, nAreas, cellOffset.data(), cell.data(), weight.data(), stationOffset.data(), stationIndex.data(), A);
    writev(out, std::vector<int32_t>{areasOk ? 1 : 0});
    if (!areasOk) { fclose(in); return fclose(out) == 0 ? 0 : 3; }

    GlocalCellsView cv{};
    MeteoView& v = cv.m;
    v.dem = dem.data();
    for (int p = 1; p < S; ++p) v.proxyMap[p] = maps.data() + (size_t)p * n;
    v.xll = geo[0]; v.yll = geo[1]; v.cellSize = geo[2];
    v.nCells = (uint32_t)n; v.nRows = nRows; v.nCols = nCols; v.flag = flag; v.nProxies = (uint32_t)S;

    for (int k = 0; k < nCases; ++k) {
        const std::vector<int32_t> iv = readv<int32_t>(in, 8);
        const std::vector<int32_t> options = readv<int32_t>(in, 3);
        const std::vector<int32_t> active = readv<int32_t>(in, S);
        const std::vector<float> fv = readv<float>(in, 2);
        const std::vector<float> threshold = readv<float>(in, S);
        const std::vector<double> range = readv<double>(in, S * 4);
        const std::vector<double> table = readv<double>(in, LOCALDETREND_TABLE_DOUBLES);
        const uint32_t m = (uint32_t)iv[7];
        const std::vector<int32_t> pointIndex = readv<int32_t>(in, m);
        const std::vector<double> sx = readv<double>(in, m), sy = readv<double>(in, m);
        const std::vector<float> pv = readv<float>(in, (size_t)S * m), sv = readv<float>(in, m);

        /* the call as the entry point takes it (slot 0 is the height), through its checks and lay-out */
        sf3d_meteo_settings_t settings{};
        sf3d_localproxies_others_t others{};
        sf3d_localdetrend_fit_t fit{};
        settings.nProxies = options[2]; settings.useMultipleDetrending = options[0]; settings.useLocalDetrending = options[1]; settings.useDetrending = iv[6];
        for (int p = 0; p < S; ++p) {
            settings.proxy[p].active = active[p]; settings.proxy[p].isHeight = p == 0;
            others.proxy[p].stdDevThreshold = threshold[p];
            for (int t = 0; t < 2; ++t) { others.proxy[p].min[t] = range[(size_t)p * 4 + t]; others.proxy[p].max[t] = range[(size_t)p * 4 + 2 + t]; }
        }
        fit.function = iv[2]; fit.nParameters = iv[3]; fit.nFirstGuess = iv[4]; fit.minPointsLocalDetrending = iv[5]; fit.stdDevThreshold = fv[0];
        const int P = SF3D_LOCALDETREND_MAX_PARAMETERS;
        for (int j = 0; j < P; ++j) {
            fit.parametersMin[j] = table[j]; fit.parametersMax[j] = table[P + j]; fit.parametersDelta[j] = table[2 * P + j];
            for (int g = 0; g < SF3D_LOCALDETREND_MAX_FIRST_GUESS; ++g) fit.firstGuess[g][j] = table[(size_t)(3 + g) * P + j];
        }
        static const float noHeight[SF3D_METEO_MAX_STATIONS] = {0.f};
        LocalProxiesSetup ps{};
        const float* row[LP_MAX_OTHERS] = {nullptr};
        const float* height = nullptr;
        std::vector<int32_t> listPoint;
        const bool ok = iv[1] >= METEO_IDW && iv[1] <= METEO_SHEPARD_MODIFIED && localCallOk(iv[0], m, sx.data(), sy.data(), noHeight, &settings, &fit, false, false) &&
                        proxiesCallOk(m, (uint32_t)S, pv.data(), &settings, &others, ps, row, &height) && glocalCallOk(A, m, pointIndex.data(), listPoint);
        if (!ok) { writev(out, std::vector<int32_t>{2}); continue; }
        std::vector<double> own(LOCALDETREND_TABLE_DOUBLES, 0.);
        LocalDetrendSetup s{};
        glocalSetup(&fit, m, fv[1], own.data(), s);
        s.table = own.data();
        s.method = iv[1]; s.useDetrending = iv[6];
        std::vector<float> rows((size_t)LP_MAX_OTHERS * METEO_MAX_STATIONS, 0.f);          /* the kernel's: METEO_MAX_STATIONS a row */
        for (int r = 0; r < ps.nOthers; ++r)
            for (uint32_t i = 0; i < m; ++i) rows[(size_t)r * METEO_MAX_STATIONS + i] = row[r][i];
        const std::vector<float> sh = height ? std::vector<float>(height, height + m) : std::vector<float>(m, 0.f);

        /* what k_glocal_areas writes */
        std::vector<GlocalAreaDev> area(nAreas);
        std::vector<float> detrended(nList, 0.f), keptValue(nList, 0.f);
        std::vector<uint16_t> keptPoint(nList, 0);
        std::vector<uint8_t> keptBit(nList, 0);
        GlocalAreasView av{};
        av.s = s; av.p = ps;
        av.stationOffset = A.stationOffset.data(); av.listPoint = listPoint.data();
        av.sv = sv.data(); av.sh = sh.data(); av.rows = rows.data();
        av.area = area.data(); av.detrended = detrended.data(); av.keptBit = keptBit.data(); av.keptPoint = keptPoint.data(); av.keptValue = keptValue.data();
        av.nAreas = nAreas;
        for (uint32_t a = 0; a < nAreas; ++a) {
            /* the wave's room: the area's list and no more */
            const size_t room = (size_t)(A.stationOffset[a + 1] - A.stationOffset[a]) + 1;
            std::vector<uint16_t> idx(room);
            std::vector<uint8_t> member(room);
            std::vector<float> d(room), val(room);
            std::vector<double> wt(room), fitRoom((size_t)LD_MAX_FIRST_GUESS * LD_FIT_STRIDE), work(LP_WORK_DOUBLES);
            float* h = reinterpret_cast<float*>(wt.data());
            LdList L{idx.data(), d.data(), h, h + room, val.data(), wt.data(), nullptr, fitRoom.data()};
            LpCtx X{rows.data(), member.data(), work.data(), fitRoom.data(), (uint32_t)ps.nOthers, 0u};
            gl_area(av, a, L, X);
        }

        /* k_glocal_cells */
        uint32_t failed = 0;
        v.sx = sx.data(); v.sy = sy.data(); v.sv = sv.data(); v.nStations = m;
        cv.s = s; cv.p = ps;
        cv.pairOffset = A.pairOffset.data(); cv.pairArea = A.pairArea.data(); cv.pairWeight = A.pairWeight.data();
        cv.stationOffset = A.stationOffset.data(); cv.area = area.data(); cv.keptPoint = keptPoint.data(); cv.keptValue = keptValue.data();
        cv.failed = &failed; cv.nPairs = (uint32_t)A.pairArea.size();
        std::vector<float> map(n, flag);
        for (uint32_t c = 0; c < n; ++c) {
            const float z = dem[c];
            if (meteo_eqf(z, flag)) continue;
            float x, y;
            meteo_cell_xy(v, c, x, y);
            map[c] = gl_cell(cv, c, z, x, y, flag);
        }

        std::vector<int32_t> significant(nAreas), psig((size_t)nAreas * S, 0), stationKept(keptBit.begin(), keptBit.end());
        std::vector<float> r2(nAreas);
        std::vector<uint32_t> fitted(nAreas), kept(nAreas);
        std::vector<double> parameters((size_t)nAreas * P), slope((size_t)nAreas * S, (double)LD_NODATA), intercept((size_t)nAreas * S, (double)LD_NODATA);
        for (uint32_t a = 0; a < nAreas; ++a) {
            const GlocalAreaDev& o = area[a];
            significant[a] = o.significant; r2[a] = o.r2; fitted[a] = o.fitted; kept[a] = o.kept;
            for (int j = 0; j < P; ++j) parameters[(size_t)a * P + j] = o.parameters[j];
            int j = 0;
            for (int r = 0; r < ps.nOthers; ++r) {
                if (!((o.mask >> r) & 1u)) continue;
                const size_t at = (size_t)a * S + ps.slot[r];
                psig[at] = 1; slope[at] = o.line[j][0]; intercept[at] = o.line[j][1];
                ++j;
            }
        }
        writev(out, std::vector<int32_t>{failed ? 1 : 0});
        writev(out, map); writev(out, significant); writev(out, r2); writev(out, parameters); writev(out, psig); writev(out, slope); writev(out, intercept);
        writev(out, fitted); writev(out, kept); writev(out, detrended); writev(out, stationKept);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
