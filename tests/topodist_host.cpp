/* host build of the per-cell text of k_topodist_maps, k_meteo_idw_td and k_topodist_matrix (criteria3d_amd/csrc/sf3d_meteo.inc and
 * sf3d_topodist.inc: the text the device compiles) for tests/test_topodist_host.py: the pin is checked on a CPU before any device runs
 * the kernels, and the same program is built once with -fsanitize=address,undefined.
 *
 *   topodist_host <input> <output>
 * input : int32 nRows, nCols, nStations, nCases, nMatrices, hand; float flag; double xll, yll, cellSize; float dem[nCells];
 *         double x[nStations], y[nStations], z[nStations]; float handMap[nCells];
 *         per case: int32 var, method, kh (0 where the distances are plain), useHand, heightActive, useDetrending; float rainfallThreshold,
 *                   radius0, slope; int32 mapIndex[nStations]; float value[nStations];
 *         per matrix: int32 useHand; int32 mapIndex[nStations].
 * output: float maps[nStations][nCells]; float caseMap[nCases][nCells]; float matrix[nMatrices][nStations][nStations].
 * useHand: map `hand` is handMap in the place of the computed one. */
#include "host_io.h"

#define SF3D_METEO_HOST
#define SF3D_METEO_FN static inline
#define SF3D_METEO_MEMBER inline
#include "sf3d_meteo.inc"
#include "sf3d_topodist.inc"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 6);
    const float flag = read1<float>(in);
    const std::vector<double> geo = readv<double>(in, 3);
    const uint32_t nRows = (uint32_t)dims[0], nCols = (uint32_t)dims[1], m = (uint32_t)dims[2];
    const int nCases = dims[3], nMatrices = dims[4], hand = dims[5];
    const size_t n = (size_t)nRows * nCols;
    const std::vector<float> dem = readv<float>(in, n);
    const std::vector<double> sx = readv<double>(in, m), sy = readv<double>(in, m), sz = readv<double>(in, m);
    const std::vector<float> handMap = readv<float>(in, n);

    TopoGridDev g{};
    g.dem = dem.data(); g.xll = geo[0]; g.yll = geo[1]; g.cellSize = geo[2]; g.invCellSize = 1.0 / geo[2];
    g.nRows = (int32_t)nRows; g.nCols = (int32_t)nCols; g.flag = flag;

    /* k_topodist_maps */
    std::vector<float> maps((size_t)m * n, flag);
    for (uint32_t p = 0; p < m; ++p)
        for (uint32_t c = 0; c < n; ++c)
            if (!meteo_eqf(dem[c], flag)) maps[(size_t)p * n + c] = topo_map_cell(g, c, dem[c], sx[p], sy[p], sz[p]);
    writev(out, maps);
    std::vector<float> withHand = maps;
    if (hand >= 0 && (uint32_t)hand < m) for (size_t c = 0; c < n; ++c) withHand[(size_t)hand * n + c] = handMap[c];

    std::vector<float> szf(m);
    for (uint32_t i = 0; i < m; ++i) szf[i] = (float)sz[i];

    /* k_meteo_idw_td */
    for (int k = 0; k < nCases; ++k) {
        const std::vector<int32_t> iv = readv<int32_t>(in, 6);
        const std::vector<float> fv = readv<float>(in, 3);
        const std::vector<int32_t> mapIndex = readv<int32_t>(in, m);
        const std::vector<float> value = readv<float>(in, m);
        MeteoView v{};
        v.dem = dem.data();
        v.xll = geo[0]; v.yll = geo[1]; v.cellSize = geo[2];
        v.nCells = (uint32_t)n; v.nRows = nRows; v.nCols = nCols; v.nStations = m; v.nProxies = 1;
        v.var = iv[0]; v.method = iv[1]; v.allZero = 0; v.useDetrending = iv[5];
        v.detrendingVar = (iv[0] == METEO_AIR_TEMPERATURE || iv[0] == METEO_AIR_DEW_TEMPERATURE) ? 1 : 0;
        v.flag = flag; v.rainfallThreshold = fv[0]; v.radius0 = fv[1];
        v.proxy[0].active = iv[4]; v.proxy[0].isHeight = 1; v.proxy[0].inversion = 0; v.proxy[0].slope = fv[2];
        std::vector<float> map(n, flag);
        for (uint32_t c = 0; c < n; ++c) {
            const float z = dem[c];
            if (meteo_eqf(z, flag)) continue;
            float x, y;
            meteo_cell_xy(v, c, x, y);
            TopoDistance dist;
            dist.g = g;
            dist.sx = sx.data(); dist.sy = sy.data(); dist.sz = szf.data(); dist.mapIndex = mapIndex.data();
            dist.maps = iv[3] ? withHand.data() : maps.data(); dist.nCells = n;
            dist.x = x; dist.y = y; dist.z = z; dist.kh = iv[2];
            map[c] = meteo_cell(v, c, z, x, y, dist, sx.data(), sy.data(), value.data(), m);
        }
        writev(out, map);
    }

    /* k_topodist_matrix */
    for (int k = 0; k < nMatrices; ++k) {
        const int32_t useHand = read1<int32_t>(in);
        const std::vector<int32_t> mapIndex = readv<int32_t>(in, m);
        const float* held = useHand ? withHand.data() : maps.data();
        std::vector<float> matrix((size_t)m * m);
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t i = 0; i < m; ++i) matrix[(size_t)j * m + i] = topo_matrix_entry(g, held, n, sx.data(), sy.data(), sz.data(), mapIndex.data(), j, i);
        writev(out, matrix);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
