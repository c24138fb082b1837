/* host build of the per-cell text of k_sink_hour and k_sink_hour_crack (criteria3d_amd/csrc/sf3d_sink.inc with map_theta / map_sentinel of
 * sf3d_maps.inc and sf3d_glibcmath.inc: the text the device compiles) behind the table builders of sf3d_sink_initialize and
 * sf3d_sink_set_cracking (sf3d_sink_setup.inc) for tests/test_sink_host.py, tests/test_crack_host.py, tests/test_gpu_sink.py and
 * tests/test_gpu_crack.py: sink_cell<false> over the raster and, with crack soils, sink_cell<true> on node sinks of its own.
 * Every table is a heap block of its own of exactly the size DeviceSolver::sink_alloc, sink_hour and root_alloc give it (the product packs
 * them into one device block, where a read past a table's end lands in the next table), the per-cell blocks of the sink and the root maps
 * are SINK_MAP_WORDS and ROOT_MAP_WORDS words per cell as on the device, and the unit table has nUnits entries.  The same program is built
 * once with -fsanitize=address,undefined.
 *
 *   sink_host <input> <output>
 * input : int32 nCells, nrLayers, nUnits, nSoils, nNodes, nSurface, nClasses, rootRows, crack; float flag; double cellSize, computationSoilDepth;
 *         float dem[nCells]; int32 cropIndex[nCells], soilIndex[nCells]; double layerDepth[nrLayers], layerThickness[nrLayers];
 *         sf3d_sink_unit_t units[nUnits]; sf3d_sink_soil_t soils[nSoils]; int32 columns[nrLayers][nCells];
 *         double H[nNodes], z[nNodes], Se[nNodes]; uint16 soilClass[nNodes]; double thetaS[nClasses], thetaR[nClasses];
 *         float et0[nCells], lai[nCells], degreeDays[nCells], liquidWater[nCells];
 *         the root program's outputs: double length[nCells]; int32 first[nCells], last[nCells], key[nCells]; double table[nrLayers][rootRows];
 *         if crack: sf3d_sink_crack_soil_t crackSoils[nSoils]; double pond[nNodes] [m].
 * output: int32 status (what sinkBuildTables returns; not 0: nothing follows), lastEvapLayer; double sinks[nNodes], evaporation[nCells],
 *         transpiration[nCells]; if crack: double maxDepth[nSoils]; int32 lastLayer[nSoils]; double sinks[nNodes], evaporation[nCells],
 *         transpiration[nCells]; float precSurfaceWater[nCells]; double crackWater[nCells]. */
#include <cstring>

#include "host_io.h"
#include "sf3d_sink_setup.inc"

#define SF3D_SNOW_HOST
#define SF3D_SNOW_FN static inline
#include "sf3d_snow.inc"
#define SF3D_MAPS_HOST
#define SF3D_MAPS_FN static inline
#include "sf3d_maps.inc"
#define SF3D_SINK_HOST
#define SF3D_SINK_FN static inline
#include "sf3d_sink.inc"

/* a map of a per-cell block whose first two maps are 8-byte maps and the others 4-byte ones (raster_cell_map of sf3d_maps.inc) */
static char* cell_map(std::vector<char>& cells, size_t nCells, int map)
{
    return (map < 2) ? cells.data() + (size_t)map * nCells * 8 : cells.data() + 16 * nCells + (size_t)(map - 2) * nCells * 4;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 9);
    const size_t n = (size_t)dims[0], nl = (size_t)dims[1], nUnits = (size_t)dims[2], nSoils = (size_t)dims[3], N = (size_t)dims[4], ns = (size_t)dims[5];
    const size_t nClasses = (size_t)dims[6], rootRows = (size_t)dims[7];
    const bool crack = dims[8] != 0;
    const float flag = read1<float>(in);
    const std::vector<double> scalars = readv<double>(in, 2);
    const double cellSize = scalars[0], computationSoilDepth = scalars[1];
    const std::vector<float> dem = readv<float>(in, n);
    const std::vector<int32_t> cropIndex = readv<int32_t>(in, n), soilIndex = readv<int32_t>(in, n);
    const std::vector<double> layerDepth = readv<double>(in, nl), layerThickness = readv<double>(in, nl);
    const std::vector<sf3d_sink_unit_t> units = readv<sf3d_sink_unit_t>(in, nUnits);
    const std::vector<sf3d_sink_soil_t> soils = readv<sf3d_sink_soil_t>(in, nSoils);
    const std::vector<int32_t> col = readv<int32_t>(in, nl * n);
    const std::vector<double> H = readv<double>(in, N), z = readv<double>(in, N), Se = readv<double>(in, N);
    const std::vector<uint16_t> cls = readv<uint16_t>(in, N);
    const std::vector<double> thetaS = readv<double>(in, nClasses), thetaR = readv<double>(in, nClasses);
    std::vector<SoilDev> classes(nClasses);
    for (size_t k = 0; k < nClasses; ++k) { std::memset(&classes[k], 0, sizeof(SoilDev)); classes[k].thetaS = thetaS[k]; classes[k].thetaR = thetaR[k]; }
    const std::vector<float> et0 = readv<float>(in, n), lai = readv<float>(in, n), dd = readv<float>(in, n), liquid = readv<float>(in, n);
    const std::vector<double> length = readv<double>(in, n);
    const std::vector<int32_t> first = readv<int32_t>(in, n), last = readv<int32_t>(in, n), key = readv<int32_t>(in, n);
    const std::vector<double> rootTable = readv<double>(in, nl * rootRows);

    SinkTablesHost T;
    const int32_t status = (int32_t)sinkBuildTables((uint32_t)nl, layerDepth.data(), layerThickness.data(), computationSoilDepth, (uint32_t)nUnits, units.data(),
                                                    (uint32_t)nSoils, soils.data(), T);
    const std::vector<int32_t> head = {status, status == 0 ? T.lastEvapLayer : 0};
    writev(out, head);
    if (status != 0) { fclose(in); return fclose(out) == 0 ? 0 : 3; }

    /* the per-cell blocks: the sink block's (sink_alloc: DEM, crop and soil index; both actual maps at the flag) and the root block's */
    std::vector<char> cells((size_t)SINK_MAP_WORDS * n * 4), rootCells((size_t)ROOT_MAP_WORDS * n * 4);
    std::vector<int32_t> ci(n), si(n);
    for (size_t c = 0; c < n; ++c) { ci[c] = cropIndex[c] < 0 ? -1 : cropIndex[c]; si[c] = soilIndex[c] < 0 ? -1 : soilIndex[c]; }      /* sf3d_sink_initialize */
    if (n) {
        std::memcpy(cell_map(cells, n, SINK_MAP_DEM), dem.data(), n * 4);
        std::memcpy(cell_map(cells, n, SINK_MAP_CROP), ci.data(), n * 4);
        std::memcpy(cell_map(cells, n, SINK_MAP_SOIL), si.data(), n * 4);
        std::memcpy(cell_map(rootCells, n, ROOT_MAP_LENGTH), length.data(), n * 8);
        std::memcpy(cell_map(rootCells, n, ROOT_MAP_FIRST), first.data(), n * 4);
        std::memcpy(cell_map(rootCells, n, ROOT_MAP_LAST), last.data(), n * 4);
        std::memcpy(cell_map(rootCells, n, ROOT_MAP_KEY), key.data(), n * 4);
    }
    /* the three layer tables are adjacent in the device block: thickness, evapCoeff, layerEvapCoeff */
    std::vector<double> layerTables(3 * nl);
    for (size_t l = 0; l < nl; ++l) { layerTables[l] = layerThickness[l]; layerTables[nl + l] = T.evapCoeff[l]; layerTables[2 * nl + l] = T.layerEvapCoeff[l]; }

    std::vector<double> sink(N, 0.);
    SinkView v{};
    v.col = col.data(); v.H = H.data(); v.Se = Se.data(); v.z = z.data(); v.cls = cls.data(); v.soils = classes.data();
    v.cells = cells.data(); v.et0 = et0.data(); v.lai = lai.data(); v.dd = dd.data(); v.liquid = liquid.data();
    v.rootCells = rootCells.data(); v.rootTable = rootTable.data(); v.units = T.units.data(); v.horizon = T.horizon.data();
    v.horizonValues = T.horizonValues.data(); v.layerTables = layerTables.data(); v.sink = sink.data(); v.mine = nullptr;
    v.area = cellSize * cellSize;
    v.ns = (uint32_t)ns; v.nCells = (uint32_t)n; v.nrLayers = (uint32_t)nl; v.nUnits = (uint32_t)nUnits; v.nSoils = (uint32_t)nSoils; v.rootRows = (uint32_t)rootRows;
    v.lastEvapLayer = T.lastEvapLayer; v.flag = flag;
    const auto write_actual = [&]() {
        writev(out, sink);
        const double* actual = reinterpret_cast<const double*>(cells.data());
        writev(out, std::vector<double>(actual, actual + 2 * n));
    };
    for (uint32_t c = 0; c < v.nCells; ++c) sink_cell<false>(v, nullptr, c);
    write_actual();

    if (crack) {
        const std::vector<sf3d_sink_crack_soil_t> crackSoils = readv<sf3d_sink_crack_soil_t>(in, nSoils);
        const std::vector<double> pond = readv<double>(in, N);
        std::vector<double> upper(nSoils * SF3D_ROOT_MAX_HORIZONS, 0.), lower(nSoils * SF3D_ROOT_MAX_HORIZONS, 0.);      /* as sf3d_sink_initialize keeps them */
        for (size_t s = 0; s < nSoils; ++s)
            for (int32_t h = 0; h < soils[s].nrHorizons; ++h) {
                upper[s * SF3D_ROOT_MAX_HORIZONS + h] = soils[s].upperDepth[h];
                lower[s * SF3D_ROOT_MAX_HORIZONS + h] = soils[s].lowerDepth[h];
            }
        std::vector<double> maxDepth;
        std::vector<int32_t> lastLayer;
        sinkCrackTables((uint32_t)nSoils, crackSoils.data(), upper.data(), lower.data(), computationSoilDepth, (uint32_t)nl, layerDepth.data(), layerThickness.data(),
                        maxDepth, lastLayer);
        writev(out, maxDepth);
        writev(out, lastLayer);
        std::vector<float> precSurfaceWater(n);
        std::vector<double> crackWater(n);
        const SinkCrackDev k{pond.data(), maxDepth.data(), lastLayer.data(), layerDepth.data(), precSurfaceWater.data(), crackWater.data()};
        sink.assign(N, 0.);
        for (uint32_t c = 0; c < v.nCells; ++c) sink_cell<true>(v, &k, c);
        write_actual();
        writev(out, precSurfaceWater);
        writev(out, crackWater);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
