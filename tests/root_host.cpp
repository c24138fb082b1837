/* host build of the text of k_root_table, k_root_cell and k_root_gather (criteria3d_amd/csrc/sf3d_root.inc with sf3d_glibcmath.inc: the text
 * the device compiles) behind the table builder of sf3d_root_initialize (sf3d_root_setup.inc) for tests/test_root_host.py and
 * tests/test_gpu_root.py: root_table_row over all rows once, then per degree-day map root_cell over the raster and root_gather_cell for a
 * layer range.  Every table is a heap block of its own of exactly the size DeviceSolver::root_alloc gives it inside its one device block
 * (the unit table: nUnits entries), so the address sanitizer sees what the device cannot show.  The same program is built once with
 * -fsanitize=address,undefined.
 *
 *   root_host <input> <output>
 * input : int32 nCells, nrLayers, nUnits, nSoils, nCases; float flag; float dem[nCells]; int32 cropIndex[nCells], soilIndex[nCells];
 *         double layerDepth[nrLayers], layerThickness[nrLayers]; sf3d_root_unit_t units[nUnits]; sf3d_root_soil_t soils[nSoils];
 *         per case: int32 layer0, layerCount; float degreeDays[nCells].
 * output: int32 status (what rootBuildTables returns; not 0: nothing follows), nRows; double table[nrLayers][nRows]; int32 rowLayers[nRows][2];
 *         per case: double length[nCells], depth[nCells]; int32 first[nCells], last[nCells], key[nCells]; double density[layerCount][nCells]. */
#include "host_io.h"
#include "sf3d_root_setup.inc"

#define SF3D_SNOW_HOST
#define SF3D_SNOW_FN static inline
#include "sf3d_snow.inc"
#define SF3D_ROOT_HOST
#define SF3D_ROOT_FN static inline
#include "sf3d_root.inc"

static_assert(sizeof(sf3d_root_unit_t) == sizeof(RootUnitDev), "the root unit table is copied as it is");

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const std::vector<int32_t> dims = readv<int32_t>(in, 5);
    const size_t n = (size_t)dims[0], nl = (size_t)dims[1], nUnits = (size_t)dims[2], nSoils = (size_t)dims[3], nCases = (size_t)dims[4];
    const float flag = read1<float>(in);
    const std::vector<float> dem = readv<float>(in, n);
    const std::vector<int32_t> cropIndex = readv<int32_t>(in, n), soilIndex = readv<int32_t>(in, n);
    const std::vector<double> layerDepth = readv<double>(in, nl), layerThickness = readv<double>(in, nl);
    const std::vector<RootUnitDev> units = readv<RootUnitDev>(in, nUnits);
    const std::vector<sf3d_root_soil_t> soils = readv<sf3d_root_soil_t>(in, nSoils);

    RootTablesHost T;
    const int32_t status = (int32_t)rootBuildTables((uint32_t)n, dem.data(), flag, (uint32_t)nl, layerDepth.data(), cropIndex.data(), soilIndex.data(), (uint32_t)nUnits,
                                                    (uint32_t)nSoils, soils.data(), T);
    const size_t rows = status == 0 ? T.rowUnit.size() : 0;
    const std::vector<int32_t> head = {status, (int32_t)rows};
    writev(out, head);
    if (status != 0) { fclose(in); return fclose(out) == 0 ? 0 : 3; }

    std::vector<double> table(rows * nl);
    std::vector<int32_t> rowLayers(2 * rows);
    RootTableView t{};
    t.units = units.data(); t.soilDepth = T.soilDepth.data(); t.layerDepth = layerDepth.data(); t.layerThickness = layerThickness.data();
    t.layerFrac = T.layerFrac.data(); t.lunette = T.lunette.data(); t.rowUnit = T.rowUnit.data(); t.rowSoil = T.rowSoil.data(); t.rowN = T.rowN.data();
    t.table = table.data(); t.rowLayers = rowLayers.data();
    t.nRows = (uint32_t)rows; t.nrLayers = (uint32_t)nl; t.lunetteMax = T.lunetteMax;
    for (uint32_t r = 0; r < t.nRows; ++r) root_table_row(t, r);
    writev(out, table);
    writev(out, rowLayers);

    std::vector<double> length(n), depth(n);
    std::vector<int32_t> first(n), last(n), key(n);
    for (size_t k = 0; k < nCases; ++k) {
        const std::vector<int32_t> range = readv<int32_t>(in, 2);
        const std::vector<float> dd = readv<float>(in, n);
        if (range[0] < 0 || range[1] < 0 || (size_t)range[0] + (size_t)range[1] > nl) { fprintf(stderr, "root_host: layer range\n"); return 2; }
        std::vector<double> gathered((size_t)range[1] * n);
        RootView v{};
        v.dem = dem.data(); v.dd = dd.data(); v.cropIndex = T.ci.data(); v.soilIndex = T.si.data();
        v.length = length.data(); v.depth = depth.data(); v.first = first.data(); v.last = last.data(); v.key = key.data();
        v.units = units.data(); v.soilDepth = T.soilDepth.data(); v.soilMaxN = T.soilMaxN.data(); v.pairRow = T.pairRow.data();
        v.rowLayers = rowLayers.data(); v.table = table.data(); v.out = gathered.data(); v.mine = nullptr;
        v.nCells = (uint32_t)n; v.nUnits = (uint32_t)nUnits; v.nSoils = (uint32_t)nSoils; v.nRows = (uint32_t)rows; v.nrLayers = (uint32_t)nl;
        v.layer0 = (uint32_t)range[0]; v.layerCount = (uint32_t)range[1]; v.flag = flag;
        for (uint32_t c = 0; c < v.nCells; ++c) root_cell(v, units.data(), c);
        for (uint32_t c = 0; c < v.nCells; ++c) root_gather_cell(v, c);
        writev(out, length); writev(out, depth); writev(out, first); writev(out, last); writev(out, key); writev(out, gathered);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
