/* sf3d_glocal_setup.inc - the host side of glocal detrending (included by sf3d_glocal_api.inc and by tests/glocal_host.cpp, after
 * sf3d_localdetrend_setup.inc, whose call checks and set-up it uses): what sf3d_glocal_set_areas and sf3d_glocal_interpolate check and
 * lay out before any device work - the areas' lists as the kernels read them, among them the cell-major pair table (per cell its
 * (area, weight) pairs, ascending area index), and per call the place of every listed station in the call's point table.  No device
 * code: the host program runs it under the sanitizers. */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "sf3d_glocal.h"

struct GlocalAreasHost {
    bool on = false;
    uint32_t nAreas = 0, nCells = 0;
    std::vector<uint32_t> stationOffset;        /* [nAreas + 1] */
    std::vector<int32_t> stationIndex;
    std::vector<uint8_t> hasCells;              /* per area */
    std::vector<uint32_t> pairOffset, pairArea; /* [nCells + 1], per pair */
    std::vector<float> pairWeight;
};

/* the row and the column the cell loop takes from the float cell number (project.cpp:3348-3349): a float quotient */
static inline void glocalRowCol(float cell, uint32_t nCols, int& row, int& col)
{
    row = int(cell / nCols);
    col = int(cell) % int(nCols);
}

/* the checks and the lay-out of sf3d_glocal_set_areas on a raster of nRows x nCols cells */
static inline bool glocalAreasOk(uint32_t nRows, uint32_t nCols, uint32_t nAreas, const uint32_t* cellOffset, const float* cell, const float* weight,
                                 const uint32_t* stationOffset, const int32_t* stationIndex, GlocalAreasHost& A)
{
    A = GlocalAreasHost();
    const uint64_t n = (uint64_t)nRows * nCols;
    if (nAreas == 0 || !cellOffset || !stationOffset || n == 0 || n > (1u << 24)) return false;
    if (cellOffset[0] != 0 || stationOffset[0] != 0) return false;
    for (uint32_t a = 0; a < nAreas; ++a) {
        if (cellOffset[a + 1] < cellOffset[a] || stationOffset[a + 1] < stationOffset[a]) return false;
        if (stationOffset[a + 1] - stationOffset[a] > SF3D_METEO_MAX_STATIONS) return false;
    }
    if ((cellOffset[nAreas] > 0 && (!cell || !weight)) || (stationOffset[nAreas] > 0 && !stationIndex)) return false;
    std::vector<uint32_t> at(cellOffset[nAreas]), seen(n, UINT32_MAX);
    A.pairOffset.assign(n + 1, 0);
    A.hasCells.assign(nAreas, 0);
    for (uint32_t a = 0; a < nAreas; ++a) {
        for (uint32_t k = cellOffset[a]; k < cellOffset[a + 1]; ++k) {
            if (!std::isfinite(cell[k]) || cell[k] < 0.f || !(cell[k] < (float)n)) return false;
            if (!std::isfinite(weight[k]) || weight[k] == 0.f || weight[k] == -9999.f) return false;
            int row, col;
            glocalRowCol(cell[k], nCols, row, col);
            if (row < 0 || (uint32_t)row >= nRows || col < 0) return false;
            const uint32_t c = (uint32_t)row * nCols + (uint32_t)col;
            if (seen[c] == a) return false;
            seen[c] = a;
            at[k] = c;
            ++A.pairOffset[c + 1];
            A.hasCells[a] = 1;
        }
    }
    for (uint64_t c = 0; c < n; ++c) A.pairOffset[c + 1] += A.pairOffset[c];
    A.pairArea.resize(cellOffset[nAreas]);
    A.pairWeight.resize(cellOffset[nAreas]);
    std::vector<uint32_t> fill(A.pairOffset.begin(), A.pairOffset.end() - 1);
    for (uint32_t a = 0; a < nAreas; ++a)                                         /* areas ascending: so are a cell's pairs */
        for (uint32_t k = cellOffset[a]; k < cellOffset[a + 1]; ++k) {
            const uint32_t p = fill[at[k]]++;
            A.pairArea[p] = a; A.pairWeight[p] = weight[k];
        }
    A.stationOffset.assign(stationOffset, stationOffset + nAreas + 1);
    A.stationIndex.assign(stationIndex, stationIndex + stationOffset[nAreas]);
    A.nAreas = nAreas; A.nCells = (uint32_t)n;
    A.on = true;
    return true;
}

/* the checks of sf3d_glocal_interpolate that read the areas, beyond localCallOk's and proxiesCallOk's; listPoint: per entry of the areas'
 * station lists the station's place in the call's point table, -1 where it has no point this hour */
static inline bool glocalCallOk(const GlocalAreasHost& A, uint32_t nStations, const int32_t* pointIndex, std::vector<int32_t>& listPoint)
{
    if (!A.on || nStations > SF3D_METEO_MAX_STATIONS || (nStations > 0 && !pointIndex)) return false;
    std::vector<std::pair<int32_t, int32_t>> byIndex(nStations);
    for (uint32_t k = 0; k < nStations; ++k) byIndex[k] = {pointIndex[k], (int32_t)k};
    std::sort(byIndex.begin(), byIndex.end());
    for (uint32_t k = 1; k < nStations; ++k)
        if (byIndex[k].first == byIndex[k - 1].first) return false;
    listPoint.assign(A.stationIndex.size(), -1);
    for (uint32_t a = 0; a < A.nAreas; ++a) {
        bool any = false;
        for (uint32_t l = A.stationOffset[a]; l < A.stationOffset[a + 1]; ++l) {
            const auto it = std::lower_bound(byIndex.begin(), byIndex.end(), std::make_pair(A.stationIndex[l], INT32_MIN));
            if (it != byIndex.end() && it->first == A.stationIndex[l]) { listPoint[l] = it->second; any = true; }
        }
        if (A.hasCells[a] && !any) return false;                                  /* interpolate() over no point: the reference fails */
    }
    return true;
}

/* the set-up every area and cell of a call shares: localSetup's table, neither minimum-points rule */
static inline void glocalSetup(const sf3d_localdetrend_fit_t* fit, uint32_t nStations, float boundingBoxArea, double* table, LocalDetrendSetup& s)
{
    sf3d_localdetrend_fit_t own = *fit;
    own.minPointsLocalDetrending = 1;                                           /* not read of the caller's; the selection's numbers are not used */
    localSetup(&own, nStations ? nStations : 1u, boundingBoxArea, table, s);
    s.minPointsLocal = 0; s.minPoints = 0; s.minPointsStep = 0; s.radiusAll = 0.f;
}
