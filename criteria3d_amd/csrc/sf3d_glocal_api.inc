/* part of sf3d_api.cpp (included after sf3d_localproxies_api.inc, whose call checks and set-up it uses) - the C entry points of
 * include/sf3d_glocal.h.  The host checks the areas and every call before any device work and lays them out as the kernels read them
 * (sf3d_glocal_setup.inc: the cell-major pair table, the place of every listed station in the call's point table); everything else
 * lives on the device (sf3d_glocal.inc). */
#include "sf3d_glocal.h"
#include "sf3d_glocal_setup.inc"

static_assert(sizeof(GlocalAreaDev) == 208, "GlocalAreaDev has no padding");

namespace {

GlocalAreasHost GL;

void glocalHostClear() { GL = GlocalAreasHost(); }

}  // namespace

extern "C" {

sf3d_error_t sf3d_glocal_set_areas(uint32_t nAreas, const uint32_t* cellOffset, const float* cell, const float* weight, const uint32_t* stationOffset,
                                   const int32_t* stationIndex)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    GlocalAreasHost A;
    if (!glocalAreasOk(MT.nRows, MT.nCols, nAreas, cellOffset, cell, weight, stationOffset, stationIndex, A)) return SF3D_PARAMETER_ERROR;
    const GlocalStatic g{A.nAreas, (uint32_t)A.stationIndex.size(), (uint32_t)A.pairArea.size(), A.stationOffset.data(), A.pairOffset.data(), A.pairArea.data(),
                         A.pairWeight.data()};
    const sf3d_error_t e = rasterFail("glocal set areas", dev().glocal_set(g));
    if (e != SF3D_OK) { glocalHostClear(); (void)dev().glocal_free(); return e; }
    GL = std::move(A);
    return SF3D_OK;
}

sf3d_error_t sf3d_glocal_interpolate(int variable, int method, uint32_t nStations, const int32_t* pointIndex, const double* x, const double* y, const float* value,
                                     uint32_t nProxies, const float* proxyValues, float boundingBoxArea, const sf3d_meteo_settings_t* settings,
                                     const sf3d_localdetrend_fit_t* fit, const sf3d_localproxies_others_t* others, float* out)
{
    static const float noHeight[SF3D_METEO_MAX_STATIONS] = {0.f};       /* the height is not active: its row is never used */
    if (!localCallOk(variable, nStations, x, y, noHeight, settings, fit, false, false)) return SF3D_PARAMETER_ERROR;
    GlocalCall g{};
    if (!proxiesCallOk(nStations, nProxies, proxyValues, settings, others, g.proxies, g.rows, &g.height)) return SF3D_PARAMETER_ERROR;
    if (!g.height) g.height = noHeight;
    /* the rest of the call is sf3d_meteo_interpolate's, which knows neither option */
    sf3d_meteo_settings_t plain = *settings;
    plain.useMultipleDetrending = 0; plain.useLocalDetrending = 0;
    MeteoCall call;
    const sf3d_error_t e = meteoPrepare(variable, method, nStations, x, y, value, boundingBoxArea, &plain, false, call);
    if (e != SF3D_OK) return e;
    if (!GL.on || !dev().glocal_areas_set()) return SF3D_PARAMETER_ERROR;
    for (int r = 0; r < g.proxies.nOthers; ++r)
        if (!dev().meteo_has_map((uint32_t)g.proxies.slot[r])) return SF3D_PARAMETER_ERROR;
    std::vector<int32_t> listPoint;
    if (!glocalCallOk(GL, nStations, pointIndex, listPoint)) return SF3D_PARAMETER_ERROR;
    double table[LOCALDETREND_TABLE_DOUBLES] = {0.};
    g.table = table; g.listPoint = listPoint.data();
    glocalSetup(fit, nStations, boundingBoxArea, table, g.setup);
    return rasterFail("glocal interpolate", dev().glocal_interpolate(call, g, mapsOwnedCells((size_t)MT.nRows * MT.nCols), out));
}

sf3d_error_t sf3d_glocal_get_area_fit(uint32_t nAreas, uint32_t nList, uint8_t* significant, float* r2, double* parameters, uint8_t* proxySignificant, double* slope,
                                      double* intercept, uint32_t* fitted, uint32_t* kept, float* detrended, uint8_t* stationKept)
{
    if (!MT.on) return SF3D_MEMORY_ERROR;
    if (!GL.on || nAreas != GL.nAreas || nList != GL.stationIndex.size() || !dev().glocal_done()) return SF3D_PARAMETER_ERROR;
    std::vector<GlocalAreaDev> area(nAreas);
    LocalProxiesSetup ps{};
    const sf3d_error_t e = dev().glocal_records(area.data(), detrended, stationKept, &ps);
    if (e != SF3D_OK) return rasterFail("glocal get area fit", e);
    const int S = SF3D_METEO_MAX_PROXIES, P = SF3D_LOCALDETREND_MAX_PARAMETERS;
    for (uint32_t a = 0; a < nAreas; ++a) {
        const GlocalAreaDev& o = area[a];
        if (significant) significant[a] = (uint8_t)(o.significant != 0);
        if (r2) r2[a] = o.r2;
        if (fitted) fitted[a] = o.fitted;
        if (kept) kept[a] = o.kept;
        for (int j = 0; parameters && j < P; ++j) parameters[(size_t)a * P + j] = o.parameters[j];
        for (int p = 0; p < S; ++p) {
            if (proxySignificant) proxySignificant[(size_t)a * S + p] = 0;
            if (slope) slope[(size_t)a * S + p] = -9999.;
            if (intercept) intercept[(size_t)a * S + p] = -9999.;
        }
        /* the device packs the lines of the significant other proxies in slot order */
        int j = 0;
        for (int r = 0; r < ps.nOthers; ++r) {
            if (!((o.mask >> r) & 1u)) continue;
            const size_t at = (size_t)a * S + (size_t)ps.slot[r];
            if (proxySignificant) proxySignificant[at] = 1;
            if (slope) slope[at] = o.line[j][0];
            if (intercept) intercept[at] = o.line[j][1];
            ++j;
        }
    }
    return SF3D_OK;
}

double sf3d_glocal_kernel_ms(int which) { return dev().glocal_kernel_ms(which); }

uint64_t sf3d_glocal_bytes(void) { return MT.on ? dev().glocal_bytes() : 0; }

sf3d_error_t sf3d_glocal_clean(void)
{
    glocalHostClear();
    (void)dev().glocal_free();
    return SF3D_OK;
}

} /* extern "C" */
