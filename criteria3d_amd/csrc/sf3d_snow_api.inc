/* part of sf3d_api.cpp (included at its end) - the C entry points of include/sf3d_snow.h.  The host keeps the raster's size, its flag, the
 * DEM and the parameters; the maps themselves live on the device (sf3d_snow.inc).  initializeSnowMaps / resetSnowModel run here, on
 * the host (once per run; snowMaps.cpp:82-108, 177-218), and upload their maps. */
#include "sf3d_snow.h"

namespace {

struct SnowHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0;
    float flag = -9999.f;
    std::vector<float> dem;
    sf3d_snow_parameters_t par;
} SN;

const sf3d_snow_parameters_t kSnowDefaults = {0.02, 0.2, 1, 0.05, 2, -0.5, 0.05};      /* initializeSnowParameters, snow.cpp:39-50 */

void snowClear() { SN = SnowHost(); (void)dev().snow_free(); }

/* resetSnowModel on `swe` (snowMaps.cpp:177-218; snow.cpp:559-579 for the energies): uploads the six other state maps and zeroes the
 * outputs; cells that hold the flag keep it in every map */
sf3d_error_t snowReset(const std::vector<float>& swe)
{
    const size_t n = swe.size();
    const double initSoilPackTemp = 3.4, initSnowSurfaceTemp = 5.0, skin = SN.par.skinThickness;
    const int surfaceBulkDensity = 1350;
    std::vector<float> ice(n, SN.flag), lwc(n, SN.flag), ie(n, SN.flag), se(n, SN.flag), ts(n, SN.flag), age(n, SN.flag), zero(n, SN.flag);
    for (size_t c = 0; c < n; ++c) {
        const float initSWE = swe[c];
        if (rasterIsFlag(initSWE, SN.flag)) continue;
        ice[c] = initSWE; lwc[c] = 0; age[c] = -9999;
        ts[c] = float(initSnowSurfaceTemp);
        if (initSWE > 0) se[c] = float(initSnowSurfaceTemp * 1000. * 2.1 * skin);                 /* computeSurfaceEnergySnow */
        else se[c] = float(initSnowSurfaceTemp * 1350 * 1.4 * skin);                                 /* computeSurfaceEnergySoil */
        ie[c] = float(initSoilPackTemp * (1000. * 2.1 * (initSWE / 1000.) * 0.001 + surfaceBulkDensity * 1.4 * 0.3));   /* computeInternalEnergy */
        zero[c] = 0;
    }
    const std::vector<float>* st[6] = {&ice, &lwc, &ie, &se, &ts, &age};
    for (int k = 0; k < 6; ++k) { const sf3d_error_t e = dev().snow_upload(SNOW_MAP_STATE + 1 + k, st[k]->data()); if (e != SF3D_OK) return e; }
    for (int k = 0; k < 6; ++k) { const sf3d_error_t e = dev().snow_upload(SNOW_MAP_OUT + k, zero.data()); if (e != SF3D_OK) return e; }
    return SF3D_OK;
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_snow_default_parameters(sf3d_snow_parameters_t* parameters)
{
    if (!parameters) return SF3D_PARAMETER_ERROR;
    *parameters = kSnowDefaults;
    return SF3D_OK;
}

sf3d_error_t sf3d_snow_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, const sf3d_snow_parameters_t* parameters)
{
    if (!rasterShapeOk(nrRows, nrCols, dem)) return SF3D_PARAMETER_ERROR;
    const uint32_t n = nrRows * nrCols;
    snowClear();
    sf3d_error_t e = dev().snow_alloc(n);
    if (e != SF3D_OK) return rasterFail("snow initialize", e);
    SN.nRows = nrRows; SN.nCols = nrCols; SN.flag = flag;
    SN.dem.assign(dem, dem + n);
    SN.par = parameters ? *parameters : kSnowDefaults;
    /* setConstantValueWithBase(0, dtm): SWE 0 on the DEM's cells, the flag elsewhere */
    std::vector<float> swe(n);
    for (uint32_t c = 0; c < n; ++c) swe[c] = rasterIsFlag(dem[c], flag) ? flag : 0.f;
    e = dev().snow_upload(SNOW_MAP_DEM, SN.dem.data());
    if (e == SF3D_OK) e = dev().snow_upload(SNOW_MAP_STATE, swe.data());
    if (e == SF3D_OK) e = snowReset(swe);
    if (e != SF3D_OK) { rasterFail("snow initialize", e); snowClear(); return e; }
    SN.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_snow_set_parameters(const sf3d_snow_parameters_t* parameters)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    if (!parameters) return SF3D_PARAMETER_ERROR;
    SN.par = *parameters;
    return SF3D_OK;
}

sf3d_error_t sf3d_snow_reset(void)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    std::vector<float> swe((size_t)SN.nRows * SN.nCols);
    sf3d_error_t e = dev().snow_download(SNOW_MAP_STATE, swe.data());
    if (e == SF3D_OK) e = snowReset(swe);
    return rasterFail("snow reset", e);
}

sf3d_error_t sf3d_snow_set_state(int which, uint32_t nrCells, const float* map)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != SN.nRows * SN.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_SNOW_STATE_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("snow set state", dev().snow_upload(SNOW_MAP_STATE + which, map));
}

sf3d_error_t sf3d_snow_get_state(int which, uint32_t nrCells, float* map)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != SN.nRows * SN.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_SNOW_STATE_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("snow get state", dev().snow_download(SNOW_MAP_STATE + which, map));
}

sf3d_error_t sf3d_snow_get_output(int which, uint32_t nrCells, float* map)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != SN.nRows * SN.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_SNOW_OUTPUT_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("snow get output", dev().snow_download(SNOW_MAP_OUT + which, map));
}

sf3d_error_t sf3d_snow_compute_hour(uint32_t nrCells, const float* airTemperature, const float* precipitation, const float* relativeHumidity,
                                    const float* windIntensity, const float* globalRadiation, const float* beamRadiation,
                                    const float* transmissivity, const float* surfaceWater, double clearSkyTransmissivity)
{
    if (!SN.on) return SF3D_MEMORY_ERROR;
    const float* in[8] = {airTemperature, precipitation, relativeHumidity, windIntensity, globalRadiation, beamRadiation, transmissivity, surfaceWater};
    if (nrCells != SN.nRows * SN.nCols) return SF3D_PARAMETER_ERROR;
    for (int k = 0; k < 7; ++k) if (!in[k]) return SF3D_PARAMETER_ERROR;
    const SnowParamsDev p = {SN.par.skinThickness, SN.par.soilAlbedo, SN.par.snowVegetationHeight, SN.par.snowWaterHoldingCapacity,
                             SN.par.tempMaxWithSnow, SN.par.tempMinWithRain, SN.par.snowSurfaceDampingDepth, clearSkyTransmissivity};
    return rasterFail("snow compute hour", dev().snow_hour(in, p, SN.flag, mapsOwnedCells(nrCells)));
}

double sf3d_snow_kernel_ms(void) { return dev().snow_kernel_ms(); }

sf3d_error_t sf3d_snow_clean(void)
{
    snowClear();
    return SF3D_OK;
}

} /* extern "C" */
