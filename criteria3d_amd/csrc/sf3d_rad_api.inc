/* part of sf3d_api.cpp (included at its end, after the sink entry points) - the C entry points of include/sf3d_rad.h.  The host keeps the
 * raster's size and the settings, evaluates what depends on the cell only (once per raster) and on the date and time only (once per
 * call) with the C library (sf3d_rad_setup.inc) and refuses what S_solpos refuses; everything per cell and hour lives on the device
 * (sf3d_rad.inc). */
#include "sf3d_rad.h"
#include "sf3d_rad_setup.inc"

static_assert(SF3D_RAD_MAP_COUNT == RAD_OUTPUTS, "sf3d_rad.h and sf3d_device.h disagree");

namespace {

struct RadHost {
    bool on = false;
    uint32_t nRows = 0, nCols = 0;
    double xll = 0., yll = 0., cellSize = 0.;  /* the raster's place: sf3d_transmissivity_api.inc asks where a station lies */
    sf3d_rad_settings_t set;
} RD;

/* Crit3DRadiationSettings::initialize, radiationSettings.cpp:41-72; Crit3DGisSettings, gis.cpp:47-54 */
const sf3d_rad_settings_t kRadDefaults = {1, SF3D_RAD_REALSKY_LINKE, 1, SF3D_RAD_MODE_FIXED, SF3D_RAD_MODE_FIXED, SF3D_RAD_TILT_DEM, 1, 1, 4.f,
                                          {-9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f, -9999.f},
                                          0.2f, 0.f, 0.f, 0.75f};

void radClear() { RD = RadHost(); (void)dev().rad_free(); }

bool radSettingsOk(const sf3d_rad_settings_t& s)
{
    if (s.realSkyAlgorithm != SF3D_RAD_REALSKY_TOTALTRANSMISSIVITY && s.realSkyAlgorithm != SF3D_RAD_REALSKY_LINKE) return false;
    if (s.linkeMode < SF3D_RAD_MODE_FIXED || s.linkeMode > SF3D_RAD_MODE_MONTHLY) return false;
    if (s.albedoMode != SF3D_RAD_MODE_FIXED && s.albedoMode != SF3D_RAD_MODE_MAP) return false;
    if (s.tiltMode != SF3D_RAD_TILT_FIXED && s.tiltMode != SF3D_RAD_TILT_DEM) return false;
    return s.timeZone >= -12 && s.timeZone <= 12;              /* validate(): fabs(timezone) > 12 */
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_rad_default_parameters(sf3d_rad_settings_t* settings)
{
    if (!settings) return SF3D_PARAMETER_ERROR;
    *settings = kRadDefaults;
    return SF3D_OK;
}

sf3d_error_t sf3d_rad_initialize(uint32_t nrRows, uint32_t nrCols, const float* dem, float flag, double xllCorner, double yllCorner, double cellSize,
                                 const float* latMap, const float* lonMap, const float* slopeMap, const float* aspectMap,
                                 const float* linkeMap, const float* albedoMap, const sf3d_rad_settings_t* settings)
{
    if (!rasterShapeOk(nrRows, nrCols, dem) || !(cellSize > 0) || !latMap || !lonMap) return SF3D_PARAMETER_ERROR;
    const sf3d_rad_settings_t s = settings ? *settings : kRadDefaults;
    if (!radSettingsOk(s)) return SF3D_PARAMETER_ERROR;
    if (s.tiltMode == SF3D_RAD_TILT_DEM && (!slopeMap || !aspectMap)) return SF3D_PARAMETER_ERROR;
    if ((s.linkeMode == SF3D_RAD_MODE_MAP && !linkeMap) || (s.albedoMode == SF3D_RAD_MODE_MAP && !albedoMap)) return SF3D_PARAMETER_ERROR;
    radClear();
    const size_t n = (size_t)nrRows * nrCols;
    std::vector<float> fl[RAD_MAP_TRANSMISSIVITY - RAD_MAP_DEM];
    std::vector<double> db[RAD_DOUBLE_MAPS];
    std::vector<int32_t> ok(n, 0);
    for (auto& v : fl) v.assign(n, flag);
    for (auto& v : db) v.assign(n, 0.);
    /* gis::updateMinMaxRasterGrid, gis.cpp:569-606: Crit3DRasterGrid::maximum of the DEM */
    float demMax = -9999.f;
    bool first = true;
    for (size_t c = 0; c < n; ++c) {
        const float z = dem[c];
        fl[0][c] = z;
        if (rasterIsFlag(z, flag)) continue;
        if (!rasterIsFlag(z, -9999.f)) { if (first || z > demMax) demMax = z; first = false; }
        const bool fixed = s.tiltMode == SF3D_RAD_TILT_FIXED;
        const RadCellDev k = radsCell(z, latMap[c], lonMap[c], fixed ? s.tilt : slopeMap[c], fixed ? s.aspect : aspectMap[c]);
        fl[1][c] = k.lat; fl[2][c] = k.lon; fl[3][c] = k.cl; fl[4][c] = k.sl; fl[5][c] = k.press; fl[6][c] = k.slope; fl[7][c] = k.aspect;
        db[0][c] = k.cp; db[1][c] = k.sp; db[2][c] = k.ct; db[3][c] = k.st; db[4][c] = k.sinSlope; db[5][c] = k.cosSlope; db[6][c] = k.Fg; db[7][c] = k.reflGeom;
        ok[c] = k.ok;
    }
    RadSetup setup{};
    setup.nRows = nrRows; setup.nCols = nrCols;
    for (int k = 0; k < RAD_MAP_TRANSMISSIVITY - RAD_MAP_DEM; ++k) setup.fl[k] = fl[k].data();
    for (int k = 0; k < RAD_DOUBLE_MAPS; ++k) setup.db[k] = db[k].data();
    setup.ok = ok.data();
    setup.xll = xllCorner; setup.yll = yllCorner; setup.cellSize = cellSize; setup.flag = flag; setup.demMax = demMax;
    const sf3d_error_t e = dev().rad_alloc(setup);
    if (e != SF3D_OK) { rasterFail("rad initialize", e); radClear(); return e; }
    RD.nRows = nrRows; RD.nCols = nrCols; RD.xll = xllCorner; RD.yll = yllCorner; RD.cellSize = cellSize; RD.set = s;
    RD.on = true;
    return SF3D_OK;
}

sf3d_error_t sf3d_rad_compute_hour(int year, int month, int day, int hour, int minute, int second, uint32_t nrCells, const float* transmissivity)
{
    /* the checks that need no raster come first: a caller learns of a date S_solpos refuses before it has one */
    if (month < 1 || month > 12 || year < 1 || day < 1 || day > radsMonthDays(year, month)) return SF3D_PARAMETER_ERROR;
    if (hour < 0 || hour > 23 || minute < 0 || minute > 59 || second < 0 || second > 59) return SF3D_PARAMETER_ERROR;
    const sf3d_rad_settings_t& s = RD.on ? RD.set : kRadDefaults;
    RadHourDev h{};
    if (!radsHour(year, month, day, hour, minute, second, s.timeZone, s.isUTC != 0, h)) return SF3D_PARAMETER_ERROR;
    /* no map handed in: the meteo block has to hold an interpolated transmissivity map on this raster (none before sf3d_rad_initialize) */
    if (!transmissivity && !dev().meteo_produced(METEO_ATM_TRANSMISSIVITY, RD.nRows, RD.nCols)) return SF3D_PARAMETER_ERROR;
    if (!RD.on) return SF3D_MEMORY_ERROR;
    if (nrCells != RD.nRows * RD.nCols) return SF3D_PARAMETER_ERROR;
    /* computeRadiationDemPoint, solarRadiation.cpp:958-964: the month of the time handed in, not of the shifted local time */
    if (s.linkeMode == SF3D_RAD_MODE_MONTHLY) h.linke = s.linkeMonthly[month - 1];
    else h.linke = (s.linkeMode == SF3D_RAD_MODE_FIXED) ? s.linke : -9999.f;
    h.albedo = (s.albedoMode == SF3D_RAD_MODE_FIXED) ? s.albedo : -9999.f;
    h.clearSky = s.clearSky;
    h.realSky = s.realSky != 0; h.realSkyAlgorithm = s.realSkyAlgorithm; h.shadowing = s.shadowing != 0;
    return rasterFail("rad compute hour", dev().rad_hour(h, transmissivity, mapsOwnedCells(nrCells)));
}

sf3d_error_t sf3d_rad_get_map(int which, uint32_t nrCells, float* map)
{
    if (!RD.on) return SF3D_MEMORY_ERROR;
    if (!map || nrCells != RD.nRows * RD.nCols) return SF3D_PARAMETER_ERROR;
    if (which < 0 || which >= SF3D_RAD_MAP_COUNT) return SF3D_INDEX_ERROR;
    return rasterFail("rad get map", dev().rad_download(which, map));
}

sf3d_error_t sf3d_rad_device_trig(int which, uint32_t count, const double* x, const double* y, double* out)
{
    if (which < 0 || which > 5 || (count && (!x || !out || (which == 5 && !y)))) return SF3D_PARAMETER_ERROR;
    return rasterFail("rad device trig", dev().rad_trig(which, count, x, y, out));
}

double sf3d_rad_kernel_ms(void) { return dev().rad_kernel_ms(); }

sf3d_error_t sf3d_rad_clean(void)
{
    radClear();
    return SF3D_OK;
}

} /* extern "C" */
