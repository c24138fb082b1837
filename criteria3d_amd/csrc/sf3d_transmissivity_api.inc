/* part of sf3d_api.cpp (included at its end, after sf3d_rad_api.inc, whose raster and settings it uses) - the C entry points of
 * include/sf3d_transmissivity.h.  The host evaluates what depends on the date and time only once per slot (radsHour) and what depends
 * on the point only once per point (radsCellAt on the point's height, float(lat), float(lon), slope 0, aspect 180), and refuses what
 * the reference cannot answer; the evaluations and the sums live on the device (sf3d_transmissivity.inc). */
#include "sf3d_transmissivity.h"

static_assert(SF3D_TRANSMISSIVITY_MAX_WIDTH == TR_MAX_WIDTH && SF3D_TRANSMISSIVITY_MAX_POINTS == TR_MAX_POINTS &&
              SF3D_TRANSMISSIVITY_WINDOW_SLOTS == TR_WINDOW_SLOTS, "sf3d_transmissivity.h and sf3d_device.h disagree");
static_assert(sizeof(sf3d_transmissivity_point_t) == 40, "sf3d_transmissivity_point_t is five doubles");

namespace {

bool trWhenOk(int year, int month, int day, int hour, int minute, int second)
{
    if (month < 1 || month > 12 || year < 1 || day < 1 || day > radsMonthDays(year, month)) return false;
    return hour >= 0 && hour <= 23 && minute >= 0 && minute <= 59 && second >= 0 && second <= 59;
}

/* the slot at `offset` seconds from the time handed in (Crit3DTime::addSeconds, then the local-time shift: radsHour normalises the sum);
 * month: of the time handed in (solarRadiation.cpp:1291-1293, 862-863) */
void trHour(const sf3d_rad_settings_t& s, int year, int month, int day, int hour, int minute, long offset, RadHourDev& h, uint8_t& ok)
{
    h = RadHourDev{};
    ok = radsHour(year, month, day, hour, minute, (int)offset, s.timeZone, s.isUTC != 0, h) ? 1 : 0;
    if (s.linkeMode == SF3D_RAD_MODE_MONTHLY) h.linke = s.linkeMonthly[month - 1];
    else h.linke = (s.linkeMode == SF3D_RAD_MODE_FIXED) ? s.linke : -9999.f;
    h.albedo = (s.albedoMode == SF3D_RAD_MODE_FIXED) ? s.albedo : -9999.f;
    h.clearSky = s.clearSky;
    h.realSky = s.realSky != 0; h.realSkyAlgorithm = s.realSkyAlgorithm; h.shadowing = s.shadowing != 0;
}

/* false: Linke or albedo in map mode and the point's row or column (getRowCol, gis.cpp:486-493) is outside the raster */
bool trPoint(const sf3d_rad_settings_t& s, const sf3d_transmissivity_point_t& in, TrPointDev& p)
{
    p = TrPointDev{};
    p.x = in.x; p.y = in.y; p.z = in.z;
    p.cell = radsCellAt(in.z, float(in.lat), float(in.lon), 0.f, 180.f);
    const double cs = RD.cellSize;
    /* gis::isOutOfGridXY, gis.cpp:840-845 */
    const bool out = (in.x < RD.xll) || (in.y < RD.yll) || (in.x >= (RD.xll + (int)RD.nCols * cs)) || (in.y >= (RD.yll + (int)RD.nRows * cs));
    p.inGrid = out ? 0 : 1;
    if (s.linkeMode == SF3D_RAD_MODE_MAP || s.albedoMode == SF3D_RAD_MODE_MAP) {
        const double inv = 1.0 / cs;
        const int r = int((in.y - RD.yll) * inv);
        const int row = ((int)RD.nRows - 1) - r;
        const int col = int((in.x - RD.xll) * inv);
        if (unsigned(row) >= unsigned(RD.nRows) || unsigned(col) >= unsigned(RD.nCols)) return false;
    }
    return true;
}

}  // namespace

extern "C" {

sf3d_error_t sf3d_transmissivity_window(int year, int month, int day, int hour, int minute, int second, int timeStepSecond,
                                        const sf3d_transmissivity_point_t* point, int32_t* windowSteps)
{
    if (!point || !windowSteps) return SF3D_PARAMETER_ERROR;
    if (timeStepSecond <= 0 || timeStepSecond > 86400 || !trWhenOk(year, month, day, hour, minute, second)) return SF3D_PARAMETER_ERROR;
    if (!RD.on) return SF3D_MEMORY_ERROR;
    const sf3d_rad_settings_t& s = RD.set;
    TrPointDev p;
    if (!trPoint(s, *point, p) || !p.cell.ok) return SF3D_PARAMETER_ERROR;
    RadHourDev hours[TR_WINDOW_SLOTS];
    uint8_t ok[TR_WINDOW_SLOTS];
    /* noon of the date handed in, shifted by -timeZone hours under isUTC (solarRadiation.cpp:871-877) */
    trHour(s, year, month, day, 12, 0, s.isUTC ? -(long)s.timeZone * 3600 : 0, hours[0], ok[0]);
    if (!ok[0]) return SF3D_PARAMETER_ERROR;
    trHour(s, year, month, day, hour, minute, second, hours[1], ok[1]);
    for (int k = 1; k <= (TR_WINDOW_SLOTS - 2) / 2; ++k) {
        trHour(s, year, month, day, hour, minute, second - (long)k * timeStepSecond, hours[2 * k], ok[2 * k]);
        trHour(s, year, month, day, hour, minute, second + (long)k * timeStepSecond, hours[2 * k + 1], ok[2 * k + 1]);
    }
    TrCall call{hours, ok, &p, nullptr, 1u, TR_WINDOW_SLOTS, TR_MODE_WINDOW, s.clearSky};
    return rasterFail("transmissivity window", dev().tr_run(call, nullptr, windowSteps));
}

sf3d_error_t sf3d_transmissivity_points(int year, int month, int day, int hour, int minute, int second, int windowWidth, int timeStepSecond,
                                        uint32_t nPoints, const sf3d_transmissivity_point_t* points, const float* measured,
                                        float* transmissivity, uint32_t* nValid)
{
    if (!nValid || (nPoints && (!points || !measured || !transmissivity))) return SF3D_PARAMETER_ERROR;
    if (windowWidth <= 0 || windowWidth % 2 != 1 || windowWidth > TR_MAX_WIDTH || nPoints > TR_MAX_POINTS) return SF3D_PARAMETER_ERROR;
    if (timeStepSecond <= 0 || timeStepSecond > 86400 || !trWhenOk(year, month, day, hour, minute, second)) return SF3D_PARAMETER_ERROR;
    if (!RD.on) return SF3D_MEMORY_ERROR;
    const sf3d_rad_settings_t& s = RD.set;
    std::vector<TrPointDev> pts(nPoints);
    for (uint32_t k = 0; k < nPoints; ++k)
        if (!trPoint(s, points[k], pts[k])) return SF3D_PARAMETER_ERROR;
    std::vector<RadHourDev> hours((size_t)windowWidth);
    std::vector<uint8_t> ok((size_t)windowWidth);
    const int centre = (windowWidth - 1) / 2;
    for (int i = 0; i < windowWidth; ++i) trHour(s, year, month, day, hour, minute, second + (long)(i - centre) * timeStepSecond, hours[i], ok[i]);
    *nValid = 0;
    TrCall call{hours.data(), ok.data(), pts.data(), measured, nPoints, windowWidth, TR_MODE_POINTS, s.clearSky};
    const sf3d_error_t e = rasterFail("transmissivity points", dev().tr_run(call, transmissivity, nullptr));
    if (e != SF3D_OK) return e;
    for (uint32_t k = 0; k < nPoints; ++k)
        if (!rasterIsFlag(transmissivity[k], -9999.f)) ++*nValid;           /* ! isEqual(transmissivity, NODATA), transmissivity.cpp:164 */
    return SF3D_OK;
}

sf3d_error_t sf3d_transmissivity_get_evaluations(uint32_t nPoints, int windowWidth, uint8_t* written, float* elevationRefr, double* global)
{
    if (!written || !elevationRefr || !global || windowWidth <= 0 || windowWidth > TR_MAX_WIDTH) return SF3D_PARAMETER_ERROR;
    if (!RD.on) return SF3D_MEMORY_ERROR;
    if (!dev().tr_evaluated(nPoints, (uint32_t)windowWidth)) return SF3D_PARAMETER_ERROR;
    return rasterFail("transmissivity get evaluations", dev().tr_evaluations(written, elevationRefr, global));
}

double sf3d_transmissivity_kernel_ms(void) { return dev().tr_kernel_ms(); }

} /* extern "C" */
