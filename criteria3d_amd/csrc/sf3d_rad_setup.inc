/* sf3d_rad_setup.inc - the host side of the radiation block's bits (included by sf3d_rad_api.inc and by tests/rad_host.cpp): what
 * S_solpos and computeRadiationRsun evaluate from the date and time only (once per call) and from the cell only (once per raster), with
 * the C library the reference calls, in its types and its order.  The results travel to the device as RadHourDev and as static maps
 * (RadCellDev), so they are the reference's bits by construction and the kernel needs no asin, atan2 or pressure formula. */
#include <cmath>

#define RADS_RADDEG 0.0174532925             /* solPos.cpp:122 */
#define RADS_DEGRAD 57.295779513             /* solPos.cpp:121 */
#define RADS_DEG_TO_RAD 0.01745329252        /* commonConstants.h:255 */
#define RADS_PI 3.1415926535898              /* commonConstants.h:249 */
#define RADS_NODATA (-9999)

static inline bool radsLeap(int y) { return (y % 4 == 0) && ((y % 100 != 0) || (y % 400 == 0)); }
static inline int radsMonthDays(int y, int m)
{
    static const int days[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return (m == 2 && radsLeap(y)) ? 29 : days[m - 1];
}

/* the cell's part of computeRadiationDemPoint / computeRadiationRsun / S_solpos (solarRadiation.cpp:734, 479-496, 534; solPos.cpp:327-344,
 * 886-890, 912-917).  slope and aspect: the maps' values (TILT_TYPE_DEM) or the fixed ones */
static inline RadCellDev radsCellAt(double h, float lat, float lon, float slope, float aspect)
{
    RadCellDev c;
    c.height = float(h); c.lat = lat; c.lon = lon; c.slope = slope; c.aspect = aspect;
    c.cl = float(std::cos(RADS_RADDEG * lat));
    c.sl = float(std::sin(RADS_RADDEG * lat));
    /* pressureFromAltitude(height) * 0.01, physics.cpp:39-47: the height is a double (a raster cell's is double(float), a station's its own) */
    const double pressure = 101325. * std::pow(1 + h * 0.0065 / 293.16, -9.80665 / (0.0065 * 287.058)) * 0.01;
    c.press = float(pressure);
    c.cp = std::cos(RADS_RADDEG * aspect);
    c.ct = std::cos(RADS_RADDEG * slope);
    c.sp = std::sin(RADS_RADDEG * aspect);
    c.st = std::sin(RADS_RADDEG * slope);
    const double slopeD = slope;
    const double slopeRad = slopeD * RADS_DEG_TO_RAD;
    c.sinSlope = std::sin(slopeRad);
    c.cosSlope = std::cos(slopeRad);
    const double half = std::sin(slopeD * 0.5 * RADS_DEG_TO_RAD);
    c.Fg = c.sinSlope - slopeRad * c.cosSlope - RADS_PI * (half * half);          /* pow(x, 2) is x * x in the object code of the pin build */
    c.reflGeom = 1. - std::cos(slopeD * RADS_DEG_TO_RAD);
    /* validate(): temperature is TEMPERATURE_DEFAULT, the shadow band is SBWID / SBRAD / SBSKY - always in range */
    bool bad = std::fabs(lon) > 180.f || std::fabs(lat) > 90.f;
    bad = bad || c.press < 0.0 || c.press > 2000.0;
    bad = bad || std::fabs(slope) > 180.0 || std::fabs(aspect) > 360.0;
    c.ok = bad ? 0 : 1;
    return c;
}
static inline RadCellDev radsCell(float height, float lat, float lon, float slope, float aspect) { return radsCellAt(height, lat, lon, slope, aspect); }

/* the call's part: the local-time shift of solarRadiation.cpp:714-726 (Crit3DTime::addSeconds, crit3dTime.cpp:145-165), validate(),
 * dom2doy() and the date-and-time part of geometry() (solPos.cpp:293-331, 373-382, 426-555), localtrig()'s declination terms and etrn.
 * false: S_solpos refuses the date or the time zone */
static inline bool radsHour(int year, int month, int day, int hour, int minute, int second, int timeZone, bool isUTC, RadHourDev& o)
{
    long t = (long)hour * 3600 + (long)minute * 60 + second;
    if (isUTC) t += (long)timeZone * 3600;
    while (!(t >= 0 && t < 86400)) {
        if (t >= 86400) {
            t -= 86400;
            if (++day > radsMonthDays(year, month)) { day = 1; if (++month > 12) { month = 1; ++year; } }
        } else {
            t += 86400;
            if (--day < 1) { if (--month < 1) { month = 12; --year; } day = radsMonthDays(year, month); }
        }
    }
    o.hour = int(t / 3600);
    o.minute = int((t - o.hour * 3600) / 60);
    o.second = int(t - o.hour * 3600 - o.minute * 60);
    o.localTime = float(int(t));
    o.timezone = float(timeZone);
    if (year < 1950 || year > 2100 || month < 1 || month > 12 || day < 1 || day > 31) return false;
    if (std::fabs(o.timezone) > 12.f) return false;
    static const int monthDays[13] = {0, 0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334};
    int daynum = day + monthDays[month];
    if (radsLeap(year) && month > 2) daynum += 1;

    const int interval = 0;
    const float dayang = float(360.0 * (daynum - 1) / 365.0);
    const double sd = std::sin(RADS_RADDEG * dayang);
    const double cd = std::cos(RADS_RADDEG * dayang);
    const double d2 = 2.0 * dayang;
    const double c2 = std::cos(RADS_RADDEG * d2);
    const double s2 = std::sin(RADS_RADDEG * d2);
    float erv = float(1.000110 + 0.034221 * cd + 0.001280 * sd);
    erv += float(0.000719 * c2 + 0.000077 * s2);
    float utime = float(o.hour * 3600.0 + o.minute * 60.0 + o.second - interval / 2.0);
    utime = float(utime / 3600.0 - o.timezone);
    const double delta = (float)(year - 1949);
    const int leap = (int)(delta / 4.0);
    const float julday = float(32916.5 + delta * 365.0 + leap + daynum + utime / 24.0);
    const float ectime = float(julday - 51545.0);
    float mnlong = float(280.460 + 0.9856474 * ectime);
    mnlong -= float(360.0 * (int)(mnlong / 360.0));
    if (mnlong < 0.0) mnlong += 360.0;
    float mnanom = float(357.528 + 0.9856003 * ectime);
    mnanom -= float(360.0 * (int)(mnanom / 360.0));
    if (mnanom < 0.0) mnanom += 360.0;
    float eclong = float(mnlong + 1.915 * std::sin(mnanom * RADS_RADDEG) + 0.020 * std::sin(2.0 * mnanom * RADS_RADDEG));
    eclong -= float(360.0 * (int)(eclong / 360.0));
    if (eclong < 0.0) eclong += 360.0;
    const float ecobli = float(23.439 - 4.0e-07 * ectime);
    o.declin = float(RADS_DEGRAD * std::asin(std::sin(ecobli * RADS_RADDEG) * std::sin(eclong * RADS_RADDEG)));
    const double top = std::cos(RADS_RADDEG * ecobli) * std::sin(RADS_RADDEG * eclong);
    const double bottom = std::cos(RADS_RADDEG * eclong);
    o.rascen = float(RADS_DEGRAD * std::atan2(top, bottom));
    if (o.rascen < 0.0) o.rascen += 360.0;
    float gmst = 6.697375f + 0.0657098242f * ectime + utime;
    gmst -= float(24.0 * (int)(gmst / 24.0));
    if (gmst < 0.0) gmst += 24.0;
    o.gmst = gmst;
    o.erv = erv;
    o.cd = float(std::cos(RADS_RADDEG * o.declin));
    o.sd = float(std::sin(RADS_RADDEG * o.declin));
    o.etrn = 1367.0f * erv;
    return true;
}
