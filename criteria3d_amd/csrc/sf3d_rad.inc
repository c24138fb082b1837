/* part of sf3d_solver.hip (included there after the sinks) - the hourly r.sun radiation maps with DEM shadows: what
 * radiation::computeRadiationDEM (agrolib/solarRadiation/solarRadiation.cpp:1045-1069) does for every DEM cell at the half hour, on the
 * device.  k_rad_hour, one thread per cell:
 *   the cell's part of S_solpos (solPos.cpp): lmst and hour angle (:560-577), zen_no_ref (:588-610), ssha (:620-644), tst (:682-701),
 *       srss (:708-722), sazm (:732-756), refrac (:767-806), amass (:816-830), etr (:851-861), tilt (:899-926); sbcf and prime are not
 *       evaluated: nothing of the radiation model reads them;
 *   computeSunPosition's incidence (solarRadiation.cpp:1126-1128), isIlluminated (:538-544), computeShadow (:547-617) - the ray marches
 *       across the DEM in global memory (the Ravone DEM is 2.5 MB and the rays of neighbouring cells run along neighbouring lines: the
 *       cache serves them, there is no LDS tile) - and the radiation arms of computeRadiationRsun (:752-829) with clearSkyBeamHorizontal,
 *       clearSkyDiffuseHorizontal, separateTransmissivity_Erbs_Reindl, getBeamInclined, getDiffuseInclined_Muneer, getReflectedIrradiance.
 * What depends on the date and time only (RadHourDev) or on the cell only (RadCellDev) comes from the host (sf3d_rad_setup.inc).
 *
 * The bar is the compiled reference's bits (tests/golden/rad_rsun.npz): its operations in its order, floats and doubles where it has
 * them, -ffp-contract=off, IEEE division and square root.  exp and the double pow are the C library's (fexp / ppow); acosf and powf are
 * the library's too (sf3d_trig.inc: solPos.cpp hands floats to acos() and pow(), so the object code of the pin build calls the float
 * routines); double sin / cos / tan are faithful routines of this project (sf3d_trig.inc), not the library's: nearly every result is
 * rounded to float at once, where a last-place double difference survives about once in 10^8 - the deviation DESIGN 19 states.  In the
 * object code of the pin build (g++ -O2) pow(airMass, 3), pow(airMass, 4), pow(tanelev, 3) and pow(tanelev, 5) are calls of the double
 * pow; pow(sin(...), 2) of Muneer's Fg is a product.
 *
 * This text also compiles for the host (tests/rad_host.cpp defines SF3D_RAD_HOST, the qualifiers and rad_exp / rad_pow), so that the
 * point function is held against the pin on a CPU before any device runs it.
 *
 * Kept from the reference on purpose:
 *  - by day a cell whose transmissivity is NODATA under realSky, or whose S_solpos range check fails, is not written: all five maps
 *    keep the previous hour's value (computeRadiationRsun returns false); by night the same cell gets four zeros and its sun elevation;
 *  - isIlluminated compares float(localTime.time) with rise / set in seconds; a shaded cell or one with incidence <= 0 has Bh = 0,
 *    Gh = dH; slope == 0 takes the horizontal arm; getReflectedIrradiance gets float(slope) and returns 0 below 1e-6; Muneer's low-sun
 *    arm (elevationRefr < 3) applies with its fmod; the 0.0022 patch of A0 applies; the sun elevation map holds the refracted elevation;
 *  - in map mode getLinke(row, col) / getAlbedo(row, col) (radiationSettings.cpp:124-136, 173-184) read their map only where the cell is
 *    OUT of the grid: every cell inside gets NODATA, which is what RadHourDev carries then.
 *  - with shadowing off the reference never sets TsunPosition::shadow (radiationDefinitions.h:84, solarRadiation.cpp:744-750) and reads
 *    it all the same (:801, 821, 501): in the pin build the stack slot holds a non-zero byte in every cell, so "shadowing off" means
 *    "every cell shaded" there - Bh = 0, Gh = dH, Muneer's shaded arm.  The bar is the compiled reference, so it does here. */

#ifndef SF3D_RAD_HOST
#define SF3D_RAD_FN __device__ __forceinline__
#define SF3D_TR_FN __device__ __forceinline__
#define SF3D_TR_TABLE __device__ const
#define rad_exp(x) fexp(x)
#define rad_pow(x, y) ppow(x, y)
#endif
#include "sf3d_trig.inc"

#define RAD_NODATA (-9999)
#define RAD_RADDEG 0.0174532925              /* solPos.cpp:122 */
#define RAD_DEGRAD 57.295779513              /* solPos.cpp:121 */
#define RAD_DEG_TO_RAD 0.01745329252         /* commonConstants.h:255 */
#define RAD_RAD_TO_DEG 57.295779513          /* commonConstants.h:256 */
#define RAD_PI 3.1415926535898               /* commonConstants.h:249 */
#define RAD_EPSILON 0.00001
#define RAD_TEMPERATURE 10.0f                /* TEMPERATURE_DEFAULT, radiationDefinitions.h:22 */
#define RAD_SHADOW_FACTOR 1.0                /* radiationDefinitions.h:34 */
#define RAD_REALSKY_TOTALTRANSMISSIVITY 0    /* SF3D_RAD_REALSKY_TOTALTRANSMISSIVITY (radiationDefinitions.h:37) */

SF3D_RAD_FN double rad_max(double a, double b) { return (a < b) ? b : a; }                          /* std::max */
SF3D_RAD_FN double rad_clamp(double v, double lo, double hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }   /* std::clamp */

struct RadSun {         /* TsunPosition */
    float rise, set, azimuth, elevationRefr, incidence, relOptAirMassCorr, extraIrradianceNormal, extraIrradianceHorizontal;
};

/* RSUN_compute_solar_position + computeSunPosition for one cell; false: S_solpos refuses the cell */
SF3D_RAD_FN bool rad_sun_position(const RadHourDev& h, const RadCellDev& c, RadSun& s)
{
    if (!c.ok) return false;
    /* geometry(): local mean sidereal time and hour angle */
    float lmst = h.gmst * 15.f + c.lon;
    lmst -= (float)(360.0 * (int)(lmst / 360.0));
    if (lmst < 0.) lmst = (float)(lmst + 360.0);
    float hrang = lmst - h.rascen;
    if (hrang < -180.0) hrang = (float)(hrang + 360.0);
    else if (hrang > 180.0) hrang = (float)(hrang - 360.0);

    /* zen_no_ref() */
    const float ch = (float)sf3d_tr_cos(RAD_RADDEG * hrang);
    float cz = h.sd * c.sl + h.cd * c.cl * ch;
    if (__builtin_fabsf(cz) > 1.0) cz = (cz >= 0.0) ? 1.0f : -1.0f;
    float zenetr = (float)(sf3d_tr_acosf(cz) * RAD_DEGRAD);
    if (zenetr > 99.0) zenetr = 99.0f;
    const float elevetr = 90.f - zenetr;

    /* ssha() */
    float ssha;
    const float cdcl = h.cd * c.cl;
    if (__builtin_fabsf(cdcl) >= 0.001) {
        const float cssha = -c.sl * h.sd / cdcl;
        if (cssha < -1.0) ssha = 180.0f;
        else if (cssha > 1.0) ssha = 0.0f;
        else ssha = (float)(RAD_DEGRAD * sf3d_tr_acosf(cssha));
    } else if ((h.declin >= 0.0 && c.lat > 0.0) || (h.declin < 0.0 && c.lat < 0.0)) ssha = 180.0f;
    else ssha = 0.0f;

    /* tst() */
    const float tst = (180.f + hrang) * 4.f;
    float tstfix = tst - (float)h.hour * 60.f - h.minute - (float)h.second / 60.f + (float)0 / 120.f;
    /* (the reference's two while loops: |hrang| <= 540 and hour < 24 bound tstfix to +-3600, three rounds at the most) */
    for (int k = 0; k < 3 && tstfix > 720.0; ++k) tstfix = (float)(tstfix - 1440.0);
    for (int k = 0; k < 3 && tstfix < -720.0; ++k) tstfix = (float)(tstfix + 1440.0);

    /* srss() */
    float sretr, ssetr;
    if (ssha <= 1.0) { sretr = 2999.0f; ssetr = -2999.0f; }
    else if (ssha >= 179.0) { sretr = -2999.0f; ssetr = 2999.0f; }
    else {
        sretr = (float)(720.0 - 4.0 * ssha - tstfix);
        ssetr = (float)(720.0 + 4.0 * ssha - tstfix);
    }

    /* sazm() */
    const float ce = (float)sf3d_tr_cos(RAD_RADDEG * elevetr);
    const float se = (float)sf3d_tr_sin(RAD_RADDEG * elevetr);
    float azim = 180.0f;
    const float cecl = ce * c.cl;
    if (__builtin_fabsf(cecl) >= 0.001) {
        float ca = (se * c.sl - h.sd) / cecl;
        if (ca > 1.0) ca = 1.0f;
        else if (ca < -1.0) ca = -1.0f;
        azim = 180.f - (float)(sf3d_tr_acosf(ca) * RAD_DEGRAD);
        if (hrang > 0) azim = 360.f - azim;
    }

    /* refrac() */
    double refcor;
    if (elevetr > 85.0) refcor = 0.0;
    else {
        const double tanelev = sf3d_tr_tan(RAD_RADDEG * elevetr);
        if (elevetr >= 5.0) refcor = 58.1 / tanelev - 0.07 / (rad_pow(tanelev, 3.0)) + 0.000086 / (rad_pow(tanelev, 5.0));
        else if (elevetr >= -0.575) refcor = 1735.0 + elevetr * (-518.2 + elevetr * (103.4 + elevetr * (-12.79 + elevetr * 0.711)));
        else refcor = -20.774 / tanelev;
        const double prestemp = (c.press * 283.0) / (1013.0 * (273.0 + RAD_TEMPERATURE));
        refcor *= (float)(prestemp / 3600.0);
    }
    float elevref = (float)(elevetr + refcor);
    if (elevref < -9.0) elevref = -9.0f;
    const float zenref = (float)(90.0 - elevref);
    const double cosZenref = sf3d_tr_cos(RAD_RADDEG * zenref);
    const float coszen = (float)cosZenref;

    /* amass() */
    float ampress;
    if (zenref > 93.0) ampress = -1.0f;
    else {
        const float amass = 1.0f / (float)(cosZenref + 0.50572f * sf3d_tr_powf(96.07995f - zenref, -1.6364f));
        ampress = amass * c.press / 1013.0f;
    }

    /* etr() */
    float etrn, etr;
    if (coszen > 0.0) { etrn = h.etrn; etr = etrn * coszen; }
    else { etrn = 0.0f; etr = 0.0f; }

    /* tilt() */
    const double ca = sf3d_tr_cos(RAD_RADDEG * azim);
    const double sa = sf3d_tr_sin(RAD_RADDEG * azim);
    const double sz = sf3d_tr_sin(RAD_RADDEG * zenref);
    const float cosinc = (float)(coszen * c.ct + sz * c.st * (ca * c.cp + sa * c.sp));

    /* computeSunPosition */
    s.relOptAirMassCorr = ampress;
    s.azimuth = azim;
    s.elevationRefr = elevref;
    s.extraIrradianceHorizontal = etr;
    s.extraIrradianceNormal = etrn;
    s.incidence = (float)rad_max(0., RAD_RAD_TO_DEG * ((RAD_PI / 2.0) - sf3d_tr_acosf(cosinc)));
    s.rise = sretr * 60.f;
    s.set = ssetr * 60.f;
    return true;
}

/* computeShadow, solarRadiation.cpp:547-617.  Every step moves the ray by at least one cell size horizontally (step >= 1), so the
 * reference leaves the grid after at most nrRows + nrCols + 2 steps: the cap keeps a wave out of the loop whatever the input holds */
SF3D_RAD_FN bool rad_shadow(const RadGridDev& g, double x0, double y0, double z0, const RadSun& sun)
{
    const double cellSize = g.cellSize;
    const double sinAz = sf3d_tr_sin(sun.azimuth * RAD_DEG_TO_RAD);
    const double cosAz = sf3d_tr_cos(sun.azimuth * RAD_DEG_TO_RAD);
    const double sinElev = sf3d_tr_sin(sun.elevationRefr * RAD_DEG_TO_RAD);
    const double cosElev = sf3d_tr_cos(sun.elevationRefr * RAD_DEG_TO_RAD);
    const double tgElev = sinElev / rad_max(cosElev, 1e-6);
    const double stepX = RAD_SHADOW_FACTOR * sinAz * cellSize;
    const double stepY = RAD_SHADOW_FACTOR * cosAz * cellSize;
    const double stepZ = RAD_SHADOW_FACTOR * cellSize * tgElev;
    const double maxDeltaH = cellSize * RAD_SHADOW_FACTOR * 2.0;
    double maxDistCount;
    if (__builtin_fabs(stepZ) < 1e-6) maxDistCount = (g.demMax - z0) / RAD_EPSILON;
    else maxDistCount = (g.demMax - z0) / stepZ;
    double stepCount = 0.0;
    double step = 1.0;
    const int cap = g.nRows + g.nCols + 2;
    for (int it = 0; it < cap && stepCount < maxDistCount; ++it) {
        stepCount += step;
        const double x = x0 + stepX * stepCount;
        const double y = y0 + stepY * stepCount;
        const double z = z0 + stepZ * stepCount;
        /* getRowCol, gis.cpp:486-493: int() truncates */
        const int r = (int)((y - g.yll) * g.invCellSize);
        const int row = (g.nRows - 1) - r;
        const int col = (int)((x - g.xll) * g.invCellSize);
        if ((unsigned)row >= (unsigned)g.nRows || (unsigned)col >= (unsigned)g.nCols) return false;       /* out of grid = not shaded */
        const double zDEM = g.dem[(size_t)row * (size_t)g.nCols + (size_t)col];
        if (zDEM != g.flag) {
            if ((zDEM - z) > 0.5) return true;
            step = (z - zDEM) / maxDeltaH;
            if (step < 1.0) step = 1.0;
        }
    }
    return false;
}

/* separateTransmissivity_Erbs_Reindl, solarRadiation.cpp:638-697 */
SF3D_RAD_FN void rad_separate(double clearSkyTransmissivity, double transmissivity, double sunElevationDeg, double sinElevDeg, double& td, double& Tt)
{
    Tt = rad_clamp(transmissivity, 1e-6, clearSkyTransmissivity);
    if (clearSkyTransmissivity <= 1e-6) { td = 0.0; return; }
    double Kt = Tt / clearSkyTransmissivity;
    Kt = rad_clamp(Kt, 0.0, 1.2);
    const double sinElev = rad_max(sinElevDeg, 1e-4);
    double Kd;
    if (Kt <= 0.22) Kd = 1.0 - 0.09 * Kt;
    else if (Kt <= 0.80) Kd = 0.9511 - 0.1604 * Kt + 4.388 * Kt * Kt - 16.638 * Kt * Kt * Kt + 12.336 * Kt * Kt * Kt * Kt;
    else Kd = 0.165;
    double Kd_reindl = Kd;
    if (sunElevationDeg > 0.0) Kd_reindl = Kd + (0.10 + 0.12 * sunElevationDeg / 90.0) * (1.0 - rad_exp(-1.0 / sinElev));
    Kd_reindl = rad_clamp(Kd_reindl, 0.0, 1.0);
    td = Tt * Kd_reindl;
}

/* computeRadiationRsun for a point at (x0, y0, z0) with the terms `c` of its place; false: nothing is written.  march: the shadow ray runs
 * (! gis::isOutOfGridXY, solarRadiation.cpp:748: a cell centre is never out of the grid, a station may be).  elev: the refracted sun
 * elevation; res: global, beam, diffuse, reflected as the doubles of TradPoint.  k_rad_hour (rad_point) and k_transmissivity_points
 * (sf3d_transmissivity.inc) share this text */
SF3D_RAD_FN bool rad_eval(const RadGridDev& g, const RadHourDev& h, const RadCellDev& c, double x0, double y0, double z0, bool march, double transmissivity,
                          float& elev, double res[4])
{
    RadSun sun;
    if (!rad_sun_position(h, c, sun)) return false;

    /* isIlluminated */
    bool lit = false;
    if (sun.rise != RAD_NODATA && sun.set != RAD_NODATA && sun.elevationRefr != RAD_NODATA)
        lit = h.localTime >= sun.rise && h.localTime <= sun.set && sun.elevationRefr > 0;
    bool shadow = true;                             /* never set with shadowing off: see the head of this file */
    if (h.shadowing) {
        shadow = !lit;
        if (lit && march) shadow = rad_shadow(g, x0, y0, z0, sun);
    }
    elev = sun.elevationRefr;
    if (!lit) { res[0] = 0.; res[1] = 0.; res[2] = 0.; res[3] = 0.; return true; }

    if (h.realSky && transmissivity == RAD_NODATA) return false;

    const double linke = h.linke, albedoIn = h.albedo, clearSky = h.clearSky;
    const double elevDeg = sun.elevationRefr;
    const double sinElevRefr = sf3d_tr_sin(sun.elevationRefr * RAD_DEG_TO_RAD);         /* the one argument of :353, 377, 399, 483, 659 */
    double Gh, dH, diffuseTransmittance, globalTransmittance;
    if (h.realSkyAlgorithm == RAD_REALSKY_TOTALTRANSMISSIVITY) {
        if (!h.realSky) transmissivity = clearSky;
        rad_separate(clearSky, transmissivity, elevDeg, sinElevRefr, diffuseTransmittance, globalTransmittance);
        Gh = sun.extraIrradianceHorizontal * transmissivity;
        dH = sun.extraIrradianceHorizontal * diffuseTransmittance;
    } else {
        /* clearSkyBeamHorizontal, :340-357 */
        const double airMass = (double)sun.relOptAirMassCorr;
        double rayleighThickness;
        if (airMass <= 20)
            rayleighThickness = 1. / (6.6296 + 1.7513 * airMass - 0.1202 * airMass * airMass + 0.0065 * rad_pow(airMass, 3.0) - 0.00013 * rad_pow(airMass, 4.0));
        else rayleighThickness = 1. / (10.4 + 0.718 * airMass);
        const double Bhc = (double)sun.extraIrradianceNormal * sinElevRefr * rad_exp(-0.8662 * linke * airMass * rayleighThickness);
        /* clearSkyDiffuseHorizontal, :365-389 */
        double Dhc = 0;
        if (!(sun.elevationRefr <= 1e-3)) {
            double Trd = -0.015843 + linke * (0.030543 + 0.0003797 * linke);
            Trd = rad_max(Trd, 1e-6);
            const double sinElev = rad_max(sinElevRefr, 1e-5);
            double A0 = 0.26463 + linke * (-0.061581 + 0.0031408 * linke);
            if ((A0 * Trd) < 0.0022) A0 = 0.002 / Trd;
            const double A1 = 2.0402 + linke * (0.018945 - 0.011161 * linke);
            const double A2 = -1.3025 + linke * (0.039231 + 0.0085079 * linke);
            const double Fd = A0 + A1 * sinElev + A2 * sinElev * sinElev;
            Dhc = sun.extraIrradianceNormal * Fd * Trd;
        }
        const double Ghc = Dhc + Bhc;
        if (h.realSky) {
            Gh = Ghc * transmissivity / clearSky;
            rad_separate(clearSky, transmissivity, elevDeg, sinElevRefr, diffuseTransmittance, globalTransmittance);
            const double dhsOverGhs = diffuseTransmittance / globalTransmittance;
            dH = dhsOverGhs * Gh;
        } else { Gh = Ghc; dH = Dhc; }
    }

    const bool direct = !shadow && sun.incidence > 0.;
    double Bh;
    if (direct) Bh = Gh - dH;
    else { Bh = 0; Gh = dH; }

    double beam, diffuse, reflected, global;
    if ((double)c.slope == 0) { beam = Bh; diffuse = dH; reflected = 0; global = Gh; }
    else {
        const double sinIncidence = sf3d_tr_sin(sun.incidence * RAD_DEG_TO_RAD);
        /* getBeamInclined, :397-403 */
        if (direct) beam = Bh * (rad_max(sinIncidence, 0.0) / rad_max(sinElevRefr, 1e-6));
        else beam = 0;
        /* getDiffuseInclined_Muneer, :472-524 */
        if (sun.elevationRefr < 1e-6) diffuse = 0.0f;
        else {
            const double aspectRad = (double)c.aspect * RAD_DEG_TO_RAD;
            const double elevationRad = sun.elevationRefr * RAD_DEG_TO_RAD;
            const double sinElev = rad_max(sinElevRefr, 1e-6);
            double Kb = Bh / (sun.extraIrradianceNormal * sinElev);
            Kb = rad_clamp(Kb, 0.0, 1.2);
            const double r_sky = (1.0 + c.cosSlope) / 2.0;
            const double Fg = c.Fg;                 /* sinSlope - slopeRad * cosSlope - PI * sin(slope / 2)^2, from the host */
            double Fx;
            if (shadow || sun.incidence <= 0.1) Fx = r_sky + Fg * 0.252271;
            else {
                const double n = 0.00263 - Kb * (0.712 + 0.6883 * Kb);
                const double termBeam = sinIncidence / sinElev;
                if (!(sun.elevationRefr < 3.0)) Fx = (n * Fg + r_sky) * (1.0 - Kb) + Kb * termBeam;
                else {
                    const double azimuthLocalDiff = __builtin_fmod(sun.azimuth * RAD_DEG_TO_RAD - aspectRad + 2 * RAD_PI, 2 * RAD_PI);
                    const double denom2 = rad_max(0.05, 0.1 - 0.008 * elevationRad);
                    Fx = (n * Fg + r_sky) * (1.0 - Kb) + Kb * c.sinSlope * sf3d_tr_cos(azimuthLocalDiff) / denom2;
                }
            }
            diffuse = dH * Fx;
        }
        /* getReflectedIrradiance(Bh, dH, albedo, float(slope)), :527-535 */
        if ((double)c.slope < 1e-6) reflected = 0.;
        else {
            const double albedo = rad_clamp(albedoIn, 0.0, 1.0);
            reflected = (albedo * (Bh + dH) * c.reflGeom / 2.);
        }
        global = beam + diffuse + reflected;
    }
    res[0] = global; res[1] = beam; res[2] = diffuse; res[3] = reflected;
    return true;
}

/* computeRadiationDemPoint + computeRadiationRsun for the cell (row, col); false: nothing is written.  out: sun elevation (refracted),
 * global, beam, diffuse, reflected as the maps store them */
SF3D_RAD_FN bool rad_point(const RadGridDev& g, const RadHourDev& h, const RadCellDev& c, int row, int col, float transmissivityF, float out[5])
{
    /* Crit3DRasterGrid::getXY, gis.cpp:473-477; the cell centre is never out of the grid */
    const double x0 = g.xll + g.cellSize * ((double)col + 0.5);
    const double y0 = g.yll + g.cellSize * ((double)(g.nRows - row) - 0.5);
    double res[4];
    if (!rad_eval(g, h, c, x0, y0, (double)c.height, true, (double)transmissivityF, out[0], res)) return false;
    out[1] = (float)res[0]; out[2] = (float)res[1]; out[3] = (float)res[2]; out[4] = (float)res[3];
    return true;
}

#ifndef SF3D_RAD_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_rad_hour(RadView v)
{
    fm_init();
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= v.nCells) return;
    if (v.mine && !v.mine[cell]) return;            /* another rank's column: this rank's maps keep the flag there */
    const size_t n = v.nCells;
    RadCellDev c;
    c.height = v.fl[cell];
    if (snow_eqf(c.height, v.grid.flag)) return;    /* computeRadiationDEM: ! isEqual(height, flag) */
    c.lat = v.fl[(RAD_MAP_LAT - RAD_MAP_DEM) * n + cell]; c.lon = v.fl[(RAD_MAP_LON - RAD_MAP_DEM) * n + cell];
    c.cl = v.fl[(RAD_MAP_CL - RAD_MAP_DEM) * n + cell]; c.sl = v.fl[(RAD_MAP_SL - RAD_MAP_DEM) * n + cell];
    c.press = v.fl[(RAD_MAP_PRESS - RAD_MAP_DEM) * n + cell];
    c.slope = v.fl[(RAD_MAP_SLOPE - RAD_MAP_DEM) * n + cell]; c.aspect = v.fl[(RAD_MAP_ASPECT - RAD_MAP_DEM) * n + cell];
    c.cp = v.db[cell]; c.sp = v.db[n + cell]; c.ct = v.db[2 * n + cell]; c.st = v.db[3 * n + cell];
    c.sinSlope = v.db[4 * n + cell]; c.cosSlope = v.db[5 * n + cell]; c.Fg = v.db[6 * n + cell]; c.reflGeom = v.db[7 * n + cell];
    c.ok = v.ok[cell];
    const int row = (int)(cell / (uint32_t)v.grid.nCols), col = (int)(cell - (uint32_t)row * (uint32_t)v.grid.nCols);
    float out[5];
    if (!rad_point(v.grid, v.hour, c, row, col, v.transmissivity[cell], out)) return;
#pragma unroll
    for (int k = 0; k < RAD_OUTPUTS; ++k) v.out[k][cell] = out[k];
}

/* test hook: the routines of sf3d_trig.inc as the device compiles them.  which: 0 sin, 1 cos, 2 tan, 3 acos (doubles); 4 acosf, 5 powf(x, y)
 * (floats, carried in doubles) */
__global__ void k_rad_trig(int which, const double* x, const double* y, double* out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = x[i];
    double r;
    switch (which) {
        case 0: r = sf3d_tr_sin(a); break;
        case 1: r = sf3d_tr_cos(a); break;
        case 2: r = sf3d_tr_tan(a); break;
        case 3: r = sf3d_tr_acos(a); break;
        case 4: r = (double)sf3d_tr_acosf((float)a); break;
        default: r = (double)sf3d_tr_powf((float)a, (float)y[i]); break;
    }
    out[i] = r;
}

sf3d_error_t DeviceSolver::rad_trig(int which, uint32_t n, const double* x, const double* y, double* out)
{
    if (n == 0) return SF3D_OK;
    const sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    DevBuf dx, dy, dz;
    RASTER_TRY(hipMalloc(&dx.p, (size_t)n * 8));
    RASTER_TRY(hipMalloc(&dy.p, (size_t)n * 8));
    RASTER_TRY(hipMalloc(&dz.p, (size_t)n * 8));
    RASTER_TRY(hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
    RASTER_TRY(hipMemcpy(dy.p, y ? y : x, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rad_trig, dim3((n + 255) / 256), dim3(256), 0, 0, which, dx.p, dy.p, dz.p, n);
    RASTER_TRY(hipGetLastError());
    RASTER_TRY(hipMemcpy(out, dz.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return SF3D_OK;
}

/* ---- host side: the outputs, the static maps and the hour's transmissivity in one block; calls go through the shared raster path at the
 * end of sf3d_maps.inc. */
sf3d_error_t DeviceSolver::rad_free()
{
    if (!impl_) return SF3D_OK;
    raster_unbind(FEED_RAD);
    raster_release({impl_->rad.base, impl_->rad.tr});
    impl_->rad = RadCache();
    return SF3D_OK;
}

static size_t rad_block_bytes(size_t n) { return n * (RAD_FLOAT_MAPS * sizeof(float) + RAD_DOUBLE_MAPS * sizeof(double) + sizeof(int32_t)); }

sf3d_error_t DeviceSolver::rad_alloc(const RadSetup& s)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    rad_free();
    Impl& I = *impl_;
    RadCache& K = I.rad;
    const size_t n = (size_t)s.nRows * s.nCols;
    /* the double maps first (8-byte aligned), then the float maps, then `ok` */
    RASTER_TRY(hipMalloc((void**)&K.base, rad_block_bytes(n)));
    K.nCells = (uint32_t)n; K.nRows = s.nRows; K.nCols = s.nCols; K.xll = s.xll; K.yll = s.yll; K.cellSize = s.cellSize; K.flag = s.flag; K.demMax = s.demMax;
    double* db = (double*)K.base;
    float* fl = (float*)(db + (size_t)RAD_DOUBLE_MAPS * n);
    int32_t* ok = (int32_t*)(fl + (size_t)RAD_FLOAT_MAPS * n);
    for (int k = 0; k < RAD_DOUBLE_MAPS; ++k) RASTER_TRY(hipMemcpyAsync(db + (size_t)k * n, s.db[k], n * sizeof(double), hipMemcpyHostToDevice, I.stream));
    for (int k = 0; k < RAD_MAP_TRANSMISSIVITY - RAD_MAP_DEM; ++k)
        RASTER_TRY(hipMemcpyAsync(fl + (size_t)(RAD_MAP_DEM + k) * n, s.fl[k], n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(ok, s.ok, n * sizeof(int32_t), hipMemcpyHostToDevice, I.stream));
    /* initializeGrid(dem): the five outputs hold the flag until an hour writes them; so does the transmissivity copy */
    const std::vector<float> empty((size_t)RAD_OUTPUTS * n, s.flag);
    e = raster_upload(fl + (size_t)RAD_MAP_OUT * n, empty.data(), empty.size() * sizeof(float));
    if (e != SF3D_OK) return e;
    return raster_upload(fl + (size_t)RAD_MAP_TRANSMISSIVITY * n, empty.data(), n * sizeof(float));
}

/* transmissivity == nullptr: the map the meteo block holds (the caller has checked meteo_has) */
sf3d_error_t DeviceSolver::rad_hour(const RadHourDev& hour, const float* transmissivity, const uint8_t* mine)
{
    Impl& I = *impl_;
    RadCache& K = I.rad;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    double* db = (double*)K.base;
    float* fl = (float*)(db + (size_t)RAD_DOUBLE_MAPS * n);
    RadView v{};
    if (transmissivity) {
        RASTER_TRY(hipMemcpyAsync(fl + (size_t)RAD_MAP_TRANSMISSIVITY * n, transmissivity, n * sizeof(float), hipMemcpyHostToDevice, I.stream));
        v.transmissivity = fl + (size_t)RAD_MAP_TRANSMISSIVITY * n;
    } else v.transmissivity = meteo_map(I.meteo, METEO_ATM_TRANSMISSIVITY);
    const sf3d_error_t e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    for (int k = 0; k < RAD_OUTPUTS; ++k) v.out[k] = fl + (size_t)(RAD_MAP_OUT + k) * n;
    v.fl = fl + (size_t)RAD_MAP_DEM * n;
    v.db = db;
    v.ok = (const int32_t*)(fl + (size_t)RAD_FLOAT_MAPS * n);
    v.grid.dem = v.fl;
    v.grid.xll = K.xll; v.grid.yll = K.yll; v.grid.cellSize = K.cellSize; v.grid.invCellSize = 1.0 / K.cellSize;
    v.grid.nRows = (int32_t)K.nRows; v.grid.nCols = (int32_t)K.nCols; v.grid.flag = K.flag; v.grid.demMax = K.demMax;
    v.hour = hour;
    v.nCells = K.nCells;
    const sf3d_error_t el = raster_launch(k_rad_hour, n, v, K.lastMs);
    if (el == SF3D_OK) { K.hourDone = true; K.trRead = v.transmissivity; K.trFromMeteo = !transmissivity; }
    return el;
}

/* ---- what the other blocks read from this one (sf3d_hour.inc), once rad_hour_done says an hour has run on their raster and the
 * transmissivity map it read is still there: the global and beam maps, and that transmissivity map - this block's copy, or the meteo
 * block's map when the hour was called with none */
bool DeviceSolver::rad_hour_done(uint32_t nRows, uint32_t nCols) const
{
    return impl_ && impl_->rad.base && impl_->rad.hourDone && impl_->rad.trRead && impl_->rad.nRows == nRows && impl_->rad.nCols == nCols;
}
static const float* rad_output(const RadCache& K, int which)
{
    return (const float*)((const double*)K.base + (size_t)RAD_DOUBLE_MAPS * K.nCells) + (size_t)(RAD_MAP_OUT + which) * K.nCells;
}
static const float* rad_global(const RadCache& K) { return rad_output(K, 1); }              /* SF3D_RAD_GLOBAL */
static const float* rad_beam(const RadCache& K) { return rad_output(K, 2); }                /* SF3D_RAD_BEAM */
static const float* rad_transmissivity_read(const RadCache& K) { return K.trRead; }

sf3d_error_t DeviceSolver::rad_download(int which, float* dst)
{
    const RadCache& K = impl_->rad;
    const float* fl = (const float*)((const double*)K.base + (size_t)RAD_DOUBLE_MAPS * K.nCells);
    return raster_download(dst, fl + (size_t)(RAD_MAP_OUT + which) * K.nCells, (size_t)K.nCells * sizeof(float));
}

double DeviceSolver::rad_kernel_ms() const { return impl_ ? impl_->rad.lastMs : 0.; }
#endif
