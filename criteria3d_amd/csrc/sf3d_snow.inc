/* part of sf3d_solver.hip (included there after the output maps) - the hourly snow model of the application on the device:
 * Crit3DProject::computeSnowModel / computeSnowPoint (bin/CRITERIA3D/criteria3DProject.cpp:1792-1878) over
 * Crit3DSnow::computeSnowBrooksModel (src/snow/snow.cpp:142-525) and the maps of Crit3DSnowMaps (snowMaps.cpp:111-174), plus the liquid
 * water assignPrecipitation (:939-953) hands to the solver.  One thread per raster cell, one launch per hour: the cells of a row are
 * neighbouring lanes, so every map is read and written as consecutive floats.  No neighbours, no reduction.
 *
 * The bar is the compiled reference's bits (tests/golden/snow_brooks.npz): the same double operations in the same order
 * (-ffp-contract=off), floats widened where the reference widens them and the state rounded to float every hour as its maps do.
 * exp / log / pow are the C library's (sf3d_glibcmath.inc through fexp / flog / ppow).  In the object code of the pin build (g++ -O2)
 * all three pow of the model - pow(T + 273.15, 4.0) twice and pow(age, -0.191) - are calls of the library's pow (gcc folds pow(x, 2)
 * only), so they are ppow here.
 *
 * Kept from the reference on purpose:
 *  - snow.cpp:482 reads `snowWaterEquivalent` (no underscore): the meteoVariable enumerator of that name (agrolib/meteo/meteo.h:103, value
 *    56 in the compiled reference), not the state - snowRatio is min(0.056, skinThickness) / snowSurfaceDampingDepth;
 *  - an invalid or free-water cell gets NODATA everywhere except its internal energy (not reset there: the map keeps its value) and its
 *    snowmelt (getSnowMelt is MAXVALUE(_snowMelt, 0): 0);
 *  - NODATA comparisons are isEqual (|a - b| < EPSILON), except the age test of snow.cpp:500 (==).
 * The application reuses one Crit3DSnow object across the cells of a thread (firstprivate): setPoint / setSnowInputData overwrite the
 * seven state members and the nine inputs, and every output member is written before it is read (computeSnowFall: _precSnow, _precRain;
 * the others are assigned, never accumulated), so nothing carries over from cell to cell.
 * The per-cell text compiles for the host too (tests/snow_host.cpp defines SF3D_SNOW_HOST; snow_eq / snow_eqf also serve the host builds
 * of sf3d_crop.inc, sf3d_root.inc and sf3d_sink.inc). */

#ifndef SF3D_SNOW_HOST
#define SF3D_SNOW_FN __device__ __forceinline__
#endif

#define SNOW_NODATA (-9999.0)
#define SNOW_EPSILON 0.00001                 /* commonConstants.h:252 */
#define SNOW_EMISSIVITY 0.97                 /* snow.h */
#define SOIL_EMISSIVITY 0.92
#define THERMO_WATER_VAPOR 0.4615
#define LATENT_HEAT_FUSION_KJ 335.
#define LATENT_HEAT_VAPORIZATION_KJ 2500.
#define SNOW_SPECIFIC_HEAT 2.1
#define SOIL_SPECIFIC_HEAT 1.4
#define DEFAULT_BULK_DENSITY 1350
#define SOIL_DAMPING_DEPTH 0.3
#define SNOW_MINIMUM_HEIGHT 1.
#define SNOW_WATER_DENSITY 1000.             /* commonConstants.h */
#define SNOW_ZEROCELSIUS 273.15
#define SNOW_STEFAN_BOLTZMANN 5.670373E-8
#define SNOW_VON_KARMAN_CONST 0.41
#define SNOW_HEAT_CAPACITY_WATER 4182000.
#define SNOW_HEAT_CAPACITY_AIR 1290.
#define SNOW_HEAT_CAPACITY_SNOW 2100000.
#define SNOW_SWE_ENUM 56                     /* meteoVariable snowWaterEquivalent */

SF3D_SNOW_FN bool snow_eq(double a, double b) { return __builtin_fabs(a - b) < SNOW_EPSILON; }               /* isEqual(double, double) */
SF3D_SNOW_FN bool snow_eqf(float a, float b) { return __builtin_fabs((double)a - (double)b) < SNOW_EPSILON; }   /* isEqual(float, float) */

/* tDewFromRelHum(double, double), agrolib/meteo/meteo.cpp:288-298 */
SF3D_SNOW_FN double snow_tdew(double RH, double T)
{
    if (snow_eq(RH, SNOW_NODATA) || snow_eq(T, SNOW_NODATA) || RH == 0) return SNOW_NODATA;
    RH = (100 < RH) ? 100 : RH;
    const double mySaturatedVaporPres = fexp((16.78 * T - 116.9) / (T + 237.3));
    const double actualVaporPres = RH / 100. * mySaturatedVaporPres;
    const double l = flog(actualVaporPres);
    return (l * 237.3 + 116.9) / (16.78 - l);
}

/* aerodynamicResistanceCampbell77(isSnow, 10, windSpeed, vegetativeHeight), snow.cpp:527-557 */
SF3D_SNOW_FN double snow_resistance(bool isSnow, double windSpeed, double vegetativeHeight)
{
    const double zRefWind = 10, zRefTemp = 2;
    windSpeed = dmax(windSpeed, 0.05);
    windSpeed = dmin(windSpeed, 10.);
    vegetativeHeight = dmax(vegetativeHeight, 0.01);
    const double zeroPlane = isSnow ? 0 : 0.64 * vegetativeHeight;
    const double momentumRoughness = isSnow ? 0.001 : 0.13 * vegetativeHeight;
    const double a = zRefWind - zeroPlane, b = zRefTemp - zeroPlane;
    const double log1 = flog(((a > 1.0 ? a : 1.0) + momentumRoughness) / momentumRoughness);
    const double heatVaporRoughness = 0.2 * momentumRoughness;
    const double log2 = flog(((b > 1.0 ? b : 1.0) + heatVaporRoughness) / heatVaporRoughness);
    return log1 * log2 / (SNOW_VON_KARMAN_CONST * SNOW_VON_KARMAN_CONST * windSpeed);
}

/* one cell of the hour */
SF3D_SNOW_FN void snow_cell(const SnowView& v, uint32_t c)
{
    const float flag = v.flag;
    if (v.mine && !v.mine[c]) {                 /* another rank's column: its state stays, the outputs say "not here" */
        for (int k = 0; k < 6; ++k) v.out[k][c] = flag;
        return;
    }
    if (snow_eqf(v.dem[c], flag)) {             /* flagMapRowCol */
        for (int k = 0; k < 7; ++k) v.st[k][c] = flag;
        for (int k = 0; k < 6; ++k) v.out[k][c] = flag;
        return;
    }
    const SnowParamsDev& P = v.p;
    /* setPoint, computeSnowPoint: floats widened to double */
    double swe = v.st[0][c], ice = v.st[1][c], lwc = v.st[2][c], internalEnergy = v.st[3][c], surfaceEnergy = v.st[4][c];
    double surfaceTemp = v.st[5][c], ageOfSnow = v.st[6][c];
    const float precF = v.in[1][c];
    const double airT = v.in[0][c], prec = precF, airRH = v.in[2][c], windInt = v.in[3][c], globalRadiation = v.in[4][c];
    const double beamRadiation = v.in[5][c], transmissivity = v.in[6][c];
    const double surfaceWaterContent = dmax(v.in[7] ? (double)v.in[7][c] : 0., 0.0);

    double precSnow, snowMelt, deltaSWE, sensibleHeat, latentHeat;
    const bool valid = !(snow_eq(airT, SNOW_NODATA) || snow_eq(prec, SNOW_NODATA) || snow_eq(globalRadiation, SNOW_NODATA)
                         || snow_eq(beamRadiation, SNOW_NODATA) || snow_eq(swe, SNOW_NODATA) || snow_eq(surfaceTemp, SNOW_NODATA));
    if (surfaceWaterContent > 100. || !valid) {
        ice = lwc = swe = surfaceEnergy = surfaceTemp = ageOfSnow = SNOW_NODATA;
        precSnow = deltaSWE = sensibleHeat = latentHeat = SNOW_NODATA;
        snowMelt = 0;                            /* getSnowMelt: MAXVALUE(NODATA, 0) */
    } else {
        /* computeSnowFall */
        double liquidWater = prec;
        if (liquidWater > 0) {
            if (airT <= P.tempMinWithRain) liquidWater = 0;
            else if (airT < P.tempMaxWithSnow) liquidWater *= (airT - P.tempMinWithRain) / (P.tempMaxWithSnow - P.tempMinWithRain);
        }
        const double dPrec = prec - liquidWater;
        precSnow = (dPrec > 0) ? dPrec : 0;
        const double precRain = liquidWater;

        const double dewPoint = snow_tdew(airRH, airT);
        double cloudCover;
        if (!snow_eq(transmissivity, SNOW_NODATA)) cloudCover = 1 - dmin(transmissivity / P.clearSky, 1.);
        else cloudCover = 0.1;

        const double maxSnowDensity = 10, maxVegetationHeight = 4;
        const double maxSnowHeight = swe * maxSnowDensity / 1000;
        const double heightVegetation = P.snowVegetationHeight - maxSnowHeight;
        const double vegetationShadowing = dmax(dmin(heightVegetation / maxVegetationHeight, 1.), 0.);
        const double solarRadTot = globalRadiation - beamRadiation * vegetationShadowing;

        const double previousSWE = swe;
        double prevInternalEnergy = internalEnergy, prevSurfaceEnergy = surfaceEnergy, prevSurfaceTemp = surfaceTemp;
        double prevIceContent = ice, prevLWaterContent = lwc;
        if (previousSWE > 0) {
            if (prevIceContent <= 0 && prevLWaterContent <= 0) {            /* a hand-edited SWE map */
                prevIceContent = previousSWE;
                prevLWaterContent = previousSWE * P.snowWaterHoldingCapacity / (1 - P.snowWaterHoldingCapacity);
                prevInternalEnergy = -previousSWE * 0.001 * LATENT_HEAT_FUSION_KJ * SNOW_WATER_DENSITY;
                prevSurfaceTemp = dmin(prevSurfaceTemp, 0.);
                prevSurfaceEnergy = prevSurfaceTemp * SNOW_WATER_DENSITY * SNOW_SPECIFIC_HEAT * dmin(previousSWE, P.skinThickness);
                ageOfSnow = 1;
            }
            const double currentRatio = previousSWE / (prevIceContent + prevLWaterContent);
            if (!snow_eq(currentRatio, 1)) {
                prevIceContent = prevIceContent * currentRatio;
                prevLWaterContent = prevLWaterContent * currentRatio;
            }
        } else {
            prevIceContent = 0;
            prevLWaterContent = 0;
            ageOfSnow = SNOW_NODATA;
        }

        if (previousSWE < SNOW_EPSILON) {                                       /* soil internal energy check */
            double estInternalEnergy = prevSurfaceTemp * DEFAULT_BULK_DENSITY * SOIL_SPECIFIC_HEAT * SOIL_DAMPING_DEPTH;
            const double absDifference = __builtin_fabs(estInternalEnergy - prevInternalEnergy);
            if (absDifference > 1000) {
                if (snow_eq(estInternalEnergy, 0)) estInternalEnergy = SNOW_EPSILON;
                const double ratio = prevInternalEnergy / estInternalEnergy;
                if ((ratio < 0.5) || (ratio > 2)) prevInternalEnergy = (prevInternalEnergy + estInternalEnergy) * 0.5;
            }
        }

        const double aerodynamicResistance = snow_resistance(previousSWE > SNOW_MINIMUM_HEIGHT, windInt, P.snowVegetationHeight);

        const double airActualVapDensity = fexp((16.78 * dewPoint - 116.9) / (dewPoint + 237.3)) / ((SNOW_ZEROCELSIUS + dewPoint) * THERMO_WATER_VAPOR);
        const double waterActualVapDensity = fexp((16.78 * prevSurfaceTemp - 116.9) / (prevSurfaceTemp + 237.3))
                                             / ((SNOW_ZEROCELSIUS + prevSurfaceTemp) * THERMO_WATER_VAPOR);

        const double longWaveAtmEmissivity = (0.72 + 0.005 * airT) * (1.0 - 0.84 * cloudCover) + 0.84 * cloudCover;

        double albedo;
        if (!snow_eq(ageOfSnow, SNOW_NODATA)) albedo = dmin(0.9, 0.74 * ppow(ageOfSnow, -0.191));
        else albedo = P.soilAlbedo;

        const double QPrecipW = (SNOW_HEAT_CAPACITY_WATER / 1000.) * (precRain / 1000.) * (dmax(0., airT) - prevSurfaceTemp);
        const double QPrecipS = (SNOW_HEAT_CAPACITY_SNOW / 1000.) * (precSnow / 1000.) * (dmin(0., airT) - prevSurfaceTemp);
        const double QPrecip = QPrecipW + QPrecipS;
        const double QWaterHeat = (SNOW_HEAT_CAPACITY_WATER / 1000.) * (surfaceWaterContent / 1000.)
                                  * (dmax(1., (prevSurfaceTemp + airT) / 2.) - prevSurfaceTemp);
        const double QWaterKinetic = 0;
        const double QSolar = (1. - albedo) * (solarRadTot * 3600.) / 1000.;
        const double surfaceEmissivity = (previousSWE > SNOW_MINIMUM_HEIGHT) ? SNOW_EMISSIVITY : SOIL_EMISSIVITY;
        const double QLongWave = SNOW_STEFAN_BOLTZMANN * 3.6 * (longWaveAtmEmissivity * ppow(airT + SNOW_ZEROCELSIUS, 4.0)
                                 - surfaceEmissivity * ppow(prevSurfaceTemp + SNOW_ZEROCELSIUS, 4.0));
        const double QTempGradient = 3600. * (SNOW_HEAT_CAPACITY_AIR / 1000.) * (airT - prevSurfaceTemp) / aerodynamicResistance;
        double QVaporGradient = 3600. * (LATENT_HEAT_VAPORIZATION_KJ + LATENT_HEAT_FUSION_KJ)
                                * (airActualVapDensity - waterActualVapDensity) / aerodynamicResistance;
        if (previousSWE < SNOW_EPSILON) QVaporGradient *= 0.4;

        const double QTotal = QSolar + QPrecip + QLongWave + QTempGradient + QVaporGradient + QWaterHeat + QWaterKinetic;
        sensibleHeat = QTempGradient;
        latentHeat = QVaporGradient;

        double sublimation = 0;
        if (previousSWE > SNOW_EPSILON) {
            sublimation = QVaporGradient / (LATENT_HEAT_FUSION_KJ + LATENT_HEAT_VAPORIZATION_KJ);
            if (sublimation < 0) sublimation = -dmin(__builtin_fabs(sublimation), previousSWE + precSnow);
        }

        double freeze_melt = 0;
        const double w = (prevInternalEnergy + QTotal) / (LATENT_HEAT_FUSION_KJ * SNOW_WATER_DENSITY);
        if (w < 0) {
            if (prevSurfaceTemp <= 0) freeze_melt = dmin(prevLWaterContent + precRain, -w * 1000.);
        } else if (w > 0) {
            freeze_melt = -dmin(prevIceContent + precSnow + sublimation, w * 1000.);
        }
        snowMelt = -freeze_melt;
        const double Qr = (freeze_melt / 1000.) * LATENT_HEAT_FUSION_KJ * SNOW_WATER_DENSITY;
        internalEnergy = prevInternalEnergy + QTotal + Qr;

        if (internalEnergy > SNOW_EPSILON) ice = 0;
        else {
            ice = prevIceContent + precSnow + sublimation + freeze_melt;
            ice = dmax(ice, 0.);
        }
        const double waterHoldingCapacity = P.snowWaterHoldingCapacity / (1 - P.snowWaterHoldingCapacity);
        if (internalEnergy > SNOW_EPSILON) lwc = 0;
        else {
            lwc = prevLWaterContent + precRain + surfaceWaterContent - freeze_melt;
            lwc = dmax(lwc, 0.);
            lwc = dmin(lwc, ice * waterHoldingCapacity);
        }
        swe = ice + lwc;
        deltaSWE = swe - previousSWE;

        double surfaceEnergySnow;
        if (swe > 0 && __builtin_fabs(internalEnergy) < SNOW_EPSILON) surfaceEnergySnow = 0.;
        else {
            const double snowRatio = dmin(SNOW_SWE_ENUM * 0.001, P.skinThickness) / P.snowSurfaceDampingDepth;      /* see the head of this file */
            surfaceEnergySnow = dmin(0., prevSurfaceEnergy + (QTotal + Qr) * snowRatio);
        }
        const double surfaceTempSnow = surfaceEnergySnow / (SNOW_WATER_DENSITY * SNOW_SPECIFIC_HEAT * P.skinThickness);
        const double surfaceEnergySoil = prevSurfaceEnergy + (QTotal + Qr) * (P.skinThickness / SOIL_DAMPING_DEPTH);
        const double surfaceTempSoil = surfaceEnergySoil / (DEFAULT_BULK_DENSITY * SOIL_SPECIFIC_HEAT * P.skinThickness);
        const double snowDepthRatio = 4.;
        const double snowFraction = dmin(swe * snowDepthRatio / 1000., P.skinThickness) / P.skinThickness;
        surfaceEnergy = (surfaceEnergySnow * snowFraction) + surfaceEnergySoil * (1 - snowFraction);
        surfaceTemp = (surfaceTempSnow * snowFraction) + surfaceTempSoil * (1 - snowFraction);

        if (swe > SNOW_EPSILON) {
            if (ageOfSnow == SNOW_NODATA || precSnow > 0.1) ageOfSnow = 0;
            else { const double oneHour = 1. / 24.; ageOfSnow += oneHour; }
        } else ageOfSnow = SNOW_NODATA;
        snowMelt = (snowMelt > 0) ? snowMelt : 0;        /* getSnowMelt */
    }

    /* updateMapRowCol: rounded to float */
    const float fall = (float)precSnow, melt = (float)snowMelt;
    v.st[0][c] = (float)swe; v.st[1][c] = (float)ice; v.st[2][c] = (float)lwc; v.st[3][c] = (float)internalEnergy;
    v.st[4][c] = (float)surfaceEnergy; v.st[5][c] = (float)surfaceTemp; v.st[6][c] = (float)ageOfSnow;
    v.out[0][c] = fall; v.out[1][c] = melt; v.out[2][c] = (float)deltaSWE; v.out[3][c] = (float)sensibleHeat; v.out[4][c] = (float)latentHeat;
    /* assignPrecipitation:939-953, in float */
    float liquid = flag;
    if (!snow_eqf(precF, flag)) {
        liquid = precF;
        if (!snow_eqf(fall, flag) && !snow_eqf(melt, flag)) liquid = precF - fall + melt;
    }
    v.out[5][c] = liquid;
}

#ifndef SF3D_SNOW_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_snow_hour(SnowView v)
{
    fm_init();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    snow_cell(v, c);
}

/* ---- host side: the maps live in one device block of SNOW_MAPS x nCells floats; a call uploads, launches on the solver's stream, and
 * copies back only what it is asked for (the shared raster path at the end of sf3d_maps.inc). */
sf3d_error_t DeviceSolver::snow_free()
{
    if (!impl_) return SF3D_OK;
    raster_unbind(FEED_SNOW);
    raster_release({impl_->snow.base});
    impl_->snow = SnowCache();
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::snow_alloc(uint32_t nCells)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    snow_free();
    SnowCache& S = impl_->snow;
    RASTER_TRY(hipMalloc((void**)&S.base, (size_t)SNOW_MAPS * nCells * sizeof(float)));
    S.nCells = nCells;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::snow_upload(int map, const float* src)
{
    const SnowCache& S = impl_->snow;
    return raster_upload(S.base + (size_t)map * S.nCells, src, (size_t)S.nCells * sizeof(float));
}

sf3d_error_t DeviceSolver::snow_download(int map, float* dst)
{
    const SnowCache& S = impl_->snow;
    return raster_download(dst, S.base + (size_t)map * S.nCells, (size_t)S.nCells * sizeof(float));
}

sf3d_error_t DeviceSolver::snow_hour(const float* const in[8], const SnowParamsDev& p, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    SnowCache& S = I.snow;
    const size_t n = S.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    for (int k = 0; k < 8; ++k)
        if (in[k]) RASTER_TRY(hipMemcpyAsync(S.base + (size_t)(SNOW_MAP_IN + k) * n, in[k], n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    const float* d[8];
    for (int k = 0; k < 8; ++k) d[k] = in[k] ? S.base + (size_t)(SNOW_MAP_IN + k) * n : nullptr;
    return snow_launch(d, 0, p, flag, mine);
}

/* the hour on eight input maps that are on the device: slots of this block (snow_hour) or maps of the FEED_* blocks in `feeds`
 * (hour_snow, sf3d_hour.inc); in[7], the surface water, may be null */
sf3d_error_t DeviceSolver::snow_launch(const float* const in[8], int feeds, const SnowParamsDev& p, float flag, const uint8_t* mine)
{
    SnowCache& S = impl_->snow;
    const size_t n = S.nCells;
    SnowView v{};
    const sf3d_error_t e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    for (int k = 0; k < 7; ++k) v.st[k] = S.base + (size_t)(SNOW_MAP_STATE + k) * n;
    for (int k = 0; k < 6; ++k) v.out[k] = S.base + (size_t)(SNOW_MAP_OUT + k) * n;
    for (int k = 0; k < 8; ++k) v.in[k] = in[k];
    v.dem = S.base + (size_t)SNOW_MAP_DEM * n;
    v.nCells = S.nCells; v.flag = flag; v.p = p;
    const sf3d_error_t el = raster_launch(k_snow_hour, n, v, S.lastMs);
    if (el == SF3D_OK) {                                   /* the input maps of this hour stay where they are (sf3d_crop_compute_hour may read them) */
        S.hourDone = true;
        for (int k = 0; k < 8; ++k) S.in[k] = in[k];
        S.feeds = feeds; S.inputsHeld = true;
    }
    return el;
}

/* ---- what the other blocks read from this one, once an hour has run on their raster */
enum { SNOW_OUT_LIQUID_WATER = 5 };                        /* SF3D_SNOW_OUT_LIQUID_WATER of include/sf3d_snow.h */

bool DeviceSolver::snow_hour_done(uint32_t nCells) const { return impl_ && impl_->snow.base && impl_->snow.hourDone && impl_->snow.nCells == nCells; }
/* the maps snow_hour_input serves are still there: none of the blocks the last hour read in place has been freed since */
bool DeviceSolver::snow_inputs_held(uint32_t nCells) const { return snow_hour_done(nCells) && impl_->snow.inputsHeld; }

/* input k of k_et0_hour among the maps the last hour read: air temperature, relative humidity, wind, global radiation, transmissivity */
static const float* snow_hour_input(const SnowCache& S, int k)
{
    static const int snowInput[5] = {0, 2, 3, 4, 6};
    return S.in[snowInput[k]];
}

static const float* snow_liquid_water(const SnowCache& S) { return S.base + (size_t)(SNOW_MAP_OUT + SNOW_OUT_LIQUID_WATER) * S.nCells; }

double DeviceSolver::snow_kernel_ms() const { return impl_ ? impl_->snow.lastMs : 0.; }
#endif
