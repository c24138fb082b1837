/* part of sf3d_solver.hip (included there after the snow model) - what Crit3DProject::runModelHour does between the snow model and the
 * solver, on the device (bin/CRITERIA3D/criteria3DProject.cpp:2130-2153):
 *   k_et0_hour  Crit3DHourlyMeteoMaps::computeET0PMMap (agrolib/project/meteoMaps.cpp:238-271) over ET0_Penman_hourly
 *               (agrolib/meteo/meteo.cpp:550-609; helpers of agrolib/mathFunctions/physics.cpp:39-47, 118-164, meteo.cpp:433-436), and
 *               updateDailyTemperatures (criteria3DProject.cpp:1994-2018) in the same pass;
 *   k_crop_day  dailyUpdateCropMaps (criteria3DProject.cpp:576-640) over Crit3DCrop::getDailyDegreeIncrease / computeSimpleLAI
 *               (agrolib/crop/crop.cpp:161-224, 333-350) and leafDevelopment::getLAICriteria / getLAISenescence (development.cpp:117-154).
 * One thread per raster cell: the cells of a row are neighbouring lanes, every map access is 64 consecutive floats.  No neighbours, no
 * atomics, no reduction.
 *
 * The bar is the compiled reference's bits (tests/golden/crop_et0.npz): the same double operations in the same order
 * (-ffp-contract=off), floats widened where the reference widens them, results rounded to float where its maps are float.  In the
 * object code of the pin build (g++ -O2) pow(tAirK, 4), the pressure law of pressureFromAltitude and pow(..., n4) of the falling LAI
 * curve are calls of the library's pow, exp and log are the library's: ppow / fexp / flog here.  sqrt is the IEEE one.
 *
 * Kept from the reference on purpose:
 *  - computeET0PMMap takes a cell for a DEM cell when int(height) != int(flag); dailyUpdateCropMaps when !isEqual(height, flag);
 *    updateDailyTemperatures does not look at the DEM at all;
 *  - transmissivity / clearSkyTransmissivity is a float division, widened afterwards;
 *  - the degree days are accumulated in float (the map's += float(dailyDD));
 *  - computeSimpleLAI starts the leaf fall of a TREE from LAImax * 0.75, whatever the LAI was.
 * The per-cell text compiles for the host too (tests/crop_host.cpp defines SF3D_CROP_HOST). */

#ifndef SF3D_CROP_HOST
#define SF3D_CROP_FN __device__ __forceinline__
#endif

#define CROP_NODATA (-9999.0)
#define CROP_TYPE_HERBACEOUS_ANNUAL 0        /* speciesType, agrolib/crop/crop.h:14 */
#define CROP_TYPE_HORTICULTURAL 2
#define CROP_TYPE_TREE 4

/* ET0_Penman_hourly, meteo.cpp:550-609 */
SF3D_CROP_FN double crop_et0_penman_hourly(double heigth, double normalizedTransmissivity, double globalIrradiance, double airTemp, double airHum,
                                           double windSpeed10)
{
    const double es = 611 * fexp(17.502 * airTemp / (airTemp + 240.97)) / 1000.;          /* saturationVaporPressure */
    const double ea = airHum * es / 100.0;
    const double emissivity = 0.34 - 0.14 * sqrt(ea);                                      /* emissivityFromVaporPressure */
    const double tAirK = airTemp + 273.15;
    const double mySigma = 5.670373E-8 * 3600.;
    const double mt = (normalizedTransmissivity < 1) ? normalizedTransmissivity : 1;       /* MINVALUE */
    const double cf = 1.35 * mt - 0.35;
    const double cloudFactor = (0 > cf) ? 0 : cf;                                          /* MAXVALUE(0, .) */
    const double netLWRadiation = cloudFactor * emissivity * mySigma * ppow(tAirK, 4);
    const double netSWRadiation = 3600 * globalIrradiance;
    const double netRadiation = (1 - 0.23) * netSWRadiation - netLWRadiation;              /* ALBEDO_CROP_REFERENCE */
    double g, Cd;
    if (netRadiation > 0) { g = 0.1 * netRadiation; Cd = 0.24; }
    else { g = 0.5 * netRadiation; Cd = 0.96; }
    const double delta = 4098. * es / ((237.3 + airTemp) * (237.3 + airTemp));             /* saturationSlope */
    /* pressureFromAltitude(height): P0 * pow(1 + height * LAPSE_RATE_MOIST_AIR / TP0, - GRAVITY / (LAPSE_RATE_MOIST_AIR * R_DRY_AIR)) */
    const double pressure = 101325. * ppow(1 + heigth * 0.0065 / 293.16, - 9.80665 / (0.0065 * 287.058)) / 1000.;
    const double lambda = 2501000. - 2369.2 * airTemp;                                     /* latentHeatVaporization */
    const double gamma = 1013. * pressure / (0.622 * lambda);                              /* psychro */
    const double windSpeed2 = windSpeed10 * 0.748;
    const double denominator = delta + gamma * (1 + Cd * windSpeed2);
    const double firstTerm = delta * (netRadiation - g) / (lambda * denominator);
    const double secondTerm = (gamma * (37 / tAirK) * windSpeed2 * (es - ea)) / denominator;
    const double sum = firstTerm + secondTerm;
    return (sum > 0) ? sum : 0;                                                            /* MAXVALUE(., 0) */
}

/* one cell of k_et0_hour */
SF3D_CROP_FN void crop_et0_cell(const CropView& v, uint32_t c)
{
    const float flag = v.flag;
    if (v.mine && !v.mine[c]) { v.et0[c] = flag; return; }          /* another rank's column: its extremes stay, its ET0 says "not here" */
    const float height = v.dem[c];
    const float temperature = v.in[0][c], relHumidity = v.in[1][c], windSpeed = v.in[2][c], globalRadiation = v.in[3][c], transmissivity = v.in[4][c];
    /* computeET0PMMap */
    float et0 = flag;
    if ((int)height != (int)flag
        && !snow_eqf(globalRadiation, flag) && !snow_eqf(transmissivity, flag) && !snow_eqf(temperature, flag) && !snow_eqf(relHumidity, flag)
        && !snow_eqf(windSpeed, flag))
        et0 = (float)crop_et0_penman_hourly((double)height, (double)(transmissivity / v.clearSky), (double)globalRadiation, (double)temperature,
                                            (double)relHumidity, (double)windSpeed);
    v.et0[c] = et0;
    /* updateDailyTemperatures */
    if (snow_eqf(temperature, flag)) return;
    const float currentTmin = v.st[2][c], currentTmax = v.st[3][c];
    v.st[2][c] = snow_eqf(currentTmin, flag) ? temperature : ((temperature < currentTmin) ? temperature : currentTmin);     /* std::min */
    v.st[3][c] = snow_eqf(currentTmax, flag) ? temperature : ((currentTmax < temperature) ? temperature : currentTmax);     /* std::max */
}

#ifndef SF3D_CROP_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_et0_hour(CropView v)
{
    fm_init();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    crop_et0_cell(v, c);
}
#endif

/* Crit3DCrop::isInsideTypicalCycle, crop.cpp:314-344 */
SF3D_CROP_FN bool crop_inside_typical_cycle(const CropUnitDev& u, int doy)
{
    const int daysFromSowing = (doy - u.sowingDoy) % 365;
    if (daysFromSowing >= 0) return daysFromSowing < u.plantCycle;
    return (doy + 365 - u.sowingDoy) < u.plantCycle;
}

/* leafDevelopment::getLAICriteria, development.cpp:132-154 */
SF3D_CROP_FN double crop_lai_criteria(const CropUnitDev& u, double myDegreeDays)
{
    const double c4 = (u.type == CROP_TYPE_TREE) ? 15.0 : 9.0;
    if (myDegreeDays <= u.degreeDaysIncrease)
        return u.LAImin + (u.LAImax - u.LAImin) / (1 + fexp(u.LAIcurve_a + u.LAIcurve_b * myDegreeDays));
    return u.LAImin + (u.LAImax - u.LAImin) / (1 + ppow(10 * ((myDegreeDays - u.degreeDaysIncrease) / dmax(u.degreeDaysDecrease, 1.)) / c4, 4.0));
}

/* Crit3DCrop::computeSimpleLAI, crop.cpp:177-224 */
SF3D_CROP_FN double crop_simple_lai(const CropUnitDev& u, double myDegreeDays, double latitude, int currentDoy)
{
    /* one inlined copy of the curve serves both branches: sown crops enter it past the emergence offset, the others with degree days > 0 */
    const bool sowing = u.type == CROP_TYPE_HERBACEOUS_ANNUAL || u.type == CROP_TYPE_HORTICULTURAL;       /* isSowingCrop */
    const bool onCurve = sowing ? !(myDegreeDays < u.degreeDaysEmergence) : (myDegreeDays > 0);
    if (sowing) myDegreeDays -= u.degreeDaysEmergence;
    double currentLAI = onCurve ? crop_lai_criteria(u, myDegreeDays) : (sowing ? 0 : u.LAImin);
    if (!sowing) {
        if (u.type == CROP_TYPE_TREE) {
            int doyStartSenescence; bool isLeafFall;
            if (latitude > 0) { doyStartSenescence = 305; isLeafFall = (currentDoy >= doyStartSenescence); }
            else { doyStartSenescence = 120; isLeafFall = ((currentDoy >= doyStartSenescence) && (currentDoy < 182)); }
            if (isLeafFall) {                                                               /* getLAISenescence(LAImin, LAImax*0.75, days), development.cpp:117-129 */
                const int daysFromStartSenescence = currentDoy - doyStartSenescence;
                if (daysFromStartSenescence > 30) currentLAI = u.LAImin;
                else {
                    const double a = flog(dmax(u.LAImax * 0.75, 0.1));
                    const double b = (flog(dmax(u.LAImin, 0.01)) - a) / 30;
                    currentLAI = fexp(a + b * daysFromStartSenescence);
                }
            }
            currentLAI += u.LAIgrass;
        }
    }
    return currentLAI;
}

/* one cell of k_crop_day; units: the crop table (v.nUnits entries).  dateDoy < 0: initializeCropFromDegreeDays
 * (criteria3DProject.cpp:524-573) - the degree days are in place, LAI from them */
SF3D_CROP_FN void crop_day_cell(const CropView& v, const CropUnitDev* units, uint32_t c)
{
    if (v.mine && !v.mine[c]) return;           /* another rank's column: untouched */
    const float flag = v.flag;
    const bool fromMap = v.dateDoy < 0;
    float dd = v.st[0][c], lai = v.st[1][c];
    const int firstDoy = (v.latitude < 0) ? 182 : 1;
    if (!fromMap && v.dateDoy == firstDoy) { dd = flag; lai = flag; }         /* emptyGrid on both maps */
    if (fromMap) lai = flag;                                                  /* initializeCropMaps */
    const int32_t index = v.index[c];
    const bool cropCell = !snow_eqf(v.dem[c], flag) && index >= 0 && index < (int32_t)v.nUnits && units[index].isCrop;
    if (fromMap && !cropCell) dd = flag;
    if (cropCell) {
        const CropUnitDev& u = units[index];
        if (fromMap) {
            if (!snow_eqf(dd, flag)) lai = (float)crop_simple_lai(u, (double)dd, v.latitude, v.currentDoy);
        } else {
            const float tminF = v.st[2][c], tmaxF = v.st[3][c];
            if (!snow_eqf(tminF, flag) && !snow_eqf(tmaxF, flag)) {
                /* getDailyDegreeIncrease, crop.cpp:161-174 */
                const double tmin = tminF, tmax = tmaxF;
                double dailyDD;
                if (snow_eq(tmin, CROP_NODATA) || snow_eq(tmax, CROP_NODATA)) dailyDD = CROP_NODATA;
                else if ((u.type == CROP_TYPE_HERBACEOUS_ANNUAL || u.type == CROP_TYPE_HORTICULTURAL) && !crop_inside_typical_cycle(u, v.currentDoy)) dailyDD = 0;
                else {
                    const double tmed = (tmin + dmin(tmax, u.upperThermalThreshold)) * 0.5;
                    dailyDD = dmax(tmed - u.thermalThreshold, 0.);
                }
                if (!snow_eq(dailyDD, CROP_NODATA)) {
                    if (snow_eqf(dd, flag)) dd = (float)dailyDD;
                    else dd += (float)dailyDD;
                    lai = (float)crop_simple_lai(u, (double)dd, v.latitude, v.currentDoy);
                }
            }
        }
    }
    v.st[0][c] = dd; v.st[1][c] = lai;
    v.st[2][c] = flag; v.st[3][c] = flag;                                     /* emptyGrid on the daily extremes (from a map: initializeCropMaps) */
}

#ifndef SF3D_CROP_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_crop_day(CropView v)
{
    __shared__ CropUnitDev units[CROP_MAX_UNITS];
    {   /* the crop table: consecutive words from memory into LDS, read from there (every lane its own unit) */
        const uint32_t* src = reinterpret_cast<const uint32_t*>(v.units);
        uint32_t* dst = reinterpret_cast<uint32_t*>(units);
        const uint32_t words = v.nUnits * (uint32_t)(sizeof(CropUnitDev) / 4);
        for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) dst[k] = src[k];
    }
    fm_init();
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    crop_day_cell(v, units, c);
}

/* ---- host side: one device block of CROP_MAPS x nCells 4-byte values and the crop table; calls go through the shared raster path at the
 * end of sf3d_maps.inc. */
sf3d_error_t DeviceSolver::crop_free()
{
    if (!impl_) return SF3D_OK;
    raster_release({impl_->crop.base, impl_->crop.units});
    impl_->crop = CropCache();
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::crop_alloc(uint32_t nCells, const CropUnitDev* units, uint32_t nUnits)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    crop_free();
    CropCache& K = impl_->crop;
    RASTER_TRY(hipMalloc((void**)&K.base, (size_t)CROP_MAPS * nCells * sizeof(float)));
    RASTER_TRY(hipMalloc((void**)&K.units, (size_t)CROP_MAX_UNITS * sizeof(CropUnitDev)));
    K.nCells = nCells; K.nUnits = nUnits;
    if (nUnits) RASTER_TRY(hipMemcpyAsync(K.units, units, (size_t)nUnits * sizeof(CropUnitDev), hipMemcpyHostToDevice, impl_->stream));
    RASTER_TRY(hipStreamSynchronize(impl_->stream));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::crop_upload(int map, const void* src)
{
    const CropCache& K = impl_->crop;
    return raster_upload(K.base + (size_t)map * K.nCells, src, (size_t)K.nCells * sizeof(float));
}

sf3d_error_t DeviceSolver::crop_download(int map, float* dst)
{
    const CropCache& K = impl_->crop;
    return raster_download(dst, K.base + (size_t)map * K.nCells, (size_t)K.nCells * sizeof(float));
}

/* ---- what the other blocks read from this one, once it is allocated on their raster */
bool DeviceSolver::crop_allocated(uint32_t nCells) const { return impl_ && impl_->crop.base && impl_->crop.nCells == nCells; }
static const float* crop_et0(const CropCache& K) { return K.base + (size_t)CROP_MAP_ET0 * K.nCells; }
static const float* crop_degree_days(const CropCache& K) { return K.base + (size_t)(CROP_MAP_STATE + 0) * K.nCells; }      /* SF3D_CROP_DEGREE_DAYS */
static const float* crop_lai(const CropCache& K) { return K.base + (size_t)(CROP_MAP_STATE + 1) * K.nCells; }              /* SF3D_CROP_LAI */

static void crop_view(CropView& v, const CropCache& K, float flag)
{
    const size_t n = K.nCells;
    for (int k = 0; k < 4; ++k) v.st[k] = K.base + (size_t)(CROP_MAP_STATE + k) * n;
    v.et0 = K.base + (size_t)CROP_MAP_ET0 * n;
    for (int k = 0; k < 5; ++k) v.in[k] = K.base + (size_t)(CROP_MAP_IN + k) * n;
    v.dem = K.base + (size_t)CROP_MAP_DEM * n;
    v.index = reinterpret_cast<const int32_t*>(K.base + (size_t)CROP_MAP_INDEX * n);
    v.units = K.units;
    v.nCells = K.nCells; v.nUnits = K.nUnits; v.flag = flag;
}

sf3d_error_t DeviceSolver::crop_hour(const float* const in[5], float clearSky, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    CropCache& K = I.crop;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    if (in)
        for (int k = 0; k < 5; ++k) RASTER_TRY(hipMemcpyAsync(K.base + (size_t)(CROP_MAP_IN + k) * n, in[k], n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    const float* d[5];
    for (int k = 0; k < 5; ++k) d[k] = in ? K.base + (size_t)(CROP_MAP_IN + k) * n : snow_hour_input(I.snow, k);      /* null: the maps the last snow hour read */
    return crop_launch(d, clearSky, flag, mine);
}

/* the hour on five input maps that are on the device: slots of this block, the snow hour's inputs (crop_hour) or maps of the meteo and
 * radiation blocks (hour_et0, sf3d_hour.inc) */
sf3d_error_t DeviceSolver::crop_launch(const float* const in[5], float clearSky, float flag, const uint8_t* mine)
{
    CropCache& K = impl_->crop;
    CropView v{};
    const sf3d_error_t e = raster_mask(mine, K.nCells, &v.mine);
    if (e != SF3D_OK) return e;
    crop_view(v, K, flag);
    for (int k = 0; k < 5; ++k) v.in[k] = in[k];
    v.clearSky = clearSky;
    return raster_launch(k_et0_hour, K.nCells, v, K.lastMs[0]);
}

sf3d_error_t DeviceSolver::crop_day(int dateDoy, int currentDoy, double latitude, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    CropCache& K = I.crop;
    RASTER_TRY(hipSetDevice(I.device));
    CropView v{};
    const sf3d_error_t e = raster_mask(mine, K.nCells, &v.mine);
    if (e != SF3D_OK) return e;
    crop_view(v, K, flag);
    v.latitude = latitude; v.dateDoy = dateDoy; v.currentDoy = currentDoy;
    return raster_launch(k_crop_day, K.nCells, v, K.lastMs[1]);
}

/* which: 0 k_et0_hour, 1 k_crop_day */
double DeviceSolver::crop_kernel_ms(int which) const { return (impl_ && (which == 0 || which == 1)) ? impl_->crop.lastMs[which] : 0.; }
#endif
