/* part of sf3d_solver.hip (included there after the station transmissivity) - the application's hour, device to device
 * (include/sf3d_hour.h): Crit3DProject::runModelHour (bin/CRITERIA3D/criteria3DProject.cpp:2074-2189) with no raster crossing the bus
 * between its stages.
 *   hour_snow / hour_et0: k_snow_hour and k_et0_hour (sf3d_snow.inc, sf3d_crop.inc: their text is untouched) on the maps the meteo and
 *       radiation blocks hold, taken through those blocks' accessors (meteo_map, rad_global, rad_beam, rad_transmissivity_read);
 *   k_hour_relhum: Crit3DHourlyMeteoMaps::computeRelativeHumidityMap (agrolib/project/meteoMaps.cpp:301-321) over relHumFromTdew(float, float)
 *       (agrolib/meteo/meteo.cpp:301-315), one thread per cell, from the meteo block's air and dew temperature maps into its humidity map;
 *   k_hour_totals: totalPrecipitation (criteria3DProject.cpp:939-957), totalEvaporation (:827-829) and totalTranspiration (:867-870) of
 *       runWaterFluxes3DModel's balance (src/project3D/project3D.cpp:1307-1386): a fixed-order sum, no atomics;
 *   k_hour_pond: Project3D::dailyUpdatePond over computeCurrentPond (src/project3D/project3D.cpp:1779-1843): the day's pond per cell.
 * The bar of k_hour_relhum and k_hour_pond is the compiled reference's bits (tests/golden/relhum_dew.npz, pond_day.npz): the reference's
 * doubles in its order (-ffp-contract=off), pow(exp(..), esp) through ppow / fexp (the C library's, sf3d_glibcmath.inc), the tangent of
 * the slope from the host (sf3d_hour_api.inc).  The reference's order of the totals
 * is an OpenMP reduction, so there are no bits to match: each term is the reference's expression in doubles, the order of the sum is fixed
 * (a tree over the 256 cells of a block in LDS, then one block adds the block partials, thread t those with index = t mod 256 by
 * rising index, and a tree again), so two runs give the same bits.
 * The per-cell text compiles for the host too (tests/hour_host.cpp defines SF3D_HOUR_HOST). */

#ifndef SF3D_HOUR_HOST
#define SF3D_HOUR_FN __device__ __forceinline__
#define hour_exp(x) fexp(x)
#define hour_pow(x, y) ppow(x, y)
#endif

#define HOUR_NODATA (-9999.f)

SF3D_HOUR_FN bool hour_eqf(float a, float b) { return __builtin_fabs((double)a - (double)b) < 0.00001; }      /* isEqual(float, float), basicMath.h:25-26 */

/* relHumFromTdew(float Td, float T), meteo.cpp:301-315 */
SF3D_HOUR_FN float hour_relhum_from_tdew(float Td, float T)
{
    if (hour_eqf(Td, HOUR_NODATA) || hour_eqf(T, HOUR_NODATA)) return HOUR_NODATA;
    const double d = 237.3;
    const double c = 17.2693882;
    const double esp = 1 / ((double)T + d);
    double rh = hour_pow(hour_exp((c * (double)Td) - ((c * (double)T / ((double)T + d))) * ((double)Td + d)), esp);
    rh *= 100;
    if (rh > 100) return 100;
    const float f = (float)rh;
    return (1.f < f) ? f : 1.f;                 /* std::max(1.f, float(rh)) */
}

/* one cell of computeRelativeHumidityMap, meteoMaps.cpp:304-317: the emptied grid keeps the flag where either input holds it; the
 * function's own NODATA test comes second (the raster's flag need not be -9999) */
SF3D_HOUR_FN float hour_relhum_cell(float airT, float dewT, float flag)
{
    if (hour_eqf(airT, flag) || hour_eqf(dewT, flag)) return flag;
    return hour_relhum_from_tdew(dewT, airT);
}

/* the three terms of a cell [m3 h-1].  rain: the cell has a surface node (and is this rank's); sunk: k_sink_hour computed the cell (its
 * actual maps hold the flag elsewhere) */
SF3D_HOUR_FN void hour_total_terms(bool rain, bool sunk, float liquidWater, double actualEvap, double actualTransp, double area, float flag, double term[3])
{
    term[0] = term[1] = term[2] = 0.;
    if (rain && !hour_eqf(liquidWater, flag) && liquidWater > 0) term[0] = area * (liquidWater / 1000.);      /* criteria3DProject.cpp:954-957 */
    if (sunk) {
        term[1] = area * (actualEvap / 1000.);                                                                /* :828 */
        term[2] = area * (actualTransp / 1000.);                                                              /* :869 */
    }
}

/* Project3D::computeCurrentPond behind its NODATA exits, project3D.cpp:1792-1816.  slope: tan(slopeDegree * DEG_TO_RAD), the host's;
 * crop: processes.computeCrop && isCrop(unit) */
SF3D_HOUR_FN float hour_pond_cell(double slope, double maximumPond, double laiMax, bool crop, float currentLai, float laiFlag)
{
    double soilMaximumPond = maximumPond / (slope + 1.);
    double currentInterception = 0;
    if (crop) {
        soilMaximumPond *= 0.5;                 /* the pond is shared between the soil and the interception */
        if (!hour_eqf(currentLai, laiFlag)) currentInterception = maximumPond * 0.5 * (currentLai / laiMax);
    }
    return (float)(soilMaximumPond + currentInterception);
}

#ifndef SF3D_HOUR_HOST
/* dailyUpdatePond, project3D.cpp:1819-1843: a cell without surface node, slope or land unit is skipped (-9999: its node's pond stays) */
__global__ void __launch_bounds__(SF3D_BLOCK) k_hour_pond(HourPondView v)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    float pond = HOUR_NODATA;
    const int32_t u = v.unit[c];
    if (!(v.mine && !v.mine[c]) && v.col[c] >= 0 && u >= 0) {
        const HourPondUnitDev unit = v.units[u];
        pond = hour_pond_cell(v.tanSlope[c], unit.maximumPond, unit.laiMax, v.lai && unit.isCrop, v.lai ? v.lai[c] : HOUR_NODATA, v.laiFlag);
    }
    v.out[c] = pond;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_hour_relhum(HourRelhumView v)
{
    fm_init();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    float rh = v.flag;                          /* emptyGrid; another rank's cell keeps it */
    if (!(v.mine && !v.mine[c])) rh = hour_relhum_cell(v.airT[c], v.dewT[c], v.flag);
    v.out[c] = rh;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_hour_totals(HourTotalsView v)
{
    __shared__ double sm[HOUR_TOTALS][SF3D_BLOCK];
    const uint32_t t = threadIdx.x;
    double term[HOUR_TOTALS] = {0., 0., 0.};
    if (v.pass == 0) {
        const uint32_t c = blockIdx.x * blockDim.x + t;
        if (c < v.nCells) {
            const bool rain = !(v.mine && !v.mine[c]) && v.col[c] >= 0;
            const bool sunk = rain && !hour_eqf(v.dem[c], v.flag);                      /* `cell` of sink_cell, sf3d_sink.inc */
            hour_total_terms(rain, sunk, v.liquid[c], v.actual[c], v.actual[(size_t)v.nCells + c], v.area, v.flag, term);
        }
    } else {
        for (uint32_t k = t; k < v.nBlocks; k += SF3D_BLOCK)
            for (int q = 0; q < HOUR_TOTALS; ++q) term[q] += v.partials[(size_t)q * v.nBlocks + k];
    }
    for (int q = 0; q < HOUR_TOTALS; ++q) sm[q][t] = term[q];
    __syncthreads();
    for (uint32_t s = SF3D_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int q = 0; q < HOUR_TOTALS; ++q) sm[q][t] += sm[q][t + s];
        __syncthreads();
    }
    if (t < HOUR_TOTALS) {
        if (v.pass == 0) v.partials[(size_t)t * v.nBlocks + blockIdx.x] = sm[t][0];
        else v.totals[t] = sm[t][0];
    }
}

/* ---- host side: the calls go through the shared raster path at the end of sf3d_maps.inc */

/* a block frees its maps: the snow block's recorded inputs, the transmissivity map the radiation hour read and the liquid water map
 * the sink hour read are forgotten where they lie in that block */
void DeviceSolver::raster_unbind(int who)
{
    Impl& I = *impl_;
    if (I.snow.feeds & who) { I.snow.feeds = 0; I.snow.inputsHeld = false; }
    if (who == FEED_METEO && I.rad.trFromMeteo) { I.rad.trRead = nullptr; I.rad.trFromMeteo = false; }
    if (I.sink.liquidFrom == who) { I.sink.liquidRead = nullptr; I.sink.liquidFrom = 0; }
}

sf3d_error_t DeviceSolver::hour_snow(const float* surfaceWater, const SnowParamsDev& p, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    SnowCache& S = I.snow;
    const size_t n = S.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    float* const water = S.base + (size_t)(SNOW_MAP_IN + 7) * n;
    if (surfaceWater) RASTER_TRY(hipMemcpyAsync(water, surfaceWater, n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    const float* in[8] = {meteo_map(I.meteo, METEO_AIR_TEMPERATURE), meteo_map(I.meteo, METEO_PRECIPITATION), meteo_map(I.meteo, METEO_AIR_REL_HUMIDITY),
                          meteo_map(I.meteo, METEO_WIND_SCALAR_INTENSITY), rad_global(I.rad), rad_beam(I.rad), rad_transmissivity_read(I.rad),
                          surfaceWater ? water : nullptr};
    return snow_launch(in, FEED_METEO | FEED_RAD, p, flag, mine);
}

sf3d_error_t DeviceSolver::hour_et0(float clearSky, float flag, const uint8_t* mine)
{
    Impl& I = *impl_;
    RASTER_TRY(hipSetDevice(I.device));
    const float* in[5] = {meteo_map(I.meteo, METEO_AIR_TEMPERATURE), meteo_map(I.meteo, METEO_AIR_REL_HUMIDITY), meteo_map(I.meteo, METEO_WIND_SCALAR_INTENSITY),
                          rad_global(I.rad), rad_transmissivity_read(I.rad)};
    return crop_launch(in, clearSky, flag, mine);
}

sf3d_error_t DeviceSolver::hour_relhum(const uint8_t* mine, float* out)
{
    Impl& I = *impl_;
    MeteoCache& K = I.meteo;
    const size_t n = K.nCells;
    RASTER_TRY(hipSetDevice(I.device));
    HourRelhumView v{};
    sf3d_error_t e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.airT = meteo_map(K, METEO_AIR_TEMPERATURE); v.dewT = meteo_map(K, METEO_AIR_DEW_TEMPERATURE);
    v.out = K.base + (1 + (size_t)K.nProxies + (size_t)METEO_AIR_REL_HUMIDITY) * n;
    v.nCells = K.nCells; v.flag = K.flag;
    e = raster_launch(k_hour_relhum, n, v, I.hour.lastMs[0]);
    if (e == SF3D_OK) K.produced[METEO_AIR_REL_HUMIDITY] = true;
    if (e != SF3D_OK || !out) return e;
    return raster_download(out, v.out, n * sizeof(float));
}

bool DeviceSolver::hour_totals_ready(uint32_t nCells) const
{
    return sink_computed() && impl_->sink.cells && impl_->sink.nCells == nCells && impl_->sink.liquidRead;
}

sf3d_error_t DeviceSolver::hour_totals(HostModel& m, const ParamsHost& p, const MapsInput& in, const uint8_t* mine, double totals[3])
{
    sf3d_error_t e = raster_columns(m, p, in);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    const SinkCache& K = I.sink;
    HourCache& H = I.hour;
    const size_t n = K.nCells;
    const uint32_t nBlocks = (uint32_t)((n + SF3D_BLOCK - 1) / SF3D_BLOCK);
    RASTER_TRY(maps_reserve(H.sums, H.sumsCap, (size_t)HOUR_TOTALS * (nBlocks + 1)));
    HourTotalsView v{};
    e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.col = I.maps.col;
    v.liquid = K.liquidRead;
    v.actual = (const double*)raster_cell_map(K.cells, n, SINK_MAP_EVAPORATION);
    v.dem = (const float*)raster_cell_map(K.cells, n, SINK_MAP_DEM);
    v.partials = H.sums + HOUR_TOTALS; v.totals = H.sums;
    v.area = K.area; v.nCells = K.nCells; v.nBlocks = nBlocks; v.flag = K.flag;
    v.pass = 0;
    double ms0 = 0.;
    e = raster_launch(k_hour_totals, n, v, ms0);
    if (e != SF3D_OK) return e;
    v.pass = 1;
    e = raster_launch(k_hour_totals, SF3D_BLOCK, v, H.lastMs[1]);
    if (e != SF3D_OK) return e;
    H.lastMs[1] += ms0;
    return raster_download(totals, H.sums, HOUR_TOTALS * sizeof(double));
}

/* the static maps go up with the first call after sf3d_hour_set_ponds; out: the pond map, nCells floats on the host */
sf3d_error_t DeviceSolver::hour_pond(HostModel& m, const ParamsHost& p, const MapsInput& in, const HourPondSetup& setup, bool computeCrop, float laiFlag,
                                     const uint8_t* mine, float* out)
{
    sf3d_error_t e = raster_columns(m, p, in);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    HourCache& H = I.hour;
    const size_t n = setup.nCells;
    const size_t unitBytes = (size_t)CROP_MAX_UNITS * sizeof(HourPondUnitDev);
    if (!H.pond || H.pondVer != setup.ver) {
        raster_release({H.pond});
        H.pond = nullptr; H.pondVer = 0; H.pondCells = 0;
        RASTER_TRY(hipMalloc((void**)&H.pond, n * 8 + unitBytes + n * 8));
        H.pondCells = setup.nCells;
        RASTER_TRY(hipMemcpyAsync(H.pond, setup.tanSlope, n * 8, hipMemcpyHostToDevice, I.stream));
        if (setup.nUnits) RASTER_TRY(hipMemcpyAsync(H.pond + n * 8, setup.units, (size_t)setup.nUnits * sizeof(HourPondUnitDev), hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipMemcpyAsync(H.pond + n * 8 + unitBytes, setup.unit, n * 4, hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipStreamSynchronize(I.stream));
        H.pondVer = setup.ver;
    }
    HourPondView v{};
    e = raster_mask(mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.col = I.maps.col;
    v.tanSlope = (const double*)H.pond;
    v.units = (const HourPondUnitDev*)(H.pond + n * 8);
    v.unit = (const int32_t*)(H.pond + n * 8 + unitBytes);
    v.out = (float*)(H.pond + n * 8 + unitBytes + n * 4);
    v.lai = computeCrop ? crop_lai(I.crop) : nullptr;
    v.nCells = setup.nCells; v.laiFlag = laiFlag;
    e = raster_launch(k_hour_pond, n, v, H.lastMs[2]);
    if (e != SF3D_OK) return e;
    return raster_download(out, v.out, n * sizeof(float));
}

sf3d_error_t DeviceSolver::hour_free()
{
    if (!impl_) return SF3D_OK;
    raster_release({impl_->hour.sums, impl_->hour.pond});
    impl_->hour = HourCache();
    return SF3D_OK;
}

double DeviceSolver::hour_kernel_ms(int which) const { return (impl_ && which >= 0 && which <= 2) ? impl_->hour.lastMs[which] : 0.; }
#endif
