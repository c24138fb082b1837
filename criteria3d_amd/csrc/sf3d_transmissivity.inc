/* part of sf3d_solver.hip (included there after sf3d_rad.inc) - the clear-sky ratio of every station over a time window and the width of
 * that window, on the device: what computeTransmissivity (agrolib/solarRadiation/transmissivity.cpp:105-169) does through
 * radiation::computePointTransmissivity (agrolib/solarRadiation/solarRadiation.cpp:1265-1367), and what
 * radiation::estimateTransmissivityWindow (:835-922) does for one point.
 *
 * k_transmissivity_points: one wave64 per point, a lane per evaluation of computeRadiationRsun (:700-832), four points per block of 256.
 * The point is horizontal (slope 0, aspect 180, :1285-1286), both transmissivities are the clear-sky value and the temperature is
 * TEMPERATURE_DEFAULT (:1304-1306); the shadow ray starts at the station's own (x, y, z) in doubles and is marched only where the
 * station is inside the DEM (:748).  The evaluation is rad_eval of sf3d_rad.inc, the text k_rad_hour runs; its result here is a written
 * flag, sunPosition.elevationRefr and the DOUBLE radPoint.global (not rounded to float, unlike the maps of k_rad_hour).  The lanes
 * leave their results in LDS (and in global memory for sf3d_transmissivity_get_evaluations); after a barrier lane 0 of each wave adds
 * them up in the reference's order - no tree, no atomics.  Beyond the exp / pow tables of fm_init the LDS holds that hand-over: 256
 * doubles, 256 floats and 256 bytes = 3 328 bytes a block.
 *
 * The order and what a skipped or failed evaluation leaves behind are the reference's:
 *  - computePointTransmissivity evaluates the centre, then for i = centre-1 .. 0 the backward slot i and the forward slot width-1-i,
 *    each only where its measurement is not NODATA; it ignores computeRadiationRsun's return value, so an evaluation that fails (the
 *    range check of S_solpos on the point, a date S_solpos refuses) adds what the previous evaluation IN THAT ORDER left in
 *    radPoint.global - NODATA (-9999, radiationDefinitions.h:99) if none has written yet;
 *  - estimateTransmissivityWindow evaluates noon, the centre and then pairs of steps until the sum reaches the threshold or the window
 *    23 steps; a step counts only where sunPosition.elevationRefr > 3, and both radPoint.global and sunPosition are what the last
 *    successful evaluation left.  All 1 + 1 + 22 candidates are evaluated in one launch and the scan decides.
 *
 * This text also compiles for the host (tests/transmissivity_host.cpp), as sf3d_rad.inc does. */

#define TR_NODATA_F (-9999.f)

SF3D_RAD_FN bool tr_eq(float a, float b) { return __builtin_fabs((double)a - (double)b) < RAD_EPSILON; }      /* isEqual(float, float), basicMath.h:25 */

/* computeTransmissivity's gate (transmissivity.cpp:121-150): the centre measurement is there and validSamples >= width * 0.66 (an int
 * against a double) */
SF3D_RAD_FN bool tr_point_go(const float* measured, int width)
{
    if (tr_eq(measured[(width - 1) / 2], TR_NODATA_F)) return false;
    int valid = 0;
    for (int i = 0; i < width; ++i) valid += tr_eq(measured[i], TR_NODATA_F) ? 0 : 1;
    return !((double)valid < (double)width * 0.66);
}

/* one evaluation of computeRadiationRsun for a station.  written: radPoint.global was written; elev: TR_NODATA_F unless the sun position
 * was computed (it is also where the evaluation then fails on a clear-sky value of NODATA, :763) */
SF3D_RAD_FN void tr_evaluate(const RadGridDev& g, const RadHourDev& h, bool hourOk, const TrPointDev& p, bool& written, float& elev, double& global)
{
    written = false; elev = TR_NODATA_F; global = RAD_NODATA;
    if (!hourOk) return;
    double res[4];
    float e = TR_NODATA_F;
    written = rad_eval(g, h, p.cell, p.x, p.y, p.z, p.inGrid != 0, (double)h.clearSky, e, res);
    elev = e;
    if (written) global = res[0];
}

/* computePointTransmissivity's sums, solarRadiation.cpp:1300-1366, over the evaluations of one point */
SF3D_RAD_FN float tr_sum_points(const float* measured, const uint8_t* written, const double* global, int width, float clearSky)
{
    const int centre = (width - 1) / 2;
    double last = RAD_NODATA;                       /* radPoint.global */
    double sumGHI = measured[centre];
    if (written[centre]) last = global[centre];
    double sumClearSky = last;
    for (int i = centre - 1; i >= 0; --i) {
        if (!tr_eq(measured[i], TR_NODATA_F)) {
            sumGHI += measured[i];
            if (written[i]) last = global[i];
            sumClearSky += last;
        }
        const int j = width - i - 1;
        if (!tr_eq(measured[j], TR_NODATA_F)) {
            sumGHI += measured[j];
            if (written[j]) last = global[j];
            sumClearSky += last;
        }
    }
    double Kt = (sumClearSky > 1e-6) ? (sumGHI / sumClearSky) : 0.0;
    Kt = rad_clamp(Kt, 0.0, 1.2);
    const double transmissivity = Kt * clearSky;
    return (float)transmissivity;
}

/* estimateTransmissivityWindow's scan, solarRadiation.cpp:884-921, over the 24 candidates of one point: slot 0 noon, 1 the centre,
 * 2 + 2k the backward and 3 + 2k the forward step k + 1 */
SF3D_RAD_FN int tr_scan_window(const uint8_t* written, const float* elev, const double* global)
{
    double last = RAD_NODATA;                       /* radPoint.global */
    float lastElev = TR_NODATA_F;                   /* sunPosition.elevationRefr (the entry point refuses what would leave it unset at noon) */
    if (written[0]) last = global[0];
    if (elev[0] != TR_NODATA_F) lastElev = elev[0];
    const float quarter = (float)(last * 0.25);
    const double threshold = (50.f < quarter) ? quarter : 50.f;         /* std::max(50.f, float(global * 0.25)) */
    if (written[1]) last = global[1];
    if (elev[1] != TR_NODATA_F) lastElev = elev[1];
    double sumPotentialRad = last;
    int windowSteps = 1;
    for (int k = 0; sumPotentialRad < threshold && windowSteps < 23; ++k) {
        windowSteps += 2;
        for (int s = 2 + 2 * k; s < 4 + 2 * k; ++s) {
            if (written[s]) last = global[s];
            if (elev[s] != TR_NODATA_F) lastElev = elev[s];
            if (lastElev > 3.0) sumPotentialRad += last;
        }
    }
    return windowSteps;
}

#ifndef SF3D_RAD_HOST
static_assert(SF3D_BLOCK % TR_WAVE == 0 && TR_MAX_WIDTH < TR_WAVE && TR_WINDOW_SLOTS <= TR_WAVE, "a lane per slot");

__global__ void __launch_bounds__(SF3D_BLOCK) k_transmissivity_points(TrView v)
{
    __shared__ double sGlobal[SF3D_BLOCK];
    __shared__ float sElev[SF3D_BLOCK];
    __shared__ uint8_t sWritten[SF3D_BLOCK];
    fm_init();
    const uint32_t t = threadIdx.x, lane = t & (TR_WAVE - 1), wave = t / TR_WAVE;
    const uint32_t point = blockIdx.x * (SF3D_BLOCK / TR_WAVE) + wave;
    const int nSlots = v.nSlots;
    const bool live = point < v.nPoints && (int)lane < nSlots;
    const size_t at = (size_t)point * (size_t)nSlots + lane;
    bool written = false;
    float elev = TR_NODATA_F;
    double global = RAD_NODATA;
    if (live) {
        bool evaluate = true;
        if (v.mode == TR_MODE_POINTS) {
            const float* row = v.measured + (size_t)point * (size_t)nSlots;
            evaluate = tr_point_go(row, nSlots) && ((int)lane == (nSlots - 1) / 2 || !tr_eq(row[lane], TR_NODATA_F));
        }
        if (evaluate) tr_evaluate(v.grid, v.hours[lane], v.hourOk[lane] != 0, v.points[point], written, elev, global);
        v.written[at] = written ? 1 : 0;
        v.elevationRefr[at] = elev;
        v.global[at] = global;
    }
    sWritten[t] = written ? 1 : 0;
    sElev[t] = elev;
    sGlobal[t] = global;
    __syncthreads();
    if (point < v.nPoints && lane == 0) {
        const uint32_t w0 = wave * TR_WAVE;
        if (v.mode == TR_MODE_POINTS) {
            const float* row = v.measured + (size_t)point * (size_t)nSlots;
            v.transmissivity[point] = tr_point_go(row, nSlots) ? tr_sum_points(row, sWritten + w0, sGlobal + w0, nSlots, v.clearSky) : TR_NODATA_F;
        } else v.windowSteps[point] = tr_scan_window(sWritten + w0, sElev + w0, sGlobal + w0);
    }
}

/* ---- host side: the scratch of the last call belongs to the radiation block (RadCache) and goes with rad_free ---- */
static size_t tr_align8(size_t b) { return (b + 7) & ~(size_t)7; }

sf3d_error_t DeviceSolver::tr_run(const TrCall& call, float* transmissivity, int32_t* windowSteps)
{
    Impl& I = *impl_;
    RadCache& K = I.rad;
    RASTER_TRY(hipSetDevice(I.device));
    const size_t nP = call.nPoints, nS = (size_t)call.nSlots, nE = nP * nS;
    K.trPoints = 0; K.trSlots = 0;
    if (nP == 0) return SF3D_OK;
    /* one block: global [nE] doubles, points, hours, results [nP] 4-byte, elevation [nE], measured [nE], written [nE], hourOk */
    size_t off[8], total = 0;
    const size_t bytes[8] = {nE * sizeof(double), nP * sizeof(TrPointDev), nS * sizeof(RadHourDev), nP * 4, nE * sizeof(float), nE * sizeof(float), nE, nS};
    for (int k = 0; k < 8; ++k) { off[k] = total; total += tr_align8(bytes[k]); }
    if (total > K.trCap) {
        raster_release({K.tr});
        K.tr = nullptr; K.trCap = 0;
        RASTER_TRY(hipMalloc((void**)&K.tr, total));
        K.trCap = total;
    }
    char* b = K.tr;
    RASTER_TRY(hipMemcpyAsync(b + off[1], call.points, bytes[1], hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(b + off[2], call.hours, bytes[2], hipMemcpyHostToDevice, I.stream));
    if (call.measured) RASTER_TRY(hipMemcpyAsync(b + off[5], call.measured, bytes[5], hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(b + off[7], call.hourOk, bytes[7], hipMemcpyHostToDevice, I.stream));
    const size_t n = K.nCells;
    TrView v{};
    v.grid.dem = (const float*)((const double*)K.base + (size_t)RAD_DOUBLE_MAPS * n) + (size_t)RAD_MAP_DEM * n;
    v.grid.xll = K.xll; v.grid.yll = K.yll; v.grid.cellSize = K.cellSize; v.grid.invCellSize = 1.0 / K.cellSize;
    v.grid.nRows = (int32_t)K.nRows; v.grid.nCols = (int32_t)K.nCols; v.grid.flag = K.flag; v.grid.demMax = K.demMax;
    v.global = (double*)(b + off[0]); v.points = (const TrPointDev*)(b + off[1]); v.hours = (const RadHourDev*)(b + off[2]);
    v.transmissivity = (float*)(b + off[3]); v.windowSteps = (int32_t*)(b + off[3]);
    v.elevationRefr = (float*)(b + off[4]); v.measured = (const float*)(b + off[5]); v.written = (uint8_t*)(b + off[6]); v.hourOk = (const uint8_t*)(b + off[7]);
    v.nPoints = call.nPoints; v.nSlots = call.nSlots; v.mode = call.mode; v.clearSky = call.clearSky;
    const sf3d_error_t e = raster_launch(k_transmissivity_points, nP * TR_WAVE, v, K.trMs);
    if (e != SF3D_OK) return e;
    K.trPoints = call.nPoints; K.trSlots = (uint32_t)call.nSlots;
    K.trOff[0] = off[0]; K.trOff[1] = off[4]; K.trOff[2] = off[6];
    return raster_download(call.mode == TR_MODE_POINTS ? (void*)transmissivity : (void*)windowSteps, b + off[3], nP * 4);
}

bool DeviceSolver::tr_evaluated(uint32_t nPoints, uint32_t nSlots) const
{
    return impl_ && impl_->rad.trPoints == nPoints && impl_->rad.trSlots == nSlots && nPoints > 0;
}

sf3d_error_t DeviceSolver::tr_evaluations(uint8_t* written, float* elevationRefr, double* global)
{
    const RadCache& K = impl_->rad;
    const size_t nE = (size_t)K.trPoints * K.trSlots;
    sf3d_error_t e = raster_download(global, K.tr + K.trOff[0], nE * sizeof(double));
    if (e == SF3D_OK) e = raster_download(elevationRefr, K.tr + K.trOff[1], nE * sizeof(float));
    if (e == SF3D_OK) e = raster_download(written, K.tr + K.trOff[2], nE);
    return e;
}

double DeviceSolver::tr_kernel_ms() const { return impl_ ? impl_->rad.trMs : 0.; }
#endif
