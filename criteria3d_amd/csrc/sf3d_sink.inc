/* part of sf3d_solver.hip (included there after the meteo maps) - the hourly water sinks of the application on the device: the cell loop of
 * Crit3DProject::assignETreal (bin/CRITERIA3D/criteria3DProject.cpp:796-911) around Project3D::assignEvaporation
 * (src/project3D/project3D.cpp:2377-2451) and Project3D::assignTranspiration (:2461-2610), and the rain term of assignPrecipitation
 * (criteria3DProject.cpp:954-964).  k_sink_hour: one thread per raster cell walks its column; the column table is [layer][cell], so the lanes
 * of a wave read one layer of 64 neighbouring cells.  Every input is already on the device: ET0, LAI and degree days (the crop block), the
 * liquid water (the snow block), root length, first / last root layer and the keyed density table (the root block), and the water content of
 * every node - what getCriteria3DVar(volumetricWaterContent) returns for the accepted state, through map_node_value of sf3d_maps.inc.
 *
 * The bar is the compiled reference's bits (tests/golden/water_sinks.npz): the same double operations in the same order
 * (-ffp-contract=off, IEEE division), exp through the C library's routine (fexp), layerTranspiration rounded to float where the reference
 * keeps it in a std::vector<float>.  No per-thread array of layers: the redistribution and the final loop evaluate layerTranspiration again
 * from the same loads, which gives the same bits.  A node's sink is read, changed and written by its own cell's thread only; every
 * subtraction is made on its own, in the reference's order (evaporation iteration by iteration, then transpiration, then rain).
 *
 * Kept from the reference on purpose:
 *  - the water content is read again, unchanged, in each of the up to three evaporation iterations;
 *  - a layer without a node takes part in the evaporation loop with the water content NODATA (nothing evaporates) and is skipped by
 *    transpiration; a layer without a horizon is skipped by both;
 *  - waterStress is 1 - 0 / 0 = NaN when every root layer was skipped: both comparisons are false and nothing is redistributed.
 * The per-cell text compiles for the host too (tests/sink_host.cpp defines SF3D_SINK_HOST). */

#ifndef SF3D_SINK_HOST
#define SF3D_SINK_FN __device__ __forceinline__
#endif

#define SINK_NODATA (-9999)
#define SINK_EPSILON 0.00001
#define SINK_DBL_EPSILON 2.220446049250313e-16

/* getCriteria3DVar(volumetricWaterContent, node), project3D.cpp:2756-2810 */
SF3D_SINK_FN double sink_vwc(const SinkView& v, int32_t n)
{
    if (n < 0) return (double)SINK_NODATA;                                 /* getNodeWaterContent: INDEX_ERROR -> NODATA */
    const double w = ((uint32_t)n < v.ns) ? (v.H[n] - v.z[n]) : map_theta(v.soils[v.cls[n]], v.Se[n]);
    return map_sentinel(w) ? (double)SINK_NODATA : w;
}

/* one root layer of assignTranspiration's first loop (:2525-2572): false when the layer is skipped; else the layer's root density, whether it
 * is stressed, and layerTranspiration as the float the reference stores */
SF3D_SINK_FN bool sink_root_layer(const SinkView& v, uint32_t c, uint32_t layer, int32_t si, int32_t key, const SinkUnitDev& u, double maxTranspiration,
                                  double& density, bool& stressed, float& layerTranspiration)
{
    const int32_t n = v.col[(size_t)layer * v.nCells + c];
    if (n < 0) return false;
    const int32_t h = v.horizon[(size_t)si * v.nrLayers + layer];
    if (h < 0) return false;
    const double* hz = v.horizonValues + ((size_t)si * ROOT_MAX_HORIZONS + (uint32_t)h) * SINK_HORIZON_VALUES;
    const double FC = hz[SINK_H_FC], WP = hz[SINK_H_WP], SAT = hz[SINK_H_SAT];
    const double waterSurplusStressFraction = u.waterSurplusResistant ? 0. : 0.5;
    const double volWaterContent = sink_vwc(v, n);
    const double volWaterSurplusThreshold = SAT - waterSurplusStressFraction * (SAT - FC);
    const double volWaterScarcityThreshold = FC - u.fRAW * (FC - WP);
    double ratio;
    if (volWaterContent <= WP) { ratio = 0; stressed = true; }
    else if (volWaterContent < volWaterScarcityThreshold) { ratio = (volWaterContent - WP) / (volWaterScarcityThreshold - WP); stressed = true; }
    else if ((volWaterContent - volWaterSurplusThreshold) > SINK_EPSILON) { ratio = (SAT - volWaterContent) / (SAT - volWaterSurplusThreshold); stressed = true; }
    else { ratio = 1; stressed = false; }
    density = v.rootTable[(size_t)layer * v.rootRows + (uint32_t)key];
    layerTranspiration = (float)(maxTranspiration * density * ratio);
    return true;
}

/* getCriteria3DVar(maxVolumetricWaterContent, node), project3D.cpp:2756-2810 */
SF3D_SINK_FN double sink_max_vwc(const SinkView& v, int32_t n)
{
    const double w = ((uint32_t)n < v.ns) ? SF3D_VAL_INDEX_ERROR : v.soils[v.cls[n]].thetaS;
    return map_sentinel(w) ? (double)SINK_NODATA : w;
}

/* voidVolumeList[layer] of computeSoilCracking's first loop (criteria3DProject.cpp:1058-1064) for a layer with a node and a horizon */
SF3D_SINK_FN double sink_void_volume(const SinkView& v, int32_t n, int32_t si, int32_t h)
{
    const double soilFraction = v.horizonValues[((size_t)si * ROOT_MAX_HORIZONS + (uint32_t)h) * SINK_HORIZON_VALUES + SINK_H_FRACTION];
    const double VWC = sink_vwc(v, n);
    const double maxVWC = sink_max_vwc(v, n);
    const double currentVoidVolume = dmax(0.0, maxVWC - VWC);
    return currentVoidVolume * soilFraction;
}

/* Crit3DProject::computeSoilCracking (criteria3DProject.cpp:978-1123) behind its tests on the soil and the layer grid, which the host made
 * (sf3d_sink_set_cracking: maxDepth, lastLayer).  The evaporation and transpiration subtractions of the column are in v.sink already; every
 * addition is made on its own.  Returns the function's float; *crackWater: the sum of layerWater over the layers filled. */
SF3D_SINK_FN float sink_soil_cracking(const SinkView& v, const SinkCrackDev& k, uint32_t c, int32_t s0, int32_t si, float precipitation, double* crackWater)
{
    const size_t nc = v.nCells;
    const uint32_t nl = v.nrLayers;
    const double* const thick = v.layerTables;
    *crackWater = 0.;
    if (si < 0) return precipitation;
    double minimumPond = (((uint32_t)s0 < v.ns) ? k.pond[s0] : SF3D_VAL_INDEX_ERROR) * 1000;      /* getCriteria3DVar(surfacePond) [mm] */
    if (map_sentinel(minimumPond)) minimumPond = (double)SINK_NODATA;
    if (precipitation <= minimumPond) return precipitation;
    const int32_t lastLayer = k.lastLayer[si];
    if (lastLayer < 0) return precipitation;                              /* the soil never cracks */
    const double maxDepth = k.maxDepth[si];
    double crackDepth = 0.0, voidsVolumeSum = 0;
    uint32_t layerIndex = 1;                                             /* :1045-1069 */
    while (layerIndex < nl && k.layerDepth[layerIndex] <= maxDepth) {
        const int32_t n = v.col[(size_t)layerIndex * nc + c];
        if (n < 0) break;
        const int32_t h = v.horizon[(size_t)si * nl + layerIndex];
        if (h < 0) break;
        voidsVolumeSum += sink_void_volume(v, n, si, h) * thick[layerIndex];
        crackDepth += thick[layerIndex];
        ++layerIndex;
    }
    if (crackDepth == 0.0) return precipitation;
    const double avgVoidVolume = voidsVolumeSum / crackDepth;
    if (avgVoidVolume <= 0.15) return precipitation;
    const double ratio = (avgVoidVolume - 0.15) / (0.20 - 0.15);
    const double crackRatio = (ratio < 0.0) ? 0.0 : ((1.0 < ratio) ? 1.0 : ratio);            /* std::clamp */
    const double maxInfiltration = precipitation * crackRatio;
    const double surfaceWater = dmax(precipitation - maxInfiltration, minimumPond);
    const double potentialInfiltration = dmax(0.0, precipitation - surfaceWater);
    const double area = v.area;
    double residualDownWater = potentialInfiltration;
    /* filling from the bottom (:1095-1119).  voidVolumeList is 0 in every layer the first loop did not reach: such a layer takes nothing */
    for (int32_t l = (lastLayer < (int32_t)layerIndex - 1) ? lastLayer : (int32_t)layerIndex - 1; l > 0; --l) {
        if (residualDownWater <= 0) break;
        const int32_t n = v.col[(size_t)l * nc + c];
        if (n < 0) continue;
        const double layerThick_mm = thick[l] * 1000;
        const double storage = dmin(sink_void_volume(v, n, si, v.horizon[(size_t)si * nl + l]), 0.05);
        double layerWater = layerThick_mm * storage;
        layerWater = dmin(layerWater, residualDownWater);
        const double flow = area * (layerWater / 1000.);
        const double flowRate = flow / 3600.;
        if (flowRate > 0.0) {
            v.sink[n] += flowRate;
            residualDownWater -= layerWater;
            *crackWater += layerWater;
        }
    }
    return (float)(surfaceWater + residualDownWater);
}

/* one cell of the hour; CRACK: the rain term goes through sink_soil_cracking (k_sink_hour_crack), else precSurfaceWater = liquidWater */
template <bool CRACK> SF3D_SINK_FN void sink_cell(const SinkView& v, const SinkCrackDev* k, uint32_t c)
{
    const size_t nc = v.nCells;
    const uint32_t nl = v.nrLayers;
    const float flag = v.flag;
    /* the sinks of the column start the hour at 0 (waterSinkSource of runModelHour) */
    const int32_t s0 = v.col[c];
    double* const actualMaps = reinterpret_cast<double*>(v.cells);                                       /* evaporation, transpiration */
    const float* const dem = reinterpret_cast<const float*>(v.cells + 16 * nc);
    const int32_t* const cropIndex = reinterpret_cast<const int32_t*>(v.cells + 16 * nc + (size_t)(SINK_MAP_CROP - 2) * nc * 4);
    const int32_t* const soilIndex = reinterpret_cast<const int32_t*>(v.cells + 16 * nc + (size_t)(SINK_MAP_SOIL - 2) * nc * 4);
    const double* const thick = v.layerTables;
    const double* const evapCoeff = v.layerTables + nl;
    const double* const layerEvapCoeff = v.layerTables + 2 * (size_t)nl;
    for (uint32_t l = 1; l < nl; ++l) {
        const int32_t n = v.col[(size_t)l * nc + c];
        if (n >= 0) v.sink[n] = 0.;
    }
    const bool cell = !(v.mine && !v.mine[c]) && !snow_eqf(dem[c], flag) && s0 >= 0;
    if (!cell) {
        if (s0 >= 0) v.sink[s0] = 0.;
        actualMaps[c] = (double)flag; actualMaps[nc + c] = (double)flag;
        if constexpr (CRACK) { k->precSurfaceWater[c] = flag; k->crackWater[c] = (double)flag; }
        return;
    }
    double surfaceSink = 0.;
    const double area = v.area;
    const int32_t siRaw = soilIndex[c];
    const int32_t si = (siRaw >= 0 && siRaw < (int32_t)v.nSoils) ? siRaw : -1;
    const double et0 = (double)v.et0[c];
    float currentLAI = 0;                                                /* assignETreal :818-824 */
    { const float laiMapValue = v.lai[c]; if (!snow_eqf(laiMapValue, flag)) currentLAI = laiMapValue; }
    const double lai = currentLAI;
    const double covSurfFraction = (lai < SINK_EPSILON) ? 0. : 1 - fexp(-0.6 * lai);       /* getCoveredSurfaceFraction :2295-2301 */

    /* ---- assignEvaporation :2377-2451 ---- */
    double actualEvaporationSum = 0;
    const double maxEvaporation = et0 * (1.0 - covSurfFraction);
    if (!(maxEvaporation < SINK_EPSILON)) {
        const double surfaceWater = sink_vwc(v, s0) * 1000;
        double surfaceEvaporation = dmin(maxEvaporation, surfaceWater);
        const double surfaceFlow = area * (surfaceEvaporation / 1000.) / 3600.;
        if (surfaceFlow <= SINK_DBL_EPSILON) surfaceEvaporation = 0.;
        else { surfaceSink -= surfaceFlow; actualEvaporationSum += surfaceEvaporation; }
        double residualEvaporation = maxEvaporation - surfaceEvaporation;
        if (!(residualEvaporation < SINK_EPSILON || si < 0)) {
            int nrIteration = 0;
            while (residualEvaporation > SINK_EPSILON && nrIteration < 3) {
                double iterationEvapSum = 0;
                for (int32_t layer = 1; layer <= v.lastEvapLayer; ++layer) {
                    const int32_t n = v.col[(size_t)layer * nc + c];
                    const int32_t h = v.horizon[(size_t)si * nl + layer];
                    if (h < 0) continue;
                    const double* hz = v.horizonValues + ((size_t)si * ROOT_MAX_HORIZONS + (uint32_t)h) * SINK_HORIZON_VALUES;
                    const double evapThreshold = hz[SINK_H_HH] + (1 - evapCoeff[layer]) * (hz[SINK_H_FC] - hz[SINK_H_HH]) * 0.5;
                    const double layerWaterContent = sink_vwc(v, n) * hz[SINK_H_FRACTION];
                    const double wcAboveThreshold = dmax(layerWaterContent - evapThreshold, 0.0);
                    const double evapAvailableWater = wcAboveThreshold * thick[layer] * 1000.;
                    const double layerEvaporation = dmin(evapAvailableWater, residualEvaporation * layerEvapCoeff[layer]);
                    if (layerEvaporation > SINK_EPSILON && n >= 0) {      /* (without a node the water content is NODATA: nothing is available) */
                        const double flow = area * (layerEvaporation / 1000.) / 3600.;
                        v.sink[n] -= flow;
                        actualEvaporationSum += layerEvaporation;
                        iterationEvapSum += layerEvaporation;
                    }
                }
                residualEvaporation -= iterationEvapSum;
                nrIteration++;
            }
        }
    }

    /* ---- assignTranspiration :2461-2610, behind the conditions of assignETreal :850-864 ---- */
    double actualTranspiration = 0;
    const int32_t ci = cropIndex[c];
    const int32_t key = reinterpret_cast<const int32_t*>(v.rootCells + 16 * nc + (size_t)(ROOT_MAP_KEY - 2) * nc * 4)[c];
    const double currentDegreeDays = (double)v.dd[c];
    bool transpire = ci >= 0 && ci < (int32_t)v.nUnits && currentLAI > 0
                     && !(lai < SINK_EPSILON || snow_eq(currentDegreeDays, (double)SINK_NODATA)) && nl > 1 && si >= 0;
    double maxTranspiration = 0.;
    if (transpire) {
        const double kcFactor = 1 + (v.units[ci].kcMax - 1) * covSurfFraction;             /* getPotentialTranspiration :2323-2328 */
        maxTranspiration = et0 * covSurfFraction * kcFactor;
        transpire = !(maxTranspiration < SINK_EPSILON);
    }
    /* the root block: length <= 0, an empty density row (no key) and NODATA root layers end the function (:2487-2498) */
    if (transpire) transpire = key >= 0 && (uint32_t)key < v.rootRows && reinterpret_cast<const double*>(v.rootCells)[c] > 0;
    int32_t firstRootLayer = SINK_NODATA, lastRootLayer = SINK_NODATA;
    if (transpire) {
        firstRootLayer = reinterpret_cast<const int32_t*>(v.rootCells + 16 * nc + (size_t)(ROOT_MAP_FIRST - 2) * nc * 4)[c];
        lastRootLayer = reinterpret_cast<const int32_t*>(v.rootCells + 16 * nc + (size_t)(ROOT_MAP_LAST - 2) * nc * 4)[c];
        transpire = firstRootLayer != SINK_NODATA && lastRootLayer != SINK_NODATA && firstRootLayer >= 0 && lastRootLayer < (int32_t)nl;
    }
    if (transpire) {
        const SinkUnitDev u = v.units[ci];
        double rootDensityWithoutStress = 0.0, transpirationSubsetMax = 0;
        for (int32_t layer = firstRootLayer; layer <= lastRootLayer; ++layer) {
            double density; bool stressed; float layerTranspiration;
            if (!sink_root_layer(v, c, (uint32_t)layer, si, key, u, maxTranspiration, density, stressed, layerTranspiration)) continue;
            if (!stressed) rootDensityWithoutStress += density;
            transpirationSubsetMax += maxTranspiration * density;
            actualTranspiration += layerTranspiration;
        }
        const double waterStress = 1 - (actualTranspiration / transpirationSubsetMax);
        const bool redistribute = waterStress > SINK_EPSILON && rootDensityWithoutStress > SINK_EPSILON;
        const double redistribution = redistribute ? transpirationSubsetMax * dmin(waterStress, rootDensityWithoutStress) : 0.;
        actualTranspiration = 0;
        for (int32_t layer = firstRootLayer; layer <= lastRootLayer; ++layer) {
            double density; bool stressed; float layerTranspiration;
            if (!sink_root_layer(v, c, (uint32_t)layer, si, key, u, maxTranspiration, density, stressed, layerTranspiration)) continue;      /* its layerTranspiration stays 0 */
            if (redistribute && !stressed && layerTranspiration > 0)
                layerTranspiration = (float)((double)layerTranspiration + redistribution * (density / rootDensityWithoutStress));
            const double flow = area * (layerTranspiration / 1000.) / 3600.;
            if (flow > SINK_DBL_EPSILON) {
                const int32_t n = v.col[(size_t)layer * nc + c];
                v.sink[n] -= flow;
                actualTranspiration += layerTranspiration;
            }
        }
    }

    /* ---- the rain term of assignPrecipitation (criteria3DProject.cpp:939-964); without cracking precSurfaceWater = liquidWater ---- */
    const float liquidWater = v.liquid[c];
    float precSurfaceWater = liquidWater;
    double crackWater = 0.;
    if (!snow_eqf(liquidWater, flag) && liquidWater > 0) {
        if constexpr (CRACK) precSurfaceWater = sink_soil_cracking(v, *k, c, s0, si, liquidWater, &crackWater);
        const double surfaceFlow = area * (precSurfaceWater / 1000.);
        if ((surfaceFlow / 3600.) > 0.) surfaceSink += surfaceFlow / 3600.;
    }
    v.sink[s0] = surfaceSink;
    actualMaps[c] = actualEvaporationSum;
    actualMaps[nc + c] = actualTranspiration;
    if constexpr (CRACK) { k->precSurfaceWater[c] = precSurfaceWater; k->crackWater[c] = crackWater; }
}

#ifndef SF3D_SINK_HOST
__global__ void __launch_bounds__(SF3D_BLOCK) k_sink_hour(SinkView v)
{
    fm_init();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= v.nCells) return;
    sink_cell<false>(v, nullptr, c);
}

/* the hour with soil cracking (sf3d_sink_set_cracking) */
__global__ void __launch_bounds__(SF3D_BLOCK) k_sink_hour_crack(SinkCrackView k)
{
    fm_init();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= k.s.nCells) return;
    sink_cell<true>(k.s, k.k, c);
}

/* ---- host side: the per-cell block, one block of tables and the node array; calls go through the shared raster path at the end of
 * sf3d_maps.inc. */
enum { SINK_T_UNITS = 0, SINK_T_HORIZON_VALUES, SINK_T_THICK, SINK_T_EVAP_COEFF, SINK_T_LAYER_EVAP_COEFF, SINK_T_HORIZON, SINK_T_END };      /* the three layer tables are adjacent */

sf3d_error_t DeviceSolver::sink_free()
{
    if (!impl_) return SF3D_OK;
    raster_release({impl_->sink.cells, impl_->sink.tables, impl_->sink.nodes, impl_->sink.crack});
    impl_->sink = SinkCache();
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::sink_alloc(const SinkSetup& S)
{
    sf3d_error_t e = ensure_device();
    if (e != SF3D_OK) return e;
    sink_free();
    Impl& I = *impl_;
    SinkCache& K = I.sink;
    const size_t n = S.nCells, nl = S.nrLayers;
    const size_t bytes[SINK_T_END] = {(size_t)CROP_MAX_UNITS * sizeof(SinkUnitDev), (size_t)S.nSoils * ROOT_MAX_HORIZONS * SINK_HORIZON_VALUES * sizeof(double),
                                      nl * sizeof(double), nl * sizeof(double), nl * sizeof(double), (size_t)S.nSoils * nl * sizeof(int32_t)};
    const void* src[SINK_T_END] = {S.units, S.horizonValues, S.thick, S.evapCoeff, S.layerEvapCoeff, S.horizon};
    const size_t srcBytes[SINK_T_END] = {S.nUnits * sizeof(SinkUnitDev), bytes[1], bytes[2], bytes[3], bytes[4], bytes[5]};
    RASTER_TRY(hipMalloc((void**)&K.cells, (size_t)SINK_MAP_WORDS * n * 4));
    K.layerDepth.assign(S.layerDepth, S.layerDepth + nl);
    K.nCells = S.nCells; K.nrLayers = S.nrLayers; K.nUnits = S.nUnits; K.nSoils = S.nSoils; K.lastEvapLayer = S.lastEvapLayer; K.area = S.area; K.flag = S.flag;
    e = raster_tables(K.tables, K.off, SINK_T_END, bytes, src, srcBytes);
    if (e != SF3D_OK) return e;
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, SINK_MAP_DEM), S.dem, n * 4, hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, SINK_MAP_CROP), S.cropIndex, n * 4, hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, SINK_MAP_SOIL), S.soilIndex, n * 4, hipMemcpyHostToDevice, I.stream));
    {   /* before the first hour both actual maps hold the flag */
        const std::vector<double> empty(2 * n, (double)S.flag);
        RASTER_TRY(hipMemcpyAsync(K.cells, empty.data(), 2 * n * 8, hipMemcpyHostToDevice, I.stream));
        RASTER_TRY(hipStreamSynchronize(I.stream));
    }
    return SF3D_OK;
}

bool DeviceSolver::sink_allocated() const { return impl_ && impl_->sink.cells; }
bool DeviceSolver::sink_computed() const { return impl_ && impl_->sink.nodes && impl_->sink.computed; }

sf3d_error_t DeviceSolver::sink_hour(HostModel& m, const ParamsHost& p, const MapsInput& in, const SinkCall& call)
{
    sf3d_error_t e = raster_columns(m, p, in);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    SinkCache& K = I.sink;
    const RootCache& R = I.root;
    const size_t n = K.nCells;
    if (!K.nodes || K.nodesN != I.v.N) {
        if (K.nodes) { (void)hipFree(K.nodes); K.nodes = nullptr; }
        K.nodesN = 0; K.computed = false;
        RASTER_TRY(hipMalloc((void**)&K.nodes, ((size_t)I.v.N ? (size_t)I.v.N : 1) * sizeof(double)));
        K.nodesN = I.v.N;
        K.nodesColVer = 0;
    }
    if (K.nodesColVer != in.colVer) {
        /* nodes of no column, and of other ranks' columns, hold 0: the kernel zeroes a node through this hour's table only, so under another table
         * (sf3d_set_output_columns, or another partition) a node that has left its column would keep the sink of the last hour */
        RASTER_TRY(hipMemsetAsync(K.nodes, 0, (size_t)I.v.N * sizeof(double), I.stream));
        K.nodesColVer = in.colVer;
    }
    const float* maps[4] = {call.et0, call.lai, call.dd, call.liquid};
    for (int k = 0; k < 4; ++k)
        if (maps[k]) RASTER_TRY(hipMemcpyAsync(raster_cell_map(K.cells, n, SINK_MAP_ET0 + k), maps[k], n * sizeof(float), hipMemcpyHostToDevice, I.stream));
    SinkView v{};
    e = raster_mask(call.mine, n, &v.mine);
    if (e != SF3D_OK) return e;
    v.col = I.maps.col;
    v.H = I.v.X[mirror_.cur]; v.Se = I.v.Se; v.z = I.v.z; v.cls = I.v.cls; v.soils = I.v.soils;
    v.cells = K.cells;
    v.et0 = call.et0 ? (const float*)raster_cell_map(K.cells, n, SINK_MAP_ET0) : crop_et0(I.crop);
    v.lai = call.lai ? (const float*)raster_cell_map(K.cells, n, SINK_MAP_LAI) : crop_lai(I.crop);
    v.dd = call.dd ? (const float*)raster_cell_map(K.cells, n, SINK_MAP_DD) : crop_degree_days(I.crop);
    v.liquid = call.liquid ? (const float*)raster_cell_map(K.cells, n, SINK_MAP_LIQUID)
               : call.liquidFromMeteo ? meteo_map(I.meteo, METEO_PRECIPITATION) : snow_liquid_water(I.snow);
    K.liquidRead = nullptr; K.liquidFrom = 0;
    v.rootCells = R.cells;
    v.rootTable = (const double*)(R.tables + R.off[ROOT_T_TABLE]); v.rootRows = R.nRows;
    v.units = (const SinkUnitDev*)(K.tables + K.off[SINK_T_UNITS]);
    v.horizon = (const int32_t*)(K.tables + K.off[SINK_T_HORIZON]);
    v.horizonValues = (const double*)(K.tables + K.off[SINK_T_HORIZON_VALUES]);
    v.layerTables = (const double*)(K.tables + K.off[SINK_T_THICK]);
    v.sink = K.nodes;
    v.area = K.area;
    v.ns = I.v.ns; v.nCells = K.nCells; v.nrLayers = K.nrLayers; v.nUnits = K.nUnits; v.nSoils = K.nSoils;
    v.lastEvapLayer = K.lastEvapLayer; v.flag = K.flag;
    K.crackComputed = false;
    if (!call.crackMaxDepth) e = raster_launch(k_sink_hour, n, v, K.lastMs);
    else {
        /* soil cracking: one block of its own - SinkCrackDev, maxDepth, layerDepth, crackWater (doubles), then lastLayer and precSurfaceWater (4 bytes) */
        const size_t ns8 = K.nSoils, nl8 = K.nrLayers;
        if (!K.crack) { RASTER_TRY(hipMalloc((void**)&K.crack, sizeof(SinkCrackDev) + (ns8 + nl8 + n) * 8 + (ns8 + n) * 4 + 8)); K.crackVer = 0; K.crackDev = SinkCrackDev{}; }
        double* const maxDepth = (double*)(K.crack + sizeof(SinkCrackDev));
        double* const layerDepth = maxDepth + ns8;
        double* const crackWater = layerDepth + nl8;
        int32_t* const lastLayer = (int32_t*)(crackWater + n);
        float* const precSurfaceWater = (float*)(lastLayer + ns8);
        if (K.crackVer != call.crackVer) {
            RASTER_TRY(hipMemcpyAsync(maxDepth, call.crackMaxDepth, ns8 * 8, hipMemcpyHostToDevice, I.stream));
            RASTER_TRY(hipMemcpyAsync(layerDepth, K.layerDepth.data(), nl8 * 8, hipMemcpyHostToDevice, I.stream));
            RASTER_TRY(hipMemcpyAsync(lastLayer, call.crackLastLayer, ns8 * 4, hipMemcpyHostToDevice, I.stream));
            RASTER_TRY(hipStreamSynchronize(I.stream));
            K.crackVer = call.crackVer;
        }
        const SinkCrackDev d{I.v.pond, maxDepth, lastLayer, layerDepth, precSurfaceWater, crackWater};
        if (std::memcmp(&d, &K.crackDev, sizeof d) != 0) {                /* (the pond array moves with a new model) */
            K.crackDev = d;
            RASTER_TRY(hipMemcpyAsync(K.crack, &K.crackDev, sizeof d, hipMemcpyHostToDevice, I.stream));
        }
        SinkCrackView k{};
        k.s = v; k.k = (const SinkCrackDev*)K.crack;
        e = raster_launch(k_sink_hour_crack, n, k, K.lastMs);
        if (e == SF3D_OK) K.crackComputed = true;
    }
    if (e == SF3D_OK) {
        K.computed = true;
        K.liquidRead = v.liquid; K.liquidFrom = call.liquid ? 0 : call.liquidFromMeteo ? FEED_METEO : FEED_SNOW;      /* what k_hour_totals sums (sf3d_hour.inc) */
    }
    return e;
}

sf3d_error_t DeviceSolver::sink_download_nodes(double* dst, uint32_t count)
{
    const SinkCache& K = impl_->sink;
    if (count != K.nodesN) { snprintf(err_, sizeof(err_), "node sinks: %u nodes asked, the device holds %u", count, K.nodesN); return SF3D_SOLVER_ERROR; }
    return raster_download(dst, K.nodes, (size_t)count * sizeof(double));
}

sf3d_error_t DeviceSolver::sink_download_cells(int map, double* dst)
{
    const SinkCache& K = impl_->sink;
    return raster_download(dst, raster_cell_map(K.cells, K.nCells, map), (size_t)K.nCells * sizeof(double));
}

bool DeviceSolver::sink_crack_computed() const { return sink_computed() && impl_->sink.crack && impl_->sink.crackComputed; }

sf3d_error_t DeviceSolver::sink_download_crack(float* precSurfaceWater, double* crackWater)
{
    const SinkCache& K = impl_->sink;
    const size_t n = K.nCells;
    const double* const water = (const double*)(K.crack + sizeof(SinkCrackDev)) + K.nSoils + K.nrLayers;
    const float* const prec = (const float*)((const int32_t*)(water + n) + K.nSoils);
    sf3d_error_t e = SF3D_OK;
    if (precSurfaceWater) e = raster_download(precSurfaceWater, prec, n * sizeof(float));
    if (e == SF3D_OK && crackWater) e = raster_download(crackWater, water, n * sizeof(double));
    return e;
}

double DeviceSolver::sink_kernel_ms() const { return impl_ ? impl_->sink.lastMs : 0.; }
#endif
