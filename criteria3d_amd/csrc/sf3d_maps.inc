/* part of sf3d_solver.hip (included there after host_step) - the output layer of the application on the device: per-layer maps of every
 * variable getCriteria3DVar serves (project3D.cpp:2756-2810, through Project3D::computeCriteria3DMap :1896-1948), the infinite-slope factor
 * of safety (computeFactorOfSafety :2614-2721) and the whole-column maps computeMinimumFoS (:2128-2157) and computeAvgDegreeOfSaturation
 * (:2076-2125).  One thread per raster cell walks its column from layer 0 down; the column table is [nLayers][nCells] (layer-major like the
 * node numbering), so the lanes of a wave read one layer of 64 neighbouring cells and write 64 consecutive floats.
 *
 * Every value is what the product's own getters return (sf3d_api.cpp "getters") for the accepted state the device holds - H of the pool
 * buffer Ctrl::cur, Se, z, the node's soil class, the link flow sums - through the same se_from_psi / ppow the property kernels use, so
 * the maps equal a host loop over the getters bit for bit.  tan / sin never run here: the host evaluates them with the C library
 * (sf3d_set_cell_slopes, sf3d_set_horizon_geotechnics) and the kernel uses IEEE + - x / and min only (-ffp-contract=off).
 *
 * Deviation: layer 0 of factorOfSafety is the flag (the application never asks for it: its depth lists are > 0 cm and computeMinimumFoS
 * starts at layer 1). */

#define MAP_GRAVITY 9.80665               /* commonConstants.h */
#define MAP_NODATA (-9999.0)
enum : int32_t {                          /* criteria3DVariable, agrolib/meteo/meteo.h:110-114 */
    MV_VWC = 0, MV_TOTAL_POTENTIAL = 1, MV_MATRIC_POTENTIAL = 2, MV_AVAILABLE_WATER = 3, MV_DEGREE_OF_SATURATION = 4, MV_AVG_DEGREE_OF_SATURATION = 5,
    MV_WATER_DEFICIT = 9, MV_WATER_INFLOW = 10, MV_WATER_OUTFLOW = 11, MV_FACTOR_OF_SAFETY = 12, MV_MINIMUM_FACTOR_OF_SAFETY = 13,
    MV_SURFACE_POND = 14, MV_MIN_VWC = 15, MV_MAX_VWC = 16
};

/* map_theta and map_sentinel also serve the host build of the sink text (tests/sink_host.cpp defines SF3D_MAPS_HOST: these two, nothing else) */
#ifndef SF3D_MAPS_HOST
#define SF3D_MAPS_FN __device__ __forceinline__
#endif
SF3D_MAPS_FN double map_theta(const SoilDev& s, double Se) { return (Se * (s.thetaS - s.thetaR)) + s.thetaR; }   /* soilPhysics.cpp:38-42 */
/* the sentinels getCriteria3DVar turns into NODATA (INDEX_ERROR, MEMORY_ERROR, TOPOGRAPHY_ERROR, MISSING_DATA_ERROR of commonConstants.h) */
SF3D_MAPS_FN bool map_sentinel(double v) { return v == -1111. || v == -2222. || v == -3333. || v == -9999.; }

#ifndef SF3D_MAPS_HOST
/* thetaFromSignedPsi for a soil node and psi < 0 (soilPhysics.cpp:50-61) */
__device__ __forceinline__ double map_theta_at(const SoilDev& s, double absPsi, uint32_t wrc) { return map_theta(s, se_from_psi(s, absPsi, wrc)); }

/* getCriteria3DVar(var, i) before its sentinel check (project3D.cpp:2756-2804 over sf3d_api.cpp's getters) */
__device__ __forceinline__ double map_node_value(const MapView& m, int32_t var, uint32_t i)
{
    const bool surf = i < m.ns;
    switch (var) {
        case MV_VWC: return surf ? (m.H[i] - m.z[i]) : map_theta(m.soils[m.cls[i]], m.Se[i]);
        case MV_TOTAL_POTENTIAL: return m.H[i];
        case MV_MATRIC_POTENTIAL: return m.H[i] - m.z[i];
        case MV_AVAILABLE_WATER: {
            if (surf) return m.H[i] - m.z[i];
            const SoilDev& s = m.soils[m.cls[i]];
            return dmax(0., map_theta(s, m.Se[i]) - map_theta_at(s, 160., m.wrc));
        }
        case MV_DEGREE_OF_SATURATION: {
            if (!surf) return m.Se[i];
            const double cur = m.H[i] - m.z[i], mx = 0.001;
            return cur <= 0 ? 0 : (cur > mx ? 1. : cur / mx);
        }
        case MV_WATER_DEFICIT: {                       /* fieldCapacity = 3.0 (project3D.cpp:2790-2795) */
            if (surf) return 0.;
            const SoilDev& s = m.soils[m.cls[i]];
            return map_theta_at(s, 3.0, m.wrc) - map_theta(s, m.Se[i]);
        }
        case MV_WATER_INFLOW:
        case MV_WATER_OUTFLOW: {
            /* lateral slots in slot order: the device keeps a node's laterals in their insertion order (sync_to_device, slot alignment) and its
             * empty slots hold 0, which neither sum takes */
            const size_t N = m.N;
            double s = 0.;
            for (int sl = 2; sl < SF3D_SLOTS; ++sl) {
                const double f = m.lflowSum[(size_t)sl * N + i];
                if (var == MV_WATER_INFLOW ? (f > 0) : (f < 0)) s += f;
            }
            return s * 1000;
        }
        case MV_SURFACE_POND: return (surf ? m.pond[i] : SF3D_VAL_INDEX_ERROR) * 1000;
        case MV_MIN_VWC: return surf ? SF3D_VAL_INDEX_ERROR : m.soils[m.cls[i]].thetaR;
        case MV_MAX_VWC: return surf ? SF3D_VAL_INDEX_ERROR : m.soils[m.cls[i]].thetaS;
        default: return SF3D_VAL_MISSING_DATA_ERROR;
    }
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_output_map(MapView m)
{
    const int32_t var = m.var;
    if (var == MV_AVAILABLE_WATER || var == MV_WATER_DEFICIT) fm_init();     /* (uniform branch) the pow tables */
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m.nCells) return;
    const size_t nc = m.nCells;
    const float flag = m.flag;

    if (var == MV_FACTOR_OF_SAFETY || var == MV_MINIMUM_FACTOR_OF_SAFETY) {
        const bool minimum = var == MV_MINIMUM_FACTOR_OF_SAFETY;
        if (!minimum && m.lay0 == 0) m.out[c] = flag;                     /* layer 0: see the head of this file */
        const double tanAngle = m.slope[c], sin2 = m.slope[nc + c];
        /* weightSum: the surface water term, then (bulkDensity + theta) g thickness of every layer down to the one asked for - the reference
         * sums it from scratch per layer, in this same order, so a running sum has the same bits */
        double weightSum = 0.;
        const int32_t s0 = m.col[c];
        if (s0 >= 0) {
            const double surfaceWater = m.H[s0] - m.z[s0];
            if (surfaceWater > 0) weightSum += (surfaceWater * MAP_GRAVITY);
        }
        double minimumValue = MAP_NODATA;
        const uint32_t last = minimum ? m.nLayers : m.lay1;
        for (uint32_t l = 1; l < last; ++l) {
            const int32_t n = m.col[(size_t)l * nc + c];
            float fos = (float)MAP_NODATA;
            if (n >= 0) {
                const MapGeo g = m.geo[m.cls[n]];
                if (g.present == 0.) *m.missing = 1;
                const double theta = map_theta(m.soils[m.cls[n]], m.Se[n]);
                const double unitWeight = (g.bulkDensity + theta) * MAP_GRAVITY;
                weightSum += unitWeight * m.thick[l];
                const double frictionEffect = g.tanFriction / tanAngle;
                const double saturationDegree = m.Se[n];
                const double matricPotential = dmin(0.0, (m.H[n] - m.z[n]) * MAP_GRAVITY);
                const double suctionStress = matricPotential * saturationDegree;
                const double rootCohesion = 0.;
                const double cohesionEffect = 2 * (g.cohesion + rootCohesion) / (weightSum * sin2);
                const double suctionEffect = (suctionStress * (tanAngle + 1 / tanAngle) * g.tanFriction) / weightSum;
                fos = (float)(frictionEffect + cohesionEffect - suctionEffect);
            }
            if (minimum) {
                const double v = fos;
                if (fabs(v - MAP_NODATA) < 0.00001) continue;                                   /* isEqual(.., NODATA) */
                if (fabs(minimumValue - MAP_NODATA) < 0.00001 || v < minimumValue) minimumValue = v;
            } else if (l >= m.lay0) {
                m.out[(size_t)(l - m.lay0) * nc + c] = ((double)fos == MAP_NODATA) ? flag : fos;
            }
        }
        if (minimum) m.out[c] = (fabs(minimumValue - MAP_NODATA) < 0.00001) ? flag : (float)minimumValue;
        return;
    }

    if (var == MV_AVG_DEGREE_OF_SATURATION) {
        float r = flag;
        if (m.col[c] >= 0) {
            double thetaS = 0, thetaR = 0, sumWC = 0;
            for (uint32_t l = 1; l < m.nLayers; ++l) {
                const int32_t n = m.col[(size_t)l * nc + c];
                if (n < 0) continue;
                double vwc = map_node_value(m, MV_VWC, (uint32_t)n);
                if (map_sentinel(vwc)) vwc = MAP_NODATA;
                if (fabs(vwc - MAP_NODATA) < 0.00001) continue;
                const double thickness = m.thick[l];
                sumWC += vwc * thickness;
                double tr = map_node_value(m, MV_MIN_VWC, (uint32_t)n); if (map_sentinel(tr)) tr = MAP_NODATA;
                thetaR += tr * thickness;
                double ts = map_node_value(m, MV_MAX_VWC, (uint32_t)n); if (map_sentinel(ts)) ts = MAP_NODATA;
                thetaS += ts * thickness;
            }
            if (sumWC > 0) r = (float)((sumWC - thetaR) / (thetaS - thetaR));
        }
        m.out[c] = r;
        return;
    }

    for (uint32_t l = m.lay0; l < m.lay1; ++l) {
        const int32_t n = m.col[(size_t)l * nc + c];
        float r = flag;
        if (n >= 0) {
            double v = map_node_value(m, var, (uint32_t)n);
            if (!map_sentinel(v)) {
                if (var == MV_VWC && l == 0) v *= 1000;       /* surface water level: [m] -> [mm] */
                r = (float)v;
            }
        }
        m.out[(size_t)(l - m.lay0) * nc + c] = r;
    }
}

/* host side: upload what changed, launch on the solver's stream after the step's work, copy the floats back.  Nothing of the solver is
 * touched: no host-mirror fetch, no stale / fresh flag, no launch of any other kernel. */
template <class T> static hipError_t maps_reserve(T*& p, size_t& cap, size_t count)
{
    if (p && cap >= count) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipMalloc((void**)&p, (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) cap = count; else p = nullptr;
    return e;
}

/* the column table of the model the device works on, for output_map and sink_hour: brings the model up to date, refuses a multi-GPU model
 * that is not connected, and uploads `col` and `thick` when their version is not the one on the device (MapsCache::colVer) */
sf3d_error_t DeviceSolver::raster_columns(HostModel& m, const ParamsHost& p, const MapsInput& in)
{
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    if (world_ > 1 && !connected_) { snprintf(err_, sizeof(err_), "multi-GPU model used before sf3d_dist_connect / sf3d_dist_finalize"); return SF3D_SOLVER_ERROR; }
    Impl& I = *impl_;
    MapsCache& C = I.maps;
    if (C.colVer == in.colVer) return SF3D_OK;
    const size_t colN = (size_t)in.nCells * in.nLayers;
    RASTER_TRY(maps_reserve(C.col, C.colCap, colN));
    RASTER_TRY(maps_reserve(C.thick, C.thickCap, in.nLayers));
    RASTER_TRY(hipMemcpyAsync(C.col, in.col, colN * 4, hipMemcpyHostToDevice, I.stream));
    RASTER_TRY(hipMemcpyAsync(C.thick, in.thick, (size_t)in.nLayers * 8, hipMemcpyHostToDevice, I.stream));
    C.colVer = in.colVer;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::output_map(HostModel& m, const ParamsHost& p, const MapsInput& in, int var, int layer, float flag, float* out, int* missing)
{
    const sf3d_error_t e = raster_columns(m, p, in);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    MapsCache& C = I.maps;
    const size_t cells = in.nCells;
    if (in.slope && C.slopeVer != in.slopeVer) {
        HIP_TRY(maps_reserve(C.slope, C.slopeCap, 2 * cells));
        HIP_TRY(hipMemcpyAsync(C.slope, in.slope, 2 * cells * 8, hipMemcpyHostToDevice, I.stream));
        C.slopeVer = in.slopeVer;
    }
    if (C.geoHost.size() != in.nGeo || (in.nGeo && std::memcmp(C.geoHost.data(), in.geo, in.nGeo * sizeof(MapGeo)) != 0)) {
        C.geoHost.assign(in.geo, in.geo + in.nGeo);
        HIP_TRY(maps_reserve(C.geo, C.geoCap, in.nGeo));
        HIP_TRY(hipMemcpyAsync(C.geo, C.geoHost.data(), in.nGeo * sizeof(MapGeo), hipMemcpyHostToDevice, I.stream));
    }
    const bool whole = var == MV_MINIMUM_FACTOR_OF_SAFETY || var == MV_AVG_DEGREE_OF_SATURATION;
    const uint32_t lay0 = whole ? 0u : (layer < 0 ? 0u : (uint32_t)layer), lay1 = whole ? 1u : (layer < 0 ? in.nLayers : (uint32_t)layer + 1);
    const size_t outN = (size_t)(lay1 - lay0) * cells;
    HIP_TRY(maps_reserve(C.out, C.outCap, outN));
    if (!C.missing) HIP_TRY(hipMalloc((void**)&C.missing, sizeof(int)));
    HIP_TRY(hipMemsetAsync(C.missing, 0, sizeof(int), I.stream));
    /* the link flow sums of the last accepted steps may still be pending: added on this stream before the kernel that reads them */
    if (var == MV_WATER_INFLOW || var == MV_WATER_OUTFLOW) HIP_TRY(I.flush_links());

    MapView mv{};
    mv.col = C.col; mv.thick = C.thick; mv.slope = C.slope; mv.geo = C.geo;
    mv.H = I.v.X[mirror_.cur]; mv.Se = I.v.Se; mv.z = I.v.z; mv.pond = I.v.pond; mv.lflowSum = I.v.lflowSum;
    mv.cls = I.v.cls; mv.soils = I.v.soils;
    mv.N = I.v.N; mv.ns = I.v.ns; mv.nCells = in.nCells; mv.nLayers = in.nLayers; mv.lay0 = lay0; mv.lay1 = lay1; mv.wrc = p.wrc;
    mv.var = var; mv.flag = flag; mv.out = C.out; mv.missing = C.missing;
    const dim3 grid((in.nCells + SF3D_BLOCK - 1) / SF3D_BLOCK);
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (I.timing) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); HIP_TRY(hipEventRecord(ev[0], I.stream)); }
    if (in.nCells) hipLaunchKernelGGL(k_output_map, grid, dim3(SF3D_BLOCK), 0, I.stream, mv);
    HIP_TRY(hipGetLastError());
    if (I.timing) HIP_TRY(hipEventRecord(ev[1], I.stream));
    HIP_TRY(hipMemcpyAsync(out, C.out, outN * sizeof(float), hipMemcpyDeviceToHost, I.stream));
    int miss = 0;
    HIP_TRY(hipMemcpyAsync(&miss, C.missing, sizeof(int), hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    if (I.timing) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
        I.launches[KID_MAPS] += 1; I.ms[KID_MAPS] += ms;
    }
    if (missing) *missing = miss;
    return SF3D_OK;
}

/* ---- shared by the six raster blocks (sf3d_snow.inc, sf3d_crop.inc, sf3d_root.inc, sf3d_meteo.inc, sf3d_sink.inc, sf3d_rad.inc) and the output maps
 * above.  A block's calls run on the solver's stream, touch nothing of the solver and synchronise the stream before they return, so the
 * caller's maps are free again and one device mask serves all of them.  The column table reaches the device through raster_columns alone
 * (the output maps and the sinks).  What one block reads from another it asks of that block's accessors, which stand in the owning
 * block's file beside the predicate that makes the read safe: snow_hour_done / snow_hour_input, snow_liquid_water (sf3d_snow.inc),
 * crop_allocated / crop_et0, crop_lai, crop_degree_days (sf3d_crop.inc), root_computed (sf3d_root.inc; its maps go to the sink kernel
 * as one block), meteo_produced / meteo_map (sf3d_meteo.inc: the transmissivity map the radiation block reads; the four maps of the hour:
 * sf3d_hour.inc), rad_hour_done / rad_global, rad_beam, rad_transmissivity_read (sf3d_rad.inc).  A block that frees its maps says so
 * (raster_unbind, sf3d_hour.inc): what another block had recorded of them - the snow hour's inputs, the transmissivity map the radiation
 * hour read, the liquid water the sink hour read - is forgotten, and the next reader is refused instead of launched on a freed pointer. */

/* a block of per-cell maps whose first two are 8-byte maps and the others 4-byte ones (RootCache::cells, SinkCache::cells) */
static void* raster_cell_map(char* cells, size_t nCells, int map)
{
    return (map < 2) ? cells + (size_t)map * nCells * 8 : cells + 16 * nCells + (size_t)(map - 2) * nCells * 4;
}

/* one block for `count` tables of bytes[k] bytes, each at a multiple of 8 (off[k]); the tables with a source are filled from it */
sf3d_error_t DeviceSolver::raster_tables(char*& tables, size_t* off, int count, const size_t* bytes, const void* const* src, const size_t* srcBytes)
{
    size_t total = 0;
    for (int k = 0; k < count; ++k) { off[k] = total; total += (bytes[k] + 7) & ~(size_t)7; }
    RASTER_TRY(hipMalloc((void**)&tables, total ? total : 8));
    for (int k = 0; k < count; ++k)
        if (src[k] && srcBytes[k]) RASTER_TRY(hipMemcpyAsync(tables + off[k], src[k], srcBytes[k], hipMemcpyHostToDevice, impl_->stream));
    return SF3D_OK;
}

/* frees a block's device memory once the stream is idle; the caller resets its cache struct */
void DeviceSolver::raster_release(std::initializer_list<void*> blocks)
{
    bool any = false;
    for (void* q : blocks) any = any || q;
    if (!any) return;
    if (impl_->stream) (void)hipStreamSynchronize(impl_->stream);
    for (void* q : blocks) if (q) (void)hipFree(q);
}

sf3d_error_t DeviceSolver::raster_upload(void* dev, const void* host, size_t bytes)
{
    RASTER_TRY(hipSetDevice(impl_->device));
    RASTER_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, impl_->stream));
    RASTER_TRY(hipStreamSynchronize(impl_->stream));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::raster_download(void* host, const void* dev, size_t bytes)
{
    RASTER_TRY(hipSetDevice(impl_->device));
    RASTER_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, impl_->stream));
    RASTER_TRY(hipStreamSynchronize(impl_->stream));
    return SF3D_OK;
}

/* strips: the mask of sf3d_maps_api.inc's mapsOwnedCells, uploaded on every call (it is derived from the column table and the partition,
 * so the buffer goes with the model: MapsCache); *dev stays null when every cell is computed */
sf3d_error_t DeviceSolver::raster_mask(const uint8_t* mine, size_t nCells, const uint8_t** dev)
{
    *dev = nullptr;
    if (!mine) return SF3D_OK;
    MapsCache& C = impl_->maps;
    RASTER_TRY(maps_reserve(C.mine, C.mineCap, nCells));
    RASTER_TRY(hipMemcpyAsync(C.mine, mine, nCells, hipMemcpyHostToDevice, impl_->stream));
    *dev = C.mine;
    return SF3D_OK;
}

template <class Arg> sf3d_error_t DeviceSolver::raster_launch(void (*kernel)(Arg), size_t count, const Arg& arg, double& ms, uint32_t gridY)
{
    Impl& I = *impl_;
    const dim3 grid((uint32_t)((count + SF3D_BLOCK - 1) / SF3D_BLOCK), gridY);
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (I.timing) { RASTER_TRY(hipEventCreate(&ev[0])); RASTER_TRY(hipEventCreate(&ev[1])); RASTER_TRY(hipEventRecord(ev[0], I.stream)); }
    hipLaunchKernelGGL(kernel, grid, dim3(SF3D_BLOCK), 0, I.stream, arg);
    RASTER_TRY(hipGetLastError());
    if (I.timing) RASTER_TRY(hipEventRecord(ev[1], I.stream));
    RASTER_TRY(hipStreamSynchronize(I.stream));
    ms = 0.;
    if (I.timing) {
        float t = 0.f;
        RASTER_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
        ms = t;
    }
    return SF3D_OK;
}
#endif
