/*
 * sf3d_model.h - host-side staging model of the MI355X soilFluxes3D library and the interface
 * of the device solver.  Setters of the C ABI only touch this staging copy (O(1) host work per
 * call, SURVEY.md 7 "chatty API"); the device is brought up to date lazily at the next
 * computeStep / initializeBalance, and getters pull a field back only when the device holds a
 * newer version of it.
 */
#ifndef SF3D_MODEL_H
#define SF3D_MODEL_H

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "sf3d.h"
#include "sf3d_device.h"

struct SoilHost {                      /* soilData_t, types.h:104-121 */
    uint16_t soilNumber; uint8_t horizonNumber;
    double alpha, n, m, he, Sc, thetaS, thetaR, Ksat, L, organicMatter, clay;
    double mualemDen;                  /* 1 - (1 - Sc^(1/m))^m, soilPhysics.cpp:201-204 */
};

struct ParamsHost {                    /* SolverParameters, types.h:291-315 (persist across re-init) */
    double MBRThreshold = 1e-3, residualTolerance = 1e-10;
    double dtMin = 1, dtMax = 600, dtCurr = SF3D_NODATA;
    uint16_t maxApprox = 10, maxIter = 200;
    uint8_t wrc = SF3D_WRC_MODIFIED_VAN_GENUCHTEN, meanType = SF3D_MEAN_LOGARITHMIC;
    double lvRatio = 4., courantThreshold = 0.5, instabilityFactor = 10.;
    double heatWeightFactor = 0.5;     /* types.h:307 */
    uint32_t numThreads = 1;
    bool lineal = false;               /* setUseLineal(true) AND SF3D_LINEAL_DEVICE_CG=1: device conjugate gradients instead of Jacobi sweeps */
};

struct Partition;
struct HostModel {
    bool initialized = false, solverReady = false;
    bool water = true, heat = false, solutes = false;
    bool cgArrays = false;           /* allocate the conjugate-gradient work vectors (SF3D_LINEAL_DEVICE_CG=1 at sf3d_initialize) */
    bool compat = false;             /* SF3D_COMPAT_STALE_LINK_FLOW=1 at sf3d_initialize: reproduce quirk 1's stale-slot reads */
    uint32_t N = 0, ns = 0;
    std::vector<double> x, y, z, size;
    std::vector<uint8_t> surf, hasClass;
    std::vector<uint16_t> cls;
    std::vector<uint8_t> btype;
    std::vector<double> bslope, bsize, bflowRate, bflowSum, prescribed;
    std::vector<uint8_t> nLat;
    std::vector<uint8_t> ltype[SF3D_SLOTS];
    std::vector<uint32_t> lto[SF3D_SLOTS];
    std::vector<double> larea[SF3D_SLOTS], lflowSum[SF3D_SLOTS];
    std::vector<double> Se, K, H, sink, pond;
    std::vector<SoilHost> soils;
    std::vector<double> roughness;
    /* coupled heat transport (heat.cpp): flags, state, atmosphere / fixed-temperature boundary inputs, boundary outputs */
    bool heatVapor = false, heatAdvection = false; uint8_t heatSave = 0;
    std::vector<double> temperature, heatSink;
    std::vector<double> bHeightWind, bHeightT, bRoughH, bT, bRH, bWind, bNetIrr, bFixT, bFixDepth;
    std::vector<double> bAero, bSoilCond, bSens, bLat, bRad, bAdv;
    std::vector<double> lfluxCache[SF3D_FLUX_TYPES]; bool lfluxValid[SF3D_FLUX_TYPES] = {false};   /* [10][N], fetched on demand */
    bool heatStateDirty = true, heatSinkDirty = true, heatBoundaryDirty = true;
    bool hostStaleHeat = false;      /* temperature and boundary outputs are newer on the device */

    /* what the device lacks */
    bool graphDirty = true;      /* topology / classes / boundary geometry: rebuild + full upload */
    bool stateDirty = true;      /* H (and Se, K) set through the API                             */
    bool sinkDirty = true, pondDirty = true, boundaryDirty = true, flowSumsDirty = true;
    bool ctrlDirty = true;       /* parameters or balances edited on the host                     */
    uint32_t sinkLo = 0, sinkHi = UINT32_MAX;   /* node range [lo, hi) touched since the last sink upload (hourly sinks usually cover the
                                                  * surface nodes only: 2 MB instead of 42 MB at 512 x 512 x 20) */
    /* multi-GPU, strip-local models (sf3d_api.cpp LocalModel): this model holds only the nodes a rank's rows touch (owned + one-cell
     * halo) in LOCAL numbering; the partition comes ready-made in local indices and the mean norm of the Jacobi sweep divides by the
     * GLOBAL node count */
    const struct Partition* presetPartition = nullptr;
    uint32_t globalN = 0;                       /* 0: this IS the global model */
    /* what the host lacks (device is newer) */
    bool hostStaleState = false; /* H, Se, K                                                      */
    bool hostStaleFlows = false; /* bflowRate, bflowSum, lflowSum                                 */
};

/* The two-colour heat sweep (sf3d_heat.inc: odd layers from the old iterate, then even layers with their Up / Down neighbours taken
 * from the values the first half has just written) is a valid, deterministic Gauss-Seidel ordering only if "layer parity" colours the
 * vertical links: layer = hops to the surface through the Up links, defined where the node above has the SMALLER index (layer-major
 * numbering), and every Up / Down link must join nodes of opposite parity.  A numbering the API accepts but this does not hold for
 * (bottom-up columns, a Down link whose target's Up is another node) would make the second half read same-colour values that the
 * same launch is writing - a race (round 4's advice).  Such graphs keep the Jacobi sweep. */
inline bool heat_two_colour_valid(const HostModel& m)
{
    std::vector<uint8_t> lp(m.N, 0);
    for (uint32_t i = m.ns; i < m.N; ++i)
        if (m.ltype[0][i] != SF3D_LINK_NONE) {
            if (m.lto[0][i] >= i) return false;
            lp[i] = (uint8_t)(lp[m.lto[0][i]] + 1);
        }
    for (uint32_t i = m.ns; i < m.N; ++i)
        for (int s = 0; s < 2; ++s)
            if (m.ltype[s][i] != SF3D_LINK_NONE && ((lp[i] ^ lp[m.lto[s][i]]) & 1u) == 0u) return false;
    return true;
}

/* Row-strip partition of the node graph for `world` ranks (host logic, no device needed):
 * a node belongs to the rank that owns its surface-cell column (the surface node reached by
 * walking Up links); surface nodes [0, ns) are cut into `world` contiguous index ranges at
 * multiples of 64.  send[p] / recv[p] are the sorted unique node lists exchanged with rank p
 * (what p's rows read from my strip / what my rows read from p's strip). */
#define SF3D_OWNER_NONE 255u       /* Partition::owner of a node that was never staged on this rank (strip-local build) */
struct Partition {
    int world = 1, rank = 0;
    std::vector<uint8_t> owner;                       /* [N]; SF3D_OWNER_NONE: absent */
    uint32_t missingFrom = UINT32_MAX, missingTo = UINT32_MAX;   /* first link from one of this rank's nodes to an absent node (SF3D_MISSING_DATA_ERROR) */
    std::vector<uint32_t> bounds;                     /* [world + 1] surface-index strip bounds */
    std::vector<std::vector<uint32_t>> send, recv;    /* [world] */
};
sf3d_error_t sf3d_compute_partition(const HostModel& m, int rank, int world, Partition& out);
sf3d_error_t sf3d_partition_bounds(uint32_t ns, int world, uint32_t* bounds);      /* [world + 1] surface-index strip bounds: a function of ns and world alone */

/* what each rank publishes to the others before the first step (sf3d_dist_export/connect) */
struct DistBlob {
    unsigned char ipcHandle[64];
    uint64_t recvOff[SF3D_MAX_RANKS];
    uint32_t recvCount[SF3D_MAX_RANKS];
    uint32_t world, rank;
    uint64_t nodes;
    uint32_t generation;            /* export count of the rank; rank 0's value stamps the self-check token of a connect */
    uint32_t heatJacobiOnly;        /* 1: this rank's part of the graph does not admit the two-colour heat sweep (heat_two_colour_valid): every rank then sweeps by Jacobi */
    unsigned char ncclId[128];     /* rank 0: ncclUniqueId of the run's RCCL communicator (all zero when RCCL is not available) */
    char pciBusId[32];             /* which physical GPU the rank runs on (start-up self-check: distinct, peer-reachable devices) */
    char shmName[48];              /* POSIX shared-memory object holding a second copy of the rank's window in HOST memory: the fall-back
                                    * transport when the device windows cannot be opened or do not carry device-initiated stores */
    uint64_t windowBytes;
    uint32_t resBlocks, resCapacity; /* resident sweep loop (sf3d_resident.inc): blocks of this rank's grid (0: its strip does not fit, or the loop is off) and how many such
                                      * blocks its GPU holds at once - the loop runs on every rank or on none (its edge rows hand over tagged records, the single
                                      * sweeps plain values), and ranks that share a GPU must fit on it TOGETHER (persistent kernels that have to take turns
                                      * wait for each other's time slices) */
    uint32_t pairRecords, pairPad;   /* paired pass with record hand-over (sf3d_pair.inc, DIST): nonzero = this rank runs the paired pass and hands its edge rows over as
                                      * records - used only if EVERY rank says so (a rank on single sweeps puts plain values and needs two exchanges per two iterations) */
};

/* what include/sf3d_maps.h set, in the numbering of the model the device works on (sf3d_api.cpp hands it over per map call; the device
 * uploads a part only when its version differs from the one it holds) */
struct MapsInput {
    uint32_t nCells = 0, nLayers = 0;
    const int32_t* col = nullptr;      /* [nLayers][nCells] node or -1 */
    const double* thick = nullptr;     /* [nLayers] */
    uint64_t colVer = 0;
    const double* slope = nullptr;     /* [2][nCells] tanAngle, sin(2 slopeAngle); null until set */
    uint64_t slopeVer = 0;
    const MapGeo* geo = nullptr;       /* [soil classes] */
    uint32_t nGeo = 0;
};

/* The device half.  All methods return an sf3d_error_t; HIP failures map to SF3D_SOLVER_ERROR
 * and leave a message retrievable with last_error(). */
class DeviceSolver {
public:
    static DeviceSolver& instance();
    sf3d_error_t set_device(int dev);
    /* bring the device up to date with every dirty part of `m` (allocates on first use) */
    sf3d_error_t sync_to_device(HostModel& m, const ParamsHost& p);
    /* one computeStep: returns the accepted dt through *dt and refreshes the Ctrl mirror */
    sf3d_error_t step(HostModel& m, ParamsHost& p, double maxTimeStep, double* dt);
    /* storage = sum(theta * size) over the device state (water.cpp:71-90) */
    sf3d_error_t total_water_content(HostModel& m, const ParamsHost& p, double* out);
    sf3d_error_t fetch_state(HostModel& m);      /* H, Se, K   -> host */
    sf3d_error_t fetch_flows(HostModel& m);      /* flow sums  -> host */
    /* heat */
    sf3d_error_t fetch_heat(HostModel& m);       /* temperature, boundary fluxes and conductances -> host */
    sf3d_error_t fetch_link_flux(HostModel& m, int type);   /* one flux type [10][N] -> m.lfluxCache[type] */
    sf3d_error_t heat_query(HostModel& m, const ParamsHost& p, int what, uint32_t node, double h, double* out);
    sf3d_error_t heat_storage(HostModel& m, const ParamsHost& p, double* out);   /* computeCurrentHeatStorage() */
    sf3d_error_t release();
    sf3d_error_t synchronize();
    Ctrl& ctrl() { return mirror_; }
    void push_ctrl() { ctrlEdited_ = true; }
    bool ready() const { return built_; }
    bool connected() const { return world_ > 1 && connected_; }   /* a multi-rank model whose windows are set up */
    const char* last_error() const { return err_; }
    /* true after a failure that leaves the device state unusable (peer time-out of the multi-GPU exchange, a heat step that
     * did not start, a HIP error): computeStep then refuses to go on instead of stalling once more per call */
    bool fatal() const { return fatal_; }
    /* multi-GPU */
    sf3d_error_t dist_prepare(int rank, int world);
    sf3d_error_t dist_export(HostModel& m, const ParamsHost& p, DistBlob* out);
    sf3d_error_t dist_connect(const DistBlob* all);
    int dist_status() const { return distStatus_; }
    int dist_transport() const;
    sf3d_error_t dist_stats(double* out, int capacity);
    void print_hops() const;
    sf3d_error_t dist_finalize(int mode);      /* 0 device windows (all ranks passed), 1 RCCL (opt-in), 2 host-memory windows (fall-back) */
    int world() const { return world_; }
    int rank() const { return rank_; }
    /* instrumentation */
    sf3d_error_t timing(int mode);               /* 0 off, 1 all node kernels, 2 only the Jacobi sweep */
    sf3d_error_t stats(int kid, uint64_t* launches, double* ms, uint64_t* nodes);
    static const char* kernel_name(int kid);
    sf3d_error_t device_log(uint32_t n, const double* x, double* out, int which = 0);   /* test hook: the kernels' log (0) / exp (1) / cbrt (2) */
    sf3d_error_t device_pow(uint32_t n, const double* x, const double* y, double* out);   /* test hook: the property kernels' pow */
    sf3d_error_t device_norm_sum(uint32_t n, const double* x, uint32_t blocks, int assoc, double* out);   /* test hook: the sweep kernels' double-double norm sum */
    uint64_t device_bytes() const;               /* bytes of device memory the model's arrays take (sum of the allocations) */
    /* output maps (sf3d_maps.inc): variable `var` of criteria3DVariable on layer `layer` (-1: all) of the accepted state -> out (floats);
     * *missing = 1 when a factor of safety needed a soil class without geotechnics */
    sf3d_error_t output_map(HostModel& m, const ParamsHost& p, const MapsInput& in, int var, int layer, float flag, float* out, int* missing);
    /* hourly snow model (sf3d_snow.inc): SNOW_MAPS float maps of nCells on the device, independent of the node model (release() keeps
     * them); map = index into the block (SNOW_MAP_*).  snow_hour_done: an hour has run on nCells cells, so its inputs and outputs are in the
     * block for the crop and sink blocks to read */
    sf3d_error_t ensure_device();                /* device choice and the solver's stream, without a model */
    sf3d_error_t snow_alloc(uint32_t nCells);
    sf3d_error_t snow_upload(int map, const float* src);
    sf3d_error_t snow_download(int map, float* dst);
    sf3d_error_t snow_hour(const float* const in[8], const SnowParamsDev& p, float flag, const uint8_t* mine);
    bool snow_hour_done(uint32_t nCells) const;
    bool snow_inputs_held(uint32_t nCells) const;      /* ... and the input maps of that hour are still where it read them */
    sf3d_error_t snow_free();
    double snow_kernel_ms() const;
    /* hourly ET0 / daily crop maps (sf3d_crop.inc): CROP_MAPS maps of nCells on the device and the crop table, independent of the node
     * model as the snow maps are; in == nullptr: k_et0_hour reads the five maps the last snow_hour left in the snow block.  crop_allocated:
     * the block holds nCells cells, so its ET0, LAI and degree-day maps are there for the root and sink blocks to read */
    sf3d_error_t crop_alloc(uint32_t nCells, const CropUnitDev* units, uint32_t nUnits);
    sf3d_error_t crop_upload(int map, const void* src);
    sf3d_error_t crop_download(int map, float* dst);
    bool crop_allocated(uint32_t nCells) const;
    sf3d_error_t crop_hour(const float* const in[5], float clearSky, float flag, const uint8_t* mine);
    sf3d_error_t crop_day(int dateDoy, int currentDoy, double latitude, float flag, const uint8_t* mine);
    sf3d_error_t crop_free();
    double crop_kernel_ms(int which) const;
    /* root length / depth / density maps (sf3d_root.inc): the per-cell maps, the tables and the keyed density table, independent of the
     * node model as the snow and crop maps are; dd == nullptr: k_root_cell reads the degree-day map of the crop block.  root_computed:
     * root_compute has run on nCells cells and nrLayers layers, so the sink block may read its maps and its density table */
    sf3d_error_t root_alloc(const RootSetup& setup);
    sf3d_error_t root_compute(const float* dd, float flag, const uint8_t* mine);
    bool root_computed(uint32_t nCells, uint32_t nrLayers) const;
    sf3d_error_t root_download(int map, void* dst);
    sf3d_error_t root_density(int layer, double* dst, float flag);
    sf3d_error_t root_free();
    double root_kernel_ms(int which) const;
    uint32_t root_table_rows() const;
    /* hourly meteo maps from station data (sf3d_meteo.inc): the DEM, the proxy rasters and one map per variable, independent of the node
     * model as the snow, crop and root maps are */
    sf3d_error_t meteo_alloc(uint32_t nRows, uint32_t nCols, const float* dem, float flag, double xll, double yll, double cellSize, uint32_t nProxies,
                             const float* const* proxyMaps);
    sf3d_error_t meteo_interpolate(const MeteoCall& call, const uint8_t* mine, float* out);
    sf3d_error_t meteo_download(int var, float* dst);
    sf3d_error_t meteo_upload(int var, const float* src);      /* the caller's map in the place of an interpolation: meteo_produced holds afterwards */
    sf3d_error_t meteo_free();
    double meteo_kernel_ms() const;
    bool meteo_produced(int var, uint32_t nRows, uint32_t nCols) const;   /* the block is on this raster and holds an interpolation of `var` */
    /* topographic distance on the meteo block's raster (sf3d_topodist.inc; the caller has checked that the raster is there and the call
     * against the caps and the maps held): the maps of gis::topographicDistanceMap, interpolate() under getUseTD() into the meteo block's
     * slot of the variable, and the station matrix.  The maps go with the raster (meteo_free).  which of topo_kernel_ms: 0 k_topodist_maps,
     * 1 k_meteo_idw_td, 2 k_topodist_matrix */
    sf3d_error_t topo_compute(uint32_t nPoints, const double* x, const double* y, const double* z, const uint8_t* mine);
    sf3d_error_t topo_download(uint32_t index, float* dst);
    sf3d_error_t topo_upload(uint32_t index, const float* src);
    sf3d_error_t topo_interpolate(const MeteoCall& call, const TopoCall& topo, const uint8_t* mine, float* out);
    sf3d_error_t topo_matrix(uint32_t nPoints, const double* x, const double* y, const double* z, const int32_t* mapIndex, float* matrix);
    sf3d_error_t topo_free();
    double topo_kernel_ms(int which) const;
    /* air and dew-point temperature with local detrending on the meteo block's raster (sf3d_localdetrend.inc; the caller has checked that
     * the raster is there and the call against the caps): the map into the meteo block's slot of the variable, and the per-cell outcome of
     * the last call (localdetrend_done: it is there).  The outcome goes with the raster (meteo_free). */
    sf3d_error_t localdetrend_interpolate(const MeteoCall& call, const LocalDetrendCall& local, const uint8_t* mine, float* out);
    bool localdetrend_done() const;
    sf3d_error_t localdetrend_fit(uint8_t* significant, float* r2, double* parameters);
    sf3d_error_t localdetrend_selection(uint32_t* count, float* radius);
    uint64_t localdetrend_bytes() const;
    sf3d_error_t localdetrend_free();
    double localdetrend_kernel_ms() const;
    /* the same with every active proxy (sf3d_localproxies.inc): the elevation's outcome goes where localdetrend_interpolate leaves its
     * own, the interpolated count and the proxies' lines (slope, intercept per slot) are this block's; meteo_has_map: the block holds a
     * raster for the proxy slot */
    sf3d_error_t localproxies_interpolate(const MeteoCall& call, const LocalProxiesCall& local, const uint8_t* mine, float* out);
    bool localproxies_done() const;
    bool meteo_has_map(uint32_t proxy) const;
    sf3d_error_t localproxies_interpolated(uint32_t* count);
    sf3d_error_t localproxies_fit(uint8_t* significant, double* lines);
    uint64_t localproxies_bytes() const;
    sf3d_error_t localproxies_free();
    double localproxies_kernel_ms() const;
    /* glocal detrending (sf3d_glocal.inc): the macro areas' tables belong to the meteo block's raster and go with it (meteo_free);
     * glocal_interpolate runs k_glocal_areas and k_glocal_cells into the meteo block's slot of the variable - SF3D_MISSING_DATA_ERROR
     * where an interpolate() gave NODATA, and the slot is then not produced; glocal_records: what k_glocal_areas left of the last call and
     * the proxies it ran with.  which of glocal_kernel_ms: 0 k_glocal_areas, 1 k_glocal_cells */
    sf3d_error_t glocal_set(const GlocalStatic& g);
    bool glocal_areas_set() const;
    sf3d_error_t glocal_interpolate(const MeteoCall& call, const GlocalCall& g, const uint8_t* mine, float* out);
    bool glocal_done() const;
    sf3d_error_t glocal_records(GlocalAreaDev* area, float* detrended, uint8_t* kept, LocalProxiesSetup* proxies);
    uint64_t glocal_bytes() const;
    sf3d_error_t glocal_free();
    double glocal_kernel_ms(int which) const;
    /* multiple detrending without areas (sf3d_multidetrend.inc): multidetrend_interpolate runs k_multidetrend_fit and, behind it on the
     * same stream, k_multidetrend_cells into the meteo block's slot of the variable; multidetrend_points evaluates the last call's fit
     * and kept stations at a list of points (k_multidetrend_points); multidetrend_records: what k_multidetrend_fit left of the last
     * call, its station count and the proxies it ran with.  which of multidetrend_kernel_ms: 0 fit, 1 cells, 2 points */
    sf3d_error_t multidetrend_interpolate(const MeteoCall& call, const MultiDetrendCall& g, const uint8_t* mine, float* out);
    bool multidetrend_done() const;
    sf3d_error_t multidetrend_points(uint32_t nPoints, uint32_t nProxies, const float* x, const float* y, const float* proxyValues, float* out);
    sf3d_error_t multidetrend_records(MultiDetrendRecord* record, float* detrended, uint8_t* kept, LocalProxiesSetup* proxies);
    uint64_t multidetrend_bytes() const;
    sf3d_error_t multidetrend_free();
    double multidetrend_kernel_ms(int which) const;
    /* hourly r.sun radiation maps (sf3d_rad.inc): the five outputs and the static maps, independent of the node model as the other raster
     * blocks; transmissivity == nullptr: k_rad_hour reads the map the meteo block holds (the caller asks meteo_produced first) */
    sf3d_error_t rad_alloc(const RadSetup& setup);
    sf3d_error_t rad_hour(const RadHourDev& hour, const float* transmissivity, const uint8_t* mine);
    sf3d_error_t rad_download(int which, float* dst);
    bool rad_hour_done(uint32_t nRows, uint32_t nCols) const;    /* an hour has run on this raster and the transmissivity map it read is still there */
    sf3d_error_t rad_free();
    double rad_kernel_ms() const;
    sf3d_error_t rad_trig(int which, uint32_t n, const double* x, const double* y, double* out);     /* test hook: the device build of sf3d_trig.inc */
    /* station transmissivity and its window (sf3d_transmissivity.inc) on the raster of the radiation block (the caller has checked that it
     * is allocated): one launch over call.nPoints x call.nSlots evaluations; the scratch is the radiation block's and goes with rad_free.
     * tr_evaluated: the last call held this many points and slots, so tr_evaluations may copy them out */
    sf3d_error_t tr_run(const TrCall& call, float* transmissivity, int32_t* windowSteps);
    bool tr_evaluated(uint32_t nPoints, uint32_t nSlots) const;
    sf3d_error_t tr_evaluations(uint8_t* written, float* elevationRefr, double* global);
    double tr_kernel_ms() const;
    /* hourly evaporation, transpiration and rain sinks (sf3d_sink.inc): the per-cell maps and the tables belong to the raster as the other
     * blocks' do, the node array to the model on the device (release() frees it); sink_hour reads the accepted state after sync_to_device as
     * output_map does and the root block's maps, and, where a map of `call` is null, the crop / snow block's */
    sf3d_error_t sink_alloc(const SinkSetup& setup);
    bool sink_allocated() const;
    sf3d_error_t sink_hour(HostModel& m, const ParamsHost& p, const MapsInput& in, const SinkCall& call);
    sf3d_error_t sink_download_nodes(double* dst, uint32_t count);     /* the device model's numbering */
    sf3d_error_t sink_download_cells(int map, double* dst);
    sf3d_error_t sink_download_crack(float* precSurfaceWater, double* crackWater);
    bool sink_crack_computed() const;
    bool sink_computed() const;
    sf3d_error_t sink_free();
    double sink_kernel_ms() const;
    /* the hour, device to device (sf3d_hour.inc, include/sf3d_hour.h): the snow and ET0 kernels on the maps the meteo and radiation blocks
     * hold (the caller has asked meteo_produced and rad_hour_done), the relative humidity map from the dew point map, the hour's three
     * totals, the day's pond per cell (computeCrop: with the crop block's LAI map; the caller has asked crop_allocated).  which of
     * hour_kernel_ms: 0 k_hour_relhum, 1 k_hour_totals, 2 k_hour_pond */
    sf3d_error_t hour_snow(const float* surfaceWater, const SnowParamsDev& p, float flag, const uint8_t* mine);
    sf3d_error_t hour_et0(float clearSky, float flag, const uint8_t* mine);
    sf3d_error_t hour_relhum(const uint8_t* mine, float* out);
    bool hour_totals_ready(uint32_t nCells) const;     /* a sink hour has run on nCells cells and the liquid water map it read is still there */
    sf3d_error_t hour_totals(HostModel& m, const ParamsHost& p, const MapsInput& in, const uint8_t* mine, double totals[3]);
    sf3d_error_t hour_pond(HostModel& m, const ParamsHost& p, const MapsInput& in, const HourPondSetup& setup, bool computeCrop, float laiFlag, const uint8_t* mine, float* out);
    sf3d_error_t hour_free();
    double hour_kernel_ms(int which) const;

private:
    DeviceSolver() = default;
    /* what the five raster blocks and the output maps share (sf3d_maps.inc): the column table of the device's model (output_map and
     * sink_hour), a copy on the solver's stream that returns once it is done, the ownership mask of a strip on the device (null stays
     * null), kernel<<<ceil(count / SF3D_BLOCK), SF3D_BLOCK>>>(arg) with its event-timed milliseconds (0 when timing is off) in `ms`, one
     * device block for a list of tables, and the release of a block's device memory */
    sf3d_error_t raster_columns(HostModel& m, const ParamsHost& p, const MapsInput& in);
    sf3d_error_t raster_upload(void* dev, const void* host, size_t bytes);
    sf3d_error_t raster_download(void* host, const void* dev, size_t bytes);
    sf3d_error_t raster_mask(const uint8_t* mine, size_t nCells, const uint8_t** dev);
    template <class Arg> sf3d_error_t raster_launch(void (*kernel)(Arg), size_t count, const Arg& arg, double& ms, uint32_t gridY = 1);
    sf3d_error_t meteo_view(const MeteoCall& call, const uint8_t* mine, MeteoView& v);       /* sf3d_meteo.inc: the station table and the view of a call */
    sf3d_error_t topo_tables(uint32_t n, const double* x, const double* y, const double* z, const int32_t* mapIndex,
                             const double*& dx, const double*& dy, const double*& dz, const int32_t*& dm);      /* sf3d_topodist.inc: a call's point tables */
    sf3d_error_t raster_tables(char*& tables, size_t* off, int count, const size_t* bytes, const void* const* src, const size_t* srcBytes);
    void raster_release(std::initializer_list<void*> blocks);
    /* block `who` (FEED_*) is about to free its maps: what other blocks hold of them is forgotten, so their next reader is refused */
    void raster_unbind(int who);
    sf3d_error_t snow_launch(const float* const in[8], int feeds, const SnowParamsDev& p, float flag, const uint8_t* mine);
    sf3d_error_t crop_launch(const float* const in[5], float clearSky, float flag, const uint8_t* mine);
    /* the three largest device-side stages of the build block of sync_to_device (sf3d_host_build.inc): the multi-GPU window set-up, the
     * resident loop's plan with its occupancy queries, the coupled-heat arrays with their colouring and Gauss-Seidel levels.  BuildState
     * is what one build's stages share */
    struct BuildState;
    sf3d_error_t build_dist_window(BuildState& st);
    sf3d_error_t build_resident_plan(const HostModel& m, BuildState& st);
    sf3d_error_t build_heat(HostModel& m, const ParamsHost& p, BuildState& st);
    /* the parts of step (sf3d_host_step.inc): the water part and the heat part each queue guarded launches and poll the control block
     * until their state machine ends (`stage`: where the water part ended); step_finish takes the step again where the resident loop gave
     * up, and otherwise hands the step's results and errors to the caller.  StepCtx is what the parts of one step share */
    struct StepCtx;
    sf3d_error_t step_water(StepCtx& c, double maxTimeStep, uint32_t& stage);
    sf3d_error_t step_heat(StepCtx& c, HostModel& m, double maxTimeStep, uint32_t& stage);
    sf3d_error_t step_finish(HostModel& m, ParamsHost& p, double maxTimeStep, double* dt, uint32_t stage);
    struct Impl;
    Impl* impl_ = nullptr;
    Ctrl mirror_{};
    bool built_ = false, ctrlEdited_ = false;
    int world_ = 1, rank_ = 0;
    bool connected_ = false;
    bool fatal_ = false;
    int distStatus_ = 0;             /* after dist_connect: 0 the windows passed their self-check, 1 they did not / RCCL was asked for */
    char distWhy_[200] = {0};
    char err_[256] = {0};
    friend struct Impl;
};

#endif
