/* part of sf3d_solver.hip (included there, in this order: physics, control, phases, host_plan, host_build, host_step) - host side, part 1: DeviceSolver::Impl, device selection, the kernel selectors and launch_view, the switches of the build and of the step driver, and sync_to_device (the stages of sf3d_host_plan.inc in their order, allocations, uploads; the multi-GPU windows, the resident loop's plan and the coupled-heat arrays in member functions of their own) */
/* ======================================================================================= */
/* host side                                                                                */
/* ======================================================================================= */

namespace {

const char* kKernelNames[KID_COUNT] = {"k_props", "k_assemble", "k_sweep", "k_post", "k_restore", "k_accept", "k_sweep_pair", "k_sweep_resident", "k_output_map"};

}  // namespace

/* compiled shapes of k_sweep_resident: K (row, layer) chunks per wave x NW waves per block (PR NZ <= K NW); smallest first */
struct ResShape { int K, NW; };
#define SF3D_RES_FOR_SHAPES(X) X(2, 5) X(2, 10) X(5, 8)
#define SF3D_RES_SHAPE(k, w) {k, w},
static const ResShape kResShapes[] = {SF3D_RES_FOR_SHAPES(SF3D_RES_SHAPE)};
#undef SF3D_RES_SHAPE

/* Every kernel of a step takes the device view by value.  A template family has one selector that returns the instantiation for run-time
 * arguments - its rows are generated from one list, the template arguments are the macro's parameters - and everything is launched by
 * launch_view.  nullptr: no such instantiation was compiled */
typedef void (*ViewKernel)(DevView);
static inline void launch_view(ViewKernel fn, dim3 grid, dim3 block, uint32_t lds, hipStream_t st, const DevView& v) { hipLaunchKernelGGL(fn, grid, block, lds, st, v); }
static ViewKernel res_kernel(int K, int NW, bool dist)
{
#define SF3D_RES_PTR(k, w) if (K == k && NW == w) return dist ? k_sweep_resident<k, w, true> : k_sweep_resident<k, w, false>;
    SF3D_RES_FOR_SHAPES(SF3D_RES_PTR)
#undef SF3D_RES_PTR
    return nullptr;
}
/* patch heights of the paired pass (pair_widx, sf3d_host_plan.inc).  records: the hand-over of records inside the launch, on a strip only */
#define SF3D_PAIR_FOR_HEIGHTS(X) X(6) X(8) X(10) X(14)
static ViewKernel pair_kernel(uint32_t W, bool nt, bool dist, bool records, bool masked)
{
#define SF3D_PAIR_PTR(w)                                                                                                                      \
    if (W == w) {                                                                                                                             \
        if (masked) return dist ? (nt ? k_sweep_pair_masked<w, true, true> : k_sweep_pair_masked<w, false, true>)                             \
                                : (nt ? k_sweep_pair_masked<w, true, false> : k_sweep_pair_masked<w, false, false>);                          \
        if (dist && records) return nt ? k_sweep_pair<w, true, true, true> : k_sweep_pair<w, false, true, true>;                              \
        return dist ? (nt ? k_sweep_pair<w, true, true> : k_sweep_pair<w, false, true>) : (nt ? k_sweep_pair<w, true, false> : k_sweep_pair<w, false, false>); \
    }
    SF3D_PAIR_FOR_HEIGHTS(SF3D_PAIR_PTR)
#undef SF3D_PAIR_PTR
    return nullptr;
}
static ViewKernel sweep_kernel(int mode, bool nt)      /* k_sweep<MODE>: 0 separate decision kernels, 1 fused decision, 2 + in-kernel exchange */
{
#define SF3D_SWEEP_PTR(m) if (mode == m) return nt ? k_sweep<m, true> : k_sweep<m, false>;
    SF3D_SWEEP_PTR(0) SF3D_SWEEP_PTR(1) SF3D_SWEEP_PTR(2)
#undef SF3D_SWEEP_PTR
    return nullptr;
}

__global__ void k_dist_ping(DistView d, unsigned long long token, long long timeoutTicks, int* out);

/* output maps (sf3d_maps.inc): device copies of what include/sf3d_maps.h set, uploaded by the first map call after a change and freed with
 * the model (release) - a rebuilt model may number its nodes differently */
struct MapsCache {
    int32_t* col = nullptr; double* thick = nullptr; double* slope = nullptr; MapGeo* geo = nullptr; float* out = nullptr; int* missing = nullptr;
    uint8_t* mine = nullptr;                    /* strips: the ownership mask of the raster call in flight (raster_mask) */
    size_t colCap = 0, thickCap = 0, slopeCap = 0, geoCap = 0, outCap = 0, mineCap = 0;
    uint64_t colVer = 0, slopeVer = 0;          /* versions of MapsInput that are on the device (0: none) */
    std::vector<MapGeo> geoHost;
    void free_all()
    {
        for (void* q : {(void*)col, (void*)thick, (void*)slope, (void*)geo, (void*)out, (void*)missing, (void*)mine}) if (q) (void)hipFree(q);
        *this = MapsCache();
    }
};

/* hourly snow model (sf3d_snow.inc): the maps of include/sf3d_snow.h; they belong to the raster and stay when the model is released */
struct SnowCache {
    float* base = nullptr; uint32_t nCells = 0; double lastMs = 0.; bool hourDone = false;
    /* the eight input maps the last hour read (snow_hour_input): slots of this block after a host-fed hour, the meteo and radiation blocks'
     * maps after sf3d_hour_snow (`feeds`: the FEED_* blocks they lie in; inputsHeld goes when one of those is freed) */
    const float* in[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int feeds = 0;
    bool inputsHeld = false;
};
/* the blocks another block may hold pointers into (DeviceSolver::raster_unbind, sf3d_hour.inc) */
enum { FEED_METEO = 1, FEED_RAD = 2, FEED_SNOW = 4 };
/* hourly ET0 and daily crop maps (sf3d_crop.inc): the maps of include/sf3d_crop.h and the crop table; as the snow maps, they belong to the raster */
struct CropCache { float* base = nullptr; CropUnitDev* units = nullptr; uint32_t nCells = 0, nUnits = 0; double lastMs[2] = {0., 0.}; };

/* root maps (sf3d_root.inc): the maps of include/sf3d_root.h, the tables and the density table; they belong to the raster too */
struct RootCache {
    char* cells = nullptr;              /* ROOT_MAP_WORDS x nCells 4-byte words: the per-cell maps */
    char* tables = nullptr;             /* units, soils, layer grid, lunette, rows, the density table: one block */
    double* out = nullptr;              /* the gathered density maps, allocated by the first getter: nrLayers x nCells */
    size_t off[16] = {0};               /* offsets of the tables in `tables` */
    uint32_t nCells = 0, nUnits = 0, nSoils = 0, nRows = 0, nrLayers = 0, lunetteMax = 0;
    bool computed = false;
    double lastMs[3] = {0., 0., 0.};
};

/* hourly meteo maps (sf3d_meteo.inc): the DEM, the proxy rasters and one map per variable of include/sf3d_meteo.h; they belong to the raster too */
struct MeteoCache {
    float* base = nullptr;              /* (1 + nProxies + METEO_VARIABLES) x nCells floats */
    char* stations = nullptr;           /* METEO_MAX_STATIONS x (x, y: doubles; value: float) */
    bool hasMap[METEO_MAX_PROXIES] = {false};
    uint32_t nCells = 0, nRows = 0, nCols = 0, nProxies = 0;
    double xll = 0., yll = 0., cellSize = 0.;
    float flag = -9999.f;
    bool produced[METEO_VARIABLES] = {false};      /* the variable's map holds an interpolation (meteo_produced) */
    double lastMs = 0.;
    /* topographic distance (sf3d_topodist.inc): the maps of the last topo_compute, sized to that call, and the point tables of a call
     * (x, y, z: doubles; mapIndex: int32; the station matrix: METEO_MAX_STATIONS floats a row, allocated with the first matrix) */
    float* topoMaps = nullptr;          /* topoPoints x nCells floats */
    char* topoTables = nullptr;
    float* topoMatrix = nullptr;
    uint32_t topoPoints = 0, topoMatrixCap = 0;
    double topoMs[3] = {0., 0., 0.};    /* k_topodist_maps, k_meteo_idw_td, k_topodist_matrix */
    /* local detrending (sf3d_localdetrend.inc): the per-cell outcome of the last call (parameters: doubles; count: uint32; radius, R2:
     * floats; significant: bytes - a map each, in this order) and the call's tables (the fit table, then the stations' heights) */
    char* localFit = nullptr;
    char* localTables = nullptr;
    bool localDone = false;
    double localMs = 0.;
    /* local detrending with every proxy (sf3d_localproxies.inc): per cell the proxies' lines (doubles), the interpolated count (uint32)
     * and the proxies' significance (bytes), in this order; the call's tables (the fit table, the height row, the other proxies' rows) */
    char* proxiesFit = nullptr;
    char* proxiesTables = nullptr;
    bool proxiesDone = false;
    double proxiesMs = 0.;
    /* glocal detrending (sf3d_glocal.inc): one block for the areas' tables and what k_glocal_areas records (GL_T_*, at glocalOff), sized
     * when the areas are set; the call's tables (the fit table, the height row, the other proxies' rows); the proxies of the last call */
    char* glocalBlock = nullptr;
    char* glocalTables = nullptr;
    size_t glocalOff[11] = {0};
    size_t glocalBytes = 0;
    uint32_t glocalAreas = 0, glocalList = 0, glocalPairs = 0;
    bool glocalDone = false;
    double glocalMs[2] = {0., 0.};      /* k_glocal_areas, k_glocal_cells */
    LocalProxiesSetup glocalProxies = {};
    /* multiple detrending without areas (sf3d_multidetrend.inc): one block of fixed size for the call's tables and what
     * k_multidetrend_fit leaves (MD_OFF_*), allocated by the first call; the points of sf3d_multidetrend_points, grown as needed; the
     * set-up and the proxies of the last call, which the points are evaluated with */
    char* multiBlock = nullptr;
    char* multiPoints = nullptr;
    size_t multiPointsCap = 0;
    uint32_t multiStations = 0;
    bool multiDone = false;
    double multiMs[3] = {0., 0., 0.};   /* k_multidetrend_fit, k_multidetrend_cells, k_multidetrend_points */
    LocalDetrendSetup multiSetup = {};
    LocalProxiesSetup multiProxies = {};
};

/* hourly radiation maps (sf3d_rad.inc): the five outputs, the static maps of include/sf3d_rad.h and the hour's transmissivity; they belong to
 * the raster too */
struct RadCache {
    char* base = nullptr;               /* RAD_DOUBLE_MAPS double maps, RAD_FLOAT_MAPS float maps, one int32 map, each of nCells */
    uint32_t nCells = 0, nRows = 0, nCols = 0;
    double xll = 0., yll = 0., cellSize = 0.;
    float flag = -9999.f, demMax = -9999.f;
    double lastMs = 0.;
    bool hourDone = false;              /* an hour has written the outputs (rad_hour_done) */
    const float* trRead = nullptr;      /* the transmissivity map the last hour read: this block's copy or the meteo block's map (null once that is freed) */
    bool trFromMeteo = false;
    /* station transmissivity (sf3d_transmissivity.inc): the inputs, evaluations and results of the last call, in one block that grows */
    char* tr = nullptr;
    size_t trCap = 0, trOff[3] = {0, 0, 0};     /* trOff: global, elevationRefr, written */
    uint32_t trPoints = 0, trSlots = 0;
    double trMs = 0.;
};

/* hourly sinks (sf3d_sink.inc): the per-cell maps and the tables of include/sf3d_sink.h belong to the raster; the node array follows the
 * model the device works on (its size and numbering) and is freed with it */
struct SinkCache {
    char* cells = nullptr;              /* SINK_MAP_WORDS x nCells 4-byte words: the per-cell maps */
    char* tables = nullptr;             /* units, horizon table, horizon values, layer grid, evaporation coefficients: one block */
    double* nodes = nullptr;            /* [nodesN] node sinks */
    size_t off[8] = {0};
    uint32_t nCells = 0, nrLayers = 0, nUnits = 0, nSoils = 0, nodesN = 0;
    uint64_t nodesColVer = 0;           /* the version of the column table `nodes` was last written under (MapsCache::colVer is shared with the output maps) */
    int32_t lastEvapLayer = 0;
    double area = 0.;
    float flag = -9999.f;
    bool computed = false;
    double lastMs = 0.;
    SinkCrackDev crackDev{};            /* what the head of `crack` holds */
    char* crack = nullptr;              /* soil cracking: SinkCrackDev, maxDepth [nSoils], layerDepth [nrLayers], crackWater [nCells] (doubles), lastLayer [nSoils], precSurfaceWater [nCells] */
    uint64_t crackVer = 0;              /* the sf3d_sink_set_cracking the tables in `crack` were uploaded from */
    bool crackComputed = false;         /* the last hour ran k_sink_hour_crack */
    std::vector<double> layerDepth;
    const float* liquidRead = nullptr;  /* the liquid water map the last hour read: this block's, the snow block's or the meteo block's (null once that is freed) */
    int liquidFrom = 0;                 /* FEED_SNOW / FEED_METEO, 0: this block's */
};

/* the hour, device to device (sf3d_hour.inc): the block partials and the three totals of k_hour_totals, in one block that grows, and the
 * static maps of the day's ponds */
struct HourCache {
    double* sums = nullptr; size_t sumsCap = 0;
    char* pond = nullptr;               /* the day's ponds: tanSlope [nCells] (doubles), the unit table, then unit [nCells] and the pond map [nCells] (4 bytes) */
    uint32_t pondCells = 0;
    uint64_t pondVer = 0;               /* the sf3d_hour_set_ponds `pond` was uploaded from (0: none) */
    double lastMs[3] = {0., 0., 0.};    /* k_hour_relhum, k_hour_totals, k_hour_pond */
};

/* the SF3D_* switches the step driver acts on (sf3d_host_step.inc): read by read_step_switches when a model is built, back to these
 * defaults at release() - tests toggle them between models of one process */
struct StepSwitches {
    bool residentGrids = true;          /* SF3D_RESIDENT_GRIDS (0: every kernel with the common 2 048-block grid) */
    bool graphs = true;                 /* SF3D_GRAPHS (0: eager launches) */
    bool asmNtOff = false;              /* SF3D_ASM_NT=0: tuning: cacheable stores of the rows */
    bool pairOddSingle = true;          /* SF3D_PAIR_ODD_SINGLE (0: the paired pass queues pairs only) */
    long residentFailAt = -1;           /* SF3D_RESIDENT_FAIL_TEST=n: tests: the resident launches of the process's n-th computeStep give up, once */
    int heatDebug = 0;                  /* SF3D_HEAT_DEBUG: 0 unset, 1 set: one line per computeStep, 2: one per poll as well */
    int slabs = 0;                      /* SF3D_SLAB_OVERLAP=S (2 .. 8, else 0), and its grids and the share of the soil rows in the first slab (0: equal slabs) */
    uint32_t slabPropsBlocks = 512, slabAsmBlocks = 512; double slabFirst = 0.;
};

struct DeviceSolver::Impl {
    int device = -1;
    hipStream_t stream = nullptr;
    int overlapAccept = -1;                /* SF3D_OVERLAP_ACCEPT=0 keeps k_accept inside the step */
    /* link flow sums in batches (plain single-GPU path): the slots of the two rings (DevView::A2x, DevView::Hring) and the time steps of the
     * accepted steps whose sums are not added yet, in acceptance order.  ring: the model has the rings (0: two matrices, sums inside the step) */
    uint32_t ring = 0;
    LinksBatch pend{};
    DevView v{};
    Ctrl* hostCtrl = nullptr;              /* pinned */
    std::vector<void*> allocs;
    uint32_t N = 0, ns = 0;
    uint32_t ownedNodes = 0;               /* nodes whose rows this rank computes (N on one GPU; the strip without its halo otherwise) */
    uint32_t lastSweeps = 8;
    uint32_t lastBatches = 1;
    uint32_t predCount = 0, pred[16] = {0};   /* sweeps each approximation of the previous computeStep took (Ctrl::seqSweeps) */
    uint32_t lastHeatSweeps = 8;
    std::vector<uint32_t> gsLevelStart;    /* SF3D_HEAT_GS=1: level l = gsOrder[gsLevelStart[l] .. gsLevelStart[l+1]) */
    uint32_t lastHeatSteps = 1;            /* heat steps (accepted + halved) of the previous computeStep: look-ahead depth */
    double* heatOut[6] = {nullptr};       /* bAero, bSoilCond, bSens, bLat, bRad, bAdv (device) */
    double* heatAirP = nullptr;            /* filled by k_heat_static once z is on the device */
    /* hipGraph cache: one instantiated graph per shape of a water batch or of a heat group (GraphKey, sf3d_host_plan.inc).  replay
     * (sf3d_host_step.inc) launches the graph of `key` on st; the first time it captures what `enqueue` queues on st and instantiates it */
    std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;
    template <class F> hipError_t replay(const GraphKey& key, hipStream_t st, F enqueue);
    int useFused = -1;                     /* SF3D_FUSED_DECIDE=0 keeps the separate decision kernel */
    StepSwitches sw;                       /* the switches of the step driver, read when the model is built */
    /* multi-GPU */
    Partition part;
    DistWindow* window = nullptr;          /* fine-grained, IPC-exported */
    size_t windowBytes = 0;
    std::vector<void*> peerMaps;           /* hipIpcOpenMemHandle results */
    DistView hostDist{};
    DistView* devDist = nullptr;
    unsigned long long* distStats = nullptr;      /* DistView::stats */
    bool heatJacobiOnly = false;                  /* this rank's graph does not admit the two-colour heat sweep (goes into the blob) */
    double hopUs[SF3D_MAX_RANKS] = {0};           /* one-way latency of a flag store to rank p and back-to-back (k_dist_hop at sf3d_dist_finalize); 0 = not measured */
    /* fall-back transport: the same window layout in HOST memory (POSIX shared memory registered with HIP on every rank) */
    void* shmOwn = nullptr; int shmFd = -1; char shmName[48] = {0};
    std::vector<std::pair<void*, size_t>> shmPeers;      /* mapped + registered windows of the peers */
    std::vector<DistBlob> blobs;                          /* what the ranks published (kept from dist_connect for dist_finalize) */
    bool hostMode = false;
    void drop_shm()
    {
        for (auto& pr : shmPeers) { (void)hipHostUnregister(pr.first); munmap(pr.first, pr.second); }
        shmPeers.clear();
        if (shmOwn) { if (hostMode) (void)hipHostUnregister(shmOwn); munmap(shmOwn, windowBytes); shmOwn = nullptr; }
        if (shmFd >= 0) { close(shmFd); shmFd = -1; }
        if (shmName[0]) { shm_unlink(shmName); shmName[0] = 0; }
        hostMode = false;
    }
    uint32_t pushBlocks = 0;
    /* RCCL exchange (SF3D_EXCHANGE=rccl, or agreed fall-back when the windows fail): resolved with dlsym, no link-time dependency */
    void* rcclLib = nullptr; ncclComm_t comm = nullptr; bool rcclMode = false;
    ncclResult_t (*pGetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*pCommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*pCommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*pSend)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*pRecv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*pAllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*pAllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*pGroupStart)() = nullptr; ncclResult_t (*pGroupEnd)() = nullptr;
    double *rcclMine = nullptr, *rcclGathered = nullptr;
    bool rcclDistinct = false; unsigned char rcclId[128] = {0};
    bool load_rccl()
    {
        if (pAllGather) return true;
        /* SF3D_RCCL_LIB: another library with the same nine entry points (tests: tests/librccl_mock.so, which carries them over shared
         * memory so that the RCCL sequencing can run with the ranks of a test sharing one GPU) */
        if (const char* le = getenv("SF3D_RCCL_LIB")) if (!rcclLib && le[0]) rcclLib = dlopen(le, RTLD_NOW | RTLD_LOCAL);
        if (!rcclLib) rcclLib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!rcclLib) rcclLib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!rcclLib) return false;
        #define SF3D_SYM(ptr, name) ptr = reinterpret_cast<decltype(ptr)>(dlsym(rcclLib, name)); if (!ptr) return false
        SF3D_SYM(pGetUniqueId, "ncclGetUniqueId"); SF3D_SYM(pCommInitRank, "ncclCommInitRank"); SF3D_SYM(pCommDestroy, "ncclCommDestroy");
        SF3D_SYM(pSend, "ncclSend"); SF3D_SYM(pRecv, "ncclRecv"); SF3D_SYM(pAllReduce, "ncclAllReduce");
        SF3D_SYM(pGroupStart, "ncclGroupStart"); SF3D_SYM(pGroupEnd, "ncclGroupEnd"); SF3D_SYM(pAllGather, "ncclAllGather");
        #undef SF3D_SYM
        return true;
    }
    /* halo of one or two fields to and from every neighbour, then (optionally) the all-gather of the partial sums */
    void rccl_halo(hipStream_t st, int fields)
    {
        pGroupStart();
        for (int p = 0; p < hostDist.world; ++p) {
            if (p == hostDist.rank) continue;
            if (hostDist.sendCount[p]) pSend(hostDist.sendBuf[p], (size_t)hostDist.sendCount[p] * fields, ncclDouble, p, comm, st);
            if (hostDist.recvCount[p]) pRecv(const_cast<double*>(hostDist.recvBuf[p]), (size_t)hostDist.recvCount[p] * fields, ncclDouble, p, comm, st);
        }
        pGroupEnd();
    }
    void rccl_gather(hipStream_t st) { pAllGather(rcclMine, rcclGathered, 4, ncclDouble, comm, st); }
    /* blocks of kernel `fn` resident at once (occupancy x CUs), remembered per kernel; SF3D_RESIDENT_GRIDS=0: the common grid */
    uint32_t resident_blocks(const void* fn)
    {
        for (auto& r : residentBlocks) if (r.first == fn) return r.second;
        int perCu = 0, dev = 0; hipDeviceProp_t prop;
        uint32_t nbk = SF3D_MAX_BLOCKS;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, fn, SF3D_BLOCK, 0) == hipSuccess && perCu > 0
            && hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            nbk = (uint32_t)perCu * (uint32_t)prop.multiProcessorCount;
        if (!sw.residentGrids) nbk = SF3D_MAX_BLOCKS;
        residentBlocks.push_back({fn, nbk});
        return nbk;
    }
    /* add the link flow sums of every pending accepted step, in their order, in one pass (k_links_flush) on the solver's stream: whatever
     * is queued on that stream afterwards - a step, a copy of the sums, an output map - finds them added */
    hipError_t flush_links()
    {
        if (pend.n == 0) return hipSuccess;
        const void* fn = v.ntStream ? (const void*)k_links_flush<true> : (const void*)k_links_flush<false>;
        const uint32_t nbk = resident_blocks(fn);
        const dim3 fgrid(v.nb < nbk ? v.nb : nbk);
        if (v.ntStream) hipLaunchKernelGGL(k_links_flush<true>, fgrid, dim3(SF3D_BLOCK), 0, stream, v, pend);
        else hipLaunchKernelGGL(k_links_flush<false>, fgrid, dim3(SF3D_BLOCK), 0, stream, v, pend);
        pend.n = 0;
        return hipGetLastError();
    }
    bool links_pending(uint32_t slot) const { for (uint32_t k = 0; k < pend.n; ++k) if (pend.slot[k] == slot) return true; return false; }
    /* device slot of every (host slot, node): empty = identity.  Laterals of nodes with fewer links than their chunk's fullest node are
     * moved to the slots where that node keeps the same neighbour offset (sync_to_device), so that a slot means one direction for the
     * whole chunk; host arrays (HostModel, what the API reads and writes) stay in insertion order, the permutation is applied where
     * per-link arrays cross the boundary (flow sums up and down, heat link fluxes down). */
    std::vector<uint8_t> dslot;
    std::vector<double> stage;             /* N x 10 staging area of those transfers */
    uint32_t connectGen = 0;               /* token of the window self-check */
    bool warnedShared = false;
    /* timing */
    int timing = 0;                       /* 0 off, 1 every node kernel, 2 only k_sweep, on every 8th step */
    std::vector<std::pair<const void*, uint32_t>> residentBlocks;   /* kernel -> blocks resident at once (occupancy x CUs) */
    std::vector<uint32_t> propsNeed;       /* [nChunks] one GPU: the rows of chunks [0, q] read node properties of chunks [0, propsNeed[q]) */
    hipStream_t stream3 = nullptr;         /* slab overlap: the node properties of the next slab beside the rows of this one */
    hipEvent_t evSlab[8] = {};
    uint32_t pairBlocks = 0;              /* grid of k_sweep_pair (0: the graph is no regular grid, or the paired sweep is off) */
    bool pairMasked = false;              /* the paired sweep runs as k_sweep_pair_masked (layered masked grid) */
    uint32_t resBlocks = 0, resLds = 0;   /* grid and dynamic LDS of k_sweep_resident (0: the rows of this grid do not fit on chip, or the resident loop is off) */
    uint32_t resCapacity = 0;             /* blocks of that kernel the device holds at once */
    uint32_t pairRecordsWish = 0;         /* paired pass on a strip, record hand-over: 0 off (SF3D_PAIR_RECORDS=0, or no paired pass), nonzero: wherever the records
                                           * are addressed without list walks (the default) */
    uint64_t stepSeq = 0;
    uint64_t stepSeqAll = 0;              /* computeSteps of this process that ran the resident loop (SF3D_RESIDENT_FAIL_TEST counts in them) */
    struct Pair { hipEvent_t a, b; int kid; };
    std::vector<Pair> pending;             /* pairs of the batch in flight, in launch order */
    std::vector<hipEvent_t> freeEvents;
    uint64_t launches[KID_COUNT] = {0};
    double ms[KID_COUNT] = {0};
    MapsCache maps;
    SnowCache snow;
    CropCache crop;
    RootCache root;
    MeteoCache meteo;
    SinkCache sink;
    RadCache rad;
    HourCache hour;
};

/* on failure: message, then drain the solver stream (async copies from pageable host vectors may still be in flight and the
 * caller is free to modify those vectors as soon as we return), mark the solver unusable, return */
#define HIP_TRY(expr)                                                                          \
    do { hipError_t e_ = (expr);                                                               \
         if (e_ != hipSuccess) {                                                               \
             snprintf(err_, sizeof(err_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
             if (impl_ && impl_->stream) (void)hipStreamSynchronize(impl_->stream);           \
             fatal_ = true;                                                                    \
             return SF3D_SOLVER_ERROR; } } while (0)

/* the raster blocks and the shared raster path (end of sf3d_maps.inc) touch nothing of the solver: a HIP failure there does not set fatal_ */
#define RASTER_TRY(expr)                                                                       \
    do { hipError_t e_ = (expr);                                                               \
         if (e_ != hipSuccess) {                                                               \
             snprintf(err_, sizeof(err_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
             if (impl_ && impl_->stream) (void)hipStreamSynchronize(impl_->stream);           \
             return SF3D_SOLVER_ERROR; } } while (0)

DeviceSolver& DeviceSolver::instance() { static DeviceSolver s; return s; }
const char* DeviceSolver::kernel_name(int kid) { return (kid >= 0 && kid < KID_COUNT) ? kKernelNames[kid] : nullptr; }

sf3d_error_t DeviceSolver::set_device(int dev)
{
    if (!impl_) impl_ = new Impl();
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (dev < 0 || dev >= count) { snprintf(err_, sizeof(err_), "device %d out of range (%d visible)", dev, count); return SF3D_SOLVER_ERROR; }
    impl_->device = dev;
    HIP_TRY(hipSetDevice(dev));
    return SF3D_OK;
}

static uint64_t g_deviceBytes = 0;          /* bytes behind the current model's allocations (sf3d_device_bytes) */
sf3d_error_t DeviceSolver::release()
{
    if (!impl_) return SF3D_OK;
    Impl& I = *impl_;
    if (I.stream) hipStreamSynchronize(I.stream);
    if (I.stream3) hipStreamSynchronize(I.stream3);
#if SF3D_RES_PROFILE
    if (built_ && I.v.res.on && I.v.res.pub) {      /* tuning builds: where block 0 of the resident sweep loop spent its time */
        double pr[32];
        if (hipMemcpy(pr, I.v.res.pub, sizeof(pr), hipMemcpyDeviceToHost) == hipSuccess && pr[16] > 0.) {
            const char* names[7] = {"compute + record stores issued", "wave sum + block partial", "halo records", "partial records of all blocks", "barrier B", "norm + decision", "(prologue: per launch, not per iteration)"};
            fprintf(stderr, "[sf3d] resident sweep loop, block 0: %.0f launches, %.2f iterations per launch, %.2f us per launch\n", pr[16], pr[15] / pr[16], pr[17] / pr[16] / 100.);
            for (int p = 0; p < 7; ++p) fprintf(stderr, "[sf3d]   %-40s %7.2f us per iteration\n", names[p], pr[8 + p] / pr[15] / 100.);
        }
    }
#endif
    I.pend.n = 0; I.ring = 0;      /* pending link flow sums go with the arrays they would read (a caller that wants them has fetched them: sync_to_device) */
    if (I.stream3) {      /* the slab experiment's stream and events go with the model (created again on demand) */
        (void)hipStreamDestroy(I.stream3); I.stream3 = nullptr;
        for (auto& ev : I.evSlab) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    }
    for (auto& p : I.pending) { I.freeEvents.push_back(p.a); I.freeEvents.push_back(p.b); }
    I.pending.clear();
    for (auto& g : I.graphs) hipGraphExecDestroy(g.second);
    I.graphs.clear();
    for (void* p : I.allocs) hipFree(p);
    I.allocs.clear();
    g_deviceBytes = 0;
    I.maps.free_all();
    if (I.sink.nodes) { (void)hipFree(I.sink.nodes); I.sink.nodes = nullptr; I.sink.nodesN = 0; I.sink.computed = false; }      /* the node sinks follow the model's numbering */
    if (I.comm && I.pCommDestroy) { I.pCommDestroy(I.comm); I.comm = nullptr; }
    I.rcclMode = false; I.rcclMine = I.rcclGathered = nullptr;
    for (void* p : I.peerMaps) hipIpcCloseMemHandle(p);
    I.peerMaps.clear();
    I.drop_shm();
    if (I.window) { hipFree(I.window); I.window = nullptr; }
    I.devDist = nullptr; I.distStats = nullptr;
    connected_ = false;
    built_ = false;
    fatal_ = false;
    /* the SF3D_* mode switches are read again when the next model is built (tests toggle them between models of one process) */
    I.overlapAccept = I.useFused = -1; I.sw = StepSwitches();
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::synchronize()
{
    if (!impl_ || !impl_->stream) return SF3D_OK;
    if (built_) HIP_TRY(impl_->flush_links());      /* where a caller asks for finished results: the link flow sums of the accepted steps still pending */
    HIP_TRY(hipStreamSynchronize(impl_->stream));
    return SF3D_OK;
}

template <class T> static hipError_t dev_alloc(std::vector<void*>& allocs, T*& p, size_t count)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) { allocs.push_back(q); p = static_cast<T*>(q); g_deviceBytes += (uint64_t)(count ? count : 1) * sizeof(T); }
    return e;
}
uint64_t DeviceSolver::device_bytes() const { return g_deviceBytes; }

static void fill_params(Ctrl& c, const ParamsHost& p)
{
    c.MBRThreshold = p.MBRThreshold; c.residualTolerance = p.residualTolerance;
    c.dtMin = p.dtMin; c.dtMax = p.dtMax; c.lvRatio = p.lvRatio;
    c.courantThreshold = p.courantThreshold; c.instabilityFactor = p.instabilityFactor;
    c.maxApprox = p.maxApprox; c.maxIter = p.maxIter; c.wrc = p.wrc; c.meanType = p.meanType;
    c.dtCurr = p.dtCurr;
    c.lineal = p.lineal ? 1u : 0u;
}

sf3d_error_t DeviceSolver::ensure_device()
{
    if (!impl_) impl_ = new Impl();
    Impl& I = *impl_;
    if (I.device < 0) {
        int dev = 0;
        if (const char* lr = getenv("LOCAL_RANK")) dev = atoi(lr);
        int count = 0;
        HIP_TRY(hipGetDeviceCount(&count));
        if (count <= 0) { snprintf(err_, sizeof(err_), "no HIP device visible: the soilFluxes3D product path has no CPU fallback"); return SF3D_SOLVER_ERROR; }
        /* SF3D_DEVICES=2 or =4,5,6,7: which GPUs an UNMODIFIED caller (no sf3d_set_device) uses - entry LOCAL_RANK of the list (SURVEY.md 5) */
        if (const char* de = getenv("SF3D_DEVICES")) {
            std::vector<int> list;
            for (const char* q = de; *q;) { char* end = nullptr; const long v = strtol(q, &end, 10); if (end == q) break; list.push_back((int)v); q = (*end == ',') ? end + 1 : end; }
            if (!list.empty()) {
                const int pick = list[(size_t)(dev < 0 ? 0 : dev) % list.size()];
                if (pick < 0 || pick >= count) { snprintf(err_, sizeof(err_), "SF3D_DEVICES names device %d, %d visible", pick, count); return SF3D_SOLVER_ERROR; }
                dev = pick;
            }
        }
        I.device = dev % count;
    }
    HIP_TRY(hipSetDevice(I.device));
    if (!I.stream) HIP_TRY(hipStreamCreateWithFlags(&I.stream, hipStreamNonBlocking));
    return SF3D_OK;
}

/* the SF3D_* switches the build block of sync_to_device reads, each parsed once at the top of that block.  Read again on every build and
 * never cached: tests toggle them between models of one process */
struct BuildSwitches {
    bool slotAlign;                     /* SF3D_SLOT_ALIGN (0: off) */
    int pairSweep;                      /* SF3D_PAIR_SWEEP: -1 unset (automatic: large grids only), 0 off, 1 on */
    bool residentSweep;                 /* SF3D_RESIDENT_SWEEP; unset: on unless SF3D_PAIR_SWEEP=1 alone asks for the paired passes (tests, measurements) */
    bool forceMasked;                   /* SF3D_PAIR_FORCE_MASKED=1: measurement: a full box through k_sweep_pair_masked */
    uint32_t asmSoilBlocks;             /* SF3D_ASM_SOIL_BLOCKS: tuning (0: unset) */
    int overlapAccept;                  /* SF3D_OVERLAP_ACCEPT */
    int ntStream;                       /* SF3D_NT_STREAM: -1 unset (by the sweep's working set), 0, 1 */
    double probeMin;                    /* SF3D_COURANT_PROBE */
    double autoCost;                    /* SF3D_PAIR_AUTO_COST */
    bool pairWSet; uint32_t pairW;      /* SF3D_PAIR_W */
    double distTimeoutS;                /* SF3D_DIST_TIMEOUT_S */
    int fusedDecide;                    /* SF3D_FUSED_DECIDE (Impl::useFused takes it at the head of the build) */
    int haloDirect;                     /* SF3D_HALO_DIRECT: -1 unset, 1 it is 1, 0 anything else */
    uint32_t pairRecordsWish;           /* SF3D_PAIR_RECORDS: Impl::pairRecordsWish */
    uint32_t residentPR;                /* SF3D_RESIDENT_PR: tests: this patch height or none (0: unset) */
    uint32_t residentPost;              /* SF3D_RESIDENT_POST */
    uint32_t heatRedBlack;              /* SF3D_HEAT_SWEEP=j: Jacobi */
    bool heatDebug, heatGS;             /* SF3D_HEAT_DEBUG, SF3D_HEAT_GS=1 */
};
static BuildSwitches read_build_switches()
{
    BuildSwitches s;
    const char* re = getenv("SF3D_SLOT_ALIGN");
    s.slotAlign = !(re && re[0] == '0');
    const char* pe = getenv("SF3D_PAIR_SWEEP");
    s.pairSweep = pe ? (pe[0] == '0' ? 0 : 1) : -1;
    const char* rse = getenv("SF3D_RESIDENT_SWEEP");
    s.residentSweep = rse ? rse[0] != '0' : s.pairSweep != 1;
    s.forceMasked = false;
    if (const char* fm = getenv("SF3D_PAIR_FORCE_MASKED")) if (fm[0] == '1') s.forceMasked = true;
    s.asmSoilBlocks = 0;
    if (const char* be = getenv("SF3D_ASM_SOIL_BLOCKS")) s.asmSoilBlocks = (uint32_t)atoi(be);
    const char* oe = getenv("SF3D_OVERLAP_ACCEPT");
    s.overlapAccept = (oe && oe[0] == '0') ? 0 : 1;
    const char* e = getenv("SF3D_NT_STREAM");
    s.ntStream = e ? (e[0] != '0') : -1;
    s.probeMin = 0.8;
    if (const char* ce = getenv("SF3D_COURANT_PROBE")) { s.probeMin = atof(ce); if (ce[0] == '0' && ce[1] == 0) s.probeMin = -1.; if (ce[0] == 'a') s.probeMin = 0.; }
    s.autoCost = 1.9;
    if (const char* ae = getenv("SF3D_PAIR_AUTO_COST")) s.autoCost = atof(ae);
    const char* we = getenv("SF3D_PAIR_W");
    s.pairWSet = we != nullptr; s.pairW = we ? (uint32_t)atoi(we) : 0u;
    {   double ts = 10.; if (const char* te = getenv("SF3D_DIST_TIMEOUT_S")) { ts = atof(te); if (!(ts >= 0.5)) ts = 0.5; if (ts > 600.) ts = 600.; }
        s.distTimeoutS = ts; }
    { const char* fe = getenv("SF3D_FUSED_DECIDE"); s.fusedDecide = (fe && fe[0] == '0') ? 0 : 1; }
    s.haloDirect = -1;
    if (const char* hd = getenv("SF3D_HALO_DIRECT")) s.haloDirect = hd[0] == '1' ? 1 : 0;
    const char* pre = getenv("SF3D_PAIR_RECORDS");
    s.pairRecordsWish = (pre && pre[0] == '0') ? 0u : ((pre && pre[0] == '1') ? 2u : 1u);
    s.residentPR = 0; if (const char* pe = getenv("SF3D_RESIDENT_PR")) s.residentPR = (uint32_t)atoi(pe);
    {   const char* pe2 = getenv("SF3D_RESIDENT_POST"); s.residentPost = (pe2 && pe2[0] == '0') ? 0u : 1u; }
    const char* se = getenv("SF3D_HEAT_SWEEP");
    s.heatRedBlack = (se && se[0] == 'j') ? 0u : 1u;
    s.heatDebug = getenv("SF3D_HEAT_DEBUG") != nullptr;
    s.heatGS = false;
    if (const char* ge = getenv("SF3D_HEAT_GS")) if (ge[0] == '1') s.heatGS = true;
    return s;
}

/* the switches of the step driver, each parsed once per model (sync_to_device keeps them in the solver's state) */
static StepSwitches read_step_switches()
{
    StepSwitches s;
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    s.residentGrids = !off("SF3D_RESIDENT_GRIDS");
    s.graphs = !off("SF3D_GRAPHS");
    s.asmNtOff = off("SF3D_ASM_NT");
    s.pairOddSingle = !off("SF3D_PAIR_ODD_SINGLE");
    if (const char* fe = getenv("SF3D_RESIDENT_FAIL_TEST")) s.residentFailAt = strtol(fe, nullptr, 10);
    if (const char* he = getenv("SF3D_HEAT_DEBUG")) s.heatDebug = he[0] == '2' ? 2 : 1;
    { const char* e = getenv("SF3D_SLAB_OVERLAP"); s.slabs = e ? atoi(e) : 0; if (s.slabs > 8) s.slabs = 8; if (s.slabs < 2) s.slabs = 0; }
    auto blocks_of = [](const char* e) -> uint32_t { const long n = e ? strtol(e, nullptr, 10) : 512L; return (uint32_t)(n < 1 ? 1 : (n > SF3D_MAX_BLOCKS ? SF3D_MAX_BLOCKS : n)); };      /* (0 or garbage would be a dim3(0) launch) */
    s.slabPropsBlocks = blocks_of(getenv("SF3D_SLAB_PROPS_BLOCKS"));
    s.slabAsmBlocks = blocks_of(getenv("SF3D_SLAB_ASM_BLOCKS"));
    if (const char* fe = getenv("SF3D_SLAB_FIRST")) s.slabFirst = atof(fe);
    return s;
}

/* what the stages of one build share: it lives for the duration of the build block of sync_to_device */
struct DeviceSolver::BuildState {
    BuildSwitches sw;
    LinkTables links;
    std::vector<ChunkDesc> cdesc;
    GridPlan grid;
    ChunkLists lists;
    EdgeRows edge;
};

/* The three device-side stages below are blocks of the build block of sync_to_device, moved as they stood: each begins by giving what it
 * shares with the rest the names it has there.  Every HIP_TRY returns from the stage, and the caller hands that on at once. */

/* multi GPU: the owner array, the send / receive lists, the in-kernel puts, where foreign neighbours arrive, k_sweep_bnd's chunks, the
 * record hand-over of the paired pass and this rank's window */
sf3d_error_t DeviceSolver::build_dist_window(BuildState& st)
{
    Impl& I = *impl_; DevView& v = I.v; const BuildSwitches& sw = st.sw;
    const uint32_t N = I.N, ns = I.ns, nChunks = v.nChunks; const size_t NS = (size_t)N * SF3D_SLOTS;
    const std::vector<uint8_t>& kind = st.links.kind; const std::vector<uint32_t>& to = st.links.to;
    std::vector<ChunkDesc>& cdesc = st.cdesc; const std::vector<uint32_t>& listSurf = st.lists.listSurf;
    const uint32_t pairNX = st.grid.NX, pairNY = st.grid.NY, pairNZ = st.grid.NZ, pairOwnLo = st.grid.ownLo, pairOwnHi = st.grid.ownHi;
    const int32_t(&edgePeer)[2] = st.edge.edgePeer; const uint32_t(&edgePut)[2] = st.edge.edgePut, (&edgeGet)[2] = st.edge.edgeGet;
    auto edge_rows_direct = [&]() -> bool { return plan_edge_rows_direct(I.part, st.grid, ns, world_, rank_, st.edge); };
    uint8_t* downer; HIP_TRY(dev_alloc(I.allocs, downer, N));
    HIP_TRY(hipMemcpy(downer, I.part.owner.data(), N, hipMemcpyHostToDevice));
    v.owner = downer;
    /* my window: mailboxes + payload areas for what each neighbour puts (2 parities x 2 fields) */
    DistView& d = I.hostDist;
    std::memset(&d, 0, sizeof(d));
    d.world = world_; d.rank = rank_; d.owner = downer;
    d.spinTicks = (long long)(sw.distTimeoutS * 1e8);
    uint64_t off = 0;
    uint32_t maxSend = 0;
    for (int pr = 0; pr < world_; ++pr) {
        d.recvCount[pr] = (uint32_t)I.part.recv[pr].size();
        d.recvOff[pr] = off;
        off += (uint64_t)d.recvCount[pr] * 2 * SF3D_DIST_FIELDS;
        d.sendCount[pr] = (uint32_t)I.part.send[pr].size();
        if (d.sendCount[pr] > maxSend) maxSend = d.sendCount[pr];
        uint32_t *si, *ri;
        HIP_TRY(dev_alloc(I.allocs, si, I.part.send[pr].size())); HIP_TRY(dev_alloc(I.allocs, ri, I.part.recv[pr].size()));
        if (d.sendCount[pr]) HIP_TRY(hipMemcpy(si, I.part.send[pr].data(), (size_t)d.sendCount[pr] * 4, hipMemcpyHostToDevice));
        if (d.recvCount[pr]) HIP_TRY(hipMemcpy(ri, I.part.recv[pr].data(), (size_t)d.recvCount[pr] * 4, hipMemcpyHostToDevice));
        d.sendIdx[pr] = si; d.recvIdx[pr] = ri;
    }
    {   /* the send lists regrouped by chunk for the in-kernel puts */
        struct Ent { uint32_t node; uint8_t peer; uint32_t slot; };
        std::vector<Ent> ents;
        for (int pr = 0; pr < world_; ++pr)
            for (uint32_t k = 0; k < I.part.send[pr].size(); ++k) ents.push_back({I.part.send[pr][k], (uint8_t)pr, k});
        std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.node != b.node ? a.node < b.node : a.peer < b.peer; });
        std::vector<uint32_t> bstart(nChunks + 1, 0), bslot(ents.size());
        std::vector<uint8_t> blane(ents.size()), bpeer(ents.size());
        for (size_t k = 0; k < ents.size(); ++k) {
            bstart[ents[k].node / SF3D_CHUNK + 1]++;
            blane[k] = (uint8_t)(ents[k].node % SF3D_CHUNK); bpeer[k] = ents[k].peer; bslot[k] = ents[k].slot;
        }
        for (uint32_t q = 0; q < nChunks; ++q) bstart[q + 1] += bstart[q];
        uint32_t *dbs, *dsl; uint8_t *dla, *dpe;
        HIP_TRY(dev_alloc(I.allocs, dbs, bstart.size())); HIP_TRY(dev_alloc(I.allocs, dsl, bslot.size()));
        HIP_TRY(dev_alloc(I.allocs, dla, blane.size())); HIP_TRY(dev_alloc(I.allocs, dpe, bpeer.size()));
        HIP_TRY(hipMemcpy(dbs, bstart.data(), bstart.size() * 4, hipMemcpyHostToDevice));
        if (!ents.empty()) {
            HIP_TRY(hipMemcpy(dsl, bslot.data(), bslot.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dla, blane.data(), blane.size(), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dpe, bpeer.data(), bpeer.size(), hipMemcpyHostToDevice));
        }
        d.bndStart = dbs; d.bndSlot = dsl; d.bndLane = dla; d.bndPeer = dpe;
    }
    v.haloDirect = I.useFused != 0 ? 1u : 0u;      /* the fused exchange only; SF3D_HALO_DIRECT=0 copies the halo after every sweep */
    if (sw.haloDirect >= 0) v.haloDirect = (sw.haloDirect == 1 && I.useFused != 0) ? 1u : 0u;
    if (v.haloDirect) {   /* where each foreign neighbour's value arrives in my window; chunks that have any are flagged */
        std::vector<uint32_t> fsrc(NS, SF3D_FSRC_NONE);
        for (uint32_t i = 0; i < N; ++i) {
            if (I.part.owner[i] != rank_) continue;
            for (int sl = 0; sl < SF3D_SLOTS; ++sl) {
                const size_t e = (size_t)sl * N + i;
                if (kind[e] == LK_NONE) continue;
                const uint32_t j = to[e];
                const int pr = I.part.owner[j];
                if (pr == rank_) continue;
                const auto& lst = I.part.recv[pr];
                const auto it = std::lower_bound(lst.begin(), lst.end(), j);
                if (it == lst.end() || *it != j) { snprintf(err_, sizeof(err_), "partition: node %u read by %u is missing from the halo list of rank %d", j, i, pr); return SF3D_TOPOGRAPHY_ERROR; }
                fsrc[e] = ((uint32_t)pr << 27) | (uint32_t)(it - lst.begin());
                cdesc[i / SF3D_CHUNK].pad0 = 1;
            }
        }
        uint32_t* dfs; HIP_TRY(dev_alloc(I.allocs, dfs, NS));
        HIP_TRY(hipMemcpy(dfs, fsrc.data(), NS * 4, hipMemcpyHostToDevice));
        d.fsrc = dfs;
    }
    v.bndList = nullptr; v.nBnd = 0;
    if (I.pairBlocks != 0) {
        /* paired sweep on a strip: k_sweep_bnd's chunks = the owned chunks that read a neighbouring strip; they must be exactly
         * the rows next to a halo row in every layer (what k_sweep_pair<DIST> leaves out), and the sweeps must take foreign
         * neighbours from the window (the fused exchange) */
        bool ok = v.haloDirect != 0;
        std::vector<uint32_t> bnd;
        if (ok && I.pairMasked) {      /* masked grid: no rows to reason with - every node gets its role (PairGrid::role) */
            std::vector<uint8_t> role(N, 0);
            for (uint32_t i = 0; i < N; ++i) if (I.part.owner[i] == rank_) role[i] = cdesc[i / SF3D_CHUNK].pad0 ? 2 : 1;
            uint8_t* dr; HIP_TRY(dev_alloc(I.allocs, dr, N));
            HIP_TRY(hipMemcpy(dr, role.data(), N, hipMemcpyHostToDevice));
            v.pair.role = dr;
            for (uint32_t q : listSurf) if (cdesc[q].pad0) bnd.push_back(q);
        } else
        for (uint32_t k = 0; k < listSurf.size() && ok; ++k) {
            const uint32_t q = listSurf[k];
            const uint32_t r = ((q * SF3D_CHUNK) % ns) / pairNX;
            const bool edge = (pairOwnLo > 0 && r == pairOwnLo) || (pairOwnHi < pairNY && r + 1 == pairOwnHi);
            const bool mineRow = r >= pairOwnLo && r < pairOwnHi;
            if ((cdesc[q].pad0 != 0) != (edge && mineRow)) ok = false;
            if (cdesc[q].pad0 && mineRow) bnd.push_back(q);
        }
        if (ok && !bnd.empty()) {
            uint32_t* db; HIP_TRY(dev_alloc(I.allocs, db, bnd.size()));
            HIP_TRY(hipMemcpy(db, bnd.data(), bnd.size() * 4, hipMemcpyHostToDevice));
            v.bndList = db; v.nBnd = (uint32_t)bnd.size();
        } else if (!ok || I.pairMasked || (pairOwnLo > 0 || pairOwnHi < pairNY)) { I.pairBlocks = 0; v.pair.NX = v.pair.NY = v.pair.NZ = 0; }
    }
    v.pair.records = 0u; d.recGet = nullptr; d.recPut = nullptr; I.pairRecordsWish = 0u;
    if (I.pairBlocks != 0) {
        if (I.pairMasked) {      /* masked grids: per-node tables - where an owned node's value goes, where a foreign node's arrives - instead of list walks */
            std::vector<RecGet> rg(N, RecGet{SF3D_FSRC_NONE, 0u});
            std::vector<RecPut> rp(N, RecPut{0u, 0u, 0u, 0u});
            bool fits = true;
            for (int pr = 0; pr < world_; ++pr) {
                const uint64_t rc = d.recvCount[pr], sc = d.sendCount[pr];
                for (uint32_t k = 0; k < rc; ++k) {
                    const uint64_t o = d.recvOff[pr] + (uint64_t)DF_RECLO * rc + k;
                    if (o + (uint64_t)2 * SF3D_DIST_FIELDS * rc >= 0xFFFFFFFFull) fits = false;
                    rg[I.part.recv[pr][k]] = RecGet{(uint32_t)o, (uint32_t)rc};
                }
                for (uint32_t k = 0; k < sc; ++k) {
                    RecPut& e = rp[I.part.send[pr][k]];
                    if (e.nDest == 0u) {
                        /* (sendOff: where MY values start in rank pr's window - known after the connect; the entry holds the position inside that area) */
                        e.off0 = (uint32_t)((uint64_t)DF_RECLO * sc + k); e.cnt = (uint32_t)sc; e.peer = (uint32_t)pr;
                    }
                    e.nDest++;
                }
            }
            if (fits) {
                RecGet* dg; RecPut* dp;
                HIP_TRY(dev_alloc(I.allocs, dg, N)); HIP_TRY(dev_alloc(I.allocs, dp, N));
                HIP_TRY(hipMemcpy(dg, rg.data(), (size_t)N * sizeof(RecGet), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(dp, rp.data(), (size_t)N * sizeof(RecPut), hipMemcpyHostToDevice));
                d.recGet = dg; d.recPut = dp;
            }
        }
        /* record hand-over (one launch, one exchange per pass; SF3D_PAIR_RECORDS=0 keeps k_sweep_bnd and its second exchange; sf3d_dist_connect
         * decides for all ranks) */
        I.pairRecordsWish = sw.pairRecordsWish;
        if (I.pairRecordsWish != 0u) {
            /* every local node of another rank must be in that rank's halo list (it is: a node nobody here reads is not staged) - it would have no record */
            bool all = true;
            for (uint32_t i = 0; i < N && all; ++i) {
                const int pr = I.part.owner[i];
                if (pr == rank_ || pr == SF3D_OWNER_NONE) continue;
                const auto& lst = I.part.recv[pr];
                const auto it = std::lower_bound(lst.begin(), lst.end(), i);
                if (it == lst.end() || *it != i) all = false;
            }
            /* regular strips whose edge rows lie in the lists as (layer) * NX + column from a base: the kernel addresses the records directly */
            v.pair.recFast = 0u; v.pair.sidePeer[0] = v.pair.sidePeer[1] = -1; v.pair.recStride = pairNX;
            if (all && !I.pairMasked && edge_rows_direct()) {
                v.pair.recFast = 1u;
                for (int side = 0; side < 2; ++side) { v.pair.sidePeer[side] = edgePeer[side]; v.pair.putBase[side] = edgePut[side]; v.pair.getBase[side] = edgeGet[side]; }
            }
            /* the hand-over exists where the records are addressed without list walks - that layout, or the per-node tables of the masked pass
             * (above): with a walk through the chunk's send list per put and a look-up chain per wait it cost more than the second launch
             * saves (profiles/r06_i_record_handover_on_strips_ab.txt, jobs 23 / 24) */
            v.pair.records = (all && (I.pairMasked ? (d.recPut != nullptr && d.recGet != nullptr && pairNZ < 128u /* (bit 7 of the patches' depth byte flags the blocks at the cut) */) : v.pair.recFast != 0u)) ? 1u : 0u;
        }
    }
    I.windowBytes = sizeof(DistWindow) + off * sizeof(double);
    void* w = nullptr;
    HIP_TRY(hipExtMallocWithFlags(&w, I.windowBytes, hipDeviceMallocFinegrained));
    HIP_TRY(hipMemset(w, 0, I.windowBytes));
    I.window = static_cast<DistWindow*>(w);
    d.win[rank_] = I.window;
    d.payload[rank_] = reinterpret_cast<double*>(reinterpret_cast<char*>(w) + sizeof(DistWindow));
    HIP_TRY(dev_alloc(I.allocs, I.devDist, 1));
    HIP_TRY(dev_alloc(I.allocs, I.distStats, 1 + 2 * SF3D_MAX_RANKS));
    HIP_TRY(hipMemset(I.distStats, 0, sizeof(unsigned long long) * (1 + 2 * SF3D_MAX_RANKS)));
    d.stats = I.distStats;
    for (double& h : I.hopUs) h = 0.;
    I.pushBlocks = (maxSend + SF3D_BLOCK - 1) / SF3D_BLOCK;
    if (I.pushBlocks == 0) I.pushBlocks = 1;
    if (I.pushBlocks > 256) I.pushBlocks = 256;
    return SF3D_OK;
}

/* the resident sweep loop: its shape from the menu by the occupancy queries, its arrays, and on a strip where the halo rows arrive */
sf3d_error_t DeviceSolver::build_resident_plan(const HostModel& m, BuildState& st)
{
    Impl& I = *impl_; DevView& v = I.v; const BuildSwitches& sw = st.sw;
    const uint32_t N = I.N, ns = I.ns;
    const std::vector<uint64_t>&pairNode = st.grid.node, &pairChunk = st.grid.chunk; const std::vector<int32_t>& pairIdxMap = st.grid.idxMap;
    const uint32_t pairNX = st.grid.NX, pairNY = st.grid.NY, pairNZ = st.grid.NZ, pairOwnLo = st.grid.ownLo, pairOwnHi = st.grid.ownHi;
    const int32_t(&edgePeer)[2] = st.edge.edgePeer; const uint32_t(&edgePut)[2] = st.edge.edgePut;
    auto edge_rows_direct = [&]() -> bool { return plan_edge_rows_direct(I.part, st.grid, ns, world_, rank_, st.edge); };
    {   /* resident sweep loop (k_sweep_resident, sf3d_resident.inc): a regular grid - or the rank's row strip of one - whose rows fit into the
         * registers of the CUs: patch height PR (a divisor of the owned rows), K chunks per wave and NW waves per block from the menu of
         * compiled shapes, every block resident at once (occupancy query).  SF3D_RESIDENT_SWEEP=0 turns it off, =1 is the default. */
        v.res = ResGrid{};
        I.resBlocks = 0; I.resLds = 0;
        const bool asked = sw.residentSweep;      /* (SF3D_PAIR_SWEEP=1 alone asks for the paired passes: tests, measurements) */
        const bool want = asked && I.useFused != 0 && !pairNode.empty() && pairIdxMap.empty() && (world_ == 1 || v.haloDirect);
        if (want) {
            const uint32_t ownRows = pairOwnHi - pairOwnLo, patchCols = pairNX / 64;
            int cus = 256; { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, I.device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount; }
            const uint32_t onlyPR = sw.residentPR;      /* tests: this patch height or none */
            for (uint32_t PR = 1; PR <= 8 && !v.res.on; ++PR) {
                if (ownRows % PR != 0 || (onlyPR != 0 && PR != onlyPR)) continue;
                const uint32_t blocks = patchCols * (ownRows / PR), T = PR * pairNZ;
                const uint32_t lds = 2u * pairNZ * (PR + 2) * SF3D_RES_RS * 8u;
                for (const ResShape& sh : kResShapes) {
                    if ((uint32_t)(sh.K * sh.NW) < T || (uint32_t)sh.NW % PR != 0) continue;     /* (a wave's chunks: one row, layers a constant stride apart) */
                    if (pairNZ * (2u * SF3D_RES_RS + 2u * PR) > (uint32_t)SF3D_RES_HM * sh.NW * 64u) continue;
                    const void* fn = (const void*)res_kernel(sh.K, sh.NW, world_ > 1);
                    if (!fn) continue;
                    if (lds > 48u * 1024u && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); continue; }
                    int perCu = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, fn, sh.NW * 64, lds) != hipSuccess || perCu < 1) { (void)hipGetLastError(); continue; }
                    if (blocks > (uint32_t)perCu * (uint32_t)cus) continue;
                    v.res.on = 1; v.res.NX = pairNX; v.res.NY = pairNY; v.res.NZ = pairNZ; v.res.PR = PR;
                    v.res.patchCols = patchCols; v.res.rowGroups = ownRows / PR; v.res.ownLo = pairOwnLo; v.res.ownHi = pairOwnHi;
                    v.res.K = (uint32_t)sh.K; v.res.NW = (uint32_t)sh.NW;
                    I.resBlocks = blocks; I.resLds = lds; I.resCapacity = (uint32_t)perCu * (uint32_t)cus;
                    break;
                }
            }
        }
        if (v.res.on) {
            if (v.pair.nodeLat && v.pair.chunkCode && !v.pair.masked && v.pair.NX == pairNX) { v.res.nodeLat = v.pair.nodeLat; v.res.chunkCode = v.pair.chunkCode; }
            else {
                uint32_t* dn; uint64_t* dq;
                std::vector<uint32_t> lat(pairNode.size());
                for (size_t k = 0; k < pairNode.size(); ++k) lat[k] = (uint32_t)(pairNode[k] >> 8);
                HIP_TRY(dev_alloc(I.allocs, dn, lat.size()));
                HIP_TRY(hipMemcpy(dn, lat.data(), lat.size() * 4, hipMemcpyHostToDevice));
                HIP_TRY(dev_alloc(I.allocs, dq, pairChunk.size()));
                HIP_TRY(hipMemcpy(dq, pairChunk.data(), pairChunk.size() * 8, hipMemcpyHostToDevice));
                v.res.nodeLat = dn; v.res.chunkCode = dq;
            }
            HIP_TRY(dev_alloc(I.allocs, v.res.bar, (size_t)SF3D_RES_LINE * 18)); HIP_TRY(hipMemset(v.res.bar, 0, (size_t)SF3D_RES_LINE * 18 * sizeof(unsigned int)));
            HIP_TRY(dev_alloc(I.allocs, v.res.rec, (size_t)4 * N)); HIP_TRY(hipMemset(v.res.rec, 0, (size_t)4 * N * sizeof(unsigned long long)));
            HIP_TRY(dev_alloc(I.allocs, v.res.prec, (size_t)8 * I.resBlocks)); HIP_TRY(hipMemset(v.res.prec, 0, (size_t)8 * I.resBlocks * sizeof(unsigned long long)));
            HIP_TRY(dev_alloc(I.allocs, v.res.gpub, 8)); HIP_TRY(hipMemset(v.res.gpub, 0, 8 * sizeof(unsigned long long)));
            HIP_TRY(dev_alloc(I.allocs, v.res.prec2, (size_t)8 * I.resBlocks)); HIP_TRY(hipMemset(v.res.prec2, 0, (size_t)8 * I.resBlocks * sizeof(unsigned long long)));
            {   v.res.fusedPost = sw.residentPost;
                if (m.heat) v.res.fusedPost = 0u; }      /* (with coupled heat k_post's successor kernels read what only k_post's launch orders: kept apart) */
            HIP_TRY(dev_alloc(I.allocs, v.res.pub, 32)); HIP_TRY(hipMemset(v.res.pub, 0, 32 * sizeof(double)));
            if (world_ > 1) {
                /* where the cells of the foreign halo rows - the row above the strip (side 0), the row below it (side 1) - arrive in my window */
                std::vector<uint32_t> hs((size_t)2 * pairNZ * pairNX, SF3D_FSRC_NONE);
                v.res.sidePeer[0] = v.res.sidePeer[1] = -1;
                bool oneRank = true;
                for (uint32_t side = 0; side < 2; ++side) {
                    if ((side == 0 && pairOwnLo == 0) || (side == 1 && pairOwnHi >= pairNY)) continue;
                    const uint32_t r = side == 0 ? pairOwnLo - 1 : pairOwnHi;
                    for (uint32_t l = 0; l < pairNZ; ++l)
                        for (uint32_t cc = 0; cc < pairNX; ++cc) {
                            const uint32_t j = l * ns + r * pairNX + cc;
                            const int pr = I.part.owner[j];
                            if (pr == rank_ || pr == SF3D_OWNER_NONE) continue;
                            const auto& lst = I.part.recv[pr];
                            const auto itp = std::lower_bound(lst.begin(), lst.end(), j);
                            if (itp != lst.end() && *itp == j) {
                                hs[((size_t)side * pairNZ + l) * pairNX + cc] = ((uint32_t)pr << 27) | (uint32_t)(itp - lst.begin());
                                if (v.res.sidePeer[side] < 0) v.res.sidePeer[side] = pr; else if (v.res.sidePeer[side] != pr) oneRank = false;
                            }
                        }
                }
                uint32_t* dh; HIP_TRY(dev_alloc(I.allocs, dh, hs.size()));
                HIP_TRY(hipMemcpy(dh, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
                v.res.haloSrc = dh;
                v.res.recFast = 0u; v.res.putBase[0] = v.res.putBase[1] = 0u;
                if (oneRank && edge_rows_direct() && edgePeer[0] == v.res.sidePeer[0] && edgePeer[1] == v.res.sidePeer[1]) {
                    v.res.recFast = 1u; v.res.putBase[0] = edgePut[0]; v.res.putBase[1] = edgePut[1];
                }
                if (!oneRank) { v.res.on = 0; I.resBlocks = 0; }      /* (a halo row shared by two ranks: strips are cut between rows, so never - the kernel counts on it) */
            }
        }
    }
    return SF3D_OK;
}

/* coupled heat transport: state, system, per-node conductivities, boundary and link flux arrays; the colours of the heat sweep and the
 * levels of the reference-order Gauss-Seidel */
sf3d_error_t DeviceSolver::build_heat(HostModel& m, const ParamsHost& p, BuildState& st)
{
    Impl& I = *impl_; DevView& v = I.v; const BuildSwitches& sw = st.sw;
    const uint32_t N = I.N, ns = I.ns, nChunks = v.nChunks; const size_t NS = (size_t)N * SF3D_SLOTS;
    const std::vector<uint8_t>& kind = st.links.kind; const std::vector<uint32_t>& to = st.links.to;
    const std::vector<uint32_t>& listSurf = st.lists.listSurf;
    HeatDev& hv = v.heat;
    hv = HeatDev{};
    hv.on = 1; hv.water = m.water ? 1u : 0u; hv.vapor = m.heatVapor ? 1u : 0u; hv.advection = m.heatAdvection ? 1u : 0u;
    hv.save = m.heatSave; hv.wf = p.heatWeightFactor;
    double* tmp = nullptr;
    for (int k = 0; k < 3; ++k) { HIP_TRY(dev_alloc(I.allocs, hv.TX[k], N)); HIP_TRY(hipMemset(hv.TX[k], 0, N * 8)); }
    auto alloc0 = [&](double*& ptr, size_t cnt) -> hipError_t { hipError_t e = dev_alloc(I.allocs, ptr, cnt); if (e == hipSuccess) e = hipMemset(ptr, 0, cnt * 8); return e; };
    HIP_TRY(alloc0(tmp, N)); hv.heatSink = tmp;
    HIP_TRY(alloc0(hv.heatFlux, N)); HIP_TRY(alloc0(hv.invariant, N));
    HIP_TRY(alloc0(hv.hC, N)); HIP_TRY(alloc0(hv.hcapTerm, N)); HIP_TRY(alloc0(hv.hb, N)); HIP_TRY(alloc0(hv.hD, N));
    HIP_TRY(dev_alloc(I.allocs, hv.hA2, NS / 2)); HIP_TRY(hipMemset(hv.hA2, 0, NS * 8));
    HIP_TRY(alloc0(hv.kHeat, N)); HIP_TRY(alloc0(hv.kIsoVap, N)); HIP_TRY(alloc0(hv.hAvg, N));
    HIP_TRY(alloc0(hv.thetaOld, N)); HIP_TRY(alloc0(hv.thAvgC, N)); HIP_TRY(alloc0(hv.thNewC, N));
    HIP_TRY(alloc0(tmp, N)); hv.airP = tmp; I.heatAirP = tmp;
    HIP_TRY(alloc0(hv.wThLiq, N)); HIP_TRY(alloc0(hv.wThVap, N)); HIP_TRY(alloc0(hv.wTm, N));
    const double** inputs[9] = {&hv.bHeightWind, &hv.bHeightT, &hv.bRoughH, &hv.bT, &hv.bRH, &hv.bWind, &hv.bNetIrr, &hv.bFixT, &hv.bFixDepth};
    for (auto* pp : inputs) { HIP_TRY(alloc0(tmp, N)); *pp = tmp; }
    double** outputs[6] = {&hv.bAero, &hv.bSoilCond, &hv.bSens, &hv.bLat, &hv.bRad, &hv.bAdv};
    const std::vector<double>* outInit[6] = {&m.bAero, &m.bSoilCond, &m.bSens, &m.bLat, &m.bRad, &m.bAdv};   /* NODATA / 0 of setNodeBoundary */
    for (int k = 0; k < 6; ++k) {
        HIP_TRY(alloc0(*outputs[k], N)); I.heatOut[k] = *outputs[k];
        HIP_TRY(hipMemcpy(*outputs[k], outInit[k]->data(), N * 8, hipMemcpyHostToDevice));
    }
    { double* wv = nullptr; HIP_TRY(alloc0(wv, NS)); hv.lwvFlux = reinterpret_cast<sf3d_f2*>(wv); }      /* 8 bytes per link: two floats */
    const int nTypes = (m.heatSave == 2) ? SF3D_FLUX_TYPES : (m.heatSave == 1 ? 1 : 0);
    {   /* never-linked slots hold 0 (calloc in the reference), linked slots NODATA (setNodeLink, soilFluxes3D.cpp:672-678) */
        std::vector<double> init(NS, 0.);
        for (size_t e = 0; e < NS; ++e) if (kind[e] != LK_NONE) init[e] = NODATA_D;
        for (int t = 0; t < nTypes; ++t) {
            HIP_TRY(dev_alloc(I.allocs, hv.lflux[t], NS));
            HIP_TRY(hipMemcpy(hv.lflux[t], init.data(), NS * 8, hipMemcpyHostToDevice));
        }
    }
    {   /* nodeDistance3D (soilPhysics.cpp:334-338) of every link between two soil nodes */
        std::vector<double> d3(NS, 1.);
        parallel_for(N, [&](uint32_t a, uint32_t b) {
            for (uint32_t i = a; i < b; ++i)
                for (int s = 0; s < SF3D_SLOTS; ++s) {
                    const size_t e = (size_t)s * N + i;
                    if (kind[e] != LK_SOIL_VERT && kind[e] != LK_SOIL_LAT) continue;
                    const uint32_t j = to[e];
                    const double dx = m.x[i] - m.x[j], dy = m.y[i] - m.y[j], dz = m.z[i] - m.z[j];
                    double nrm = 0; nrm += dx * dx; nrm += dy * dy; nrm += dz * dz;
                    d3[e] = std::sqrt(nrm);
                }
        });
        HIP_TRY(alloc0(tmp, NS)); hv.hdist = tmp;
        HIP_TRY(hipMemcpy(tmp, d3.data(), NS * 8, hipMemcpyHostToDevice));
    }
    {   /* colours of the heat sweep: layer = hops to the surface through the Up links (layer-major numbering: the node above has
         * a smaller index); a halo node of a strip-local model that lost its Up link is never swept here */
        std::vector<uint8_t> lp(N, 0);
        for (uint32_t i = ns; i < N; ++i) if (kind[i] != LK_NONE && to[i] < i) lp[i] = (uint8_t)(lp[to[i]] + 1);
        uint8_t* dlp; HIP_TRY(dev_alloc(I.allocs, dlp, N));
        HIP_TRY(hipMemcpy(dlp, lp.data(), N, hipMemcpyHostToDevice));
        hv.lpar = dlp;
        /* (a rank of a sharded run: plus, in BOTH lists, the chunks that owe values to a neighbouring rank - every wave puts all the
         * entries of its chunk in each half, the nodes of the other colour with the value they have at that moment) */
        std::vector<uint8_t> owesHeat(nChunks, 0);
        if (world_ > 1) for (int pr = 0; pr < world_; ++pr) for (uint32_t node : I.part.send[pr]) owesHeat[node / SF3D_CHUNK] = 1;
        for (int col = 0; col < 2; ++col) {         /* col 0: odd layers (first half), col 1: even layers */
            std::vector<uint32_t> cl;
            for (uint32_t q : listSurf) {
                const uint32_t i0 = q * SF3D_CHUNK, i1 = (i0 + SF3D_CHUNK < N) ? i0 + SF3D_CHUNK : N;
                bool any = owesHeat[q] != 0;
                for (uint32_t i = i0; i < i1 && !any; ++i) any = ((lp[i] & 1u) != 0u) == (col == 0);
                if (any) cl.push_back(q);
            }
            uint32_t* dcl; HIP_TRY(dev_alloc(I.allocs, dcl, cl.size()));
            if (!cl.empty()) HIP_TRY(hipMemcpy(dcl, cl.data(), cl.size() * 4, hipMemcpyHostToDevice));
            hv.colourList[col] = dcl; hv.nColour[col] = (uint32_t)cl.size();
        }
        hv.redBlack = sw.heatRedBlack;
        /* only where layer parity really colours the vertical links (heat_two_colour_valid, sf3d_model.h).  A rank of a sharded run
         * sees its strip only: its finding travels in its blob and dist_connect turns the two-colour sweep off on EVERY rank if any
         * rank found a violation - all ranks must run the same protocol */
        const bool colourable = heat_two_colour_valid(m);
        I.heatJacobiOnly = !colourable;
        if (hv.redBlack && !colourable) {
            hv.redBlack = 0u;
            if (sw.heatDebug) fprintf(stderr, "sf3d: heat sweep: the node numbering is not layer-major along the Up links - Jacobi instead of the two-colour sweep\n");
        }
    }
    I.gsLevelStart.clear();
    if (sw.heatGS) {
        if (world_ > 1) { snprintf(err_, sizeof(err_), "SF3D_HEAT_GS=1 (reference-order Gauss-Seidel) is a single-GPU verification mode"); return SF3D_PARAMETER_ERROR; }
        /* dependency levels of the serial sweep: a node waits for its linked heat nodes with a smaller index */
        std::vector<uint32_t> level(N, 0u);
        uint32_t maxLevel = 0;
        for (uint32_t i = ns; i < N; ++i) {
            uint32_t l = 0;
            for (int sl = 0; sl < SF3D_SLOTS; ++sl) {
                const size_t e = (size_t)sl * N + i;
                if ((kind[e] == LK_SOIL_VERT || kind[e] == LK_SOIL_LAT) && to[e] < i && level[to[e]] + 1 > l) l = level[to[e]] + 1;
            }
            level[i] = l;
            if (l > maxLevel) maxLevel = l;
        }
        std::vector<uint32_t> start(maxLevel + 2, 0u), order(N > ns ? N - ns : 0);
        for (uint32_t i = ns; i < N; ++i) start[level[i] + 1]++;
        for (uint32_t l = 0; l <= maxLevel; ++l) start[l + 1] += start[l];
        std::vector<uint32_t> pos(start.begin(), start.end() - 1);
        for (uint32_t i = ns; i < N; ++i) order[pos[level[i]]++] = i;
        uint32_t* dord; HIP_TRY(dev_alloc(I.allocs, dord, order.size()));
        if (!order.empty()) HIP_TRY(hipMemcpy(dord, order.data(), order.size() * 4, hipMemcpyHostToDevice));
        hv.gsOrder = dord; hv.gs = 1;
        I.gsLevelStart = start;
    }
    m.heatStateDirty = m.heatSinkDirty = m.heatBoundaryDirty = true;
    m.hostStaleHeat = false;
    for (int t = 0; t < SF3D_FLUX_TYPES; ++t) m.lfluxValid[t] = false;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::sync_to_device(HostModel& m, const ParamsHost& p)
{
    { const sf3d_error_t e = ensure_device(); if (e != SF3D_OK) return e; }
    Impl& I = *impl_;
    /* pending link flow sums are added before anything below re-creates the arrays they read (release) or uploads sums or state */
    if (I.pend.n && built_ && (m.graphDirty || m.stateDirty || m.flowSumsDirty)) HIP_TRY(I.flush_links());
    if (!I.hostCtrl) HIP_TRY(hipHostMalloc((void**)&I.hostCtrl, sizeof(Ctrl), hipHostMallocDefault));

    const uint32_t N = m.N, ns = m.ns;
    const size_t NS = (size_t)N * SF3D_SLOTS;

    if (m.graphDirty || !built_) {
        BuildState st;
        st.sw = read_build_switches();
        const BuildSwitches& sw = st.sw;
        /* a connected strip is frozen: its build arrays may be gone (trimHostStaging drops surf / hasClass / the link tables of the
         * strip-local copy), so this refusal comes BEFORE anything reads them (round 4's advice: an edit after connect segfaulted in
         * the validation loop below and left the peers in their 60 s all-gather time-outs) */
        if (world_ > 1 && connected_) { snprintf(err_, sizeof(err_), "topology changed after sf3d_dist_connect: call sf3d_dist_prepare / export / connect again"); return SF3D_TOPOGRAPHY_ERROR; }
        if (m.surf.size() < N || m.hasClass.size() < N) { snprintf(err_, sizeof(err_), "the model's build arrays were released (a trimmed strip): re-initialise before changing the topology"); return SF3D_TOPOGRAPHY_ERROR; }
        /* the solver relies on surface nodes being exactly [0, ns) (SURVEY.md 8a quirk 5) */
        for (uint32_t i = 0; i < N; ++i) {
            if ((m.surf[i] != 0) != (i < ns)) { snprintf(err_, sizeof(err_), "node %u: surface nodes must be exactly the first nrSurfaceNodes indices", i); return SF3D_TOPOGRAPHY_ERROR; }
            if (!m.hasClass[i]) { snprintf(err_, sizeof(err_), "node %u has no soil/surface class", i); return SF3D_MISSING_DATA_ERROR; }
        }
        /* pull anything newer on the device before the arrays are re-created */
        if (built_) { if (m.hostStaleState) fetch_state(m); if (m.hostStaleFlows) fetch_flows(m); if (m.heat && m.hostStaleHeat && I.v.heat.on) fetch_heat(m); }
        release();
        I.sw = read_step_switches();
        if (I.useFused < 0) I.useFused = sw.fusedDecide;
        I.N = N; I.ns = ns;
        DevView& v = I.v;
        v = DevView{};
        v.N = N; v.ns = ns; v.Nnorm = m.globalN ? m.globalN : N;
        v.nChunks = (N + SF3D_CHUNK - 1) / SF3D_CHUNK;
        v.qSplit = (ns + SF3D_CHUNK - 1) / SF3D_CHUNK;
        if (v.qSplit > v.nChunks) v.qSplit = v.nChunks;

        /* the graph analysis: the stages of sf3d_host_plan.inc, in their order (DESIGN.md 3) */
        I.dslot = plan_slot_alignment(m, sw.slotAlign);
        { const sf3d_error_t e = plan_link_tables(m, I.dslot, rank_, st.links, err_, sizeof(err_)); if (e != SF3D_OK) return e; }
        const std::vector<uint8_t>& kind = st.links.kind; const std::vector<double>&dist = st.links.dist, &area = st.links.area; const std::vector<uint32_t>& to = st.links.to;
        const uint32_t nChunks = v.nChunks;
        st.cdesc = plan_chunk_descriptors(st.links, N, ns);
        std::vector<ChunkDesc>& cdesc = st.cdesc;
        /* (world > 1: the rank's strip + halo rows in local numbering - or the whole grid with SF3D_DIST_LOCAL=0 - is such a grid when
         * the strips are cut between rows; which rows are the rank's is found below, once the partition is known.  The resident sweep loop
         * needs the same description of the grid as the paired passes) */
        const bool regular = (sw.pairSweep != 0 || sw.residentSweep) && !sw.forceMasked && plan_regular_box(st.links, m, st.grid);
        if (!regular && sw.pairSweep != 0) plan_masked_grid(st.links, m, world_, rank_, st.grid);
        const std::vector<uint64_t>&pairNode = st.grid.node, &pairChunk = st.grid.chunk;
        const std::vector<int32_t>& pairIdxMap = st.grid.idxMap;            /* non-empty: the graph is a layered masked grid, not a full box */
        const uint32_t &pairNX = st.grid.NX, &pairNY = st.grid.NY, &pairNZ = st.grid.NZ, &pairOwnLo = st.grid.ownLo, &pairOwnHi = st.grid.ownHi;

        /* ownership + chunk lists (identity lists on one GPU) */
        {
            if (m.presetPartition) I.part = *m.presetPartition;      /* strip-local model: owners and halo lists in local indices */
            else {
                sf3d_error_t pe = sf3d_compute_partition(m, rank_, world_, I.part);
                if (pe != SF3D_OK) { snprintf(err_, sizeof(err_), "partition failed"); return pe; }
            }
        }
        st.lists = plan_chunk_lists(I.part, st.links, N, ns, world_, rank_);
        I.ownedNodes = st.lists.ownedNodes;
        I.propsNeed.swap(st.lists.propsNeed);
        const std::vector<uint32_t>& listSurf = st.lists.listSurf;
        {
            const uint32_t per = SF3D_BLOCK / SF3D_CHUNK;
            v.nListSurf = st.lists.nListSurf;
            v.nList = st.lists.nList;
            auto blocks = [&](uint32_t chunks) { uint32_t b = (chunks + per - 1) / per; if (b > SF3D_MAX_BLOCKS) b = SF3D_MAX_BLOCKS; return b; };
            v.nb = blocks(v.nList); if (v.nb == 0) v.nb = 1;
            v.nbSurf = blocks(v.nListSurf); if (v.nbSurf == 0) v.nbSurf = 1;
            v.nbSoil = blocks(v.nList - v.nListSurf);      /* grids of the two halves of k_assemble */
            if (sw.asmSoilBlocks > 0 && sw.asmSoilBlocks < v.nbSoil) v.nbSoil = sw.asmSoilBlocks;   /* tuning */
            v.world = world_; v.rank = rank_;
        }
        v.pLo = 0; v.pHi = v.nList; v.aLo = v.nListSurf; v.aHi = v.nList;
        double *z, *size, *pond, *sink, *bslope, *bsize, *prescribed, *roughness, *larea, *ldist;
        uint16_t* cls; uint8_t *btype, *lkind; uint32_t* lto; SoilDev* soils; ChunkDesc* dcdesc;
        HIP_TRY(dev_alloc(I.allocs, z, N)); HIP_TRY(dev_alloc(I.allocs, size, N));
        HIP_TRY(dev_alloc(I.allocs, pond, N)); HIP_TRY(dev_alloc(I.allocs, sink, N));
        HIP_TRY(dev_alloc(I.allocs, cls, N)); HIP_TRY(dev_alloc(I.allocs, btype, N));
        HIP_TRY(dev_alloc(I.allocs, bslope, N)); HIP_TRY(dev_alloc(I.allocs, bsize, N));
        HIP_TRY(dev_alloc(I.allocs, prescribed, N));
        HIP_TRY(dev_alloc(I.allocs, lto, NS)); HIP_TRY(dev_alloc(I.allocs, lkind, NS));
        HIP_TRY(dev_alloc(I.allocs, larea, NS)); HIP_TRY(dev_alloc(I.allocs, ldist, NS));
        HIP_TRY(dev_alloc(I.allocs, v.lflowSum, NS)); HIP_TRY(dev_alloc(I.allocs, v.A2x[0], NS / 2)); HIP_TRY(dev_alloc(I.allocs, v.A2x[1], NS / 2));
        {   /* link flow sums in batches - the plain single-GPU path (SF3D_OVERLAP_ACCEPT not 0, no quirk-1 compat rows): SF3D_LINKS_RING matrices
             * instead of two and as many copies of an accepted head, R x 88 B per node.  Memory that is not there is no error: the model
             * then runs with the two matrices and adds the sums inside every step */
            I.overlapAccept = sw.overlapAccept;
            I.ring = 0; I.pend.n = 0;
            if (I.overlapAccept && world_ == 1 && !m.compat) {
                const size_t keep = I.allocs.size(); const uint64_t bytesBefore = g_deviceBytes;
                bool ok = true;
                for (int k = 2; k < SF3D_LINKS_RING && ok; ++k) ok = dev_alloc(I.allocs, v.A2x[k], NS / 2) == hipSuccess;
                for (int k = 0; k < SF3D_LINKS_RING && ok; ++k) ok = dev_alloc(I.allocs, v.Hring[k], N) == hipSuccess;
                if (ok) I.ring = SF3D_LINKS_RING;
                else {
                    (void)hipGetLastError();
                    while (I.allocs.size() > keep) { (void)hipFree(I.allocs.back()); I.allocs.pop_back(); }
                    g_deviceBytes = bytesBefore;
                    for (int k = 2; k < SF3D_LINKS_RING; ++k) v.A2x[k] = nullptr;
                    for (int k = 0; k < SF3D_LINKS_RING; ++k) v.Hring[k] = nullptr;
                }
            }
        }
        HIP_TRY(dev_alloc(I.allocs, v.b, N)); HIP_TRY(dev_alloc(I.allocs, v.C, N));
        for (int k = 0; k < SF3D_POOL; ++k) HIP_TRY(dev_alloc(I.allocs, v.X[k], N));
        HIP_TRY(dev_alloc(I.allocs, v.Se, N)); HIP_TRY(dev_alloc(I.allocs, v.K, N)); HIP_TRY(dev_alloc(I.allocs, v.SeHold, N));
        HIP_TRY(dev_alloc(I.allocs, dcdesc, (size_t)nChunks));
        uint32_t* dlist; HIP_TRY(dev_alloc(I.allocs, dlist, listSurf.size()));
        if (!listSurf.empty()) HIP_TRY(hipMemcpy(dlist, listSurf.data(), listSurf.size() * 4, hipMemcpyHostToDevice));
        v.chunkList = dlist;
        v.asmList = dlist;              /* the assembly walks the chunks in list order */
        v.owner = nullptr; v.dist = nullptr;
        {   /* bytes one rank touches per sweep: 152 B per owned node.  Below the 256 MiB Infinity Cache the whole
             * sweep working set stays cached between sweeps and bypassing costs ~8 % (measured at 0.98 M nodes);
             * above it the coefficient stream would thrash x, b, z: bypass gains ~13 % at 5.2 M nodes */
            const double sweepBytes = 152.0 * (double)v.nList * SF3D_CHUNK;
            v.ntStream = sw.ntStream >= 0 ? sw.ntStream : (sweepBytes > 256.0 * 1024 * 1024);
        }
        {   /* early Courant check (k_courant_probe): on while the last Courant number is >= 0.8 (the reference doubles dt while it is below 0.5, so quiet runs sit between 0.5 and 1: C4 F20 measured 43.6 sim-h/s without the check, 42.5 with a threshold of 0.5, 43.3 with 0.8; C4 F60 hour 0 5.23 -> 5.39 / 5.43); SF3D_COURANT_PROBE=0 turns it off,
             * any other number is the threshold (0: before every approximation) */
            v.probeMin = sw.probeMin;
        }
        I.pairBlocks = 0; I.pairMasked = false; v.pair.masked = 0;
        plan_strip_rows(I.part, N, ns, world_, rank_, st.grid);
        if (!pairNode.empty()) {
            /* the paired sweep pays where the sweep streams from HBM (ntStream: above the Infinity Cache) - below that the plain sweep
             * is cache-resident and faster; SF3D_PAIR_SWEEP=1 forces it on any regular grid (tests on small grids) */
            /* (masked grids, k_sweep_pair_masked: measured at the Ravone project, 5.85 M nodes, 249 us per pair against 2 x 147 us of
             * k_sweep - profiles/README.md; a first version that read the link table was slower than two sweeps) */
            bool on = sw.pairSweep >= 0 ? (sw.pairSweep != 0) : (v.ntStream != 0);      /* (SF3D_PAIR_SWEEP=0: the grid was only described for the resident sweep loop) */
            /* below the Infinity Cache the pass still pays where the patches fill the machine: one of four strips of C4 (1.31 M nodes) 59.4 us
             * per pair against 2 x 36.5, C3 (0.98 M nodes) 45.2 against 2 x 29.0 - cost 1.69 in the model below; one of eight strips of C4
             * (53.4 against 2 x 22.4 us: cost 3.1) and anything smaller keep single sweeps (profiles/r04_pair_W_sweep.txt).
             * SF3D_PAIR_AUTO_COST=x moves the threshold (0: only above the Infinity Cache, round 3's rule) */
            const double autoCost = sw.autoCost;
            const bool tryAuto = sw.pairSweep < 0 && !on && autoCost > 0.;
            if (on || tryAuto) {
                int cus = 256; { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, I.device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount; }
                const PairPlan pp = plan_pair_patches(st.grid, I.part, world_, rank_, cus, SF3D_PAIR_WAVES, tryAuto, autoCost, sw.pairWSet, sw.pairW);
                const uint32_t bestW = pp.bestW, ownRows = pairOwnHi - pairOwnLo;
                const std::vector<uint32_t>(&plist)[4] = pp.plist; const std::vector<uint8_t>(&pdepth)[4] = pp.pdepth;
                if (bestW) {
                    uint32_t* dn; uint64_t* dq;
                    {   /* the kernels decode the eight lateral nibbles only (slots 2 .. 9: bits 8 .. 39 of a node's code) */
                        std::vector<uint32_t> lat(pairNode.size());
                        for (size_t k = 0; k < pairNode.size(); ++k) lat[k] = (uint32_t)(pairNode[k] >> 8);
                        HIP_TRY(dev_alloc(I.allocs, dn, lat.size()));
                        HIP_TRY(hipMemcpy(dn, lat.data(), lat.size() * 4, hipMemcpyHostToDevice));
                    }
                    HIP_TRY(dev_alloc(I.allocs, dq, pairChunk.size()));
                    HIP_TRY(hipMemcpy(dq, pairChunk.data(), pairChunk.size() * 8, hipMemcpyHostToDevice));
                    v.pair.NX = pairNX; v.pair.NY = pairNY; v.pair.NZ = pairNZ; v.pair.W = bestW;
                    v.pair.ownLo = pairOwnLo; v.pair.ownHi = pairOwnHi;
                    v.pair.patchCols = pairNX / 64; v.pair.patchRows = (ownRows + bestW - 3) / (bestW - 2);
                    v.pair.nodeLat = dn; v.pair.chunkCode = dq;
                    I.pairBlocks = v.pair.patchCols * v.pair.patchRows;
                    v.pair.masked = 0; I.pairMasked = false;
                    if (!pairIdxMap.empty()) {
                        const int wi = pair_widx(bestW);
                        int32_t* dm; uint32_t* dl; uint8_t* dd;
                        HIP_TRY(dev_alloc(I.allocs, dm, pairIdxMap.size())); HIP_TRY(dev_alloc(I.allocs, dl, plist[wi].size())); HIP_TRY(dev_alloc(I.allocs, dd, pdepth[wi].size()));
                        HIP_TRY(hipMemcpy(dm, pairIdxMap.data(), pairIdxMap.size() * 4, hipMemcpyHostToDevice));
                        HIP_TRY(hipMemcpy(dl, plist[wi].data(), plist[wi].size() * 4, hipMemcpyHostToDevice));
                        HIP_TRY(hipMemcpy(dd, pdepth[wi].data(), pdepth[wi].size(), hipMemcpyHostToDevice));
                        v.pair.masked = 1; v.pair.idxMap = dm; v.pair.patchList = dl; v.pair.patchDepth = dd;
                        I.pairBlocks = (uint32_t)plist[wi].size(); I.pairMasked = true;
                    }
                }
            }
        }
        if (world_ > 1) { const sf3d_error_t e = build_dist_window(st); if (e != SF3D_OK) return e; }
        { const sf3d_error_t e = build_resident_plan(m, st); if (e != SF3D_OK) return e; }
        if (m.compat) {      /* quirk-1 emulation: calloc'd like the reference's rows (soilFluxes3D.cpp:76-155) */
            HIP_TRY(dev_alloc(I.allocs, v.compatCv, (size_t)N * (SF3D_SLOTS + 2))); HIP_TRY(hipMemset(v.compatCv, 0, (size_t)N * (SF3D_SLOTS + 2) * 8));
            HIP_TRY(dev_alloc(I.allocs, v.compatCn, N)); HIP_TRY(hipMemset(v.compatCn, 0, N));
            HIP_TRY(dev_alloc(I.allocs, v.compatDiag, N)); HIP_TRY(hipMemset(v.compatDiag, 0, (size_t)N * 8));
        }
        if (m.cgArrays && world_ == 1) {      /* device conjugate gradients (SF3D_LINEAL_DEVICE_CG=1) */
            HIP_TRY(dev_alloc(I.allocs, v.cgDiag, N)); HIP_TRY(dev_alloc(I.allocs, v.cgR, N)); HIP_TRY(dev_alloc(I.allocs, v.cgP, N)); HIP_TRY(dev_alloc(I.allocs, v.cgQ, N));
            HIP_TRY(hipMemset(v.cgDiag, 0, (size_t)N * 8)); HIP_TRY(hipMemset(v.cgR, 0, (size_t)N * 8)); HIP_TRY(hipMemset(v.cgP, 0, (size_t)N * 8)); HIP_TRY(hipMemset(v.cgQ, 0, (size_t)N * 8));
        }
        HIP_TRY(dev_alloc(I.allocs, v.flow, N)); HIP_TRY(dev_alloc(I.allocs, v.bflowRate, N));
        HIP_TRY(dev_alloc(I.allocs, v.bflowSum, N));
        {   const size_t np = std::max<size_t>(v.nb + v.nbSurf, I.pairBlocks) + 8;
            HIP_TRY(dev_alloc(I.allocs, v.part0, np)); HIP_TRY(dev_alloc(I.allocs, v.part1, np));
            HIP_TRY(dev_alloc(I.allocs, v.part2, np)); HIP_TRY(dev_alloc(I.allocs, v.part3, np)); }
        HIP_TRY(dev_alloc(I.allocs, v.arrive, 16 * 17)); HIP_TRY(hipMemset(v.arrive, 0, 16 * 17 * sizeof(unsigned int)));
        HIP_TRY(dev_alloc(I.allocs, v.gridBar, 16)); HIP_TRY(hipMemset(v.gridBar, 0, 16 * sizeof(unsigned int)));
        HIP_TRY(dev_alloc(I.allocs, soils, m.soils.size())); HIP_TRY(dev_alloc(I.allocs, roughness, m.roughness.size()));
        HIP_TRY(dev_alloc(I.allocs, v.ctrl, 1));
        v.z = z; v.size = size; v.pond = pond; v.sink = sink; v.cls = cls; v.btype = btype;
        v.bslope = bslope; v.bsize = bsize; v.prescribed = prescribed;
        v.lto = lto; v.lkind = lkind; v.larea = larea; v.ldist = ldist; v.soils = soils; v.roughness = roughness;
        v.cdesc = dcdesc;

        I.heatAirP = nullptr;
        if (m.heat) { const sf3d_error_t e = build_heat(m, p, st); if (e != SF3D_OK) return e; }

        std::vector<SoilDev> sd(m.soils.size());
        for (size_t k = 0; k < sd.size(); ++k) {
            const SoilHost& s = m.soils[k];
            sd[k] = SoilDev{s.alpha, s.n, s.m, s.he, s.Sc, 1.0 / s.Sc, s.thetaS, s.thetaR, s.Ksat, s.L, 1.0 / s.m, s.mualemDen, s.clay, s.organicMatter};
        }
        HIP_TRY(hipMemcpy(z, m.z.data(), N * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(size, m.size.data(), N * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(cls, m.cls.data(), N * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(lto, to.data(), NS * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(lkind, kind.data(), NS, hipMemcpyHostToDevice));
        {   /* which end of a runoff link the early Courant check evaluates (DevView::probeMask) */
            const std::vector<uint8_t> pm = plan_probe_mask(st.links, N, ns);
            /* the check looks at the lateral slots only; a caller may also link two surface nodes Up / Down (setNodeLink allows it and the
             * assembly counts that link's Courant term): the partial maximum would then refuse with another dt than checkCourant - off */
            for (int sl = 0; sl < 2 && v.probeMin >= 0.; ++sl)
                for (uint32_t i = 0; i < ns; ++i) if (kind[(size_t)sl * N + i] == LK_RUNOFF) { v.probeMin = -1.; break; }
            uint8_t* dpm; HIP_TRY(dev_alloc(I.allocs, dpm, (size_t)(ns ? ns : 1)));
            if (ns) HIP_TRY(hipMemcpy(dpm, pm.data(), ns, hipMemcpyHostToDevice));
            v.probeMask = dpm;
        }
        {   std::vector<uint16_t> mask(N, 0);
            for (int sl = 0; sl < SF3D_SLOTS; ++sl) { const uint8_t* kk = kind.data() + (size_t)sl * N; for (uint32_t i = 0; i < N; ++i) if (kk[i] != LK_NONE) mask[i] |= (uint16_t)(1u << sl); }
            uint16_t* dm; HIP_TRY(dev_alloc(I.allocs, dm, N));
            HIP_TRY(hipMemcpy(dm, mask.data(), (size_t)N * 2, hipMemcpyHostToDevice));
            v.lmask = dm; }
        HIP_TRY(hipMemcpy(larea, area.data(), NS * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ldist, dist.data(), NS * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dcdesc, cdesc.data(), cdesc.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice));
        if (!sd.empty()) HIP_TRY(hipMemcpy(soils, sd.data(), sd.size() * sizeof(SoilDev), hipMemcpyHostToDevice));
        if (!m.roughness.empty()) HIP_TRY(hipMemcpy(roughness, m.roughness.data(), m.roughness.size() * 8, hipMemcpyHostToDevice));
        for (uint32_t k = 0; k < (I.ring ? I.ring : 2u); ++k) HIP_TRY(hipMemset(v.A2x[k], 0, NS * 8));
        for (uint32_t k = 0; k < I.ring; ++k) HIP_TRY(hipMemset(v.Hring[k], 0, N * 8));
        HIP_TRY(hipMemset(v.b, 0, N * 8)); HIP_TRY(hipMemset(v.C, 0, N * 8));
        HIP_TRY(hipMemset(v.flow, 0, N * 8)); HIP_TRY(hipMemset(v.bflowRate, 0, N * 8)); HIP_TRY(hipMemset(v.SeHold, 0, N * 8));
        for (int k = 0; k < SF3D_POOL; ++k) HIP_TRY(hipMemset(v.X[k], 0, N * 8));
        if (m.heat && I.heatAirP) hipLaunchKernelGGL(k_heat_static, dim3(v.nb), dim3(SF3D_BLOCK), 0, 0, v, I.heatAirP);
        HIP_TRY(hipDeviceSynchronize());      /* null-stream fills must land before the (non-blocking) solver stream runs */

        std::memset(&mirror_, 0, sizeof(mirror_));
        mirror_.cur = 0; mirror_.hold = 0; mirror_.best = -1; mirror_.stage = ST_IDLE;
        mirror_.bestMBR = NODATA_D;
        mirror_.tCur = 0; mirror_.tOld = 0; mirror_.hStage = HS_IDLE;
        mirror_.aRing = I.ring ? I.ring : 2u;
        built_ = true;
        m.graphDirty = false;
        m.stateDirty = m.sinkDirty = m.pondDirty = m.boundaryDirty = m.flowSumsDirty = m.ctrlDirty = true;
        m.sinkLo = 0; m.sinkHi = UINT32_MAX;
        m.hostStaleState = m.hostStaleFlows = false;
    }

    DevView& v = I.v;
    if (m.stateDirty) {
        HIP_TRY(hipMemcpyAsync(v.X[mirror_.cur], m.H.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        HIP_TRY(hipMemcpyAsync(v.Se, m.Se.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        HIP_TRY(hipMemcpyAsync(v.K, m.K.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        mirror_.seSource = 0; m.ctrlDirty = true;      /* Se now comes from the host's libm: the next attempt recomputes it on the device */
        m.stateDirty = false;
    }
    if (m.sinkDirty) {
        const uint32_t lo = m.sinkLo < N ? m.sinkLo : 0u, hi = m.sinkHi > N ? N : m.sinkHi;      /* only the range the setters touched */
        if (hi > lo) HIP_TRY(hipMemcpyAsync((void*)(v.sink + lo), m.sink.data() + lo, (size_t)(hi - lo) * 8, hipMemcpyHostToDevice, I.stream));
        m.sinkDirty = false; m.sinkLo = 0; m.sinkHi = 0;
    }
    if (m.pondDirty) { HIP_TRY(hipMemcpyAsync((void*)v.pond, m.pond.data(), N * 8, hipMemcpyHostToDevice, I.stream)); m.pondDirty = false; }
    if (m.boundaryDirty) {
        HIP_TRY(hipMemcpyAsync((void*)v.btype, m.btype.data(), N, hipMemcpyHostToDevice, I.stream));
        HIP_TRY(hipMemcpyAsync((void*)v.bslope, m.bslope.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        HIP_TRY(hipMemcpyAsync((void*)v.bsize, m.bsize.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        HIP_TRY(hipMemcpyAsync((void*)v.prescribed, m.prescribed.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        m.boundaryDirty = false;
    }
    if (m.flowSumsDirty) {
        HIP_TRY(hipMemcpyAsync(v.bflowSum, m.bflowSum.data(), N * 8, hipMemcpyHostToDevice, I.stream));
        if (I.dslot.empty()) {
            for (int s = 0; s < SF3D_SLOTS; ++s)
                HIP_TRY(hipMemcpyAsync(v.lflowSum + (size_t)s * N, m.lflowSum[s].data(), N * 8, hipMemcpyHostToDevice, I.stream));
        } else {                                   /* insertion order -> device slots */
            I.stage.resize(NS);
            for (int s = 0; s < SF3D_SLOTS; ++s) {
                const uint8_t* d = I.dslot.data() + (size_t)s * N; const double* src = m.lflowSum[s].data();
                for (uint32_t i = 0; i < N; ++i) I.stage[(size_t)d[i] * N + i] = src[i];
            }
            HIP_TRY(hipMemcpyAsync(v.lflowSum, I.stage.data(), NS * 8, hipMemcpyHostToDevice, I.stream));
            HIP_TRY(hipStreamSynchronize(I.stream));
        }
        m.flowSumsDirty = false;
    }
    if (v.heat.on) {
        HeatDev& hv = v.heat;
        if (m.heatStateDirty) {      /* setNodeTemperature sets temperature and oldTemperature (soilFluxes3D.cpp:1308-1309) */
            if (mirror_.tOld != mirror_.tCur) { mirror_.tOld = mirror_.tCur; m.ctrlDirty = true; }
            HIP_TRY(hipMemcpyAsync(hv.TX[mirror_.tCur], m.temperature.data(), N * 8, hipMemcpyHostToDevice, I.stream));
            m.heatStateDirty = false;
        }
        if (m.heatSinkDirty) { HIP_TRY(hipMemcpyAsync((void*)hv.heatSink, m.heatSink.data(), N * 8, hipMemcpyHostToDevice, I.stream)); m.heatSinkDirty = false; }
        if (m.heatBoundaryDirty) {
            const std::vector<double>* src[9] = {&m.bHeightWind, &m.bHeightT, &m.bRoughH, &m.bT, &m.bRH, &m.bWind, &m.bNetIrr, &m.bFixT, &m.bFixDepth};
            const double* dst[9] = {hv.bHeightWind, hv.bHeightT, hv.bRoughH, hv.bT, hv.bRH, hv.bWind, hv.bNetIrr, hv.bFixT, hv.bFixDepth};
            for (int k = 0; k < 9; ++k) HIP_TRY(hipMemcpyAsync((void*)dst[k], src[k]->data(), N * 8, hipMemcpyHostToDevice, I.stream));
            m.heatBoundaryDirty = false;
        }
    }
    if (m.ctrlDirty || ctrlEdited_) {
        if (mirror_.wrc != p.wrc) mirror_.seSource = 0;      /* another retention curve: the stored Se belongs to the old one */
        fill_params(mirror_, p);
        HIP_TRY(hipMemcpyAsync(v.ctrl, &mirror_, sizeof(Ctrl), hipMemcpyHostToDevice, I.stream));
        m.ctrlDirty = false; ctrlEdited_ = false;
    }
    /* pageable-source async copies return once staged, but be explicit before host buffers change */
    HIP_TRY(hipStreamSynchronize(I.stream));
    return SF3D_OK;
}

