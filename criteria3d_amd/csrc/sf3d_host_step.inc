/* part of sf3d_solver.hip (included there, in this order: physics, control, phases, host_plan, host_build, host_step) - host side, part 2: read-backs, heat queries, the multi-GPU set-up (export / connect / finalize), device math probes, kernel timing, and the step driver: the one graph cache (Impl::replay), StepCtx (what the parts of a step share, and the queueing of node properties, a water batch, the slabs and a heat group), the water and heat poll loops (step_water, step_heat), the end of a step with the resident loop's retry (step_finish) and DeviceSolver::step, which plans (plan_step, sf3d_host_plan.inc) and calls them in turn */
sf3d_error_t DeviceSolver::fetch_state(HostModel& m)
{
    Impl& I = *impl_;
    HIP_TRY(hipMemcpyAsync(m.H.data(), I.v.X[mirror_.cur], (size_t)m.N * 8, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipMemcpyAsync(m.Se.data(), I.v.Se, (size_t)m.N * 8, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipMemcpyAsync(m.K.data(), I.v.K, (size_t)m.N * 8, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    /* the API reports Se = 1 and K = NODATA / 0 for surface nodes as the setters left them */
    m.hostStaleState = false;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::fetch_flows(HostModel& m)
{
    Impl& I = *impl_;
    const size_t N = m.N;
    HIP_TRY(I.flush_links());      /* link flow sums of the accepted steps still pending: added on the stream the copies below are queued on */
    HIP_TRY(hipMemcpyAsync(m.bflowSum.data(), I.v.bflowSum, N * 8, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipMemcpyAsync(m.bflowRate.data(), I.v.bflowRate, N * 8, hipMemcpyDeviceToHost, I.stream));
    if (I.dslot.empty()) {
        for (int s = 0; s < SF3D_SLOTS; ++s)
            HIP_TRY(hipMemcpyAsync(m.lflowSum[s].data(), I.v.lflowSum + (size_t)s * N, N * 8, hipMemcpyDeviceToHost, I.stream));
        HIP_TRY(hipStreamSynchronize(I.stream));
    } else {                                       /* device slots -> insertion order */
        I.stage.resize(N * SF3D_SLOTS);
        HIP_TRY(hipMemcpyAsync(I.stage.data(), I.v.lflowSum, N * SF3D_SLOTS * 8, hipMemcpyDeviceToHost, I.stream));
        HIP_TRY(hipStreamSynchronize(I.stream));
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            const uint8_t* d = I.dslot.data() + (size_t)s * N; double* dst = m.lflowSum[s].data();
            for (size_t i = 0; i < N; ++i) dst[i] = I.stage[(size_t)d[i] * N + i];
        }
    }
    m.hostStaleFlows = false;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::fetch_heat(HostModel& m)
{
    Impl& I = *impl_;
    const size_t N = m.N;
    if (!I.v.heat.on) return SF3D_OK;
    HIP_TRY(hipMemcpyAsync(m.temperature.data(), I.v.heat.TX[mirror_.tCur], N * 8, hipMemcpyDeviceToHost, I.stream));
    std::vector<double>* dst[6] = {&m.bAero, &m.bSoilCond, &m.bSens, &m.bLat, &m.bRad, &m.bAdv};
    for (int k = 0; k < 6; ++k) HIP_TRY(hipMemcpyAsync(dst[k]->data(), I.heatOut[k], N * 8, hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    m.hostStaleHeat = false;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::fetch_link_flux(HostModel& m, int type)
{
    Impl& I = *impl_;
    if (type < 0 || type >= SF3D_FLUX_TYPES || !I.v.heat.on || !I.v.heat.lflux[type]) return SF3D_MISSING_DATA_ERROR;
    const size_t NS = (size_t)m.N * SF3D_SLOTS;
    m.lfluxCache[type].resize(NS);
    if (I.dslot.empty()) {
        HIP_TRY(hipMemcpyAsync(m.lfluxCache[type].data(), I.v.heat.lflux[type], NS * 8, hipMemcpyDeviceToHost, I.stream));
        HIP_TRY(hipStreamSynchronize(I.stream));
    } else {                                       /* device slots -> insertion order */
        I.stage.resize(NS);
        HIP_TRY(hipMemcpyAsync(I.stage.data(), I.v.heat.lflux[type], NS * 8, hipMemcpyDeviceToHost, I.stream));
        HIP_TRY(hipStreamSynchronize(I.stream));
        const size_t N = m.N;
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            const uint8_t* d = I.dslot.data() + (size_t)s * N; double* dst = m.lfluxCache[type].data() + (size_t)s * N;
            for (size_t i = 0; i < N; ++i) dst[i] = I.stage[(size_t)d[i] * N + i];
        }
    }
    m.lfluxValid[type] = true;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::heat_query(HostModel& m, const ParamsHost& p, int what, uint32_t node, double h, double* out)
{
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    if (!I.v.heat.on) return SF3D_MISSING_DATA_ERROR;
    hipLaunchKernelGGL(k_heat_query, dim3(1), dim3(1), 0, I.stream, I.v, what, node, h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&I.hostCtrl->query[1], &I.v.ctrl->query[1], sizeof(double), hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    *out = I.hostCtrl->query[1];
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::heat_storage(HostModel& m, const ParamsHost& p, double* out)
{
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    Impl& I = *impl_;
    if (!I.v.heat.on) return SF3D_MISSING_DATA_ERROR;
    hipLaunchKernelGGL(k_heat_storage, dim3(I.v.nb), dim3(SF3D_BLOCK), 0, I.stream, I.v);
    hipLaunchKernelGGL(k_decide_query, dim3(1), dim3(SF3D_BLOCK), 0, I.stream, I.v);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(I.hostCtrl, I.v.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    mirror_ = *I.hostCtrl;
    *out = mirror_.query[0];
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::dist_prepare(int rank, int world)
{
    if (world < 1 || world > SF3D_MAX_RANKS || rank < 0 || rank >= world) { snprintf(err_, sizeof(err_), "dist_prepare: bad rank/world %d/%d", rank, world); return SF3D_PARAMETER_ERROR; }
    if (built_) release();            /* a model built for another (or the same) partition: drop it, sf3d_initialize follows */
    world_ = world; rank_ = rank; connected_ = false;
    return SF3D_OK;
}

/* builds the device state (so the window exists) and returns what the peers need to reach it */
sf3d_error_t DeviceSolver::dist_export(HostModel& m, const ParamsHost& p, DistBlob* out)
{
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    std::memset(out, 0, sizeof(*out));
    out->world = world_; out->rank = rank_; out->nodes = m.globalN ? m.globalN : m.N;
    if (world_ == 1) return SF3D_OK;
    Impl& I = *impl_;
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, I.window));
    static_assert(sizeof(h) <= sizeof(out->ipcHandle), "ipc handle size");
    std::memcpy(out->ipcHandle, &h, sizeof(h));
    for (int r = 0; r < world_; ++r) { out->recvOff[r] = I.hostDist.recvOff[r]; out->recvCount[r] = I.hostDist.recvCount[r]; }
    if (hipDeviceGetPCIBusId(out->pciBusId, (int)sizeof(out->pciBusId), I.device) != hipSuccess) out->pciBusId[0] = 0;
    out->generation = ++I.connectGen;
    out->heatJacobiOnly = (I.v.heat.on && I.heatJacobiOnly) ? 1u : 0u;
    out->resBlocks = I.v.res.on ? I.resBlocks : 0u; out->resCapacity = I.resCapacity;
    out->pairRecords = (I.pairBlocks != 0 && I.v.pair.records) ? I.pairRecordsWish : 0u; out->pairPad = 0u;
    {   /* the fall-back transport: the same window layout in a POSIX shared-memory object (zero-filled by ftruncate); it is only mapped
         * into the GPUs' address spaces if the ranks decide for it (dist_finalize(2)).  Failing to create it is not an error here. */
        I.drop_shm();
        snprintf(I.shmName, sizeof(I.shmName), "/sf3d_win_%d_%d_%u", (int)getpid(), rank_, I.connectGen);
        I.shmFd = shm_open(I.shmName, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (I.shmFd >= 0 && (ftruncate(I.shmFd, (off_t)I.windowBytes) != 0 || posix_fallocate(I.shmFd, 0, (off_t)I.windowBytes) != 0)) { close(I.shmFd); I.shmFd = -1; shm_unlink(I.shmName); }
        if (I.shmFd >= 0) {
            void* ptr = mmap(nullptr, I.windowBytes, PROT_READ | PROT_WRITE, MAP_SHARED, I.shmFd, 0);
            if (ptr == MAP_FAILED) { close(I.shmFd); I.shmFd = -1; shm_unlink(I.shmName); } else I.shmOwn = ptr;
        }
        if (I.shmFd < 0) I.shmName[0] = 0;
        std::memcpy(out->shmName, I.shmName, sizeof(out->shmName));
        out->windowBytes = I.windowBytes;
    }
    {   /* the communicator id only when the RCCL exchange was asked for: ncclGetUniqueId starts RCCL's bootstrap root (listener thread and
         * socket), which the default window path has no use for */
        const char* xe = getenv("SF3D_EXCHANGE");
        if (rank_ == 0 && xe && std::strcmp(xe, "rccl") == 0 && I.load_rccl()) {
            ncclUniqueId id;
            if (I.pGetUniqueId(&id) == ncclSuccess) { static_assert(sizeof(id) <= sizeof(out->ncclId), "ncclUniqueId size"); std::memcpy(out->ncclId, &id, sizeof(id)); }
        }
    }
    return SF3D_OK;
}

static int dist_ping(hipStream_t st, const DistView& d, unsigned long long token, double timeoutS, int world, char* who, size_t whoLen);
void DeviceSolver::print_hops() const
{
    char line[400] = {0}; int pos = 0;
    for (int r = 0; r < world_ && pos < (int)sizeof(line) - 40; ++r) if (r != rank_) pos += snprintf(line + pos, sizeof(line) - pos, " rank %d %.2f us", r, impl_->hopUs[r]);
    fprintf(stderr, "sf3d: rank %d/%d: flag hop through the windows (store to the peer + its polling load, %s):%s\n", rank_, world_,
            impl_->hostMode ? "host memory over PCIe" : "device memory", line);
}
/* out[0] = exchange epochs closed since connect; per rank p: out[1 + 3 p] = flag-hop latency measured at sf3d_dist_finalize [us] (0: not
 * measured - own rank, RCCL transport), out[2 + 3 p] = mean wait for rank p's mailbox per epoch [us], out[3 + 3 p] = longest wait [us] */
sf3d_error_t DeviceSolver::dist_stats(double* out, int capacity)
{
    if (world_ <= 1 || !impl_ || !connected_) { snprintf(err_, sizeof(err_), "dist_stats: no connected multi-GPU model"); return SF3D_MISSING_DATA_ERROR; }
    if (capacity < 1 + 3 * world_) return SF3D_MEMORY_ERROR;
    Impl& I = *impl_;
    unsigned long long st[1 + 2 * SF3D_MAX_RANKS] = {0};
    if (I.distStats) { HIP_TRY(hipStreamSynchronize(I.stream)); HIP_TRY(hipMemcpy(st, I.distStats, sizeof(st), hipMemcpyDeviceToHost)); }
    out[0] = (double)st[0];
    for (int p = 0; p < world_; ++p) {
        out[1 + 3 * p] = I.hopUs[p];
        out[2 + 3 * p] = st[0] ? (double)st[1 + p] / 100. / (double)st[0] : 0.;
        out[3 + 3 * p] = (double)st[1 + SF3D_MAX_RANKS + p] / 100.;
    }
    return SF3D_OK;
}
int DeviceSolver::dist_transport() const { return (world_ > 1 && connected_ && impl_) ? (impl_->rcclMode ? 3 : (impl_->hostMode ? 2 : 1)) : 0; }

sf3d_error_t DeviceSolver::dist_connect(const DistBlob* all)
{
    if (world_ == 1) { connected_ = true; return SF3D_OK; }
    if (!built_) { snprintf(err_, sizeof(err_), "dist_connect before dist_export"); return SF3D_SOLVER_ERROR; }
    Impl& I = *impl_;
    HIP_TRY(hipSetDevice(I.device));
    static_assert(SF3D_MAX_RANKS >= 8, "a node has eight MI355X");
    DistView& d = I.hostDist;
    char why[200] = {0};                  /* why the window exchange is not usable on this rank (empty: it is) */
    for (int r = 0; r < world_; ++r) {
        const DistBlob& b = all[r];
        if ((int)b.world != world_ || (int)b.rank != r || b.nodes != all[rank_].nodes) { snprintf(err_, sizeof(err_), "dist_connect: blob %d does not match (world %u rank %u nodes %llu)", r, b.world, b.rank, (unsigned long long)b.nodes); return SF3D_PARAMETER_ERROR; }
        if (r == rank_) continue;
        /* both sides derived the lists from the same global graph: counts must agree */
        if (b.recvCount[rank_] != d.sendCount[r]) { snprintf(err_, sizeof(err_), "dist_connect: rank %d expects %u nodes from me, I send %u", r, b.recvCount[rank_], d.sendCount[r]); return SF3D_TOPOGRAPHY_ERROR; }
        d.sendOff[r] = b.recvOff[rank_];
        hipIpcMemHandle_t h;
        std::memcpy(&h, b.ipcHandle, sizeof(h));
        void* ptr = nullptr;
        const hipError_t oe = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
        if (oe != hipSuccess) {
            (void)hipGetLastError();
            if (!why[0]) snprintf(why, sizeof(why), "hipIpcOpenMemHandle of rank %d's window failed: %s", r, hipGetErrorString(oe));
            d.win[r] = I.window; d.payload[r] = d.payload[rank_];        /* never dereferenced in the RCCL mode; keeps the view well-formed */
            continue;
        }
        I.peerMaps.push_back(ptr);
        d.win[r] = static_cast<DistWindow*>(ptr);
        d.payload[r] = reinterpret_cast<double*>(static_cast<char*>(ptr) + sizeof(DistWindow));
    }
    /* ---- which physical GPUs: distinct?  peer-reachable? ---- */
    const bool shareOk = getenv("SF3D_BENCH_SHARE_GPU") && getenv("SF3D_BENCH_SHARE_GPU")[0] == '1';
    const char* mine = all[rank_].pciBusId;
    bool distinct = true;
    for (int a = 0; a < world_; ++a)
        for (int r = a + 1; r < world_; ++r)
            if (!all[a].pciBusId[0] || !all[r].pciBusId[0] || std::strncmp(all[a].pciBusId, all[r].pciBusId, sizeof(all[r].pciBusId)) == 0) distinct = false;
    for (int r = 0; r < world_; ++r) {
        if (r == rank_ || !mine[0] || !all[r].pciBusId[0]) continue;
        if (std::strncmp(mine, all[r].pciBusId, sizeof(all[r].pciBusId)) == 0) {
            if (!shareOk && !I.warnedShared) { fprintf(stderr, "sf3d: warning: ranks %d and %d run on the same GPU (%s): one process per GPU is the intended layout (set LOCAL_RANK / sf3d_set_device)\n", rank_, r, mine); I.warnedShared = true; }
            continue;
        }
        int peerDev = -1, can = 1;
        if (hipDeviceGetByPCIBusId(&peerDev, all[r].pciBusId) == hipSuccess && peerDev >= 0 && peerDev != I.device
            && hipDeviceCanAccessPeer(&can, I.device, peerDev) == hipSuccess && !can && !why[0])
            snprintf(why, sizeof(why), "GPU %s (rank %d) cannot access GPU %s (rank %d) peer-to-peer", mine, rank_, all[r].pciBusId, r);
        (void)hipGetLastError();     /* a peer that is not visible to this process (one device per process) is checked by the ping alone */
    }
    const char* xe = getenv("SF3D_EXCHANGE");
    const bool forceRccl = xe && std::strcmp(xe, "rccl") == 0;
    const bool forceHost = xe && std::strcmp(xe, "host") == 0;      /* test / measurement: the host-memory windows although the device windows work */
    I.blobs.assign(all, all + world_);
    if (I.v.heat.on) {      /* the heat sweep's ordering is one decision for the run: Jacobi everywhere if any rank's strip does not admit two colours */
        bool anyJacobi = false;
        for (int r = 0; r < world_; ++r) anyJacobi = anyJacobi || all[r].heatJacobiOnly != 0;
        if (anyJacobi && I.v.heat.redBlack) {
            I.v.heat.redBlack = 0u;
            if (getenv("SF3D_HEAT_DEBUG")) fprintf(stderr, "sf3d: rank %d: heat sweep: a rank's strip is not layer-major along the Up links - Jacobi on every rank\n", rank_);
        }
    }
    {   /* the resident sweep loop: on every rank or on none, and only where the ranks that share a GPU fit on it together */
        bool resAll = true;
        for (int r = 0; r < world_; ++r) {
            if (all[r].resBlocks == 0) resAll = false;
            uint64_t together = 0;
            for (int q = 0; q < world_; ++q)
                if (q == r || (all[r].pciBusId[0] && all[q].pciBusId[0] && std::strncmp(all[r].pciBusId, all[q].pciBusId, sizeof(all[r].pciBusId)) == 0)) together += all[q].resBlocks;
            if (together > all[r].resCapacity) resAll = false;
        }
        if (!resAll && I.v.res.on) {
            I.v.res.on = 0; I.resBlocks = 0;
            if (const char* ve = getenv("SF3D_DIST_VERBOSE")) if (ve[0] == '1') fprintf(stderr, "sf3d: rank %d/%d: resident sweep loop off (a rank's strip does not fit on chip, or ranks sharing a GPU do not fit on it together): sweeps as separate launches on every rank\n", rank_, world_);
        }
    }
    {   /* the paired pass with record hand-over: on every rank or on none (a rank on single sweeps, or on the two-launch pass, puts plain values
         * and counts two exchanges where the hand-over counts one) */
        bool recAll = true;
        for (int r = 0; r < world_; ++r) if (all[r].pairRecords == 0u) recAll = false;
        if (!recAll && I.v.pair.records) {
            I.v.pair.records = 0u;
            if (const char* ve = getenv("SF3D_DIST_VERBOSE")) if (ve[0] == '1') fprintf(stderr, "sf3d: rank %d/%d: paired pass: record hand-over off (not every rank runs it): two launches and two exchanges per pass\n", rank_, world_);
        }
    }
    if (forceHost && !why[0]) snprintf(why, sizeof(why), "SF3D_EXCHANGE=host");
    HIP_TRY(hipMemcpy(I.devDist, &d, sizeof(DistView), hipMemcpyHostToDevice));
    I.v.dist = I.devDist;
    /* ---- one value through every window, both ways, within a bound ---- */
    if (!why[0] && !forceRccl) {
        double timeoutS = 5.0;
        if (const char* te = getenv("SF3D_DIST_PING_TIMEOUT_S")) { const double t = atof(te); if (t > 0) timeoutS = t; }
        const unsigned long long token = 0x5F3D000000000000ull + (unsigned long long)all[0].generation;    /* the same on every rank */
        char who[96] = {0};
        const int missing = dist_ping(I.stream, d, token, timeoutS, world_, who, sizeof(who));
        if (missing < 0) { (void)hipGetLastError(); snprintf(why, sizeof(why), "the window self-check kernel failed (cross-device IPC mapping unusable?)"); }
        else if (missing > 0) snprintf(why, sizeof(why), "no answer through the window of rank(s)%s within %.0f s (peer not connected, or device-initiated stores do not cross GPUs here)", who, timeoutS);
    }
    if (const char* ve = getenv("SF3D_DIST_VERBOSE")) if (ve[0] == '1') {
        /* one line per rank: which exchange came up, so that a failed first contact between real GPUs can be read off the launcher's stderr */
        char peers[400] = {0}; int pos = 0;
        for (int r = 0; r < world_ && pos < (int)sizeof(peers) - 80; ++r) {
            if (r == rank_) continue;
            const char* rel = "other GPU";
            int peerDev = -1, can = -1;
            if (mine[0] && all[r].pciBusId[0] && std::strncmp(mine, all[r].pciBusId, sizeof(all[r].pciBusId)) == 0) rel = "SAME GPU";
            else if (hipDeviceGetByPCIBusId(&peerDev, all[r].pciBusId) == hipSuccess && peerDev >= 0) { if (hipDeviceCanAccessPeer(&can, I.device, peerDev) != hipSuccess) can = -1; }
            (void)hipGetLastError();
            pos += snprintf(peers + pos, sizeof(peers) - pos, " [rank %d %s %s%s send %u recv %u]", r, all[r].pciBusId[0] ? all[r].pciBusId : "?", rel,
                            can == 1 ? ", peer access yes" : (can == 0 ? ", peer access NO" : ""), d.sendCount[r], d.recvCount[r]);
        }
        fprintf(stderr, "sf3d: rank %d/%d on GPU %s: exchange %s - windows %s%s%s;%s\n", rank_, world_, mine[0] ? mine : "?",
                forceRccl ? "RCCL (SF3D_EXCHANGE=rccl)" : "HIP-IPC windows", (why[0] || forceRccl) ? ((forceRccl || forceHost) ? "not used" : "FAILED") : "passed the self-check",
                why[0] ? ": " : "", why, peers);
    }
    /* what this rank found; the launcher gathers the ranks' findings and calls dist_finalize with the common decision */
    distStatus_ = (why[0] || forceRccl) ? 1 : 0;
    std::snprintf(distWhy_, sizeof(distWhy_), "%s", forceRccl ? "SF3D_EXCHANGE=rccl" : why);
    if (why[0] && !forceRccl) (void)hipGetLastError();
    I.rcclDistinct = distinct;
    std::memcpy(I.rcclId, all[0].ncclId, sizeof(I.rcclId));
    connected_ = false;                   /* the ranks' common decision comes with sf3d_dist_finalize: one rank whose windows failed while the
                                           * others' passed must not leave the others spinning in the in-kernel exchange */
    return SF3D_OK;
}

/* the common decision of all ranks: keep the windows (all passed), or - only with SF3D_EXCHANGE=rccl - exchange over RCCL */
/* one value through every window, both ways, within a bound (dist_connect: the device windows; dist_finalize(2): the host windows) */
__global__ void k_dist_hop(DistView d, unsigned long long base, int iters, int skip, long long timeoutTicks, unsigned long long* out);
/* flag-hop latency to every peer (us), measured once the ranks' common decision for a window transport is taken: every rank runs this */
static void dist_measure_hops(hipStream_t st, const DistView& d, unsigned generation, int world, double* hopUs)
{
    constexpr int iters = 272, skip = 16;
    unsigned long long* dres = nullptr;
    for (int r = 0; r < world; ++r) hopUs[r] = 0.;
    if (hipMalloc(&dres, sizeof(unsigned long long) * SF3D_MAX_RANKS) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipMemsetAsync(dres, 0, sizeof(unsigned long long) * SF3D_MAX_RANKS, st) == hipSuccess) {
        const unsigned long long base = 0x6000000000000000ull + ((unsigned long long)generation << 32);
        hipLaunchKernelGGL(k_dist_hop, dim3(1), dim3(64 * world), 0, st, d, base, iters, skip, (long long)(20. * 1e8), dres);
        unsigned long long res[SF3D_MAX_RANKS] = {0};
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(res, dres, sizeof(res), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
            for (int r = 0; r < world; ++r) hopUs[r] = (double)res[r] / 100. / (double)(iters - skip);
    }
    (void)hipGetLastError();
    (void)hipFree(dres);
}

static int dist_ping(hipStream_t st, const DistView& d, unsigned long long token, double timeoutS, int world, char* who, size_t whoLen)
{
    int* dres = nullptr;
    /* (the clear on the SAME stream as the kernel: the solver stream is non-blocking, a null-stream hipMemset is not ordered with it and
     * could land after the kernel's answers - every rank then reads as silent: round 4, job 33) */
    if (hipMalloc(&dres, sizeof(int) * SF3D_MAX_RANKS) != hipSuccess) return -1;
    if (hipMemsetAsync(dres, 0, sizeof(int) * SF3D_MAX_RANKS, st) != hipSuccess) { (void)hipFree(dres); return -1; }
    hipLaunchKernelGGL(k_dist_ping, dim3(1), dim3(64), 0, st, d, token, (long long)(timeoutS * 1e8), dres);
    if (hipGetLastError() != hipSuccess) { (void)hipFree(dres); return -1; }      /* (a launch that never happened must not read as "nobody answered") */
    int res[SF3D_MAX_RANKS] = {0};
    hipError_t pe = hipMemcpyAsync(res, dres, sizeof(res), hipMemcpyDeviceToHost, st);
    if (pe == hipSuccess) pe = hipStreamSynchronize(st);
    (void)hipFree(dres);
    if (pe != hipSuccess) return -1;
    int pos = 0, missing = 0;
    for (int r = 0; r < world; ++r) if (!res[r]) { pos += snprintf(who + pos, whoLen - pos, " %d", r); ++missing; }
    return missing;
}

sf3d_error_t DeviceSolver::dist_finalize(int mode)
{
    if (world_ == 1) { connected_ = true; return SF3D_OK; }
    if (!built_ || !impl_->v.dist) { snprintf(err_, sizeof(err_), "dist_finalize before dist_connect"); return SF3D_SOLVER_ERROR; }
    Impl& I = *impl_;
    const bool useRccl = mode == 1;
    if (mode == 2) {
        /* The ranks' common decision: the device windows failed somewhere (or SF3D_EXCHANGE=host).  Every rank maps every rank's
         * host-memory window - POSIX shared memory, registered with HIP so that the kernels reach it with the same system-scope loads
         * and stores over PCIe - and repeats the self-check through them.  Slower than device windows (both ends of an exchange cross
         * the host), same protocol, same bits. */
        HIP_TRY(hipSetDevice(I.device));
        DistView& d = I.hostDist;
        if ((int)I.blobs.size() != world_ || !I.shmOwn) { snprintf(err_, sizeof(err_), "rank %d: no host-memory window to fall back to (shm_open failed: /dev/shm missing or full?)", rank_); fatal_ = true; return SF3D_SOLVER_ERROR; }
        HIP_TRY(hipHostRegister(I.shmOwn, I.windowBytes, hipHostRegisterMapped | hipHostRegisterPortable));
        I.hostMode = true;
        void* dptr = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dptr, I.shmOwn, 0));
        d.win[rank_] = static_cast<DistWindow*>(dptr);
        d.payload[rank_] = reinterpret_cast<double*>(static_cast<char*>(dptr) + sizeof(DistWindow));
        for (int r = 0; r < world_; ++r) {
            if (r == rank_) continue;
            const DistBlob& b = I.blobs[r];
            if (!b.shmName[0]) { snprintf(err_, sizeof(err_), "rank %d: rank %d published no host-memory window", rank_, r); fatal_ = true; return SF3D_SOLVER_ERROR; }
            char name[sizeof(b.shmName) + 1] = {0};
            std::memcpy(name, b.shmName, sizeof(b.shmName));
            const int fd = shm_open(name, O_RDWR, 0600);
            void* ptr = fd >= 0 ? mmap(nullptr, (size_t)b.windowBytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
            if (fd >= 0) close(fd);
            if (ptr == MAP_FAILED) { snprintf(err_, sizeof(err_), "rank %d: cannot map the host-memory window of rank %d (%s)", rank_, r, name); fatal_ = true; return SF3D_SOLVER_ERROR; }
            if (hipHostRegister(ptr, (size_t)b.windowBytes, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) {
                (void)hipGetLastError(); munmap(ptr, (size_t)b.windowBytes);
                snprintf(err_, sizeof(err_), "rank %d: hipHostRegister of rank %d's host-memory window failed", rank_, r); fatal_ = true; return SF3D_SOLVER_ERROR;
            }
            I.shmPeers.push_back({ptr, (size_t)b.windowBytes});
            void* pd = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&pd, ptr, 0));
            d.win[r] = static_cast<DistWindow*>(pd);
            d.payload[r] = reinterpret_cast<double*>(static_cast<char*>(pd) + sizeof(DistWindow));
        }
        d.rccl = 0;
        HIP_TRY(hipMemcpy(I.devDist, &d, sizeof(DistView), hipMemcpyHostToDevice));
        I.v.dist = I.devDist;
        double timeoutS = 20.0;      /* (the peers reach this point at their own pace: map + register of every window) */
        if (const char* te = getenv("SF3D_DIST_PING_TIMEOUT_S")) { const double t = atof(te); if (t > 0) timeoutS = 4. * t; }
        char who[96] = {0};
        const unsigned long long token = 0x5F3D480000000000ull + (unsigned long long)I.blobs[0].generation;
        const int missing = dist_ping(I.stream, d, token, timeoutS, world_, who, sizeof(who));
        if (missing != 0) {
            snprintf(err_, sizeof(err_), "rank %d: host-memory windows: %s%s", rank_, missing < 0 ? "the self-check kernel failed" : "no answer from rank(s)", who);
            fatal_ = true; return SF3D_SOLVER_ERROR;
        }
        /* every peer's token arrived through ITS mapping of my window: the name is no longer needed (the mappings stay valid) - a rank
         * that is killed later leaves nothing behind in /dev/shm */
        if (I.shmName[0]) { shm_unlink(I.shmName); I.shmName[0] = 0; }
        dist_measure_hops(I.stream, d, I.blobs[0].generation, world_, I.hopUs);
        if (getenv("SF3D_DIST_VERBOSE") && getenv("SF3D_DIST_VERBOSE")[0] == '1') {
            fprintf(stderr, "sf3d: rank %d/%d: exchange through HOST-MEMORY windows (POSIX shared memory over PCIe; the device windows: %.120s) - self-check passed\n", rank_, world_, distWhy_);
            print_hops();
        }
        connected_ = true;
        return SF3D_OK;
    }
    if (!useRccl) {
        if (distStatus_ != 0) { snprintf(err_, sizeof(err_), "dist_finalize(windows), but rank %d: %.160s", rank_, distWhy_); return SF3D_SOLVER_ERROR; }
        I.drop_shm();          /* the device windows carry the run: the host-memory copy of the window (tmpfs pages, a name in /dev/shm) goes now, not at release */
        dist_measure_hops(I.stream, I.hostDist, I.blobs.empty() ? 0u : I.blobs[0].generation, world_, I.hopUs);
        if (getenv("SF3D_DIST_VERBOSE") && getenv("SF3D_DIST_VERBOSE")[0] == '1') print_hops();
        connected_ = true;
        return SF3D_OK;
    }
    HIP_TRY(hipSetDevice(I.device));
    DistView& d = I.hostDist;
    const char* xe = getenv("SF3D_EXCHANGE");
    if (!(xe && std::strcmp(xe, "rccl") == 0)) {
        /* The RCCL exchange is opt-in: it has not run on hardware yet (its collectives are queued unconditionally inside look-ahead
         * batches and have no bounded wait), so a failed window check is a hard error on every rank instead of a silent switch */
        snprintf(err_, sizeof(err_), "rank %d: the window exchange failed its self-check on some rank (%.150s); the RCCL exchange is opt-in (SF3D_EXCHANGE=rccl)",
                 rank_, distWhy_[0] ? distWhy_ : "this rank's windows passed");
        fatal_ = true;
        return SF3D_SOLVER_ERROR;
    }
    bool haveId = false;
    for (size_t k = 0; k < sizeof(I.rcclId); ++k) if (I.rcclId[k]) haveId = true;
    /* (RCCL itself refuses two ranks on one device; SF3D_RCCL_SHARED_GPU=1 - set by the tests together with SF3D_RCCL_LIB=<mock> - lets
     * the sequencing run on the one GPU of a test box) */
    const char* sg = getenv("SF3D_RCCL_SHARED_GPU");
    if (sg && sg[0] == '1') I.rcclDistinct = true;
    if ((xe && std::strcmp(xe, "ipc") == 0) || !I.rcclDistinct || !haveId || !I.load_rccl()) {
        snprintf(err_, sizeof(err_), "rank %d: the window exchange is not usable (%.120s) and RCCL is not available either (%s)", rank_, distWhy_,
                 !I.rcclDistinct ? "ranks share a GPU: RCCL needs one GPU per rank" : (!haveId ? "no communicator id in rank 0's blob" : "SF3D_EXCHANGE=ipc / librccl not loadable"));
        return SF3D_SOLVER_ERROR;
    }
    if (I.v.heat.on) { snprintf(err_, sizeof(err_), "the RCCL exchange does not carry the coupled heat step (window exchange only)"); return SF3D_SOLVER_ERROR; }
    ncclUniqueId id;
    std::memcpy(&id, I.rcclId, sizeof(id));
    if (I.pCommInitRank(&I.comm, world_, id, rank_) != ncclSuccess) { I.comm = nullptr; snprintf(err_, sizeof(err_), "rank %d: ncclCommInitRank failed", rank_); return SF3D_SOLVER_ERROR; }
    HIP_TRY(dev_alloc(I.allocs, I.rcclMine, 4)); HIP_TRY(dev_alloc(I.allocs, I.rcclGathered, (size_t)4 * world_ + 1));
    d.rccl = 1; d.mine = I.rcclMine; d.gathered = I.rcclGathered;
    for (int r = 0; r < world_; ++r) {
        double *sb = nullptr, *rb = nullptr;
        HIP_TRY(dev_alloc(I.allocs, sb, (size_t)d.sendCount[r] * 2)); HIP_TRY(dev_alloc(I.allocs, rb, (size_t)d.recvCount[r] * 2));
        d.sendBuf[r] = sb; d.recvBuf[r] = rb;
    }
    I.drop_shm();                        /* (no host-memory windows in this mode either) */
    I.v.haloDirect = 0;                  /* sweeps read the halo from the arrays the unpack filled, not from a window */
    I.useFused = 0;                      /* the exchange sits BETWEEN the kernels: separate decision kernels */
    I.rcclMode = true;
    if (rank_ == 0) fprintf(stderr, "sf3d: multi-GPU exchange over RCCL (ncclSend/ncclRecv halos + ncclAllGather of the partial sums)%s%s\n", distWhy_[0] ? ": " : "", distWhy_);
    HIP_TRY(hipMemcpy(I.devDist, &d, sizeof(DistView), hipMemcpyHostToDevice));
    connected_ = true;
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::total_water_content(HostModel& m, const ParamsHost& p, double* out)
{
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    if (world_ > 1 && !connected_) { snprintf(err_, sizeof(err_), "multi-GPU model used before sf3d_dist_connect / sf3d_dist_finalize%s%.150s", distWhy_[0] ? ": " : "", distWhy_); return SF3D_SOLVER_ERROR; }
    Impl& I = *impl_;
    hipLaunchKernelGGL(k_storage, dim3(I.v.nb), dim3(SF3D_BLOCK), 0, I.stream, I.v);
    if (I.rcclMode) { hipLaunchKernelGGL(k_local_reduce, dim3(1), dim3(SF3D_BLOCK), 0, I.stream, I.v, 0); I.rccl_gather(I.stream); }
    hipLaunchKernelGGL(k_decide_query, dim3(1), dim3(SF3D_BLOCK), 0, I.stream, I.v);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(I.hostCtrl, I.v.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, I.stream));
    HIP_TRY(hipStreamSynchronize(I.stream));
    mirror_ = *I.hostCtrl;
    *out = mirror_.query[0];
    return SF3D_OK;
}

/* start-up self-check of the sharded path (dist_connect): thread p stores a token into rank p's window through the IPC mapping
 * (system-scope store over xGMI) and waits until rank p's token shows up in the own window; out[p] = 1 answered, 0 timed out */
__global__ void k_dist_ping(DistView d, unsigned long long token, long long timeoutTicks, int* out)
{
    const int p = threadIdx.x;
    if (p >= d.world) return;
    if (p == d.rank) { out[p] = 1; return; }
    __hip_atomic_store(&d.win[p]->ping[d.rank], token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const long long t0 = wall_clock64();        /* 100 MHz */
    int ok = 1;
    /* (>=: tokens only grow within the life of a window - ping tokens 0x5F3D..., then the hop measurement's 0x6000... - so a peer that is
     * already measuring hops when this rank's ping kernel gets to look has answered all the same: round 5's advisor, the host-memory
     * windows run their hop measurement right behind their ping without a barrier of the control plane in between) */
    while (__hip_atomic_load(&d.win[d.rank]->ping[p], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < token) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > timeoutTicks) { ok = 0; break; }
    }
    out[p] = ok;
}

/* what one exchange costs between connected ranks: thread p and its counterpart on rank p hand a counter back and forth through the
 * ping slots of each other's windows - iteration k stores token base + k into rank p's window and waits until rank p's k-th token
 * shows up here - `iters` times back to back.  Once the two are in step an iteration takes ONE flag hop (a system-scope store crossing
 * to the peer and being seen by its polling load); out[p] = ticks (100 MHz) of the iterations after the first `skip`, 0 on a time-out.
 * Tokens only grow (the waits compare with >=), so nothing left in a slot can be mistaken for an answer. */
__global__ void k_dist_hop(DistView d, unsigned long long base, int iters, int skip, long long timeoutTicks, unsigned long long* out)
{
    /* one WAVE per peer (lane 0 works): the lanes of one wave would march through the iterations together and every peer would read as
     * the slowest */
    const int p = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) != 0u || p >= d.world) return;
    if (p == d.rank) { out[p] = 0; return; }
    long long tStart = 0;
    const long long t00 = wall_clock64();
    for (int k = 0; k < iters; ++k) {
        if (k == skip) tStart = wall_clock64();
        const unsigned long long tok = base + (unsigned long long)k;
        __hip_atomic_store(&d.win[p]->ping[d.rank], tok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        while (__hip_atomic_load(&d.win[d.rank]->ping[p], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < tok) {
            __builtin_amdgcn_s_sleep(1);
            if (wall_clock64() - t00 > timeoutTicks) { out[p] = 0; return; }
        }
    }
    out[p] = (unsigned long long)(wall_clock64() - tStart);
}

/* which set of elementary functions the kernels were compiled with (sf3d_physics.inc): 1 = the reference C library's operations
 * (sf3d_glibcmath.inc), 0 = the 0.50-ulp table routines (sf3d_fastmath.inc, -DSF3D_LIBM_GLIBC=0) */
extern "C" int sf3d_libm_set(void) { return SF3D_LIBM_GLIBC; }

__global__ void k_device_log(const double* x, double* y, uint32_t n)
{
    fm_init();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = flog(x[i]);
}
__global__ void k_device_exp(const double* x, double* y, uint32_t n)
{
    fm_init();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fexp(x[i]);
}
__global__ void k_device_cbrt(const double* x, double* y, uint32_t n)
{
    fm_init();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = pcbrt(x[i]);
}
__global__ void k_device_pow(const double* x, const double* e, double* y, uint32_t n)
{
    fm_init();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = ppow(x[i], e[i]);
}

/* test hook for "the norm of a Jacobi sweep" (sf3d_physics.inc): the terms x[0 .. n) summed with the sweep kernels' own helpers in two
 * of their associations - assoc 0: k_sweep's (256-thread blocks walking the array with a grid stride, block_sum_dd, then one block over
 * the partials: reduce_partials_sum_dd); assoc 1: the paired passes' (blocks of 11 waves on contiguous runs, the waves of a block merged
 * in order by one thread, then sum_published_dd + wave merges) - as double-doubles (out[0] = hi + lo) and, for contrast, with the same
 * association in plain doubles (out[1]) */
__global__ void k_dd_sum_a(const double* x, uint32_t n, double* ph, double* pl, double* pp)
{
    double hi = 0., lo = 0., plain = 0.;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { dd_add(hi, lo, x[i]); plain += x[i]; }
    block_sum_dd(hi, lo);
    plain = block_sum(plain);
    if (threadIdx.x == 0) { ph[blockIdx.x] = hi; pl[blockIdx.x] = lo; pp[blockIdx.x] = plain; }
}
__global__ void k_dd_sum_a2(const double* ph, const double* pl, const double* pp, uint32_t nb, double* out)
{
    double hi, lo;
    reduce_partials_sum_dd(ph, pl, nb, hi, lo);
    const double plain = reduce_partials_sum(pp, nb);
    if (threadIdx.x == 0) { out[0] = hi + lo; out[1] = plain; }
}
__global__ void k_dd_sum_b(const double* x, uint32_t n, double* ph, double* pl, double* pp)
{
    __shared__ double sm[3][16];
    const uint32_t per = (n + gridDim.x - 1) / gridDim.x, a = blockIdx.x * per, b = (a + per < n) ? a + per : n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    double hi = 0., lo = 0., plain = 0.;
    for (uint32_t i = a + threadIdx.x; i < b; i += blockDim.x) { dd_add(hi, lo, x[i]); plain += x[i]; }
    wave_sum_dd(hi, lo);
    for (int off = 32; off > 0; off >>= 1) plain += __shfl_down(plain, off, 64);
    if (lane == 0) { sm[0][wave] = hi; sm[1][wave] = lo; sm[2][wave] = plain; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0., sl = 0., sp = 0.;
        for (int w = 0; w < nw; ++w) { dd_merge(s, sl, sm[0][w], sm[1][w]); sp += sm[2][w]; }
        ph[blockIdx.x] = s; pl[blockIdx.x] = sl; pp[blockIdx.x] = sp;
    }
}
__global__ void k_dd_sum_b2(const double* ph, const double* pl, const double* pp, uint32_t nb, double* out)
{
    __shared__ double sm[3][SF3D_BLOCK / 64];
    double hi, lo, plain = 0.;
    sum_published_dd(ph, pl, nb, hi, lo);
    for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK) plain += pp[k];
    wave_sum_dd(hi, lo);
    for (int off = 32; off > 0; off >>= 1) plain += __shfl_down(plain, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { sm[0][wave] = hi; sm[1][wave] = lo; sm[2][wave] = plain; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = sm[0][0], al = sm[1][0], p = sm[2][0];
        for (int w = 1; w < SF3D_BLOCK / 64; ++w) { dd_merge(a, al, sm[0][w], sm[1][w]); p += sm[2][w]; }
        out[0] = a + al; out[1] = p;
    }
}

/* test hooks: the kernels' logarithm / pow on host values */
namespace {
struct DevBuf {                      /* scratch device array, released on every exit path */
    double* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
}
sf3d_error_t DeviceSolver::device_log(uint32_t n, const double* x, double* out, int which)
{
    if (n == 0) return SF3D_OK;
    DevBuf dx, dy;
    HIP_TRY(hipMalloc(&dx.p, (size_t)n * 8));
    HIP_TRY(hipMalloc(&dy.p, (size_t)n * 8));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
    if (which == 1) hipLaunchKernelGGL(k_device_exp, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, dy.p, n);
    else if (which == 2) hipLaunchKernelGGL(k_device_cbrt, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, dy.p, n);
    else hipLaunchKernelGGL(k_device_log, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, dy.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dy.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::device_norm_sum(uint32_t n, const double* x, uint32_t blocks, int assoc, double* out)
{
    if (blocks == 0 || blocks > SF3D_MAX_BLOCKS) return SF3D_PARAMETER_ERROR;
    DevBuf dx, dp, dout;
    HIP_TRY(hipMalloc(&dx.p, (size_t)(n ? n : 1) * 8));
    HIP_TRY(hipMalloc(&dp.p, (size_t)blocks * 3 * 8));
    HIP_TRY(hipMalloc(&dout.p, 2 * 8));
    if (n) HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
    double *ph = dp.p, *pl = dp.p + blocks, *pp = dp.p + 2 * (size_t)blocks;
    if (assoc == 0) {
        hipLaunchKernelGGL(k_dd_sum_a, dim3(blocks), dim3(SF3D_BLOCK), 0, 0, dx.p, n, ph, pl, pp);
        hipLaunchKernelGGL(k_dd_sum_a2, dim3(1), dim3(SF3D_BLOCK), 0, 0, ph, pl, pp, blocks, dout.p);
    } else {
        hipLaunchKernelGGL(k_dd_sum_b, dim3(blocks), dim3(11 * 64), 0, 0, dx.p, n, ph, pl, pp);
        hipLaunchKernelGGL(k_dd_sum_b2, dim3(1), dim3(SF3D_BLOCK), 0, 0, ph, pl, pp, blocks, dout.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.p, 2 * 8, hipMemcpyDeviceToHost));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::device_pow(uint32_t n, const double* x, const double* y, double* out)
{
    if (n == 0) return SF3D_OK;
    DevBuf dx, dy, dz;
    HIP_TRY(hipMalloc(&dx.p, (size_t)n * 8));
    HIP_TRY(hipMalloc(&dy.p, (size_t)n * 8));
    HIP_TRY(hipMalloc(&dz.p, (size_t)n * 8));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy.p, y, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_device_pow, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, dy.p, dz.p, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dz.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::timing(int enable)
{
    if (!impl_) impl_ = new Impl();
    impl_->timing = enable;
    if (enable) { for (int k = 0; k < KID_COUNT; ++k) { impl_->launches[k] = 0; impl_->ms[k] = 0; } }
    return SF3D_OK;
}

sf3d_error_t DeviceSolver::stats(int kid, uint64_t* launches, double* ms, uint64_t* nodes)
{
    if (!impl_ || kid < 0 || kid >= KID_COUNT) return SF3D_INDEX_ERROR;
    *launches = impl_->launches[kid]; *ms = impl_->ms[kid]; *nodes = impl_->ownedNodes;      /* what one launch of this rank works on: its strip, halo excluded */
    return SF3D_OK;
}

/* Profiler ranges (SURVEY.md 5: "add rocprofv3 markers").  SF3D_ROCTX=1 brackets every computeStep, every poll group of water
 * approximations and every poll group of heat sub-steps with roctx ranges (rocprofv3 --marker-trace shows them above the kernels: a
 * trace of config 5 + heat is ~40 000 launches per simulated hour).  The library is resolved at run time - librocprofiler-sdk-roctx,
 * else the older libroctx64 - and nothing is linked or called without the switch. */
namespace {
struct Roctx {
    using push_t = int (*)(const char*); using pop_t = int (*)();
    static push_t& push() { static push_t f = nullptr; return f; }
    static pop_t& pop() { static pop_t f = nullptr; return f; }
    static bool on()
    {
        static int state = -1;
        if (state < 0) {
            state = 0;
            const char* e = getenv("SF3D_ROCTX");
            if (e && e[0] == '1') {
                void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
                if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
                if (h) { push() = reinterpret_cast<push_t>(dlsym(h, "roctxRangePushA")); pop() = reinterpret_cast<pop_t>(dlsym(h, "roctxRangePop")); }
                if (push() && pop()) state = 1;
                else fprintf(stderr, "sf3d: SF3D_ROCTX=1 but no roctx library could be loaded: no ranges\n");
            }
        }
        return state == 1;
    }
};
struct RoctxRange {
    bool active;
    explicit RoctxRange(const char* name) : active(Roctx::on()) { if (active) Roctx::push()(name); }
    ~RoctxRange() { if (active) Roctx::pop()(); }
    RoctxRange(const RoctxRange&) = delete; RoctxRange& operator=(const RoctxRange&) = delete;
};
}  // namespace

/* ---- the step driver ----
 * One computeStep (soilFluxes3D.cpp:1785-1821 -> CPUSolver::run -> waterMainLoop).  The host queues one approximation per batch - every
 * kernel guarded by the device stage - and polls the control block once per batch.  Which launch forms a step takes is decided by
 * plan_step (sf3d_host_plan.inc) from scalars; StepCtx queues what the plan says; step_water and step_heat poll; step_finish ends the step. */

/* The ~25 launches of a batch are replayed from an instantiated hipGraph (one per shape): small grids are bound by the host's launch
 * rate otherwise.  Event timing needs eager launches. */
template <class F> hipError_t DeviceSolver::Impl::replay(const GraphKey& key, hipStream_t st, F enqueue)
{
    for (auto& g : graphs) if (g.first == key) return hipGraphLaunch(g.second, st);
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return e;
    enqueue();
    e = hipStreamEndCapture(st, &graph);
    if (e != hipSuccess) return e;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return e;
    graphs.push_back({key, exec});
    return hipGraphLaunch(exec, st);
}

static ViewKernel assemble_kernel(bool fused, bool nt, bool heat)      /* (coupled heat with separate decision kernels: cacheable stores only) */
{
    if (heat) return fused ? (nt ? k_assemble<true, true, true> : k_assemble<true, false, true>) : k_assemble<false, false, true>;
    return fused ? (nt ? k_assemble<true, true, false> : k_assemble<true, false, false>) : (nt ? k_assemble<false, true, false> : k_assemble<false, false, false>);
}

/* the device counters the attribution of event pairs reads, as of the last poll */
struct StepCounts {
    uint64_t counters[8], pairLaunches, singleLaunches, earlyCourant, residentLaunches;
    explicit StepCounts(const Ctrl& c) : pairLaunches(c.pairLaunches), singleLaunches(c.singleLaunches), earlyCourant(c.earlyCourant), residentLaunches(c.residentLaunches)
    { std::memcpy(counters, c.counters, sizeof(counters)); }
};

/* what the parts of one step share: the solver's state, the device view, the plan, the stream and the grids */
struct DeviceSolver::StepCtx {
    Impl& I;
    const DevView& v;
    const StepPlan P;
    const hipStream_t st;
    const bool multi, heatOn;
    const dim3 grid, block, one, pgrid;
    dim3 propsGrid, propsHeatGrid, acceptGrid;                          /* water part (water_grids) */
    ViewKernel sweepFn = nullptr;                                       /* the resident loop's or the paired pass's kernel, where the plan has one */
    dim3 gSaveWater, gBoundary, gHProps, gHAsm, gHPost, gHSave;         /* heat part (heat_grids) */
    bool slabFailed = false;       /* a launch or an event call of the slab experiment failed: the batch is not trusted (checked after the enqueue) */

    StepCtx(Impl& impl, const StepPlan& plan, bool multiRank)
        : I(impl), v(impl.v), P(plan), st(impl.stream), multi(multiRank), heatOn(impl.v.heat.on != 0), grid(impl.v.nb), block(SF3D_BLOCK), one(1), pgrid(impl.pushBlocks ? impl.pushBlocks : 1) {}

    /* grids of the register-heavy kernels: exactly as many blocks as are resident at once - equal work per block, no tail
     * round (at 70 VGPRs only 1 792 of 2 048 blocks fit and the remaining 256 ran alone afterwards).  Every kernel walks the
     * chunk list with its own gridDim, and the fused reductions count gridDim partials, so any grid is valid. */
    dim3 resident(ViewKernel fn) const
    {
        const uint32_t nbk = I.resident_blocks((const void*)fn);
        return dim3(v.nb < nbk ? v.nb : nbk);
    }
    void launch(ViewKernel fn, dim3 g) const { launch_view(fn, g, block, 0, st, v); }
    template <class F> void timed(int kid, F queue)
    {
        if (!P.timedStep || (I.timing == 2 && kid != KID_SWEEP && kid != KID_SWEEP_PAIR && kid != KID_SWEEP_RES)) { queue(); return; }
        hipEvent_t a, b;
        if (I.freeEvents.size() >= 2) { a = I.freeEvents.back(); I.freeEvents.pop_back(); b = I.freeEvents.back(); I.freeEvents.pop_back(); }
        else { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
        (void)hipEventRecord(a, st); queue(); (void)hipEventRecord(b, st);
        I.pending.push_back({a, b, kid});
    }
    void timed_launch(int kid, ViewKernel fn, dim3 g) { timed(kid, [&] { launch(fn, g); }); }

    /* the kernels and grids of the water part; false: the plan names a kernel that was not compiled */
    bool water_grids()
    {
        propsGrid = resident(k_props<0, false>); propsHeatGrid = resident(k_props<0, true>);
        acceptGrid = resident(v.ntStream ? k_accept<true> : k_accept<false>);
        if (P.resOn) sweepFn = res_kernel((int)v.res.K, (int)v.res.NW, multi);
        else if (P.pairOn) sweepFn = pair_kernel(v.pair.W, v.ntStream != 0, multi, v.pair.records != 0, I.pairMasked);
        return sweepFn != nullptr || !(P.resOn || P.pairOn);
    }
    void heat_grids()
    {
        gSaveWater = resident(v.ntStream ? k_heat_save_water<true> : k_heat_save_water<false>); gBoundary = resident(k_heat_boundary);
        gHProps = resident(k_heat_props); gHAsm = resident(v.ntStream ? k_heat_assemble<true> : k_heat_assemble<false>);
        gHPost = resident(k_heat_post); gHSave = resident(k_heat_save);
    }

    /* node properties of one approximation */
    void enqueue_props()
    {
        if (heatOn && multi) {      /* sharded heat always uses the fused exchange; halo conductivities are recomputed locally */
            timed_launch(KID_PROPS, k_props<2, true>, grid);
            launch(k_halo_copy<0>, pgrid);
            launch(k_heat_halo_water, pgrid);
        }
        else if (heatOn) timed_launch(KID_PROPS, k_props<0, true>, propsHeatGrid);
        else if (multi && P.fusedMulti) { timed_launch(KID_PROPS, k_props<2, false>, grid); launch(k_halo_copy<0>, pgrid); }
        else timed_launch(KID_PROPS, k_props<0, false>, propsGrid);
        if (multi && !P.fusedMulti) {
            launch(k_push_kf, pgrid);
            if (I.rcclMode) I.rccl_halo(st, 2);
            launch(k_sync_kf, one);
        }
    }
    /* SF3D_SLAB_OVERLAP=S (experiment, one GPU, no heat): an approximation's node properties and rows queued in S slabs of the chunk
     * list - the rows of slab k (k_assemble: waits for memory at 4 waves per SIMD, VALU half busy) next to the properties of slab
     * k + 1 (k_props: dependent pow chains, a third of the byte roof) on a second stream, both with reduced grids so that their
     * waves share the SIMDs.  What a slab of rows needs of the properties is Impl::propsNeed (sf3d_host_build.inc); the surface rows
     * and the Courant decision go with the last slab.  Same arithmetic per node, a maximum is a maximum: same bits. */
    void enqueue_slabs()
    {
        auto chk = [&](hipError_t e) { if (e != hipSuccess) slabFailed = true; };
        const int S = I.sw.slabs;
        const uint32_t soil = v.nList - v.nListSurf;
        uint32_t aEnd[8], pEnd[8];
        for (int k = 0; k < S; ++k) {
            double share = (double)(k + 1) / S;
            if (I.sw.slabFirst > 0. && I.sw.slabFirst < 1.) share = (k + 1 == S) ? 1. : I.sw.slabFirst + (1. - I.sw.slabFirst) * (double)k / (double)(S - 1);
            aEnd[k] = (k + 1 == S) ? v.nList : v.nListSurf + (uint32_t)(share * soil);
            pEnd[k] = (k + 1 == S) ? v.nList : I.propsNeed[aEnd[k] - 1];
            if (k > 0 && pEnd[k] < pEnd[k - 1]) pEnd[k] = pEnd[k - 1];
        }
        DevView w = v;
        /* properties of slab 0 on the solver's stream, of the others on the second one behind it */
        w.pLo = 0; w.pHi = pEnd[0];
        launch_view(k_props<0, false>, propsGrid, block, 0, st, w); chk(hipGetLastError());
        chk(hipEventRecord(I.evSlab[0], st));
        chk(hipStreamWaitEvent(I.stream3, I.evSlab[0], 0));
        for (int k = 1; k < S; ++k) {
            w.pLo = pEnd[k - 1]; w.pHi = pEnd[k];
            if (w.pHi > w.pLo) { launch_view(k_props<0, false>, dim3(I.sw.slabPropsBlocks), block, 0, I.stream3, w); chk(hipGetLastError()); }
            chk(hipEventRecord(I.evSlab[k], I.stream3));
        }
        /* rows: slab k waits for the properties of slab k; the last one carries the surface rows and the decision */
        w = v;
        for (int k = 0; k < S; ++k) {
            const bool last = k + 1 == S;
            if (k > 0) chk(hipStreamWaitEvent(st, I.evSlab[k], 0));
            w.aLo = k == 0 ? v.nListSurf : aEnd[k - 1]; w.aHi = aEnd[k];
            if (!last) { w.nbSurf = 0; w.nbSoil = I.sw.slabAsmBlocks; }
            else { w.nbSurf = v.nbSurf; w.nbSoil = v.nbSoil; }
            launch_view(assemble_kernel(last, P.asmNT, false), dim3(w.nbSurf + w.nbSoil), block, 0, st, w);
        }
    }
    /* one approximation's worth of guarded kernels: with its head (node properties, rows, Courant decision), `chunk` sweeps, the
     * post-solve part; with its tail, restore-best and the flow sums of the accepted step: once per poll group */
    void enqueue_batch(bool withHead, bool withTail, uint32_t chunk)
    {
        if (withHead) {
            if (P.probeNow) {     /* early Courant check: two small guarded launches (the device looks at the Courant number of the moment) */
                launch(k_props_surface, dim3(v.nbSurf));
                launch(P.asmNT ? k_courant_probe<true> : k_courant_probe<false>, dim3(v.nbSurf));
            }
            if (P.slabOn) enqueue_slabs();
            else {
                enqueue_props();
                timed_launch(KID_ASSEMBLE, assemble_kernel(P.useFused, P.asmNT, heatOn), dim3(v.nbSurf + v.nbSoil));
                if (!P.useFused) {
                    if (!heatOn && I.rcclMode) { hipLaunchKernelGGL(k_local_reduce, one, block, 0, st, v, 1); I.rccl_gather(st); }
                    launch(k_decide_courant, one);
                }
            }
            if (P.compat) launch(k_compat_rows, grid);
        }
        if (P.linealOn) {     /* conjugate gradients instead of Jacobi sweeps: `chunk` counts Jacobi sweeps, CG needs far fewer iterations */
            launch(k_cg_init, grid);
            for (uint32_t k = 0; k < chunk; ++k) timed(KID_SWEEP, [&] { launch(k_cg_matvec, grid); launch(k_cg_update, grid); launch(k_cg_dir, grid); });
            launch(k_cg_finish, grid);
        }
        else if (P.resOn) timed(KID_SWEEP_RES, [&] { launch_view(sweepFn, dim3(I.resBlocks), dim3(v.res.NW * 64), I.resLds, st, v); });
        else if (P.pairOn) {      /* two Jacobi iterations per launch (pair_schedule) */
            const dim3 pgr(I.pairBlocks), pbl((v.pair.W + 1) * 64), bgr((v.nBnd + SF3D_BLOCK / SF3D_CHUNK - 1) / (SF3D_BLOCK / SF3D_CHUNK));
            const PairSchedule s = pair_schedule(chunk, I.sw.pairOddSingle);
            for (uint32_t k = 0; k < s.nPairs; ++k) {
                if (k == s.singleAfter) timed_launch(KID_SWEEP, sweep_kernel(multi ? 2 : 1, v.ntStream != 0), grid);
                timed(KID_SWEEP_PAIR, [&] {
                    launch_view(sweepFn, pgr, pbl, 0, st, v);
                    /* a strip: the pass (x' everywhere, x'' away from the neighbours) + the rows next to the neighbours - unless records were handed
                     * over: every row got both iterations in that launch */
                    if (multi && !v.pair.records) launch(v.ntStream ? k_sweep_bnd<true> : k_sweep_bnd<false>, bgr);
                });
            }
        }
        else for (uint32_t k = 0; k < chunk; ++k) {
            timed_launch(KID_SWEEP, sweep_kernel(P.fused ? 1 : (P.fusedMulti ? 2 : 0), v.ntStream != 0), grid);
            if (P.useFused) continue;
            if (multi) launch(k_push_x, pgrid);
            if (I.rcclMode) { I.rccl_halo(st, 1); hipLaunchKernelGGL(k_local_reduce, one, block, 0, st, v, 3); I.rccl_gather(st); }
            launch(k_decide_sweep, one);
        }
        if (P.useFused) {
            /* (the resident sweep loop does k_post's work in its own launch when the solve ends well - sf3d_resident.inc; k_post follows only as the
             * guard of the cases it leaves out would: none - a solve that ends badly goes back to ST_APPROX, not to ST_POST; and with its fused
             * post-solve part the resident launch stores the halo of its result itself) */
            if (!P.resFusedPost) timed_launch(KID_POST, k_post<true>, grid);
            if (multi && v.haloDirect && !P.resFusedPost) launch(k_halo_copy<1>, pgrid);
        }
        else {
            timed_launch(KID_POST, k_post<false>, grid);
            if (I.rcclMode) { hipLaunchKernelGGL(k_local_reduce, one, block, 0, st, v, 2); I.rccl_gather(st); }
            launch(k_decide_balance, one);
        }
        if (withTail) {
            timed_launch(KID_RESTORE, P.useFused ? (heatOn ? k_restore<true, true> : k_restore<true, false>) : (heatOn ? k_restore<false, true> : k_restore<false, false>), grid);
            if (!P.useFused) {
                if (I.rcclMode) { hipLaunchKernelGGL(k_local_reduce, one, block, 0, st, v, 2); I.rccl_gather(st); }
                launch(k_decide_restore, one);
            }
            if (P.overlap) launch(k_accept_boundary, grid);
            else timed_launch(KID_ACCEPT, v.ntStream ? k_accept<true> : k_accept<false>, acceptGrid);
        }
    }
    hipError_t launch_batch(bool withHead, bool withTail, uint32_t chunk)
    {
        if (!P.replayWater) { enqueue_batch(withHead, withTail, chunk); return hipSuccess; }
        return I.replay(water_graph_key(P, withHead, withTail, chunk), st, [&] { enqueue_batch(withHead, withTail, chunk); });
    }
    /* one poll group of the heat part = `steps` guarded heat steps: boundary, node properties, rows, a run of sweeps, balance, flux bookkeeping */
    void enqueue_heat(uint32_t steps, uint32_t chunk)
    {
        for (uint32_t bq = 0; bq < steps; ++bq) {
            launch(k_heat_boundary, gBoundary);
            launch(k_heat_props, gHProps);
            launch(v.ntStream ? k_heat_assemble<true> : k_heat_assemble<false>, gHAsm);
            if (v.heat.gs) {
                for (uint32_t k = 0; k < chunk; ++k) {
                    launch(k_heat_gs_begin, grid);
                    for (size_t l = 0; l + 1 < I.gsLevelStart.size(); ++l) {
                        const uint32_t first = I.gsLevelStart[l], cnt = I.gsLevelStart[l + 1] - first;
                        if (cnt) hipLaunchKernelGGL(k_heat_gs_level, dim3((cnt + SF3D_BLOCK - 1) / SF3D_BLOCK), block, 0, st, v, first, cnt);
                    }
                    hipLaunchKernelGGL(k_heat_gs_decide, one, one, 0, st, v.ctrl);
                }
            } else
            for (uint32_t k = 0; k < chunk; ++k) {
                if (v.heat.redBlack) { launch(v.ntStream ? k_heat_sweep<0, true> : k_heat_sweep<0, false>, grid); launch(v.ntStream ? k_heat_sweep<1, true> : k_heat_sweep<1, false>, grid); }
                else launch(k_heat_sweep<-1, false>, grid);
            }
            launch(k_heat_post, gHPost);
            if (v.heat.save != 0) launch(k_heat_save, gHSave);
        }
    }
    hipError_t launch_heat(uint32_t steps, uint32_t chunk)
    {
        if (!P.replayHeat) { enqueue_heat(steps, chunk); return hipSuccess; }
        return I.replay(heat_graph_key(steps, chunk, v.heat.save != 0), st, [&] { enqueue_heat(steps, chunk); });
    }
    /* attribute event pairs only to launches that really ran: how many of each kernel ran comes from the device counters (c: now,
     * before: at the last poll); guarded no-op launches are the shortest of a group */
    void attribute_events(const Ctrl& c, const StepCounts& before)
    {
        uint64_t ran[KID_COUNT];
        ran[KID_PROPS] = ran[KID_ASSEMBLE] = (c.counters[2] - before.counters[2]) - (c.earlyCourant - before.earlyCourant);      /* (an attempt the early check refused ran neither) */
        ran[KID_SWEEP] = P.pairOn ? c.singleLaunches - before.singleLaunches : (P.resOn ? 0 : c.counters[3] - before.counters[3]);
        ran[KID_SWEEP_RES] = c.residentLaunches - before.residentLaunches;
        ran[KID_SWEEP_PAIR] = c.pairLaunches - before.pairLaunches;
        ran[KID_POST] = c.counters[7] - before.counters[7];
        ran[KID_RESTORE] = c.counters[6] - before.counters[6];
        ran[KID_ACCEPT] = c.counters[1] - before.counters[1];
        std::vector<float> el[KID_COUNT];
        for (auto& pr : I.pending) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, pr.a, pr.b) == hipSuccess) el[pr.kid].push_back(t);
            I.freeEvents.push_back(pr.a); I.freeEvents.push_back(pr.b);
        }
        I.pending.clear();
        for (int k = 0; k < KID_COUNT; ++k) {
            std::sort(el[k].begin(), el[k].end(), [](float x, float y) { return x > y; });
            for (size_t q = 0; q < el[k].size() && q < ran[k]; ++q) { I.ms[k] += el[k][q]; I.launches[k]++; }
        }
    }
};

/* the water part: look-ahead batches (water_look_ahead), then one batch per poll until the step is accepted or fails */
sf3d_error_t DeviceSolver::step_water(StepCtx& c, double maxTimeStep, uint32_t& stage)
{
    Impl& I = c.I; const DevView& v = c.v; const StepPlan& P = c.P; hipStream_t st = c.st;
    if (!c.water_grids()) { snprintf(err_, sizeof(err_), "no kernel was compiled for the sweep form of this model (%s)", P.resOn ? "resident loop" : "paired pass"); fatal_ = true; return SF3D_SOLVER_ERROR; }
    {   /* this step assembles into the next slot of the ring (k_step_begin): if the sums of the step that used it are still pending the
         * ring is full, and everything pending is added first.  So it is before a step that adds its own sums inside the step
         * (event-timed steps): the sums are added in the order the steps were accepted in. */
        const uint32_t ringSlots = mirror_.aRing < 2u ? 2u : mirror_.aRing;
        if (I.pend.n && (!P.overlap || I.links_pending((mirror_.aBuf + 1u) % ringSlots))) HIP_TRY(I.flush_links());
    }
    hipLaunchKernelGGL(k_step_begin, c.one, c.one, 0, st, v.ctrl, maxTimeStep);
    stage = ST_APPROX;                      /* k_step_begin opens the first attempt */
    StepCounts before(mirror_);
    const uint64_t approxAtStart = mirror_.counters[2];
    int guard = 0;
    if (P.slabOn && !I.stream3) {
        HIP_TRY(hipStreamCreateWithFlags(&I.stream3, hipStreamNonBlocking));
        for (auto& ev : I.evSlab) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    uint32_t look = water_look_ahead(I.lastBatches);
    uint32_t batchIndex = 0;
    while (true) {
        RoctxRange pollRange(look > 1 ? "sf3d water: look-ahead batches of approximations + poll" : "sf3d water: one approximation batch + poll");
        for (uint32_t bq = 0; bq < look; ++bq) {
            const bool head = bq > 0 || stage == ST_APPROX;
            HIP_TRY(c.launch_batch(head, bq + 1 == look, predicted_sweeps(batchIndex, head, I.predCount, I.pred, I.lastSweeps)));
            if (head) ++batchIndex;
        }
        look = 1;
        HIP_TRY(hipGetLastError());
        if (c.slabFailed) { I.sw.slabs = 0; snprintf(err_, sizeof(err_), "SF3D_SLAB_OVERLAP: a launch or an event call of the slab experiment failed - its rows may have read stale node properties"); (void)hipStreamSynchronize(st); fatal_ = true; return SF3D_SOLVER_ERROR; }
        HIP_TRY(hipMemcpyAsync(I.hostCtrl, v.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const Ctrl& hc = *I.hostCtrl;
        if (P.timedStep) c.attribute_events(hc, before);
        before = StepCounts(hc);

        stage = hc.stage;
        if (stage != ST_SWEEP && hc.iter > 0) I.lastSweeps = hc.iter;
        if (stage == ST_ACCEPT || stage == ST_FAIL) break;   /* ST_ACCEPT: bookkeeping done and k_accept has run */
        if (++guard > 1000000) { snprintf(err_, sizeof(err_), "step state machine did not terminate (stage %u)", stage); return SF3D_SOLVER_ERROR; }
    }
    {   /* approximations this step took (rejected attempts included) = batches the next one will queue up front */
        const uint64_t used = I.hostCtrl->counters[2] - approxAtStart;
        I.lastBatches = used < 1 ? 1u : (uint32_t)used;
        I.predCount = I.hostCtrl->seqCount < 16u ? I.hostCtrl->seqCount : 16u;
        for (uint32_t k = 0; k < I.predCount; ++k) I.pred[k] = I.hostCtrl->seqSweeps[k];
    }
    if (P.overlap && stage == ST_ACCEPT) {      /* what k_links_flush needs of this step: where its matrix and head are, and its dt */
        const Ctrl& hc = *I.hostCtrl;
        if (I.pend.n >= (uint32_t)SF3D_LINKS_RING) HIP_TRY(I.flush_links());      /* (never: a full ring was emptied before the step) */
        I.pend.slot[I.pend.n] = hc.acceptABuf < (uint32_t)SF3D_LINKS_RING ? hc.acceptABuf : 0u; I.pend.dt[I.pend.n] = hc.acceptDt; ++I.pend.n;
    }
    return SF3D_OK;
}

/* heat part of computeStep (soilFluxes3D.cpp:1802-1818): every kernel is guarded by Ctrl::hStage; polled once per group of heat steps
 * (heat_look_ahead), which is replayed from an instantiated hipGraph per shape like the water batches */
sf3d_error_t DeviceSolver::step_heat(StepCtx& c, HostModel& m, double maxTimeStep, uint32_t& stage)
{
    Impl& I = c.I; const DevView& v = c.v; hipStream_t st = c.st;
    hipLaunchKernelGGL(k_heat_begin, c.one, c.one, 0, st, v.ctrl, maxTimeStep, m.water ? 1 : 0);
    c.heat_grids();
    c.launch(k_heat_save_water_props, c.resident(k_heat_save_water_props));
    c.launch(v.ntStream ? k_heat_save_water<true> : k_heat_save_water<false>, c.gSaveWater);
    int hguard = 0;
    const uint32_t lookH = heat_look_ahead(I.lastHeatSteps, v.heat.gs != 0);
    RoctxRange heatRange("sf3d heat part of computeStep");
    while (true) {
        RoctxRange heatPoll("sf3d heat: sub-steps + poll");
        HIP_TRY(c.launch_heat(lookH, heat_chunk(I.lastHeatSweeps)));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(I.hostCtrl, v.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const Ctrl& hc = *I.hostCtrl;
        if (hc.hSweepsLast > 0) I.lastHeatSweeps = hc.hSweepsLast;
        if (I.sw.heatDebug == 2) fprintf(stderr, "gpu heatLoop stage %u next dt %g outer %g/%g sweeps %u MBR %.6e storage %.12e sink %.6e courant %.6e\n", hc.hStage, hc.hDt, hc.hOuterDt, hc.hOuterSum, hc.hSweepsLast, hc.heatCur.MBR, hc.heatCur.storage, hc.heatCur.sinkSource, hc.hCourant);
        if (hc.hStage == HS_FINISHED) { I.lastHeatSteps = hc.hRows + hc.hPad; break; }
        if (hc.hStage == HS_IDLE) { snprintf(err_, sizeof(err_), "heat step did not start (water stage %u)", hc.stage); stage = ST_FAIL; fatal_ = true; break; }
        if (++hguard > 1000000) { snprintf(err_, sizeof(err_), "heat state machine did not terminate (stage %u)", hc.hStage); return SF3D_SOLVER_ERROR; }
    }
    if (I.sw.heatDebug) fprintf(stderr, "heat: water dt %g: %u heat steps accepted, %u halved, last dt %g, last sweeps %u, courant %g, MBR %g\n", I.hostCtrl->dtWater, I.hostCtrl->hRows, I.hostCtrl->hPad, I.hostCtrl->hDt, I.hostCtrl->hSweepsLast, I.hostCtrl->hCourant, I.hostCtrl->heatCur.MBR);
    m.hostStaleHeat = true;
    return SF3D_OK;
}

/* the end of a step: the resident loop's retry, or the control block, the error texts and the result */
sf3d_error_t DeviceSolver::step_finish(HostModel& m, ParamsHost& p, double maxTimeStep, double* dtOut, uint32_t stage)
{
    Impl& I = *impl_; const DevView& v = I.v; hipStream_t st = I.stream;
    if (world_ == 1 && stage == ST_FAIL && I.hostCtrl->barTimeout && !I.hostCtrl->distError && I.resBlocks != 0) {
        /* The resident sweep loop gave up: a block waited seconds for the records of another one - its blocks were not on the device together (a
         * GPU shared with another process's long kernels).  Nothing of the step was accepted: put the control block of the step's start back (mirror_
         * still is that; Se of the starting state is evaluated again, the attempt that failed may have overwritten it), turn the loop off for this
         * model and take the step again with the sweeps as separate launches - the same bits, and no drop-in caller sees a solver error for it. */
        fprintf(stderr, "sf3d: warning: resident sweep loop: a wait for another block's records expired (%u blocks not on the device together: is the GPU shared?) - "
                        "the step is taken again with the sweeps as separate launches, and so are the following ones\n", I.resBlocks);
        I.resBlocks = 0; I.v.res.on = 0; I.v.res.forceTimeout = 0;
        Ctrl c0 = mirror_;
        c0.seSource = 0; c0.barTimeout = 0;
        mirror_ = c0;
        HIP_TRY(hipMemcpyAsync(v.ctrl, &mirror_, sizeof(Ctrl), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return step(m, p, maxTimeStep, dtOut);
    }
    mirror_ = *I.hostCtrl;
    if (mirror_.distError) {
        char who[96] = ""; size_t at = 0;
        for (int p = 0; p < world_ && at + 6 < sizeof(who); ++p) if ((mirror_.distSilent >> p) & 1u) at += (size_t)snprintf(who + at, sizeof(who) - at, "%s%d", at ? ", " : "", p);
        snprintf(err_, sizeof(err_), "rank %d: no mail from rank(s) %s within the bounded wait of an exchange epoch%s (multi-GPU exchange: the peer died, hangs or runs far behind)", rank_, who[0] ? who : "?", mirror_.pairRecTimeout ? " (the records of a paired pass: SF3D_PAIR_RECORDS=0 exchanges plain values between two launches)" : "");
        fatal_ = true;
    }
    else if (mirror_.barTimeout) { snprintf(err_, sizeof(err_), "resident sweep loop: a wait for another block's records expired (%u blocks not resident at once?%s); SF3D_RESIDENT_SWEEP=0 runs the sweeps as separate launches", I.resBlocks, world_ > 1 ? " or a neighbouring rank's records did not arrive within SF3D_DIST_TIMEOUT_S" : ""); fatal_ = true; }
    else if (stage != ST_ACCEPT && !fatal_) snprintf(err_, sizeof(err_), "the mass balance is not a number at the minimum time step (stepNan, cpusolver.cpp:176-180): state left as the reference leaves it");
    p.dtCurr = mirror_.dtCurr;
    *dtOut = mirror_.dt;
    m.hostStaleState = true;
    m.hostStaleFlows = true;
    return (stage == ST_ACCEPT) ? SF3D_OK : SF3D_SOLVER_ERROR;
}

/* bring the model up to date, plan, water part, heat part, finish */
sf3d_error_t DeviceSolver::step(HostModel& m, ParamsHost& p, double maxTimeStep, double* dtOut)
{
    RoctxRange stepRange("sf3d computeStep");
    sf3d_error_t e = sync_to_device(m, p);
    if (e != SF3D_OK) return e;
    if (world_ > 1 && !connected_) { snprintf(err_, sizeof(err_), "multi-GPU model used before sf3d_dist_connect / sf3d_dist_finalize%s%.150s", distWhy_[0] ? ": " : "", distWhy_); return SF3D_SOLVER_ERROR; }
    Impl& I = *impl_;
    StepFacts f;
    {
        const DevView& v = I.v; const StepSwitches& sw = I.sw;
        f.multi = world_ > 1; f.heatOn = v.heat.on != 0; f.useFused = I.useFused != 0;
        f.lineal = p.lineal; f.haveCg = v.cgDiag != nullptr;
        f.resAvail = v.res.on && I.resBlocks != 0; f.resFusedPost = v.res.fusedPost != 0;
        f.haloDirect = v.haloDirect != 0; f.rccl = I.rcclMode; f.nBnd = v.nBnd; f.pairAvail = I.pairBlocks != 0;
        f.timing = I.timing; f.sampled = I.timing == 2 && (I.stepSeq++ % 8 == 0);
        f.overlapAccept = I.overlapAccept != 0; f.ring = I.ring != 0; f.compat = v.compatCv != nullptr;
        f.ntStream = v.ntStream != 0; f.asmNtOff = sw.asmNtOff;
        f.probeMin = v.probeMin; f.courant = mirror_.courant; f.probeBudget = mirror_.probeBudget;
        f.slabs = sw.slabs; f.havePropsNeed = !I.propsNeed.empty(); f.nList = v.nList; f.nListSurf = v.nListSurf;
        f.useGraphs = sw.graphs; f.heatGs = v.heat.gs != 0;
        f.residentFailAt = sw.residentFailAt; f.residentSteps = I.stepSeqAll;
    }
    StepCtx c(I, plan_step(f), f.multi);
    I.useFused = c.P.useFused ? 1 : 0;
    if (c.P.countsResidentStep) { I.v.res.forceTimeout = c.P.forceTimeout ? 1u : 0u; ++I.stepSeqAll; }

    if (c.heatOn) {                         /* computeStep head, soilFluxes3D.cpp:1787-1791 */
        if (c.v.heat.save == 2) c.launch(k_heat_reset_water_fluxes, c.grid);
        c.launch(k_heat_conductance, c.grid);
        for (int t = 0; t < SF3D_FLUX_TYPES; ++t) m.lfluxValid[t] = false;
    }
    uint32_t stage = ST_ACCEPT;
    if (m.water) { e = step_water(c, maxTimeStep, stage); if (e != SF3D_OK) return e; }
    if (c.heatOn && stage == ST_ACCEPT) { e = step_heat(c, m, maxTimeStep, stage); if (e != SF3D_OK) return e; }
    else if (!m.water) {
        HIP_TRY(hipMemcpyAsync(I.hostCtrl, c.v.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
    }
    return step_finish(m, p, maxTimeStep, dtOut, stage);
}
