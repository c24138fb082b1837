/* part of sf3d_solver.hip (included there, in this order: physics, control, phases, host_build, host_step) - device side of the multi-GPU exchange, the last-block hand-off inside a launch, and the one-block control kernels of the step state machine */
/* ======================================================================================= */
/* multi-GPU exchange (device side)                                                          */
/* ======================================================================================= */

#define SYS_STORE(p, x) __hip_atomic_store((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
#define SYS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)

/* a double as two tagged 8-byte words: (low 32 bits | tag << 32), (high 32 bits | tag << 32) */
__device__ __forceinline__ unsigned long long rec_lo(double x, uint32_t tag) { return ((unsigned long long)__double_as_longlong(x) & 0xFFFFFFFFull) | ((unsigned long long)tag << 32); }
__device__ __forceinline__ unsigned long long rec_hi(double x, uint32_t tag) { return ((unsigned long long)__double_as_longlong(x) >> 32) | ((unsigned long long)tag << 32); }
__device__ __forceinline__ bool rec_ok(unsigned long long a, unsigned long long b, uint32_t tag) { return (uint32_t)(a >> 32) == tag && (uint32_t)(b >> 32) == tag; }
__device__ __forceinline__ double rec_value(unsigned long long a, unsigned long long b) { return __longlong_as_double((long long)((a & 0xFFFFFFFFull) | (b << 32))); }

/* One block.  All-gather of up to four doubles per rank through the peers' windows, combined in
 * rank order (identical bits on every rank).  op 0 = sum, 1 = max, 2 = sum with (v0, v1) a double-double (the norm of a sweep),
 * 3 = (v0, v1) and (v2, v3) double-doubles (both norms of a paired pass).  Advances the epoch.
 * Returns false (and raises distError / ST_FAIL, the silent peers in Ctrl::distSilent) when a peer does not answer within DistView::spinTicks (10 s; SF3D_DIST_TIMEOUT_S). */
__device__ __forceinline__ void dist_combine(double (&acc)[4], const double (&x)[4], int K, int op, bool first)
{
    if (first) { for (int k = 0; k < K; ++k) acc[k] = x[k]; return; }
    if (op == 1) { for (int k = 0; k < K; ++k) acc[k] = dmax(acc[k], x[k]); return; }
    if (op >= 2) {
        dd_merge(acc[0], acc[1], x[0], x[1]);
        if (op == 3) dd_merge(acc[2], acc[3], x[2], x[3]); else for (int k = 2; k < K; ++k) acc[k] += x[k];
        return;
    }
    for (int k = 0; k < K; ++k) acc[k] += x[k];
}
template <int K>
__device__ __forceinline__ bool dist_allgather(const DevView& v, Ctrl* c, double (&vals)[K], int op)
{
    static_assert(K >= 1 && K <= 4, "a mailbox holds four values");
    if (v.world <= 1) return true;
    if (v.dist->rccl) {        /* the host queued k_local_reduce + ncclAllGather (four doubles per rank) before this kernel: combine in rank order */
        __shared__ double shR[4];
        if (threadIdx.x == 0) {
            const double* g = v.dist->gathered;
            double acc[4] = {0., 0., 0., 0.};
            for (int p = 0; p < v.world; ++p) { const double x[4] = {g[4 * p], g[4 * p + 1], g[4 * p + 2], g[4 * p + 3]}; dist_combine(acc, x, K, op, p == 0); }
            for (int k = 0; k < 4; ++k) shR[k] = acc[k];
            c->epoch = c->epoch + 1;
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) vals[k] = shR[k];
        return true;
    }
    __shared__ double shIn[SF3D_MAX_RANKS][4];
    __shared__ double sh[4];
    __shared__ int shOk;
    __shared__ unsigned int shSilent;                /* bit p: rank p's mail did not arrive within the bound */
    const DistView* d = v.dist;
    const uint32_t e = c->epoch, par = e & 1u;
    const uint32_t tag = e + 1u;
    if (threadIdx.x == 0) { shOk = 1; shSilent = 0u; }
    __syncthreads();
    if ((int)threadIdx.x < v.world) {            /* thread p talks to rank p: the stores and the waits of all peers overlap */
        const int p = threadIdx.x;
        __threadfence_system();                  /* halo puts of the preceding kernels first */
        /* the values as tagged records: value and flag in the same words - the peer's poll that sees the tag has the value (rounds 2-5: four
         * plain stores, a second fence, a release store of a sequence number; the peer's acquire load of it, then four loads) */
        DistMail* m = &d->win[p]->mail[par][v.rank];
        for (int k = 0; k < K; ++k) { SYS_STORE(&m->w[2 * k], rec_lo(vals[k], tag)); SYS_STORE(&m->w[2 * k + 1], rec_hi(vals[k], tag)); }
        DistMail* in = &d->win[v.rank]->mail[par][p];
        bool ok = true;
        const long long t0 = wall_clock64();     /* 100 MHz */
        long long tArrived = t0;                 /* when THIS peer's mail was seen (the lanes of the wave leave the loop together: taken inside it) */
        unsigned long long w[2 * K];
        while (true) {
            bool all = true;
            for (int k = 0; k < 2 * K; ++k) w[k] = SYS_LOAD(&in->w[k]);
            for (int k = 0; k < K; ++k) all = all && rec_ok(w[2 * k], w[2 * k + 1], tag);
            if (all) { tArrived = wall_clock64(); break; }
            __builtin_amdgcn_s_sleep(1);
            if (wall_clock64() - t0 > d->spinTicks) { ok = false; tArrived = wall_clock64(); break; }      /* (10 s by default, SF3D_DIST_TIMEOUT_S) */
        }
        __threadfence_system();                  /* (acquire side: what the peers put before their mail is read after this) */
        if (ok) for (int k = 0; k < K; ++k) shIn[p][k] = rec_value(w[2 * k], w[2 * k + 1]);
        else { shOk = 0; atomicOr(&shSilent, 1u << p); }
        if (d->stats) {                          /* (one block, one thread per peer: plain read-modify-writes) */
            const unsigned long long w = (unsigned long long)(tArrived - t0);
            d->stats[1 + p] += w;
            if (w > d->stats[1 + SF3D_MAX_RANKS + p]) d->stats[1 + SF3D_MAX_RANKS + p] = w;
            if (p == v.rank) d->stats[0] += 1ull;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc[4] = {0., 0., 0., 0.};
        if (shOk)
            for (int p = 0; p < v.world; ++p) {  /* rank order: identical bits on every rank */
                double x[4] = {0., 0., 0., 0.};
                for (int k = 0; k < K; ++k) x[k] = shIn[p][k];
                dist_combine(acc, x, K, op, p == 0);
            }
        for (int k = 0; k < 4; ++k) sh[k] = acc[k];
        c->epoch = e + 1;
        if (!shOk) { c->distError = 1; c->distSilent = shSilent; c->stage = ST_FAIL; }
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) vals[k] = sh[k];
    return shOk != 0;
}

/* whole block: copy field `field` of the payload every neighbour put for epoch parity `par` into dst.
 * Eight independent system-scope loads per thread are in flight before the first store: the payload lives in
 * fine-grained memory (uncached reads, ~1-2 us each), and this runs in ONE block on the critical path of every sweep. */
__device__ __forceinline__ void dist_unpack(const DevView& v, uint32_t par, int field, double* __restrict__ dst)
{
    const DistView* d = v.dist;
    constexpr uint32_t U = 8;
    for (int p = 0; p < v.world; ++p) {
        const uint32_t cnt = d->recvCount[p];
        if (cnt == 0) continue;
        const uint32_t* idx = d->recvIdx[p];
        if (d->rccl) {             /* packed buffer filled by ncclRecv: slot 0 = the sweep iterate or K, slot 1 = waterFlow */
            const double* rb = d->recvBuf[p] + (size_t)(field == DF_FLOW ? 1 : 0) * cnt;
            for (uint32_t k = threadIdx.x; k < cnt; k += SF3D_BLOCK) dst[idx[k]] = rb[k];
            continue;
        }
        const double* src = d->payload[v.rank] + d->recvOff[p] + (size_t)(par * SF3D_DIST_FIELDS + field) * cnt;
        for (uint32_t k0 = threadIdx.x; k0 < cnt; k0 += SF3D_BLOCK * U) {
            double val[U]; uint32_t id[U];
            #pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t k = k0 + u * SF3D_BLOCK;
                if (k < cnt) { id[u] = idx[k]; val[u] = SYS_LOAD(&src[k]); }
            }
            #pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const uint32_t k = k0 + u * SF3D_BLOCK;
                if (k < cnt) dst[id[u]] = val[u];
            }
        }
    }
}

/* grid-stride: put field values of my boundary nodes into every neighbour's window */
__device__ __forceinline__ void dist_push(const DevView& v, uint32_t par, int field, const double* __restrict__ src)
{
    const DistView* d = v.dist;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int p = 0; p < v.world; ++p) {
        const uint32_t cnt = d->sendCount[p];
        if (cnt == 0) continue;
        const uint32_t* idx = d->sendIdx[p];
        if (d->rccl) {             /* pack for ncclSend */
            double* sb = d->sendBuf[p] + (size_t)(field == DF_FLOW ? 1 : 0) * cnt;
            for (uint32_t k = tid; k < cnt; k += nth) sb[k] = src[idx[k]];
            continue;
        }
        double* dst = d->payload[p] + d->sendOff[p] + (size_t)(par * SF3D_DIST_FIELDS + field) * cnt;
        for (uint32_t k = tid; k < cnt; k += nth) SYS_STORE(&dst[k], src[idx[k]]);
    }
}

/* after k_sweep: the new iterate of my boundary nodes -> neighbours (consumed by their k_decide_sweep) */
__global__ void __launch_bounds__(SF3D_BLOCK) k_push_x(DevView v)
{
    const Ctrl* c = v.ctrl;
    if (c->stage != ST_SWEEP) return;
    dist_push(v, c->epoch & 1u, 0, v.X[free_buffer(c)]);
    __threadfence_system();
}
/* after k_props: K and waterFlow of my boundary nodes -> neighbours (consumed by their k_sync_kf) */
__global__ void __launch_bounds__(SF3D_BLOCK) k_push_kf(DevView v)
{
    const Ctrl* c = v.ctrl;
    if (c->stage != ST_APPROX) return;
    dist_push(v, c->epoch & 1u, DF_K, v.K);
    dist_push(v, c->epoch & 1u, DF_FLOW, v.flow);
    __threadfence_system();
}
/* barrier + halo of K / waterFlow before the assembly reads neighbours */
__global__ void __launch_bounds__(SF3D_BLOCK) k_sync_kf(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_APPROX) return;
    const uint32_t par = c->epoch & 1u;
    __syncthreads();
    double vals[3] = {0., 0., 0.};
    if (!dist_allgather(v, c, vals, 0)) return;
    dist_unpack(v, par, DF_K, v.K);
    dist_unpack(v, par, DF_FLOW, v.flow);
}

/* SF3D_EXCHANGE=rccl: this rank's partial sums for the ncclAllGather the host queues next.  what: 0 = sum of part0[nb] (storage query), 3 = the double-double (part0, part1)[nb] (sweep norm), 1 = maximum of part0[nbSurf] (Courant), 2 = the double-doubles (part0, part1)[nb] and (part2, part3)[nb] (the two balance sums); the same reductions, in the
 * same order, as the decision kernel that follows would make for itself */
__global__ void __launch_bounds__(SF3D_BLOCK) k_local_reduce(DevView v, int what)
{
    double a = 0., b = 0., c2 = 0., d2 = 0.;
    if (what == 1) a = reduce_partials_max(v.part0, v.nbSurf);
    else if (what == 3) reduce_partials_sum_dd(v.part0, v.part1, v.nb, a, b);          /* the norm of a sweep: a double-double */
    else if (what == 2) { reduce_partials_sum_dd(v.part0, v.part1, v.nb, a, b); reduce_partials_sum_dd(v.part2, v.part3, v.nb, c2, d2); }      /* the two balance sums: double-doubles */
    else a = reduce_partials_sum(v.part0, v.nb);
    if (threadIdx.x == 0) { double* m = v.dist->mine; m[0] = a; m[1] = b; m[2] = c2; m[3] = d2; }
}

/* ---- last-block hand-off inside a launch ---------------------------------------------------
 * Every block calls this once, after a block-wide barrier that follows its last store.  Thread 0
 * publishes the block's partial results write-through (sc1), drains them and arrives on a two-level
 * agent-scope counter (16 shard counters on separate lines, then one top counter: a single counter
 * serialises ~12 ns per block).  Returns true in every thread of the ONE block that arrived last;
 * that block may then read all partials with sc1 loads (MI355X_MICROARCH.md "Valid forms": sc1 payload
 * + drain + agent atomic add, consumer = the workgroup whose add came last). */
__device__ __forceinline__ bool arrive_last(const DevView& v, double p0, double p1, bool twoValues)
{
    __shared__ int sLast;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&v.part0[blockIdx.x], p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (twoValues) __hip_atomic_store(&v.part1[blockIdx.x], p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int shard = blockIdx.x & 15u;
        const unsigned int inShard = (gridDim.x + 15u - shard) >> 4;
        const unsigned int shards = gridDim.x < 16u ? gridDim.x : 16u;
        int last = 0;
        if (__hip_atomic_fetch_add(&v.arrive[16u * (shard + 1u)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == inShard - 1u) {
            __hip_atomic_store(&v.arrive[16u * (shard + 1u)], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = __hip_atomic_fetch_add(&v.arrive[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u;
            if (last) __hip_atomic_store(&v.arrive[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        sLast = last;
    }
    __syncthreads();
    return sLast != 0;
}
/* the same with four published values per block (both norms of a paired pass as double-doubles: part0/1 and part2/3) */
__device__ __forceinline__ bool arrive_last4(const DevView& v, double p0, double p1, double p2, double p3)
{
    if (threadIdx.x == 0) {
        __hip_atomic_store(&v.part2[blockIdx.x], p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&v.part3[blockIdx.x], p3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return arrive_last(v, p0, p1, true);          /* (thread 0 publishes the other two, drains all four and arrives) */
}
/* last block only: the published double-double partials (ph, pl)[nb] -> one double-double, in every thread of the first 256 */
__device__ __forceinline__ void sum_published_dd(const double* ph, const double* pl, uint32_t nb, double& hi, double& lo)
{
    hi = 0.; lo = 0.;
    if (threadIdx.x < SF3D_BLOCK)
        for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK)
            dd_merge(hi, lo, __hip_atomic_load(&ph[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(&pl[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
/* last block only: fixed-order sum of the published partials (same order as reduce_partials_sum) */
__device__ __forceinline__ double sum_published(const double* p, uint32_t nb)
{
    double s = 0.;
    for (uint32_t k = threadIdx.x; k < nb; k += SF3D_BLOCK) s += __hip_atomic_load(&p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return block_sum(s);
}

/* A wave puts the values its chunk owes to neighbouring ranks (multi-GPU, in-kernel halo put).
 * All 64 lanes must call it; `val` is the lane's freshly computed value. */
__device__ __forceinline__ void dist_put_chunk(const DevView& v, uint32_t q, uint32_t lane, uint32_t par, int field, double val)
{
    const DistView* d = v.dist;
    const uint32_t b0 = d->bndStart[q], b1 = d->bndStart[q + 1];           /* wave-uniform */
    for (uint32_t base = b0; base < b1; base += 64) {
        const uint32_t t = base + lane;
        const bool on = t < b1;
        const double x = __shfl(val, on ? (int)d->bndLane[t] : 0, 64);
        if (on) {
            const uint32_t p = d->bndPeer[t];
            double* dst = d->payload[p] + d->sendOff[p] + (size_t)(par * SF3D_DIST_FIELDS + field) * d->sendCount[p] + d->bndSlot[t];
            SYS_STORE(dst, x);
        }
    }
}

/* K and waterFlow of the chunk's boundary nodes as tagged records (fields DF_KLO .. DF_FHI, tag = exchange epoch + 1): one walk through the
 * chunk's list, four stores per entry.  The reader's k_halo_copy<0> waits for the tags - no barrier between the ranks for them */
__device__ __forceinline__ void dist_put_chunk_kf(const DevView& v, uint32_t q, uint32_t lane, uint32_t par, uint32_t tag, double K, double fl)
{
    const DistView* d = v.dist;
    const uint32_t b0 = d->bndStart[q], b1 = d->bndStart[q + 1];           /* wave-uniform */
    for (uint32_t base = b0; base < b1; base += 64) {
        const uint32_t t = base + lane;
        const bool on = t < b1;
        const int src = on ? (int)d->bndLane[t] : 0;
        const double k = __shfl(K, src, 64), f = __shfl(fl, src, 64);
        if (on) {
            const uint32_t p = d->bndPeer[t];
            const size_t cnt = d->sendCount[p];
            double* dst = d->payload[p] + d->sendOff[p] + (size_t)(par * SF3D_DIST_FIELDS) * cnt + d->bndSlot[t];
            SYS_STORE(dst + (size_t)DF_KLO * cnt, __longlong_as_double((long long)rec_lo(k, tag)));
            SYS_STORE(dst + (size_t)DF_KHI * cnt, __longlong_as_double((long long)rec_hi(k, tag)));
            SYS_STORE(dst + (size_t)DF_FLO * cnt, __longlong_as_double((long long)rec_lo(f, tag)));
            SYS_STORE(dst + (size_t)DF_FHI * cnt, __longlong_as_double((long long)rec_hi(f, tag)));
        }
    }
}

/* the same for ONE node (kernels whose lanes are not a chunk: the masked paired sweep): the node's entries are found in its chunk's list */
__device__ __forceinline__ void dist_put_node(const DevView& v, uint32_t i, uint32_t par, int field, double val)
{
    const DistView* d = v.dist;
    const uint32_t q = i >> 6, lane = i & 63u;
    for (uint32_t t = d->bndStart[q], t1 = d->bndStart[q + 1]; t < t1; ++t)
        if (d->bndLane[t] == lane) {
            const uint32_t p = d->bndPeer[t];
            SYS_STORE(d->payload[p] + d->sendOff[p] + (size_t)(par * SF3D_DIST_FIELDS + field) * d->sendCount[p] + d->bndSlot[t], val);
        }
}

/* ======================================================================================= */
/* control kernels (one thread / one block)                                                 */
/* ======================================================================================= */

/* waterMainLoop body head, cpusolver.cpp:155-162 (Hold = H is an index copy) */
__device__ __forceinline__ void begin_attempt(Ctrl* c)
{
    c->dt = dmin(c->dtCurr, c->maxTimeStep);
    c->hold = c->cur;
    c->best = -1;
    c->bestMBR = NODATA_D;
    c->approx = 0;
    c->counters[0]++;
    c->stage = ST_APPROX;
}

__global__ void k_step_begin(Ctrl* c, double maxTimeStep)
{
    c->maxTimeStep = maxTimeStep;
    c->seqCount = 0;
    {   /* the next slot of the ring: the matrices of the steps accepted before stay intact until their link flow sums are added (k_links_flush) */
        const uint32_t ring = c->aRing < 2u ? 2u : (c->aRing > (uint32_t)SF3D_LINKS_RING ? (uint32_t)SF3D_LINKS_RING : c->aRing);
        const uint32_t nx = c->aBuf + 1u;
        c->aBuf = nx < ring ? nx : 0u;
    }
    begin_attempt(c);
}

/* a refused attempt restores H = Hold (cpusolver.cpp:182-186) and the loop starts the next one */
__device__ __forceinline__ void reject_attempt(Ctrl* c)
{
    c->seSource = 2;                   /* the next attempt starts from Hold again: its Se is what approximation 0 stored in SeHold */
    c->cur = c->hold;
    begin_attempt(c);
}

#ifndef SF3D_PROBE_BUDGET
#define SF3D_PROBE_BUDGET 8u     /* approximations the early Courant check stays on for after a refusal (Ctrl::probeBudget) */
#endif
/* checkCourant, cpusolver.cpp:248-281, then the iteration budget of solver.h:55-59 (one thread) */
__device__ __forceinline__ void courant_decision(Ctrl* c, double cmax)
{
    c->counters[2]++;
    c->courant = cmax;
    c->asmSeq++; c->asmSurfOnly = (cmax < 1.01 || c->dt <= c->dtMin) ? 0u : 1u;
    if (cmax < 1.01 || c->dt <= c->dtMin) {
        uint32_t budget = (uint32_t)((c->approx + 1) * ((float)c->maxIter / (float)c->maxApprox));
        c->iterBudget = budget > 25u ? budget : 25u;
        c->iter = 0;
        c->bestNorm = 1.;
        c->linearValid = 1;
        c->stage = ST_SWEEP;
        return;
    }
    double d = c->dtCurr / cmax;
    int mult = 0;
    while (d < 1.) { d *= 10.; ++mult; }
    d = floor(d);
    for (int k = 0; k < mult; ++k) d /= 10.;
    c->dtCurr = dmax(c->dtMin, d);
    c->counters[4]++;
    c->probeBudget = SF3D_PROBE_BUDGET;
    if (c->seqCount < 16u) c->seqSweeps[c->seqCount] = 0;
    c->seqCount++;
    reject_attempt(c);
}
__global__ void __launch_bounds__(SF3D_BLOCK) k_decide_courant(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_APPROX) return;
    double vals[3] = {reduce_partials_max(v.part0, v.nbSurf), 0., 0.};
    if (!dist_allgather(v, c, vals, 1)) return;
    if (threadIdx.x == 0) courant_decision(c, vals[0]);
}

/* the rule of solveLinearSystem's loop (cpusolver.cpp:672-703) on the four scalars it reads and writes: true when the loop ends, `valid`
 * false when it ends because the norm grew tenfold.  A function of its own so that the resident sweep loop (sf3d_resident.inc), where
 * every thread follows the loop with a private copy of these scalars, applies the text the control block's decision applies. */
struct SweepRule { double tol, bestNorm; uint32_t iter, budget; };
__device__ __forceinline__ bool sweep_rule(SweepRule& r, double norm, bool& valid)
{
    r.iter++;
    valid = true;
    if (norm < r.tol) return true;
    if (norm > (r.bestNorm * 10)) { valid = false; return true; }
    if (norm < r.bestNorm) r.bestNorm = norm;
    return r.iter >= r.budget;
}
/* solveLinearSystem loop control, cpusolver.cpp:672-703 + :442-447 (one thread) */
__device__ __forceinline__ void sweep_decision(Ctrl* c, int nxt, double norm)
{
    c->cur = nxt;                     /* std::swap(vectorNewX, vectorX), water.cpp:598 */
    c->counters[3]++;
    c->lastNorm = norm;
    SweepRule r{c->residualTolerance, c->bestNorm, c->iter, c->iterBudget};
    bool valid = true;
    const bool done = sweep_rule(r, norm, valid);
    c->iter = r.iter; c->bestNorm = r.bestNorm;
    if (!done) return;
    if (c->seqCount < 16u) c->seqSweeps[c->seqCount] = c->iter;
    c->seqCount++;
    c->linearValid = valid ? 1 : 0;
    if (!valid) c->counters[5]++;
    if (!valid && c->dt > c->dtMin) {
        c->dtCurr = dmax(c->dtMin, c->dtCurr / 2.);
        reject_attempt(c);
    } else
        c->stage = ST_POST;
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_decide_sweep(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_SWEEP) return;
    const int nxt = free_buffer(c);              /* the buffer k_sweep wrote */
    const uint32_t par = c->epoch & 1u;
    double vals[3] = {0., 0., 0.};
    reduce_partials_sum_dd(v.part0, v.part1, v.nb, vals[0], vals[1]);
    if (!dist_allgather(v, c, vals, 2)) return;
    if (v.world > 1) dist_unpack(v, par, 0, v.X[nxt]);     /* neighbours' new iterate on my halo */
    if (threadIdx.x != 0) return;
    sweep_decision(c, nxt, (vals[0] + vals[1]) / v.Nnorm);
}

/* computeCurrentMassBalance, water.cpp:96-123 */
__device__ __forceinline__ void mass_balance(Ctrl* c, double storage, double sink)
{
    BalanceDev b;
    b.storage = storage;
    const double dS = b.storage - c->prevStep.storage;
    b.sinkSource = sink;
    b.MBE = dS - b.sinkSource;
    const double timePct = 0.001 * dmax(c->dt, 30.0) / 3600.;
    double minRef = b.storage * timePct;
    minRef = dmax(minRef, 0.001);
    const double ref = dmax(fabs(b.sinkSource), minRef);
    b.MBR = b.MBE / ref;
    c->curStep = b;
}
/* scalar part of acceptStep, water.cpp:233-237 */
__device__ __forceinline__ void accept_bookkeeping(Ctrl* c)
{
    c->prevStep.storage = c->curStep.storage;
    c->prevStep.sinkSource = c->curStep.sinkSource;
    c->curPeriod.sinkSource += c->curStep.sinkSource;
    c->counters[1]++;
    c->acceptDt = c->dt; c->acceptBuf = c->cur; c->acceptABuf = c->aBuf;
    c->seSource = 1;                   /* Se = Se(H accepted): k_post, or k_restore for a restored best step */
    c->stage = ST_ACCEPT;              /* k_accept (flow sums) is the last kernel of the step */
}
__device__ __forceinline__ void halve_and_reject(Ctrl* c)
{
    c->dtCurr = dmax(c->dtCurr * 0.5, c->dtMin);
    reject_attempt(c);
}

/* evaluateWaterBalance, water.cpp:165-227 (one thread) */
__device__ __forceinline__ void balance_decision(Ctrl* c, double storage, double sink)
{
    c->counters[7]++;
    mass_balance(c, storage, sink);
    const double err = fabs(c->curStep.MBR);
    const uint32_t approx = c->approx;
    if (isnan(err)) {
        if (c->dt > c->dtMin) halve_and_reject(c);
        else if (approx > 0) { c->cur = c->best; c->stage = ST_RESTORE; }
        else c->stage = ST_FAIL;
        return;
    }
    if (err < c->MBRThreshold) {
        accept_bookkeeping(c);
        if (approx < 3 && err < c->MBRThreshold * 0.1 && c->courant < c->courantThreshold)
            c->dtCurr = dmin(c->dtMax, c->dtCurr * 2);
        return;
    }
    if (approx == 0 || err < c->bestMBR) { c->best = c->cur; c->bestMBR = err; }   /* keep-best = index copy */
    if (err > (c->bestMBR * c->instabilityFactor) || approx == (c->maxApprox - 1)) {
        if (c->dt > c->dtMin) { halve_and_reject(c); return; }
        c->cur = c->best;                                                          /* restoreBestStep: H = Hbest */
        c->stage = ST_RESTORE;
        return;
    }
    c->approx = approx + 1;
    c->stage = ST_APPROX;
}
__global__ void __launch_bounds__(SF3D_BLOCK) k_decide_balance(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_POST) return;
    double vals[4];
    reduce_partials_sum_dd(v.part0, v.part1, v.nb, vals[0], vals[1]);
    reduce_partials_sum_dd(v.part2, v.part3, v.nb, vals[2], vals[3]);
    if (!dist_allgather(v, c, vals, 3)) return;
    if (threadIdx.x == 0) balance_decision(c, vals[0] + vals[1], vals[2] + vals[3]);
}

/* tail of restoreBestStep (water.cpp:266) followed by acceptStep (one thread) */
__device__ __forceinline__ void restore_decision(Ctrl* c, double storage, double sink)
{
    c->counters[6]++;
    mass_balance(c, storage, sink);
    accept_bookkeeping(c);
}
__global__ void __launch_bounds__(SF3D_BLOCK) k_decide_restore(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_RESTORE) return;
    double vals[4];
    reduce_partials_sum_dd(v.part0, v.part1, v.nb, vals[0], vals[1]);
    reduce_partials_sum_dd(v.part2, v.part3, v.nb, vals[2], vals[3]);
    if (!dist_allgather(v, c, vals, 3)) return;
    if (threadIdx.x == 0) restore_decision(c, vals[0] + vals[1], vals[2] + vals[3]);
}

__global__ void __launch_bounds__(SF3D_BLOCK) k_decide_query(DevView v)
{
    double vals[3] = {reduce_partials_sum(v.part0, v.nb), 0., 0.};
    if (!dist_allgather(v, v.ctrl, vals, 0)) return;
    if (threadIdx.x == 0) v.ctrl->query[0] = vals[0];
}

