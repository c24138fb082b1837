/* part of sf3d_solver.hip (included there just before sf3d_host_build.inc) - host side, part 0: the graph analysis of the device build as
 * plain functions over HostModel, and at its end the decisions of one computeStep as plain functions over scalars (plan_step).  No HIP call,
 * no solver object, no environment: this file also compiles with a plain C++ compiler after sf3d_model.h (tests/plan_host.cpp holds every
 * stage's claims against the link data, and the step's plan to the rules between its flags).  What a stage reads from the environment or
 * from the device arrives as an argument; sync_to_device (sf3d_host_build.inc) calls the stages in the order they stand here. */
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

template <class F> void parallel_for(uint32_t n, F f)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (nt > 16) nt = 16;
    if (n < 65536 || nt == 1) { f(0u, n); return; }
    std::vector<std::thread> th;
    const uint32_t chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        const uint32_t a = t * chunk, b = (a + chunk < n) ? a + chunk : n;
        if (a >= b) break;
        th.emplace_back([=] { f(a, b); });
    }
    for (auto& t : th) t.join();
}

}  // namespace

/* ---- row-strip partition (host logic; also used by CPU tests through sf3d_dist_owner/halo) ----
 * Strip-local build: a rank may stage only the nodes its strip touches - the columns it owns (sf3d_dist_bounds says which surface
 * nodes those are) and the one-cell ring of columns around them, each column whole.  A node that never received its soil / surface
 * class is ABSENT (owner SF3D_OWNER_NONE): it joins no list, and a link to it from a node of another rank's halo is ignored.  What
 * must not happen is a link from one of THIS rank's nodes to an absent node - the caller forgot a halo column (or a class): that is
 * SF3D_MISSING_DATA_ERROR here instead of a wrong answer later.  With every node staged (the global build) nothing changes. */
sf3d_error_t sf3d_partition_bounds(uint32_t ns, int world, uint32_t* bounds)
{
    if (world < 1 || world > SF3D_MAX_RANKS || !bounds) return SF3D_PARAMETER_ERROR;
    for (int r = 0; r <= world; ++r) {
        uint64_t b = (uint64_t)ns * r / world;
        if (r > 0 && r < world) b = (b / SF3D_CHUNK) * SF3D_CHUNK;      /* cut at chunk boundaries */
        bounds[r] = (uint32_t)b;
    }
    bounds[world] = ns;
    for (int r = 1; r <= world; ++r) if (bounds[r] < bounds[r - 1]) bounds[r] = bounds[r - 1];
    return SF3D_OK;
}
sf3d_error_t sf3d_compute_partition(const HostModel& m, int rank, int world, Partition& out)
{
    const uint32_t N = m.N, ns = m.ns;
    if (world < 1 || world > SF3D_MAX_RANKS || rank < 0 || rank >= world) return SF3D_PARAMETER_ERROR;
    out.world = world; out.rank = rank;
    out.owner.assign(N, 0);
    out.bounds.assign(world + 1, 0);
    out.send.assign(world, {}); out.recv.assign(world, {});
    out.missingFrom = out.missingTo = UINT32_MAX;
    sf3d_partition_bounds(ns, world, out.bounds.data());
    if (world == 1) return SF3D_OK;
    auto present = [&](uint32_t i) { return m.hasClass[i] != 0; };
    /* column id = surface ancestor through Up links (layer-major numbering: one pass suffices) */
    std::vector<uint32_t> col(N, UINT32_MAX);
    for (uint32_t i = 0; i < ns && i < N; ++i) col[i] = i;
    for (int pass = 0; pass < 64; ++pass) {
        bool changed = false, missing = false;
        for (uint32_t i = ns; i < N; ++i) {
            if (col[i] != UINT32_MAX || !present(i)) continue;
            if (m.ltype[0][i] == SF3D_LINK_NONE) { col[i] = 0; changed = true; continue; }   /* orphan: rank 0 */
            const uint32_t up = m.lto[0][i];
            if (col[up] != UINT32_MAX) { col[i] = col[up]; changed = true; } else missing = true;
        }
        if (!missing || !changed) break;
    }
    for (uint32_t i = 0; i < N; ++i) {
        if (!present(i)) { out.owner[i] = SF3D_OWNER_NONE; continue; }
        const uint32_t cidx = col[i] == UINT32_MAX ? 0u : col[i];
        int r = 0;
        while (r + 1 < world && cidx >= out.bounds[r + 1]) ++r;
        out.owner[i] = (uint8_t)r;
    }
    for (int s = 0; s < SF3D_SLOTS; ++s)
        for (uint32_t i = 0; i < N; ++i) {
            if (m.ltype[s][i] == SF3D_LINK_NONE || out.owner[i] == SF3D_OWNER_NONE) continue;
            if (s >= 2 && s - 2 >= m.nLat[i]) continue;
            const uint32_t j = m.lto[s][i];
            const int a = out.owner[i], b = out.owner[j];
            if (b == SF3D_OWNER_NONE) {          /* a link into what was never staged: harmless from another rank's halo node, an error from one of mine */
                if (a == rank && out.missingFrom == UINT32_MAX) { out.missingFrom = i; out.missingTo = j; }
                continue;
            }
            if (a == b) continue;
            if (a == rank) out.recv[b].push_back(j);       /* my row i reads node j of rank b */
            if (b == rank) out.send[a].push_back(j);       /* rank a's row i reads my node j   */
        }
    for (int r = 0; r < world; ++r) {
        for (auto* v : {&out.send[r], &out.recv[r]}) {
            std::sort(v->begin(), v->end());
            v->erase(std::unique(v->begin(), v->end()), v->end());
        }
    }
    return out.missingFrom == UINT32_MAX ? SF3D_OK : SF3D_MISSING_DATA_ERROR;
}

/* ---- what the stages hand on ---- */
struct LinkTables {                     /* [10][N] in device slots: link kind (LK_*), link distance, interface area, neighbour */
    std::vector<uint8_t> kind;
    std::vector<double> dist, area;
    std::vector<uint32_t> to;
};
struct GridPlan {                       /* the graph as an NX x NY x NZ grid (paired sweep, resident loop); node empty: it is none */
    std::vector<uint64_t> node, chunk;  /* per node: one nibble per slot naming the neighbour; per chunk: that code | bit 63 where all 64 agree */
    std::vector<int32_t> idxMap;        /* non-empty: the graph is a layered masked grid, not a full box: [NZ][NY][NX] node or -1 */
    uint32_t NX = 0, NY = 0, NZ = 0;
    uint32_t ownLo = 0, ownHi = 0;      /* the rows of this rank's strip (plan_strip_rows) */
};
struct ChunkLists {
    std::vector<uint32_t> listSurf;     /* the rank's chunks: surface then soil, in each part the chunks that owe values to a neighbouring rank first */
    uint32_t nListSurf = 0, nList = 0, ownedNodes = 0;
    std::vector<uint32_t> propsNeed;    /* [nChunks] one GPU: the rows of chunks [0, q] read node properties of chunks [0, propsNeed[q]) */
};
struct PairPlan {                       /* patch height of the paired pass (0: single sweeps) and, on masked grids, the patches of every W */
    uint32_t bestW = 0;
    std::vector<uint32_t> plist[4]; std::vector<uint8_t> pdepth[4];
};
struct EdgeRows { int32_t edgePeer[2] = {-1, -1}; uint32_t edgePut[2] = {0u, 0u}, edgeGet[2] = {0u, 0u}; };
inline int pair_widx(uint32_t W) { return W == 6 ? 0 : (W == 8 ? 1 : (W == 10 ? 2 : 3)); }

/* Slot alignment.  setNodeLink puts a node's k-th lateral link into slot 2 + k, so a node at the edge of a grid (fewer
 * laterals) holds OTHER directions in its slots than its 63 chunk mates and the whole chunk falls back to per-lane link
 * kinds and indices (two dependent round trips per group of links in the assembly instead of one: a quarter of the soil
 * chunks of a 512-wide grid).  On the device such a node's laterals sit in the slots where the chunk's fullest node has the
 * same neighbour offset and link kind, in the same relative order - the sums of a row are taken over the existing links in
 * slot order, so every result keeps its bits.  Nodes that do not fit the pattern keep their own order.
 * Returns the device slot of every (host slot, node); empty: the identity (nothing moved, or `align` is off). */
inline std::vector<uint8_t> plan_slot_alignment(const HostModel& m, bool align)
{
    const uint32_t N = m.N, ns = m.ns;
    const size_t NS = (size_t)N * SF3D_SLOTS;
    std::vector<uint8_t> dslot;
    if (align) {
        std::vector<uint8_t> ds(NS);
        for (int sl = 0; sl < SF3D_SLOTS; ++sl) std::memset(ds.data() + (size_t)sl * N, sl, N);
        std::atomic<bool> moved{false};
        const uint32_t nq = (N + SF3D_CHUNK - 1) / SF3D_CHUNK;
        auto lateral_kind = [&](uint32_t i, int sl) -> int {      /* 0: no lateral link in host slot sl */
            if (sl - 2 >= m.nLat[i] || m.ltype[sl][i] == SF3D_LINK_NONE) return 0;
            const bool si = i >= ns, sj = m.lto[sl][i] >= ns;
            return (si && sj) ? 1 + (m.ltype[sl][i] == SF3D_LINK_LATERAL ? 0 : 1) : ((!si && !sj) ? 3 : 4);
        };
        parallel_for(nq, [&](uint32_t qa, uint32_t qb) {
            for (uint32_t q = qa; q < qb; ++q) {
                const uint32_t i0 = q * SF3D_CHUNK, i1 = (i0 + SF3D_CHUNK < N) ? i0 + SF3D_CHUNK : N;
                /* the pattern: the node with the most laterals, if they fill its slots 2 .. 2 + n - 1 */
                uint32_t tmpl = i0; int tn = -1;
                for (uint32_t i = i0; i < i1; ++i) {
                    int n = 0; bool dense = true;
                    for (int sl = 2; sl < SF3D_SLOTS; ++sl) { const bool on = lateral_kind(i, sl) != 0; if (on) { if (sl - 2 != n) dense = false; ++n; } }
                    if (dense && n > tn) { tn = n; tmpl = i; }
                }
                if (tn <= 0) continue;
                int64_t td[SF3D_SLOTS]; int tk[SF3D_SLOTS];
                for (int p = 0; p < tn; ++p) { td[p] = (int64_t)m.lto[2 + p][tmpl] - (int64_t)tmpl; tk[p] = lateral_kind(tmpl, 2 + p); }
                for (uint32_t i = i0; i < i1; ++i) {
                    if (i == tmpl) continue;
                    uint8_t map[SF3D_SLOTS]; bool fits = true, differs = false; int p = 0;
                    for (int sl = 2; sl < SF3D_SLOTS && fits; ++sl) {
                        const int kk = lateral_kind(i, sl);
                        map[sl] = (uint8_t)sl;
                        if (!kk) continue;
                        const int64_t dd = (int64_t)m.lto[sl][i] - (int64_t)i;
                        while (p < tn && !(td[p] == dd && tk[p] == kk)) ++p;
                        if (p >= tn) { fits = false; break; }
                        map[sl] = (uint8_t)(2 + p); if (map[sl] != sl) differs = true;
                        ++p;
                    }
                    if (!fits || !differs) continue;
                    /* host slots without a link take the device slots that are left, so that the map stays a permutation */
                    bool used[SF3D_SLOTS] = {false};
                    for (int sl = 2; sl < SF3D_SLOTS; ++sl) if (lateral_kind(i, sl)) used[map[sl]] = true;
                    int free_ = 2;
                    for (int sl = 2; sl < SF3D_SLOTS; ++sl) {
                        if (lateral_kind(i, sl)) continue;
                        while (used[free_]) ++free_;
                        map[sl] = (uint8_t)free_; used[free_] = true;
                    }
                    for (int sl = 2; sl < SF3D_SLOTS; ++sl) ds[(size_t)sl * N + i] = map[sl];
                    moved = true;
                }
            }
        });
        if (moved) dslot.swap(ds);
    }
    return dslot;
}

/* derived static graph data: link kind and link distance (host, libm - exactly the
 * reference's nodeDistance2D/3D arithmetic, soilPhysics.cpp:328-338).  dslotv: plan_slot_alignment's result; rank: the rank whose
 * rows this device computes.  The one refusal leaves its text in err. */
inline sf3d_error_t plan_link_tables(const HostModel& m, const std::vector<uint8_t>& dslotv, int rank, LinkTables& t, char* err, size_t errLen)
{
    const uint32_t N = m.N, ns = m.ns;
    const size_t NS = (size_t)N * SF3D_SLOTS;
    std::vector<uint8_t> kind(NS, LK_NONE);
    std::vector<double> dist(NS, 0.), area(NS, 0.);
    std::vector<uint32_t> to(NS, 0u);
    std::atomic<bool> bad{false};
    const uint8_t* dslot = dslotv.empty() ? nullptr : dslotv.data();
    parallel_for(N, [&](uint32_t a, uint32_t b) {
        for (uint32_t i = a; i < b; ++i) {
            const int nl = m.nLat[i];
            for (int s = 0; s < SF3D_SLOTS; ++s) {
                if (s >= 2 && s - 2 >= nl) continue;            /* lateral loop bound, cpusolver.cpp:360 */
                if (m.ltype[s][i] == SF3D_LINK_NONE) continue;
                const uint32_t j = m.lto[s][i];
                const size_t e = (size_t)(dslot ? dslot[(size_t)s * N + i] : s) * N + i;
                to[e] = j; area[e] = m.larea[s][i];
                const bool si = i >= ns, sj = j >= ns;
                if (si && sj) {
                    if (m.ltype[s][i] == SF3D_LINK_LATERAL) {
                        kind[e] = LK_SOIL_LAT;
                        const double dx = m.x[i] - m.x[j], dy = m.y[i] - m.y[j], dz = m.z[i] - m.z[j];
                        double nrm = 0; nrm += dx * dx; nrm += dy * dy; nrm += dz * dz;
                        dist[e] = std::sqrt(nrm);
                    } else { kind[e] = LK_SOIL_VERT; dist[e] = std::fabs(m.z[i] - m.z[j]); }
                } else if (!si && !sj) {
                    kind[e] = LK_RUNOFF;
                    const double dx = m.x[i] - m.x[j], dy = m.y[i] - m.y[j];
                    double nrm = 0; nrm += dx * dx; nrm += dy * dy;
                    dist[e] = std::sqrt(nrm);
                } else {
                    kind[e] = LK_INFILTRATION;
                    const uint32_t su = sj ? i : j, so = sj ? j : i;
                    dist[e] = m.z[su] - m.z[so];
                }
            }
            if (m.btype[i] == SF3D_BND_FREE_DRAINAGE && m.ltype[0][i] == SF3D_LINK_NONE
                && (m.presetPartition == nullptr || m.presetPartition->owner[i] == rank)) bad = true;   /* assert water.cpp:682 (a strip-local model's halo nodes may have lost the link: their rows and boundaries are the neighbour's) */
        }
    });
    if (bad) { snprintf(err, errLen, "FreeDrainage node without an Up link"); return SF3D_BOUNDARY_ERROR; }
    t.kind.swap(kind); t.dist.swap(dist); t.area.swap(area); t.to.swap(to);
    return SF3D_OK;
}

/* per (64-node chunk, slot) descriptors: uniform kind + uniform index offset => the kernels
 * never read lto/lkind for that chunk and slot */
inline std::vector<ChunkDesc> plan_chunk_descriptors(const LinkTables& t, uint32_t N, uint32_t ns)
{
    const std::vector<uint8_t>& kind = t.kind; const std::vector<double>&dist = t.dist, &area = t.area; const std::vector<uint32_t>& to = t.to;
    const uint32_t nChunks = (N + SF3D_CHUNK - 1) / SF3D_CHUNK;
    std::vector<ChunkDesc> cdesc(nChunks);
    parallel_for(nChunks, [&](uint32_t qa, uint32_t qb) {
        for (uint32_t q = qa; q < qb; ++q) {
            const uint32_t i0 = q * SF3D_CHUNK, i1 = (i0 + SF3D_CHUNK < N) ? i0 + SF3D_CHUNK : N;
            ChunkDesc d;
            std::memset(&d, 0, sizeof(d));
            d.rowType = (i1 <= ns) ? 0 : (i0 >= ns ? 1 : 2);
            for (int s = 0; s < SF3D_SLOTS; ++s) {
                bool any = false, all = true, same = true, sameDelta = true;
                uint8_t k0 = LK_NONE; int64_t d0 = 0;
                for (uint32_t i = i0; i < i1; ++i) {
                    const size_t e = (size_t)s * N + i;
                    if (kind[e] == LK_NONE) { all = false; continue; }
                    const int64_t dd = (int64_t)to[e] - (int64_t)i;
                    if (!any) { any = true; k0 = kind[e]; d0 = dd; }
                    else { if (kind[e] != k0 || dd != d0) same = false; if (dd != d0) sameDelta = false; }
                }
                const bool fits = d0 >= INT32_MIN && d0 <= INT32_MAX;
                uint8_t ck = CK_NONE;
                if (any) ck = (all && same && fits) ? k0 : (uint8_t)CK_MIXED;
                d.kind[s] = ck;
                d.ukind[s] = any ? ((same && fits) ? k0 : (uint8_t)CK_MIXED) : (uint8_t)CK_NONE;
                d.delta[s] = (ck != CK_NONE && ck != CK_MIXED) ? (int32_t)d0 : 0;
                if (ck == CK_MIXED && sameDelta && fits) { d.delta[s] = (int32_t)d0; d.sweepUniform |= (uint16_t)(1u << s); }
                if (any) {                                   /* one interface area for the whole chunk? */
                    bool first = true, uni = true; double a0 = 0.;
                    for (uint32_t i = i0; i < i1 && uni; ++i) {
                        const size_t e = (size_t)s * N + i;
                        if (kind[e] == LK_NONE) continue;
                        if (first) { a0 = area[e]; first = false; }
                        else if (area[e] != a0) uni = false;
                    }
                    if (uni) { d.areaUniform |= (uint16_t)(1u << s); d.area[s] = a0; }
                    first = true; uni = true; double d0v = 0.;
                    for (uint32_t i = i0; i < i1 && uni; ++i) {
                        const size_t e = (size_t)s * N + i;
                        if (kind[e] == LK_NONE) continue;
                        if (first) { d0v = dist[e]; first = false; }
                        else if (dist[e] != d0v) uni = false;
                    }
                    if (uni) { d.distUniform |= (uint16_t)(1u << s); d.dist[s] = d0v; }
                }
            }
            {   /* scalar-geometry path of k_assemble: full 64-node soil chunk, every slot empty or uniform soil-soil */
                bool su = d.rowType == 1 && i1 - i0 == SF3D_CHUNK, partial = false;
                for (int s = 0; s < SF3D_SLOTS && su; ++s) {
                    if (d.kind[s] == CK_NONE) continue;
                    if (d.kind[s] == CK_MIXED) partial = true;      /* same kind and offset wherever the link exists (ukind, sweepUniform), some nodes without it */
                    su = (d.ukind[s] == LK_SOIL_VERT || d.ukind[s] == LK_SOIL_LAT) && (d.kind[s] != CK_MIXED || ((d.sweepUniform >> s) & 1u))
                         && ((d.areaUniform >> s) & 1u) && ((d.distUniform >> s) & 1u);
                }
                d.soilUniform = su ? (partial ? 2 : 1) : 0;
            }
            cdesc[q] = d;
        }
    });
    return cdesc;
}

/* paired sweep (k_sweep_pair): is the graph a regular NX x NY x NZ grid in layer-major numbering, and which neighbour
 * does every link slot of every node name?  (host logic; the same structure sf3d_get_regular_grid reports)
 * sf3d_get_regular_grid (sf3d_api.cpp) is a second, older recogniser with other thresholds: it is left as it is.
 * Returns whether it is; if not, g describes nothing. */
inline bool plan_regular_box(const LinkTables& t, const HostModel& m, GridPlan& g)
{
    const std::vector<uint8_t>& kind = t.kind; const std::vector<uint32_t>& to = t.to;
    std::vector<uint64_t>&pairNode = g.node, &pairChunk = g.chunk;
    uint32_t &pairNX = g.NX, &pairNY = g.NY, &pairNZ = g.NZ;
    const uint32_t N = m.N, ns = m.ns, nChunks = (N + SF3D_CHUNK - 1) / SF3D_CHUNK;
    bool regular = ns >= 64 && N % ns == 0 && N / ns >= 2 && N < (1u << 28);   /* 32-bit byte offsets in the kernel */
    int64_t maxOff = 0;
    if (regular) {
        for (int sl = 2; sl < SF3D_SLOTS && regular; ++sl)
            for (uint32_t i = 0; i < N; ++i) {
                const size_t e = (size_t)sl * N + i;
                if (kind[e] == LK_NONE) continue;
                const int64_t o = std::llabs((int64_t)to[e] - (int64_t)i);
                if (o > maxOff) maxOff = o;
            }
        const int64_t NX = maxOff - 1;
        regular = NX >= 64 && NX % 64 == 0 && ns % (uint64_t)NX == 0 && ns / (uint64_t)NX >= 6;
        if (regular) { pairNX = (uint32_t)NX; pairNY = (uint32_t)(ns / (uint64_t)NX); pairNZ = N / ns; }
    }
    if (regular) {
        pairNode.assign(N, 0);
        std::atomic<bool> irregular{false};
        const int64_t NX = pairNX, NY = pairNY;
        parallel_for(N, [&](uint32_t a, uint32_t b) {
            for (uint32_t i = a; i < b && !irregular.load(std::memory_order_relaxed); ++i) {
                const int64_t l = i / ns, r = (i % ns) / NX, cidx = i % NX;
                uint64_t code = 0; unsigned seen = 0;
                for (int sl = 0; sl < SF3D_SLOTS; ++sl) {
                    const size_t e = (size_t)sl * N + i;
                    uint64_t nib = SF3D_PAIR_NONE;
                    if (kind[e] != LK_NONE) {
                        const int64_t off = (int64_t)to[e] - (int64_t)i;
                        if (sl == 0) { if (off != -(int64_t)ns) irregular = true; nib = SF3D_PAIR_UP; }
                        else if (sl == 1) { if (off != (int64_t)ns) irregular = true; nib = SF3D_PAIR_DOWN; }
                        else {
                            const int64_t rr = (off >= 0) ? (off + NX / 2) / NX : -((-off + NX / 2) / NX), cc = off - rr * NX;
                            if (rr < -1 || rr > 1 || cc < -1 || cc > 1 || (rr == 0 && cc == 0) || r + rr < 0 || r + rr >= NY || cidx + cc < 0 || cidx + cc >= NX
                                || (int64_t)(to[e] / ns) != l) { irregular = true; break; }
                            nib = (uint64_t)((rr + 1) * 3 + (cc + 1));
                            if (seen & (1u << nib)) irregular = true;      /* two links to one neighbour */
                            seen |= 1u << nib;
                        }
                    }
                    code |= nib << (4 * sl);
                }
                pairNode[i] = code;
            }
        });
        regular = !irregular;
    }
    if (regular) {
        pairChunk.assign(nChunks, 0);
        for (uint32_t q = 0; q < nChunks; ++q) {
            bool same = (size_t)(q + 1) * SF3D_CHUNK <= N;
            for (uint32_t k = 1; k < SF3D_CHUNK && same; ++k) same = pairNode[(size_t)q * SF3D_CHUNK + k] == pairNode[(size_t)q * SF3D_CHUNK];
            if (same) pairChunk[q] = pairNode[(size_t)q * SF3D_CHUNK] | (1ull << 63);
        }
    } else { pairNode.clear(); pairNX = pairNY = pairNZ = 0; }
    return regular;
}

/* not a full box: a LAYERED MASKED grid?  (a DEM outline with holes, soil columns of different depth - what
 * Project3D::setCrit3DTopography builds, project3D.cpp:941-1103.)  Every node gets (layer, row, column): layer = number of Up
 * hops to the surface, row / column from the surface node's coordinates; every link must go to one of the 26 grid neighbours.
 * Called on a g that describes nothing; returns whether it now describes such a grid. */
inline bool plan_masked_grid(const LinkTables& t, const HostModel& m, int world, int rank, GridPlan& g)
{
    const std::vector<uint8_t>& kind = t.kind; const std::vector<uint32_t>& to = t.to;
    std::vector<uint64_t>&pairNode = g.node, &pairChunk = g.chunk; std::vector<int32_t>& pairIdxMap = g.idxMap;
    uint32_t &pairNX = g.NX, &pairNY = g.NY, &pairNZ = g.NZ;
    const uint32_t N = m.N, ns = m.ns, nChunks = (N + SF3D_CHUNK - 1) / SF3D_CHUNK;
    if (ns >= 64 && N < (1u << 28) && m.x.size() == N && m.y.size() == N) {
        bool ok = true;
        std::vector<int32_t> lay(N, -1), row(N, -1), colv(N, -1);
        double cell = 0.;
        for (int sl = 2; sl < SF3D_SLOTS; ++sl)
            for (uint32_t i = 0; i < ns; ++i) {
                const size_t e = (size_t)sl * N + i;
                if (kind[e] == LK_NONE) continue;
                const double dx = std::fabs(m.x[to[e]] - m.x[i]), dy = std::fabs(m.y[to[e]] - m.y[i]);
                const double d = dx > 0 ? (dy > 0 ? std::min(dx, dy) : dx) : dy;
                if (d > 0 && (cell == 0. || d < cell)) cell = d;
            }
        ok = cell > 0.;
        double xmin = 0, ymin = 0, ymax = 0;
        bool northFirst = false;
        auto place_rc = [&](uint32_t i) -> bool {           /* row / column of a node from its coordinates */
            const double fc = (m.x[i] - xmin) / cell, fr = (northFirst ? (ymax - m.y[i]) : (m.y[i] - ymin)) / cell;
            const long long c = std::llround(fc), r = std::llround(fr);
            if (std::fabs(fc - (double)c) > 1e-6 || std::fabs(fr - (double)r) > 1e-6 || c < 0 || r < 0 || c > 60000 || r > 60000) return false;
            row[i] = (int32_t)r; colv[i] = (int32_t)c;
            return true;
        };
        if (ok) {
            xmin = m.x[0]; ymin = ymax = m.y[0];
            const uint32_t nb = world > 1 ? N : ns;         /* (a strip-local model may hold halo soil nodes whose surface node it does not hold) */
            for (uint32_t i = 1; i < nb; ++i) { xmin = std::min(xmin, m.x[i]); ymin = std::min(ymin, m.y[i]); ymax = std::max(ymax, m.y[i]); }
            northFirst = m.y[0] > m.y[ns - 1];
            for (uint32_t i = 0; i < ns && ok; ++i) { lay[i] = 0; ok = place_rc(i); }
        }
        std::vector<uint32_t> orphans;
        for (uint32_t i = ns; i < N && ok; ++i) {           /* soil nodes: below the node their Up link names (layer-major: it has a smaller index) */
            if (kind[i] == LK_NONE || to[i] >= i || lay[to[i]] < 0) {
                /* a strip-local model: a HALO node may have lost its Up link (the node above it is read by none of this rank's rows) */
                if (world > 1 && m.presetPartition != nullptr && m.presetPartition->owner[i] != rank) { orphans.push_back(i); continue; }
                ok = false; break;
            }
            lay[i] = lay[to[i]] + 1; row[i] = row[to[i]]; colv[i] = colv[to[i]];
        }
        for (int pass = 0; pass < 8 && ok && !orphans.empty(); ++pass) {
            /* such a node lies in the layer of the node that reads it through a lateral link, at the place its coordinates say */
            for (int sl = 2; sl < SF3D_SLOTS; ++sl)
                for (uint32_t i = 0; i < N; ++i) {
                    const size_t e = (size_t)sl * N + i;
                    if (kind[e] == LK_NONE || lay[i] < 0) continue;
                    const uint32_t j = to[e];
                    if (lay[j] < 0) { lay[j] = lay[i]; if (!place_rc(j)) ok = false; }
                }
            std::vector<uint32_t> left;
            for (uint32_t i : orphans) {
                if (lay[i] >= 0) continue;
                if (kind[i] != LK_NONE && to[i] < i && lay[to[i]] >= 0) { lay[i] = lay[to[i]] + 1; row[i] = row[to[i]]; colv[i] = colv[to[i]]; }
                else left.push_back(i);
            }
            if (left.size() == orphans.size()) break;
            orphans.swap(left);
        }
        for (uint32_t i : orphans) if (lay[i] < 0) ok = false;
        int32_t mr = 0, mc = 0, ml = 0;
        if (ok) for (uint32_t i = 0; i < N; ++i) { mr = std::max(mr, row[i]); mc = std::max(mc, colv[i]); ml = std::max(ml, lay[i]); }
        const uint32_t gNX = ok ? (uint32_t)((mc + 64) / 64 * 64) : 0, gNY = (uint32_t)mr + 1, gNZ = (uint32_t)ml + 1;
        if (ok && ((uint64_t)gNX * gNY * gNZ > (1ull << 30) || gNZ < 2 || gNY < 6)) ok = false;
        std::vector<int32_t> idxMap;
        if (ok) {
            idxMap.assign((size_t)gNX * gNY * gNZ, -1);
            for (uint32_t i = 0; i < N && ok; ++i) {
                int32_t& cellIdx = idxMap[((size_t)lay[i] * gNY + (size_t)row[i]) * gNX + (size_t)colv[i]];
                if (cellIdx >= 0) ok = false;                /* two nodes in one cell */
                cellIdx = (int32_t)i;
            }
        }
        if (ok) {
            pairNode.assign(N, 0);
            std::atomic<bool> bad{false};
            parallel_for(N, [&](uint32_t a, uint32_t b) {
                for (uint32_t i = a; i < b && !bad.load(std::memory_order_relaxed); ++i) {
                    uint64_t code = 0; unsigned seen = 0;
                    for (int sl = 0; sl < SF3D_SLOTS; ++sl) {
                        const size_t e = (size_t)sl * N + i;
                        uint64_t nib = SF3D_PAIR_NONE;
                        if (kind[e] != LK_NONE) {
                            const uint32_t j = to[e];
                            const int32_t dl = lay[j] - lay[i], dr = row[j] - row[i], dc = colv[j] - colv[i];
                            if (sl == 0) { if (dl != -1 || dr != 0 || dc != 0) bad = true; nib = SF3D_PAIR_UP; }
                            else if (sl == 1) { if (dl != 1 || dr != 0 || dc != 0) bad = true; nib = SF3D_PAIR_DOWN; }
                            else {
                                if (dl != 0 || dr < -1 || dr > 1 || dc < -1 || dc > 1 || (dr == 0 && dc == 0)) { bad = true; break; }
                                nib = (uint64_t)((dr + 1) * 3 + (dc + 1));
                                if (seen & (1u << nib)) bad = true;
                                seen |= 1u << nib;
                            }
                        }
                        code |= nib << (4 * sl);
                    }
                    pairNode[i] = code;
                }
            });
            ok = !bad;
        }
        if (ok) { pairNX = gNX; pairNY = gNY; pairNZ = gNZ; pairIdxMap.swap(idxMap); pairChunk.assign(nChunks, 0); }
        else { pairNode.clear(); }
    }
    return !pairNode.empty();
}

/* ownership + chunk lists (identity lists on one GPU) */
inline ChunkLists plan_chunk_lists(const Partition& part, const LinkTables& t, uint32_t N, uint32_t ns, int world, int rank)
{
    const std::vector<uint8_t>& kind = t.kind; const std::vector<uint32_t>& to = t.to;
    const uint32_t nChunks = (N + SF3D_CHUNK - 1) / SF3D_CHUNK, qSplit = std::min((ns + SF3D_CHUNK - 1) / SF3D_CHUNK, nChunks);
    ChunkLists c;
    std::vector<uint32_t>& listSurf = c.listSurf;
    c.ownedNodes = N;
    if (world > 1) { uint32_t cnt = 0; for (uint32_t i = 0; i < N; ++i) cnt += part.owner[i] == rank; c.ownedNodes = cnt; }
    std::vector<uint32_t> listSoil;
    for (uint32_t q = 0; q < nChunks; ++q) {
        bool mine = world == 1;
        if (!mine) {
            const uint32_t i0 = q * SF3D_CHUNK, i1 = (i0 + SF3D_CHUNK < N) ? i0 + SF3D_CHUNK : N;
            for (uint32_t i = i0; i < i1 && !mine; ++i) mine = part.owner[i] == rank;
        }
        if (mine) (q < qSplit ? listSurf : listSoil).push_back(q);
    }
    c.nListSurf = (uint32_t)listSurf.size();
    c.nList = (uint32_t)(listSurf.size() + listSoil.size());
    if (world > 1) {
        /* chunks that owe values to a neighbouring rank go first: their halo puts are on the wire while the interior
         * is still being computed, instead of being the last thing every sweep waits for */
        std::vector<uint8_t> owes(nChunks, 0);
        for (int pr = 0; pr < world; ++pr) for (uint32_t node : part.send[pr]) owes[node / SF3D_CHUNK] = 1;
        auto first = [&](uint32_t q) { return owes[q] != 0; };
        std::stable_partition(listSurf.begin(), listSurf.end(), first);
        std::stable_partition(listSoil.begin(), listSoil.end(), first);
    }
    listSurf.insert(listSurf.end(), listSoil.begin(), listSoil.end());
    /* An approximation queued in slabs (SF3D_SLAB_OVERLAP, sf3d_host_step.inc): the rows of the list entries [0, e) read the node
     * properties of list entries [0, propsNeed[e - 1]) - the furthest node any of their links names, whatever the numbering
     * (layer-major: one layer further).  One GPU: the list is the identity. */
    if (world == 1 && c.nList == nChunks) {
        c.propsNeed.assign(nChunks, 0);
        parallel_for(nChunks, [&](uint32_t a, uint32_t b) {
            for (uint32_t q = a; q < b; ++q) {
                uint32_t far = q;
                const uint32_t i0 = q * SF3D_CHUNK, i1 = (i0 + SF3D_CHUNK < N) ? i0 + SF3D_CHUNK : N;
                for (int sl = 0; sl < SF3D_SLOTS; ++sl)
                    for (uint32_t i = i0; i < i1; ++i) {
                        const size_t e = (size_t)sl * N + i;
                        if (kind[e] != LK_NONE && to[e] / SF3D_CHUNK > far) far = to[e] / SF3D_CHUNK;
                    }
                c.propsNeed[q] = far + 1;
            }
        });
        for (uint32_t q = 1; q < nChunks; ++q) if (c.propsNeed[q] < c.propsNeed[q - 1]) c.propsNeed[q] = c.propsNeed[q - 1];
    }
    return c;
}

/* which rows of the grid are the rank's (g.ownLo, g.ownHi).  Returns false where that leaves no paired sweep: g then describes nothing. */
inline bool plan_strip_rows(const Partition& part, uint32_t N, uint32_t ns, int world, int rank, GridPlan& g)
{
    std::vector<uint64_t>&pairNode = g.node, &pairChunk = g.chunk; const std::vector<int32_t>& pairIdxMap = g.idxMap;
    uint32_t &pairNX = g.NX, &pairNY = g.NY, &pairNZ = g.NZ, &pairOwnLo = g.ownLo, &pairOwnHi = g.ownHi;
    pairOwnLo = 0; pairOwnHi = pairNY;
    if (!pairNode.empty() && world > 1) {
        /* paired sweep on a strip: the rank must own whole rows of the grid, one contiguous run of them, the same in every layer */
        bool ok = true;
        std::vector<int8_t> rowMine(pairNY, -1);
        for (uint32_t i = 0; i < N && ok && pairIdxMap.empty(); ++i) {      /* (masked grids are cut mid-row: PairGrid::role instead, below) */
            const uint32_t r = (i % ns) / pairNX;
            const int8_t mine = part.owner[i] == rank ? 1 : 0;
            if (rowMine[r] < 0) rowMine[r] = mine; else if (rowMine[r] != mine) ok = false;
        }
        uint32_t lo = 0, hi = pairNY;
        if (ok && pairIdxMap.empty()) {
            while (lo < pairNY && rowMine[lo] != 1) ++lo;
            hi = lo;
            while (hi < pairNY && rowMine[hi] == 1) ++hi;
            for (uint32_t r = hi; r < pairNY && ok; ++r) if (rowMine[r] == 1) ok = false;
            if (hi <= lo) ok = false;
        }
        if (ok) { pairOwnLo = lo; pairOwnHi = hi; }
        else { pairNode.clear(); pairChunk.clear(); pairNX = pairNY = pairNZ = 0; }
    }
    return !pairNode.empty();
}

/* the patch lists of a masked grid and the patch height W of the paired pass, by the cost model below.  cus: the device's compute units;
 * pairWaves: SF3D_PAIR_WAVES of the kernel; tryAuto: nobody asked for the pass, it runs only where its cost is below autoCost;
 * wSet, onlyW: SF3D_PAIR_W names the one patch height to look at */
inline PairPlan plan_pair_patches(const GridPlan& g, const Partition& part, int world, int rank, int cus, int pairWaves, bool tryAuto, double autoCost,
                                  bool wSet, uint32_t onlyW)
{
    const std::vector<int32_t>& pairIdxMap = g.idxMap;
    const uint32_t pairNX = g.NX, pairNY = g.NY, pairNZ = g.NZ, pairOwnLo = g.ownLo, pairOwnHi = g.ownHi;
    PairPlan pp;
    uint32_t& bestW = pp.bestW; double bestCost = 1e30;
    /* masked grids: the non-empty patches (a patch owns rows pr (W - 2) .. + W - 3 and 64 columns) and the layers they reach */
    std::vector<uint32_t>(&plist)[4] = pp.plist; std::vector<uint8_t>(&pdepth)[4] = pp.pdepth;
    if (!pairIdxMap.empty()) {
        std::vector<uint8_t> colDepth((size_t)pairNX * pairNY, 0);          /* deepest layer + 1 of every cell's column */
        for (uint32_t l = 0; l < pairNZ; ++l)
            for (size_t k = 0; k < colDepth.size(); ++k)
                if (pairIdxMap[(size_t)l * colDepth.size() + k] >= 0) colDepth[k] = (uint8_t)(l + 1);
        std::vector<uint8_t> colMine(colDepth.size(), 1);                   /* multi GPU: the column is this rank's (a patch must own at least one such) */
        if (world > 1) for (size_t k = 0; k < colMine.size(); ++k) colMine[k] = pairIdxMap[k] >= 0 && part.owner[(uint32_t)pairIdxMap[k]] == rank;
        /* a band of W - 2 rows is covered from left to right: a patch starts at the first column that still holds a node
         * of the band (not at a multiple of 64: at the Ravone outline 921 patches instead of 974 at W = 10, fill 0.90
         * instead of 0.85); patch columns fit 12 bits of the list entry (wider grids keep to multiples of 64, below) */
        int wi = 0;
        for (uint32_t W : {6u, 8u, 10u, 14u}) {
            const uint32_t prs = (pairNY + W - 3) / (W - 2);
            std::vector<uint8_t> band(pairNX);
            for (uint32_t pr = 0; pr < prs; ++pr) {
                const int64_t r0 = (int64_t)pr * (W - 2) - 1;
                std::fill(band.begin(), band.end(), 0);
                for (int64_t r = r0 + 1; r < r0 + (int64_t)W - 1 && r < (int64_t)pairNY; ++r)
                    for (uint32_t cc = 0; cc < pairNX; ++cc) if (colDepth[(size_t)r * pairNX + cc] && colMine[(size_t)r * pairNX + cc]) band[cc] = 1;
                uint32_t cc = 0;
                while (cc < pairNX) {
                    if (!band[cc]) { ++cc; continue; }
                    const uint32_t c0 = pairNX <= 4096 ? cc : cc / 64 * 64;
                    uint8_t depth = 0;
                    for (int64_t r = r0; r < r0 + (int64_t)W; ++r) {
                        if (r < 0 || r >= (int64_t)pairNY) continue;
                        for (int64_t x = (int64_t)c0 - 1; x < (int64_t)c0 + 65; ++x) {
                            if (x < 0 || x >= (int64_t)pairNX) continue;
                            const uint8_t d = colDepth[(size_t)r * pairNX + (size_t)x];
                            if (d > depth) depth = d;
                        }
                    }
                    /* multi GPU: bit 7 = a column of another rank lies in the patch's footprint (the patch, its ring and the outer ring of the staged
                     * old iterate): after the first pass of an approximation the block takes such cells' values from the window (k_sweep_pair_masked) */
                    if (world > 1 && pairNZ < 128u)
                        for (int64_t r = r0 - 1; r < r0 + (int64_t)W + 1 && !(depth & 0x80u); ++r) {
                            if (r < 0 || r >= (int64_t)pairNY) continue;
                            for (int64_t x = (int64_t)c0 - 2; x < (int64_t)c0 + 66; ++x) {
                                if (x < 0 || x >= (int64_t)pairNX) continue;
                                const size_t k = (size_t)r * pairNX + (size_t)x;
                                if (colDepth[k] && !colMine[k]) { depth |= 0x80u; break; }
                            }
                        }
                    plist[wi].push_back(pairNX <= 4096 ? ((pr << 12) | c0) : ((pr << 12) | (c0 / 64)));
                    pdepth[wi].push_back(depth);
                    cc = c0 + 64;
                }
            }
            {   /* workgroup b runs on XCD b % 8 and takes entry run(b % 8) + b / 8 of the list (k_sweep_pair_masked): inside every
                 * XCD's contiguous run the DEEPEST patches go first (stable: spatial order among equals), so that what is left for
                 * the tail round - 921 patches over 512 resident blocks at the Ravone project - are the shallow ones */
                const uint32_t nbk = (uint32_t)plist[wi].size(), per = nbk >> 3, rem = nbk & 7u;
                uint32_t at = 0;
                for (uint32_t x = 0; x < 8 && nbk >= 8; ++x) {
                    const uint32_t len = per + (x < rem ? 1u : 0u);
                    std::vector<uint32_t> ord(len);
                    for (uint32_t k = 0; k < len; ++k) ord[k] = at + k;
                    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return pdepth[wi][a] > pdepth[wi][b]; });
                    std::vector<uint32_t> pl(len); std::vector<uint8_t> pd(len);
                    for (uint32_t k = 0; k < len; ++k) { pl[k] = plist[wi][ord[k]]; pd[k] = pdepth[wi][ord[k]]; }
                    std::copy(pl.begin(), pl.end(), plist[wi].begin() + at); std::copy(pd.begin(), pd.end(), pdepth[wi].begin() + at);
                    at += len;
                }
            }
            ++wi;
        }
    }
    const uint32_t ownRows = pairOwnHi - pairOwnLo;
    for (uint32_t W : {6u, 8u, 10u, 14u}) {
        if (pairNY < W || (wSet && onlyW != W)) continue;
        if (W == 8 && !wSet) continue;          /* W = 8 is not in the fitted cost model: SF3D_PAIR_W=8 only (DESIGN.md 12) */
        const uint64_t blocks = pairIdxMap.empty() ? (uint64_t)((ownRows + W - 3) / (W - 2)) * (pairNX / 64) : (uint64_t)plist[pair_widx(W)].size();
        if (blocks == 0) continue;
        /* relative time per node of a pass, fitted to measurements on one MI355X (profiles/r04_pair_W_sweep.txt: the full C4
         * grid and one of two / of four strips of it at W = 6 / 10 / 14): redundant halo rows x tail round of the blocks x a
         * latency term in the waves a busy CU holds, and the square root of the share of CUs that have a block at all (a
         * strip of 128 rows gives W = 10 only 128 blocks for 256 CUs: 72 us against 59 us at W = 6) */
        const uint64_t perCU = (uint64_t)(4 * pairWaves / (W + 1)), resident = perCU * cus;     /* blocks of W + 1 waves per CU (LDS allows as many) */
        double quant = 1., busyShare = 1., wavesPerCU = (double)(perCU * (W + 1));
        if (blocks >= resident) { const uint64_t rounds = (blocks + resident - 1) / resident; quant = (double)(rounds * resident) / (double)blocks; }
        else { const uint64_t busy = std::min<uint64_t>(blocks, (uint64_t)cus); busyShare = (double)busy / cus; wavesPerCU = (double)blocks / (double)busy * (W + 1); }
        const double cost = (1. + 0.6 / (double)(W - 2)) * quant * (1. + 3.26 / (busyShare * wavesPerCU)) / std::sqrt(busyShare);
        if (cost < bestCost) { bestCost = cost; bestW = W; }
    }
    if (tryAuto && !(bestCost < autoCost)) bestW = 0;
    return pp;
}

/* multi GPU, regular row strips: are the edge rows laid out in the send / receive lists as (layer) * NX + column from a base?  Then the kernels
 * that hand records over inside a launch (the paired pass, the resident loop) address them directly - no walk through a chunk's send list
 * between a value and its store (that walk is the latency of a per-layer / per-iteration lock-step of two ranks' edge blocks) */
inline bool plan_edge_rows_direct(const Partition& part, const GridPlan& g, uint32_t ns, int world, int rank, EdgeRows& er)
{
    const uint32_t pairNX = g.NX, pairNY = g.NY, pairNZ = g.NZ, pairOwnLo = g.ownLo, pairOwnHi = g.ownHi;
    int32_t(&edgePeer)[2] = er.edgePeer; uint32_t(&edgePut)[2] = er.edgePut, (&edgeGet)[2] = er.edgeGet;
    if (pairNX == 0 || pairOwnHi - pairOwnLo < 2) return false;
    for (uint32_t side = 0; side < 2; ++side) {
        if ((side == 0 && pairOwnLo == 0) || (side == 1 && pairOwnHi >= pairNY)) continue;
        const uint32_t rEdge = side == 0 ? pairOwnLo : pairOwnHi - 1, rHalo = side == 0 ? pairOwnLo - 1 : pairOwnHi;
        const int pr = part.owner[rHalo * pairNX];
        if (pr == rank || pr == SF3D_OWNER_NONE || pr >= world) return false;
        const auto& sl = part.send[pr]; const auto& rl = part.recv[pr];
        const auto si = std::lower_bound(sl.begin(), sl.end(), rEdge * pairNX), ri = std::lower_bound(rl.begin(), rl.end(), rHalo * pairNX);
        if (si == sl.end() || ri == rl.end()) return false;
        const size_t sb = (size_t)(si - sl.begin()), rb = (size_t)(ri - rl.begin());
        for (uint32_t l = 0; l < pairNZ; ++l)
            for (uint32_t cc = 0; cc < pairNX; ++cc) {
                const size_t ks = sb + (size_t)l * pairNX + cc, kr = rb + (size_t)l * pairNX + cc;
                if (ks >= sl.size() || kr >= rl.size() || sl[ks] != l * ns + rEdge * pairNX + cc || rl[kr] != l * ns + rHalo * pairNX + cc
                    || part.owner[l * ns + rHalo * pairNX + cc] != pr) return false;
            }
        edgePeer[side] = pr; edgePut[side] = (uint32_t)sb; edgeGet[side] = (uint32_t)rb;
    }
    return true;
}

/* which end of a runoff link the early Courant check evaluates (DevView::probeMask) */
inline std::vector<uint8_t> plan_probe_mask(const LinkTables& t, uint32_t N, uint32_t ns)
{
    const std::vector<uint8_t>& kind = t.kind; const std::vector<uint32_t>& to = t.to;
    std::vector<uint8_t> pm(ns, 0);
    parallel_for(ns, [&](uint32_t a, uint32_t b) {
        for (uint32_t i = a; i < b; ++i)
            for (int sl = 2; sl < SF3D_SLOTS; ++sl) {
                const size_t e = (size_t)sl * N + i;
                if (kind[e] != LK_RUNOFF) continue;
                const uint32_t j = to[e];
                bool mineToDo = j > i;
                if (!mineToDo) {                     /* the other end does it - if it has the link back */
                    bool back = false;
                    for (int s2 = 2; s2 < SF3D_SLOTS && !back; ++s2) back = kind[(size_t)s2 * N + j] == LK_RUNOFF && to[(size_t)s2 * N + j] == i;
                    mineToDo = !back || j == i;
                }
                if (mineToDo) pm[i] |= (uint8_t)(1u << (sl - 2));
            }
    });
    return pm;
}

/* ---- one computeStep: which launch forms it takes (sf3d_host_step.inc), decided from scalars ----
 * StepFacts is what the step driver reads to decide - copied from the solver's state, the device view, the control block of the last step
 * and the switches; plan_step turns them into the mode flags the driver acts on.  tests/plan_host.cpp enumerates the boolean facts and holds
 * the plan to the rules between the flags. */
struct StepFacts {
    bool multi = false;                 /* more than one rank */
    bool heatOn = false;                /* coupled heat */
    bool useFused = true;               /* SF3D_FUSED_DECIDE as the model holds it (the RCCL exchange turns it off) */
    bool lineal = false, haveCg = false;            /* the caller asked for the linealia hook; the model has the conjugate gradients' arrays */
    bool resAvail = false, resFusedPost = false;    /* the resident loop has a grid that fits; its launch does the post-solve part too */
    bool haloDirect = false, rccl = false;
    uint32_t nBnd = 0;                  /* chunks of the rows next to a neighbouring rank (k_sweep_bnd) */
    bool pairAvail = false;             /* the paired pass has a grid */
    int timing = 0; bool sampled = false;           /* kernel timing mode; mode 2: this is a sampled step */
    bool overlapAccept = false, ring = false;       /* SF3D_OVERLAP_ACCEPT; the model has the rings of matrices and heads */
    bool compat = false;                /* quirk-1 emulation: rows are stored raw and normalised by k_compat_rows after the Courant decision */
    bool ntStream = false, asmNtOff = false;        /* streaming stores; SF3D_ASM_NT=0 */
    double probeMin = -1., courant = 0.; uint32_t probeBudget = 0;      /* early Courant check: threshold, the Courant number and the budget the host saw last */
    int slabs = 0; bool havePropsNeed = false; uint32_t nList = 0, nListSurf = 0;      /* SF3D_SLAB_OVERLAP and what it needs of the chunk list */
    bool useGraphs = true, heatGs = false;          /* SF3D_GRAPHS; SF3D_HEAT_GS=1 */
    long residentFailAt = -1; uint64_t residentSteps = 0;       /* SF3D_RESIDENT_FAIL_TEST and the computeSteps it counts in */
};
struct StepPlan {
    bool useFused;                      /* what the model holds from now on: sharded heat exists only in the fused-exchange form */
    bool fused, fusedMulti;             /* sweep + convergence decision in one launch (one GPU); + in-kernel halo puts and all-gather (several) */
    bool linealOn;                      /* the linealia stand-in: device conjugate gradients */
    bool resOn;                         /* all iterations of an approximation in ONE launch, the rows resident on chip (sf3d_resident.inc) */
    bool resFusedPost;                  /* ... which also does k_post's work */
    bool countsResidentStep, forceTimeout;          /* tests: this step counts for SF3D_RESIDENT_FAIL_TEST; its resident launches give up */
    bool pairOn;                        /* k_sweep_pair instead of k_sweep (on a strip: + k_sweep_bnd) */
    bool timedStep;                     /* launches carry HIP events: eager */
    bool overlap;                       /* the accepted step's link flow sums are added later, in one pass over the rings (k_links_flush) */
    bool compat, asmNT;
    bool probeNow;                      /* early Courant check queued with the batches of this step */
    bool slabOn;                        /* the slab experiment */
    bool replayWater, replayHeat;       /* batches / heat groups are replayed from captured graphs (else launched eagerly) */
};
inline StepPlan plan_step(const StepFacts& f)
{
    StepPlan P;
    P.useFused = f.useFused || (f.heatOn && f.multi);
    P.fused = !f.multi && P.useFused;
    P.fusedMulti = f.multi && P.useFused;
    P.linealOn = f.lineal && f.haveCg && !f.multi && P.useFused;
    /* the resident loop: grids that fit, fused decisions, window exchange */
    P.resOn = f.resAvail && (P.fused || (P.fusedMulti && f.haloDirect && !f.rccl)) && !P.linealOn;
    P.resFusedPost = P.resOn && f.resFusedPost;
    P.countsResidentStep = P.resOn && !f.multi;
    P.forceTimeout = P.countsResidentStep && f.residentFailAt >= 0 && (long)f.residentSteps == f.residentFailAt;
    P.pairOn = !P.resOn && (P.fused || (P.fusedMulti && f.haloDirect && f.nBnd != 0)) && f.pairAvail && !P.linealOn;
    /* mode 2 samples: the sweeps of every 8th computeStep carry HIP events (eager launches); the other steps replay captured graphs, so the
     * measurement costs ~1 % instead of ~6 % */
    P.timedStep = f.timing == 1 || (f.timing == 2 && f.sampled);
    /* plain single-GPU path, untimed steps only, so that the per-kernel event timing sees every kernel of a step inside the step
     * (compat: k_compat_rows rewrites what the sums read) */
    P.overlap = f.overlapAccept && !f.multi && f.ring && !P.timedStep && f.timing != 1 && !f.compat;
    P.compat = f.compat;
    P.asmNT = f.ntStream && !f.asmNtOff;      /* SF3D_ASM_NT=0: tuning: cacheable stores of the rows */
    /* queued while the Courant number the host saw last (end of the step before) is within reach of the threshold - far below it the two
     * launches would be guarded no-ops in every approximation */
    P.probeNow = f.probeMin >= 0. && !f.heatOn && !f.multi && !f.compat && f.courant >= 0.75 * f.probeMin && (f.probeBudget > 0 || f.probeMin == 0.);
    P.slabOn = f.slabs >= 2 && !f.multi && !f.heatOn && P.useFused && !f.compat && !P.timedStep && f.timing != 1 && f.havePropsNeed
               && f.nList > f.nListSurf + 64u * (uint32_t)f.slabs;
    P.replayWater = f.useGraphs && !P.timedStep && !f.rccl;      /* event timing needs eager launches; RCCL calls are queued eagerly */
    P.replayHeat = f.useGraphs && !f.heatGs;                     /* (a heat group carries no events: it is replayed in a timed step too) */
    return P;
}

/* how many sweeps to queue for the `index`-th approximation of a step: what the same approximation of the previous step took, plus one
 * (Ctrl::seqSweeps; a sweep queued in vain is a guarded no-op of ~4 us, one too few costs a poll; sweeps that a later batch queued simply
 * continue an unfinished approximation); without a record, the last count plus two */
inline uint32_t predicted_sweeps(uint32_t index, bool withHead, uint32_t predCount, const uint32_t* pred, uint32_t lastSweeps)
{
    uint32_t chunk;
    if (withHead && index < predCount && index < 16u) { chunk = pred[index] + 1; if (chunk < 2) chunk = 2; }
    else { chunk = lastSweeps + 2; if (chunk < 4) chunk = 4; }
    if (chunk > 40) chunk = 40;
    return chunk;
}
/* the paired pass, two Jacobi iterations per launch.  `chunk` = expected iterations + 1: floor(expected / 2) pairs, a single sweep when the
 * expectation is odd (122 us instead of a 175 us pair whose second half would be thrown away), then one more pair as the margin (a guarded
 * no-op when the expectation holds).  oddSingle off (SF3D_PAIR_ODD_SINGLE=0): pairs only.  The single sweep goes in front of pair
 * number singleAfter (UINT32_MAX: there is none). */
struct PairSchedule { uint32_t nPairs, singleAfter; };
inline PairSchedule pair_schedule(uint32_t chunk, bool oddSingle)
{
    const uint32_t expected = chunk > 1 ? chunk - 1 : 1;
    return {oddSingle ? expected / 2 + 1 : (chunk + 1) / 2, (oddSingle && (expected & 1u)) ? expected / 2 : UINT32_MAX};
}
/* sweeps per heat solve: one more than the last solve took, even: few graph shapes (a guarded no-op launch costs ~5 us) */
inline uint32_t heat_chunk(uint32_t lastHeatSweeps)
{
    const uint32_t chunk = ((lastHeatSweeps + 1 + 1) / 2) * 2;
    return chunk < 4 ? 4 : (chunk > 64 ? 64 : chunk);
}
/* Look-ahead: the previous step needed `lastBatches` approximations; that many guarded batches are queued before the first poll (a batch
 * queued in vain costs ~25 no-op launches, a poll costs a full host round trip while the GPU idles).  Heat: as many guarded heat steps as
 * the last computeStep needed; Gauss-Seidel has one launch per dependency level: the queue is kept short */
inline uint32_t water_look_ahead(uint32_t lastBatches) { return lastBatches < 1 ? 1 : (lastBatches > 6 ? 6 : lastBatches); }
inline uint32_t heat_look_ahead(uint32_t lastHeatSteps, bool gs) { return gs ? 1 : (lastHeatSteps < 1 ? 1 : (lastHeatSteps > 8 ? 8 : lastHeatSteps)); }

/* what an instantiated graph is remembered under: everything that changes the launches of a water batch or of a heat group within the
 * life of a model.  Counts have fields of their own, so no two of them can run into each other or into a flag */
enum : uint32_t { GK_HEAT = 1u, GK_HEAD = 2u, GK_TAIL = 4u, GK_RES = 8u, GK_RES_POST = 16u, GK_RES_FAIL = 32u, GK_OVERLAP = 64u, GK_PAIR = 128u,
                  GK_LINEAL = 256u, GK_PROBE = 512u, GK_SLAB = 1024u, GK_SAVE = 2048u };
struct GraphKey {
    uint32_t flags, sweeps, steps;
    bool operator==(const GraphKey& o) const { return flags == o.flags && sweeps == o.sweeps && steps == o.steps; }
};
inline GraphKey water_graph_key(const StepPlan& P, bool withHead, bool withTail, uint32_t chunk)
{
    const uint32_t flags = (withHead ? GK_HEAD : 0u) | (withTail ? GK_TAIL : 0u) | (P.resOn ? GK_RES : 0u) | (P.resFusedPost ? GK_RES_POST : 0u) | (P.forceTimeout ? GK_RES_FAIL : 0u)
                           | (P.overlap ? GK_OVERLAP : 0u) | (P.pairOn ? GK_PAIR : 0u) | (P.linealOn ? GK_LINEAL : 0u) | (P.probeNow ? GK_PROBE : 0u) | (P.slabOn ? GK_SLAB : 0u);
    return {flags, P.resOn ? 0u : chunk, 0u};      /* (the resident loop: one launch whatever the number of iterations: one graph shape) */
}
inline GraphKey heat_graph_key(uint32_t steps, uint32_t chunk, bool save) { return {GK_HEAT | (save ? GK_SAVE : 0u), chunk, steps}; }
