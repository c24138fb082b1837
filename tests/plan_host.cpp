/* The graph analysis of the device build (criteria3d_amd/csrc/sf3d_host_plan.inc) without a device: this program builds small HostModels
 * itself, with links in setNodeLink's insertion order (Up -> slot 0, Down -> slot 1, the k-th lateral -> slot 2 + k), runs every stage and
 * holds what the stage claims against the link data, node by node.  Nothing here is a pinned digest.  tests/test_plan_host.py compiles and
 * runs it, once more with -fsanitize=address,undefined.  Exit status 0 and one "ok" line per group, or the first claim that failed. */
#include "sf3d_model.h"
#include "sf3d_host_plan.inc"

#include <set>
#include <string>

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static const int kLateral[8][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};      /* (row, column) steps, the order the models link them in */
static const double kCell = 10., kThick = 0.5;

static void resize_model(HostModel& m, uint32_t N, uint32_t ns)
{
    m.N = N; m.ns = ns;
    m.x.assign(N, 0.); m.y.assign(N, 0.); m.z.assign(N, 0.);
    m.surf.assign(N, 0); m.hasClass.assign(N, 1); m.btype.assign(N, SF3D_BND_NONE); m.nLat.assign(N, 0);
    for (uint32_t i = 0; i < ns; ++i) m.surf[i] = 1;
    for (int s = 0; s < SF3D_SLOTS; ++s) { m.ltype[s].assign(N, SF3D_LINK_NONE); m.lto[s].assign(N, 0); m.larea[s].assign(N, 0.); }
}
static void set_link(HostModel& m, uint32_t i, uint32_t j, int dir, double area)      /* sf3d_set_node_link */
{
    int s = dir == SF3D_LINK_UP ? 0 : (dir == SF3D_LINK_DOWN ? 1 : 2 + m.nLat[i]);
    if (dir == SF3D_LINK_LATERAL) { CHECK(m.nLat[i] < 8, "node %u", i); m.nLat[i]++; }
    m.ltype[s][i] = (uint8_t)dir; m.lto[s][i] = j; m.larea[s][i] = area;
}
/* layers of cells: index[l][r][c] = node or -1, numbered layer by layer, row by row; row 0 is the northernmost */
static HostModel layered_model(const std::vector<std::vector<int32_t>>& index, uint32_t rows, uint32_t cols)
{
    uint32_t N = 0, ns = 0;
    for (size_t l = 0; l < index.size(); ++l) for (int32_t v : index[l]) if (v >= 0) { ++N; if (l == 0) ++ns; }
    HostModel m; resize_model(m, N, ns);
    const int NZ = (int)index.size();
    for (int l = 0; l < NZ; ++l)
        for (int r = 0; r < (int)rows; ++r)
            for (int c = 0; c < (int)cols; ++c) {
                const int32_t i = index[l][(size_t)r * cols + c];
                if (i < 0) continue;
                m.x[i] = 1000. + kCell * c; m.y[i] = 5000. + kCell * (rows - 1 - r); m.z[i] = 100. - 0.01 * c - 0.02 * r - kThick * l;
                const double area = kCell * kCell, lat = kCell * kThick * (l == 0 ? 0.1 : 1.);
                if (l > 0) set_link(m, i, index[l - 1][(size_t)r * cols + c], SF3D_LINK_UP, area);
                if (l + 1 < NZ && index[l + 1][(size_t)r * cols + c] >= 0) set_link(m, i, index[l + 1][(size_t)r * cols + c], SF3D_LINK_DOWN, area);
                for (auto& d : kLateral) {
                    const int rr = r + d[0], cc = c + d[1];
                    if (rr < 0 || rr >= (int)rows || cc < 0 || cc >= (int)cols || index[l][(size_t)rr * cols + cc] < 0) continue;
                    set_link(m, i, index[l][(size_t)rr * cols + cc], SF3D_LINK_LATERAL, (d[0] && d[1]) ? lat * 0.5 : lat);
                }
            }
    return m;
}
static HostModel box_model(uint32_t NX, uint32_t NY, uint32_t NZ)
{
    std::vector<std::vector<int32_t>> index(NZ, std::vector<int32_t>((size_t)NX * NY));
    int32_t n = 0;
    for (auto& layer : index) for (int32_t& v : layer) v = n++;
    return layered_model(index, NY, NX);
}
/* an outline of 70 x 7 cells with a hole of 2 x 2 cells; columns two and three layers deep */
static HostModel masked_model(std::vector<std::vector<int32_t>>* indexOut = nullptr)
{
    const uint32_t cols = 70, rows = 7;
    std::vector<std::vector<int32_t>> index(3, std::vector<int32_t>((size_t)cols * rows, -1));
    int32_t n = 0;
    for (uint32_t l = 0; l < 3; ++l)
        for (uint32_t r = 0; r < rows; ++r)
            for (uint32_t c = 0; c < cols; ++c) {
                const bool hole = (r == 3 || r == 4) && (c == 30 || c == 31);
                const uint32_t depth = (c * 7 + r * 3) % 5 < 2 ? 2 : 3;
                if (!hole && l < depth) index[l][(size_t)r * cols + c] = n++;
            }
    if (indexOut) *indexOut = index;
    return layered_model(index, rows, cols);
}

struct Plan { std::vector<uint8_t> dslot; LinkTables t; std::vector<ChunkDesc> cdesc; GridPlan g; };
static Plan plan_graph(const HostModel& m, bool align = true)
{
    Plan p; char err[256] = {0};
    p.dslot = plan_slot_alignment(m, align);
    CHECK(plan_link_tables(m, p.dslot, 0, p.t, err, sizeof(err)) == SF3D_OK && err[0] == 0, "%s", err);
    p.cdesc = plan_chunk_descriptors(p.t, m.N, m.ns);
    if (!plan_regular_box(p.t, m, p.g)) plan_masked_grid(p.t, m, 1, 0, p.g);
    return p;
}
static bool has_link(const HostModel& m, int s, uint32_t i) { return m.ltype[s][i] != SF3D_LINK_NONE && (s < 2 || s - 2 < m.nLat[i]); }

/* dslot: a permutation of 2 .. 9 per node that keeps a node's links, and their relative order; the link tables hold every link where dslot says */
static void check_slots_and_tables(const HostModel& m, const Plan& p, bool expectMovedInEveryChunk)
{
    const uint32_t N = m.N, ns = m.ns;
    const size_t NS = (size_t)N * SF3D_SLOTS;
    CHECK(p.t.kind.size() == NS && p.t.to.size() == NS && p.t.area.size() == NS && p.t.dist.size() == NS, "sizes");
    CHECK(p.dslot.empty() || p.dslot.size() == NS, "dslot size %zu", p.dslot.size());
    std::vector<uint8_t> movedChunk((N + 63) / 64, 0);
    size_t links = 0;
    for (uint32_t i = 0; i < N; ++i) {
        int last = 1; unsigned used = 0;
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            const int d = p.dslot.empty() ? s : p.dslot[(size_t)s * N + i];
            if (s < 2) CHECK(d == s, "node %u slot %d -> %d", i, s, d);
            else { CHECK(d >= 2 && d < SF3D_SLOTS && !(used & (1u << d)), "node %u: slot %d -> %d is no permutation of 2..9", i, s, d); used |= 1u << d; }
            if (d != s) movedChunk[i / 64] = 1;
            if (!has_link(m, s, i)) continue;
            ++links;
            if (s >= 2) { CHECK(d > last, "node %u: host slot %d -> device slot %d breaks the order of its links", i, s, d); last = d; }
            const size_t e = (size_t)d * N + i;
            const uint32_t j = m.lto[s][i];
            const bool si = i >= ns, sj = j >= ns;
            const uint8_t want = (si && sj) ? (m.ltype[s][i] == SF3D_LINK_LATERAL ? LK_SOIL_LAT : LK_SOIL_VERT) : ((!si && !sj) ? LK_RUNOFF : LK_INFILTRATION);
            CHECK(p.t.kind[e] == want && p.t.to[e] == j && p.t.area[e] == m.larea[s][i], "node %u host slot %d", i, s);
            const double dx = m.x[i] - m.x[j], dy = m.y[i] - m.y[j], dz = m.z[i] - m.z[j];
            const double d2 = want == LK_SOIL_LAT ? dx * dx + dy * dy + dz * dz : (want == LK_RUNOFF ? dx * dx + dy * dy : dz * dz);
            CHECK(std::fabs(p.t.dist[e] * p.t.dist[e] - d2) <= 1e-12 * d2 && (want != LK_INFILTRATION || p.t.dist[e] > 0.), "node %u host slot %d: distance %g", i, s, p.t.dist[e]);
        }
    }
    size_t inTables = 0;
    for (size_t e = 0; e < NS; ++e) inTables += p.t.kind[e] != LK_NONE;
    CHECK(inTables == links, "%zu links in the tables, %zu in the model", inTables, links);
    if (expectMovedInEveryChunk) for (size_t q = 0; q < movedChunk.size(); ++q) CHECK(movedChunk[q], "chunk %zu: no node moved", q);
}

/* every field of a ChunkDesc that claims uniformity holds for all nodes of the chunk, and a uniform chunk is not reported mixed */
static void check_chunk_descriptors(const HostModel& m, const Plan& p)
{
    const uint32_t N = m.N, ns = m.ns, nChunks = (N + 63) / 64;
    CHECK(p.cdesc.size() == nChunks && sizeof(ChunkDesc) == 240, "%zu descriptors of %zu bytes", p.cdesc.size(), sizeof(ChunkDesc));
    for (uint32_t q = 0; q < nChunks; ++q) {
        const ChunkDesc& d = p.cdesc[q];
        const uint32_t i0 = q * 64, i1 = std::min(i0 + 64, N);
        CHECK(d.rowType == (i1 <= ns ? 0 : (i0 >= ns ? 1 : 2)) && d.pad0 == 0, "chunk %u rowType %d", q, d.rowType);
        bool soilUniform = d.rowType == 1 && i1 - i0 == 64, partial = false;
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            std::set<uint8_t> kinds; std::set<int64_t> deltas; std::set<double> areas, dists; uint32_t n = 0;
            for (uint32_t i = i0; i < i1; ++i) {
                const size_t e = (size_t)s * N + i;
                if (p.t.kind[e] == LK_NONE) continue;
                ++n; kinds.insert(p.t.kind[e]); deltas.insert((int64_t)p.t.to[e] - (int64_t)i); areas.insert(p.t.area[e]); dists.insert(p.t.dist[e]);
            }
            const bool one = kinds.size() == 1 && deltas.size() == 1, all = n == i1 - i0;
            const unsigned bit = 1u << s;
            if (n == 0) { CHECK(d.kind[s] == CK_NONE && d.ukind[s] == CK_NONE && d.delta[s] == 0 && !((d.areaUniform | d.distUniform | d.sweepUniform) & bit), "chunk %u slot %d: empty", q, s); continue; }
            CHECK(d.kind[s] == ((all && one) ? *kinds.begin() : CK_MIXED), "chunk %u slot %d: kind %d, %u links of %zu kinds and %zu offsets", q, s, d.kind[s], n, kinds.size(), deltas.size());
            CHECK(d.ukind[s] == (one ? *kinds.begin() : CK_MIXED), "chunk %u slot %d: ukind %d", q, s, d.ukind[s]);
            CHECK(((d.sweepUniform & bit) != 0) == (d.kind[s] == CK_MIXED && deltas.size() == 1), "chunk %u slot %d: sweepUniform", q, s);
            CHECK(d.delta[s] == ((d.kind[s] != CK_MIXED || (d.sweepUniform & bit)) ? *deltas.begin() : 0), "chunk %u slot %d: delta %d", q, s, d.delta[s]);
            CHECK(((d.areaUniform & bit) != 0) == (areas.size() == 1) && (areas.size() != 1 || d.area[s] == *areas.begin()), "chunk %u slot %d: areaUniform", q, s);
            CHECK(((d.distUniform & bit) != 0) == (dists.size() == 1) && (dists.size() != 1 || d.dist[s] == *dists.begin()), "chunk %u slot %d: distUniform", q, s);
            if (!all) partial = true;
            soilUniform = soilUniform && one && (*kinds.begin() == LK_SOIL_VERT || *kinds.begin() == LK_SOIL_LAT) && areas.size() == 1 && dists.size() == 1;
        }
        CHECK(d.soilUniform == (soilUniform ? (partial ? 2 : 1) : 0), "chunk %u: soilUniform %d", q, d.soilUniform);
    }
}

/* (layer, row, column) of every node of a described grid */
struct Place { int32_t l, r, c; };
static std::vector<Place> places(const HostModel& m, const GridPlan& g)
{
    std::vector<Place> at(m.N, Place{-1, -1, -1});
    if (g.idxMap.empty()) { for (uint32_t i = 0; i < m.N; ++i) at[i] = Place{(int32_t)(i / m.ns), (int32_t)((i % m.ns) / g.NX), (int32_t)(i % g.NX)}; return at; }
    CHECK(g.idxMap.size() == (size_t)g.NX * g.NY * g.NZ, "idxMap size");
    size_t cells = 0;
    for (uint32_t l = 0; l < g.NZ; ++l) for (uint32_t r = 0; r < g.NY; ++r) for (uint32_t c = 0; c < g.NX; ++c) {
        const int32_t i = g.idxMap[((size_t)l * g.NY + r) * g.NX + c];
        if (i < 0) continue;
        ++cells;
        CHECK((uint32_t)i < m.N && at[i].l < 0, "idxMap names node %d twice", i);
        at[i] = Place{(int32_t)l, (int32_t)r, (int32_t)c};
    }
    CHECK(cells == m.N, "idxMap holds %zu nodes of %u", cells, m.N);      /* with the line above: idxMap and (layer, row, column) are inverse */
    return at;
}
/* for every node and slot, the neighbour that the nibble of pairNode names equals `to`; bit 63 of pairChunk exactly where all 64 codes agree */
static void check_grid(const HostModel& m, const Plan& p, uint32_t NX, uint32_t NY, uint32_t NZ, bool masked)
{
    const GridPlan& g = p.g;
    const uint32_t N = m.N, nChunks = (N + 63) / 64;
    CHECK(g.NX == NX && g.NY == NY && g.NZ == NZ && g.node.size() == N && g.chunk.size() == nChunks && g.idxMap.empty() == !masked, "grid %u x %u x %u, %zu codes", g.NX, g.NY, g.NZ, g.node.size());
    const std::vector<Place> at = places(m, g);
    auto node_at = [&](int32_t l, int32_t r, int32_t c) -> int64_t {
        if (l < 0 || r < 0 || c < 0 || l >= (int32_t)NZ || r >= (int32_t)NY || c >= (int32_t)NX) return -1;
        return masked ? g.idxMap[((size_t)l * NY + r) * NX + c] : (int64_t)((size_t)l * m.ns + (size_t)r * NX + c);
    };
    for (uint32_t i = 0; i < N; ++i)
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            const size_t e = (size_t)s * N + i;
            const uint32_t nib = (uint32_t)(g.node[i] >> (4 * s)) & 15u;
            if (p.t.kind[e] == LK_NONE) { CHECK(nib == SF3D_PAIR_NONE, "node %u slot %d: code %u without a link", i, s, nib); continue; }
            int64_t j;
            if (s == 0) { CHECK(nib == SF3D_PAIR_UP, "node %u", i); j = node_at(at[i].l - 1, at[i].r, at[i].c); }
            else if (s == 1) { CHECK(nib == SF3D_PAIR_DOWN, "node %u", i); j = node_at(at[i].l + 1, at[i].r, at[i].c); }
            else { CHECK(nib < 9 && nib != 4, "node %u slot %d: code %u", i, s, nib); j = node_at(at[i].l, at[i].r + (int32_t)(nib / 3) - 1, at[i].c + (int32_t)(nib % 3) - 1); }
            CHECK(j == (int64_t)p.t.to[e], "node %u slot %d: the code names node %lld, the link node %u", i, s, (long long)j, p.t.to[e]);
        }
    for (uint32_t q = 0; q < nChunks; ++q) {
        bool same = (size_t)(q + 1) * 64 <= N && !masked;      /* (the masked pass decodes per node: its chunk codes are all 0) */
        for (uint32_t k = 1; k < 64 && same; ++k) same = g.node[(size_t)q * 64 + k] == g.node[(size_t)q * 64];
        CHECK(g.chunk[q] == (same ? (g.node[(size_t)q * 64] | (1ull << 63)) : 0ull), "chunk %u: code %llx", q, (unsigned long long)g.chunk[q]);
    }
    if (masked)      /* the places are the ones the coordinates and the Up links give */
        for (uint32_t i = 0; i < N; ++i) {
            CHECK(at[i].c == (int32_t)std::llround((m.x[i] - 1000.) / kCell) && at[i].r == (int32_t)std::llround((m.y[0] - m.y[i]) / kCell), "node %u at row %d column %d", i, at[i].r, at[i].c);
            CHECK(at[i].l == (i < m.ns ? 0 : at[m.lto[0][i]].l + 1), "node %u in layer %d", i, at[i].l);
        }
}

/* the chunk lists contain every owned chunk exactly once, surface chunks first, in each part the chunks that owe values first; propsNeed is
 * monotone and not below the furthest chunk any link names */
static ChunkLists check_chunk_lists(const HostModel& m, const Plan& p, const Partition& part, int world, int rank)
{
    const uint32_t N = m.N, ns = m.ns, nChunks = (N + 63) / 64, qSplit = (ns + 63) / 64;
    const ChunkLists c = plan_chunk_lists(part, p.t, N, ns, world, rank);
    std::vector<uint8_t> mine(nChunks, 0), owes(nChunks, 0);
    uint32_t owned = 0;
    for (uint32_t i = 0; i < N; ++i) if (world == 1 || part.owner[i] == rank) { mine[i / 64] = 1; ++owned; }
    if (world > 1) for (int pr = 0; pr < world; ++pr) for (uint32_t node : part.send[pr]) { CHECK(part.owner[node] == rank, "send list"); owes[node / 64] = 1; }
    CHECK(c.ownedNodes == owned && c.nList == c.listSurf.size() && c.nListSurf <= c.nList, "%u owned nodes, list of %u", c.ownedNodes, c.nList);
    std::vector<uint8_t> seen(nChunks, 0);
    for (uint32_t k = 0; k < c.nList; ++k) {
        const uint32_t q = c.listSurf[k];
        CHECK(q < nChunks && mine[q] && !seen[q], "list entry %u: chunk %u", k, q);
        seen[q] = 1;
        CHECK((k < c.nListSurf) == (q < qSplit), "list entry %u: chunk %u on the wrong side of the split", k, q);
        if (k > 0 && k != c.nListSurf) {
            const uint32_t b = c.listSurf[k - 1];
            CHECK(owes[b] > owes[q] || (owes[b] == owes[q] && b < q), "list entries %u, %u: chunks %u, %u out of order", k - 1, k, b, q);
        }
    }
    for (uint32_t q = 0; q < nChunks; ++q) CHECK(seen[q] == mine[q], "chunk %u: owned %d, listed %d", q, mine[q], seen[q]);
    if (world > 1) { CHECK(c.propsNeed.empty(), "propsNeed on a strip"); return c; }
    CHECK(c.propsNeed.size() == nChunks, "propsNeed size");
    uint32_t far = 0;
    for (uint32_t q = 0; q < nChunks; ++q) {
        for (int s = 0; s < SF3D_SLOTS; ++s) for (uint32_t i = q * 64; i < std::min(q * 64 + 64, N); ++i)
            if (p.t.kind[(size_t)s * N + i] != LK_NONE) far = std::max(far, p.t.to[(size_t)s * N + i] / 64);
        CHECK(c.propsNeed[q] >= std::max(far, q) + 1 && c.propsNeed[q] <= nChunks && (q == 0 || c.propsNeed[q] >= c.propsNeed[q - 1]), "propsNeed[%u] = %u, furthest chunk %u", q, c.propsNeed[q], far);
    }
    return c;
}

/* every patch of a list contains at least one owned column, and every owned column lies in exactly one patch; the depth byte is the
 * deepest column of the patch's footprint, bit 7 a column of another rank around it */
static void check_patches(const GridPlan& g, const PairPlan& pp, const Partition& part, int world, int rank)
{
    const uint32_t NX = g.NX, NY = g.NY;
    std::vector<uint8_t> depth((size_t)NX * NY, 0), mine((size_t)NX * NY, 0);
    for (uint32_t l = 0; l < g.NZ; ++l) for (size_t k = 0; k < depth.size(); ++k) if (g.idxMap[(size_t)l * depth.size() + k] >= 0) depth[k] = (uint8_t)(l + 1);
    for (size_t k = 0; k < depth.size(); ++k) mine[k] = depth[k] && (world == 1 || part.owner[(uint32_t)g.idxMap[k]] == rank);
    for (uint32_t W : {6u, 10u}) {
        const int wi = pair_widx(W);
        CHECK(!pp.plist[wi].empty() && pp.plist[wi].size() == pp.pdepth[wi].size(), "W = %u: %zu patches", W, pp.plist[wi].size());
        std::vector<uint8_t> covered(depth.size(), 0);
        for (size_t k = 0; k < pp.plist[wi].size(); ++k) {
            const int64_t pr = pp.plist[wi][k] >> 12, c0 = pp.plist[wi][k] & 4095u, r0 = pr * (W - 2);
            uint32_t own = 0; uint8_t deepest = 0; bool foreign = false;
            for (int64_t r = r0 - 2; r < r0 + W; ++r) for (int64_t c = c0 - 2; c < c0 + 66; ++c) {
                if (r < 0 || r >= (int64_t)NY || c < 0 || c >= (int64_t)NX) continue;
                const size_t cell = (size_t)r * NX + (size_t)c;
                if (r >= r0 && r < r0 + W - 2 && c >= c0 && c < c0 + 64 && mine[cell]) { ++own; CHECK(!covered[cell], "W = %u: row %lld column %lld in two patches", W, (long long)r, (long long)c); covered[cell] = 1; }
                if (r >= r0 - 1 && r < r0 + W - 1 && c >= c0 - 1 && c < c0 + 65) deepest = std::max(deepest, depth[cell]);      /* the patch and its ring */
                if (depth[cell] && !mine[cell]) foreign = true;      /* ... and the outer ring of the staged old iterate */
            }
            CHECK(own > 0, "W = %u: patch %zu owns no column", W, k);
            CHECK((pp.pdepth[wi][k] & 0x7Fu) == deepest && ((pp.pdepth[wi][k] & 0x80u) != 0) == (world > 1 && foreign), "W = %u: patch %zu depth byte %02x, deepest column %u", W, k, pp.pdepth[wi][k], deepest);
        }
        for (size_t cell = 0; cell < depth.size(); ++cell) CHECK(covered[cell] == mine[cell], "W = %u: column %zu owned %d covered %d", W, cell, mine[cell], covered[cell]);
    }
}

/* each runoff link between two surface nodes is evaluated by exactly one of its ends - by the end that has it where the other has no link back */
static void check_probe_mask(const HostModel& m, const Plan& p)
{
    const uint32_t N = m.N, ns = m.ns;
    const std::vector<uint8_t> pm = plan_probe_mask(p.t, N, ns);
    CHECK(pm.size() == ns, "mask size");
    uint32_t links = 0;
    for (uint32_t i = 0; i < ns; ++i)
        for (int s = 2; s < SF3D_SLOTS; ++s) {
            const size_t e = (size_t)s * N + i;
            const bool bit = (pm[i] >> (s - 2)) & 1u;
            if (p.t.kind[e] != LK_RUNOFF) { CHECK(!bit, "node %u slot %d: a bit without a runoff link", i, s); continue; }
            const uint32_t j = p.t.to[e];
            int back = -1;
            for (int s2 = 2; s2 < SF3D_SLOTS && back < 0; ++s2) if (p.t.kind[(size_t)s2 * N + j] == LK_RUNOFF && p.t.to[(size_t)s2 * N + j] == i) back = s2;
            if (back < 0 || j == i) CHECK(bit, "node %u slot %d: nobody evaluates the link to %u", i, s, j);
            else CHECK(bit != (bool)((pm[j] >> (back - 2)) & 1u), "nodes %u and %u: the link between them is evaluated %s", i, j, bit ? "twice" : "by neither");
            ++links;
        }
    CHECK(links > 0, "no runoff link");
}

static uint32_t best_w(uint32_t NX, uint32_t NY, uint32_t ownRows, bool tryAuto)      /* a full box is described by its shape alone */
{
    GridPlan g; g.NX = NX; g.NY = NY; g.NZ = 2; g.ownLo = 0; g.ownHi = ownRows;
    return plan_pair_patches(g, Partition(), 1, 0, 256, 6, tryAuto, 1.9, false, 0).bestW;
}

/* ---- the step's plan (plan_step and the functions beside it) ---- */
#include <map>
#include <tuple>

typedef std::tuple<uint32_t, uint32_t, uint32_t> KeyTuple;
static KeyTuple key_tuple(const GraphKey& k) { return KeyTuple(k.flags, k.sweeps, k.steps); }
/* the launches a water batch queues, as far as they can differ within the life of a model (heat, ranks, the decision form, compat rows,
 * streaming stores and the odd-single rule are fixed with the model): the head part, the form and the number of the sweeps, the post-solve
 * part, the tail part */
typedef std::tuple<int, int, uint32_t, uint32_t, int, int> BatchShape;
static BatchShape batch_shape(const StepPlan& P, bool head, bool tail, uint32_t chunk, bool oddSingle)
{
    const int headPart = head ? 1 + (P.probeNow ? 1 : 0) + (P.slabOn ? 2 : 0) : 0, tailPart = tail ? (P.overlap ? 2 : 1) : 0;
    if (P.linealOn) return BatchShape(headPart, 4, chunk, 0u, 1, tailPart);
    if (P.resOn) return BatchShape(headPart, 3, P.forceTimeout ? 1u : 0u, 0u, P.resFusedPost ? 0 : 1, tailPart);
    if (P.pairOn) { const PairSchedule s = pair_schedule(chunk, oddSingle); return BatchShape(headPart, 2, s.nPairs, s.singleAfter, 1, tailPart); }
    return BatchShape(headPart, 1, chunk, 0u, 1, tailPart);
}
typedef std::tuple<bool, bool, bool, bool, bool, bool, bool, bool> PlanShape;      /* what of a plan a water batch's launches depend on */

static unsigned g_seen[12];
static void check_plan(const StepFacts& f, std::set<PlanShape>& shapes)
{
    const StepPlan P = plan_step(f);
    const bool one = !f.multi;
    CHECK((int)P.linealOn + (int)P.resOn + (int)P.pairOn <= 1, "two sweep forms at once");
    CHECK(!(P.linealOn || P.resOn || P.pairOn) || P.useFused, "a sweep form without fused decisions");
    CHECK(P.useFused == (f.useFused || (f.heatOn && f.multi)), "useFused");
    CHECK(P.fused == (one && P.useFused) && P.fusedMulti == (f.multi && P.useFused), "fused / fusedMulti");
    CHECK(!P.linealOn || (one && f.lineal && f.haveCg), "conjugate gradients");
    CHECK(!(f.multi && (P.resOn || P.pairOn)) || f.haloDirect, "a strip's resident loop or paired pass without the direct halo");
    CHECK(!(f.multi && P.resOn) || !f.rccl, "the resident loop under RCCL");
    CHECK(!(f.multi && P.pairOn) || f.nBnd != 0, "a strip's paired pass without boundary chunks");
    CHECK((!P.resOn || f.resAvail) && (!P.pairOn || f.pairAvail), "a sweep form the model has no grid for");
    CHECK(P.resFusedPost == (P.resOn && f.resFusedPost), "resFusedPost");
    if (one && P.useFused && !P.linealOn) CHECK(P.resOn == f.resAvail && P.pairOn == (!f.resAvail && f.pairAvail), "one GPU: the resident loop where it fits, else the paired pass where it has a grid");
    CHECK(P.linealOn == (f.lineal && f.haveCg && one && P.useFused), "conjugate gradients wherever they are asked for and possible");
    CHECK(P.timedStep == (f.timing == 1 || (f.timing == 2 && f.sampled)), "timedStep");
    CHECK(P.overlap == (one && f.ring && f.overlapAccept && !P.timedStep && f.timing != 1 && !f.compat), "overlap");
    CHECK(!P.slabOn || (one && !f.heatOn && P.useFused && !f.compat && !P.timedStep && f.slabs >= 2 && f.nList > f.nListSurf + 64u * (uint32_t)f.slabs), "slabOn");
    CHECK(P.slabOn || !(one && !f.heatOn && P.useFused && !f.compat && !P.timedStep && f.slabs >= 2 && f.havePropsNeed && f.nList > f.nListSurf + 64u * (uint32_t)f.slabs), "slabOn off");
    CHECK(P.probeNow == (!f.heatOn && one && !f.compat && f.probeMin >= 0. && f.courant >= 0.75 * f.probeMin && (f.probeBudget > 0 || f.probeMin == 0.)), "probeNow");
    CHECK(P.replayWater == (f.useGraphs && !P.timedStep && !f.rccl), "replayWater");
    CHECK(P.replayHeat == (f.useGraphs && !f.heatGs), "replayHeat");
    CHECK(P.compat == f.compat && P.asmNT == (f.ntStream && !f.asmNtOff), "compat / asmNT");
    CHECK(P.countsResidentStep == (P.resOn && one), "countsResidentStep");
    CHECK(P.forceTimeout == (P.countsResidentStep && f.residentFailAt >= 0 && (long)f.residentSteps == f.residentFailAt), "forceTimeout");
    const bool flags[12] = {P.linealOn, P.resOn, P.pairOn, P.overlap, P.slabOn, P.probeNow, P.replayWater, P.replayHeat, P.forceTimeout, P.resFusedPost, P.timedStep, P.fusedMulti && P.pairOn};
    for (int k = 0; k < 12; ++k) g_seen[k] += flags[k];
    shapes.insert(PlanShape(P.resOn, P.resFusedPost, P.forceTimeout, P.overlap, P.pairOn, P.linealOn, P.probeNow, P.slabOn));
}

static void check_step_plan()
{
    std::set<PlanShape> shapes;
    for (unsigned bits = 0; bits < (1u << 17); ++bits) {      /* every combination of the boolean facts */
        StepFacts f;
        unsigned b = bits;
        for (bool* q : {&f.multi, &f.heatOn, &f.useFused, &f.lineal, &f.haveCg, &f.resAvail, &f.resFusedPost, &f.haloDirect, &f.rccl, &f.pairAvail, &f.sampled,
                        &f.overlapAccept, &f.ring, &f.compat, &f.havePropsNeed, &f.useGraphs, &f.heatGs}) { *q = b & 1u; b >>= 1; }
        f.nBnd = 5; f.probeMin = 0.8; f.courant = 1.; f.probeBudget = 1; f.nListSurf = 10; f.nList = 1000;
        for (int timing = 0; timing < 3; ++timing) for (int slabs : {0, 2, 8}) for (uint32_t spare : {0u, 1u}) {      /* spare 0: a chunk list too short for the slabs */
            StepFacts g = f; g.timing = timing; g.slabs = slabs; g.nList = g.nListSurf + 64u * (uint32_t)slabs + spare;
            check_plan(g, shapes);
        }
        for (double probeMin : {-1., 0., 0.8}) for (double side : {-0.01, 0.01}) for (uint32_t budget : {0u, 1u}) {
            StepFacts g = f; g.probeMin = probeMin; g.courant = 0.75 * probeMin + side; g.probeBudget = budget;
            check_plan(g, shapes);
        }
        for (uint32_t nBnd : {0u, 5u}) for (long failAt : {-1L, 0L, 3L}) for (uint64_t steps : {0ull, 3ull}) {
            StepFacts g = f; g.nBnd = nBnd; g.residentFailAt = failAt; g.residentSteps = steps;
            check_plan(g, shapes);
        }
    }
    for (int nt = 0; nt < 2; ++nt) for (int off = 0; off < 2; ++off) { StepFacts f; f.ntStream = nt; f.asmNtOff = off; check_plan(f, shapes); }
    for (int k = 0; k < 12; ++k) CHECK(g_seen[k] > 0, "flag %d is never set", k);      /* none of the claims above holds because a flag is dead */

    /* graph keys: two batches that queue different launches have different keys, and no water key is a heat key */
    std::map<KeyTuple, BatchShape> water[2];
    for (const PlanShape& s : shapes) {
        StepPlan P = plan_step(StepFacts());
        std::tie(P.resOn, P.resFusedPost, P.forceTimeout, P.overlap, P.pairOn, P.linealOn, P.probeNow, P.slabOn) = s;
        for (int odd = 0; odd < 2; ++odd) for (int head = 0; head < 2; ++head) for (int tail = 0; tail < 2; ++tail) for (uint32_t chunk = 0; chunk <= 40; ++chunk) {
            const KeyTuple k = key_tuple(water_graph_key(P, head, tail, chunk));
            const BatchShape shape = batch_shape(P, head, tail, chunk, odd);
            const auto at = water[odd].emplace(k, shape);
            CHECK(at.second || at.first->second == shape, "two water batches with other launches under one key (flags %x, %u sweeps)", std::get<0>(k), std::get<1>(k));
        }
    }
    CHECK(shapes.size() > 20 && water[0].size() > 1000, "%zu plans, %zu keys", shapes.size(), water[0].size());
    std::set<KeyTuple> heat;
    for (uint32_t steps = 1; steps <= 8; ++steps) for (uint32_t chunk = 4; chunk <= 64; ++chunk) for (int save = 0; save < 2; ++save) {
        const KeyTuple k = key_tuple(heat_graph_key(steps, chunk, save));
        CHECK(heat.insert(k).second, "two heat groups under one key");
        CHECK(!water[0].count(k) && !water[1].count(k), "a heat group under a water batch's key");
        GraphKey a = heat_graph_key(steps, chunk, save), b = a;
        CHECK(a == b, "a key differs from itself");
        b.steps ^= 1u; CHECK(!(a == b), "keys with other step counts compare equal");
    }

    /* the paired pass's schedule */
    for (uint32_t chunk = 2; chunk <= 40; ++chunk) {
        const uint32_t expected = chunk - 1;
        const PairSchedule s = pair_schedule(chunk, true);
        if (expected & 1u) {
            CHECK(s.singleAfter < s.nPairs && 2 * s.singleAfter + 1 == expected, "chunk %u: %u pairs and the single sweep are not %u iterations", chunk, s.singleAfter, expected);
            CHECK(s.nPairs - s.singleAfter == 1, "chunk %u: %u pairs after the single sweep", chunk, s.nPairs - s.singleAfter);
        }
        else CHECK(s.singleAfter == UINT32_MAX && 2 * (s.nPairs - 1) == expected, "chunk %u: %u pairs for %u iterations and the margin", chunk, s.nPairs, expected);
        const PairSchedule p = pair_schedule(chunk, false);
        CHECK(p.singleAfter == UINT32_MAX && 2 * p.nPairs >= chunk && 2 * p.nPairs <= chunk + 1, "chunk %u: %u pairs", chunk, p.nPairs);
    }
    CHECK(pair_schedule(0, true).nPairs == 1 && pair_schedule(1, true).nPairs == 1 && pair_schedule(1, true).singleAfter == 0, "the smallest chunks");

    /* predicted counts and look-ahead depths */
    const uint32_t edge[] = {0u, 1u, 2u, 3u, 7u, 38u, 39u, 40u, 41u, 62u, 63u, 64u, 1000u, UINT32_MAX - 1, UINT32_MAX};
    for (uint32_t last : edge) {
        uint32_t pred[16];
        for (uint32_t& q : pred) q = last;
        for (uint32_t count : {0u, 1u, 16u, 40u}) for (uint32_t index : {0u, 1u, 15u, 16u, 100u}) for (int head = 0; head < 2; ++head) {
            const uint32_t n = predicted_sweeps(index, head, count, pred, last);
            const bool record = head && index < count && index < 16u;
            CHECK(n >= (record ? 2u : 4u) && n <= 40u, "predicted_sweeps %u (record %d, last %u)", n, record, last);
            if (last < 30u) CHECK(n == std::max(last + (record ? 1u : 2u), record ? 2u : 4u), "predicted_sweeps %u after %u", n, last);
        }
        const uint32_t h = heat_chunk(last);
        CHECK(h % 2 == 0 && h >= 4 && h <= 64 && (last >= 63u || h > last || h == 4), "heat chunk %u after %u sweeps", h, last);
        CHECK(water_look_ahead(last) == std::min(std::max(last, 1u), 6u) && heat_look_ahead(last, false) == std::min(std::max(last, 1u), 8u) && heat_look_ahead(last, true) == 1, "look-ahead after %u", last);
    }
}

int main()
{
    Partition one; one.owner.clear();
    {   /* box 64 x 6 x 2: the smallest regular grid; every row is an edge row or next to one */
        const HostModel m = box_model(64, 6, 2);
        CHECK(m.N == 768 && m.ns == 384, "%u nodes", m.N);
        const Plan p = plan_graph(m);
        CHECK(!p.dslot.empty(), "nothing aligned");
        check_slots_and_tables(m, p, true);
        check_chunk_descriptors(m, p);
        for (const ChunkDesc& d : p.cdesc) for (int s = 2; s < SF3D_SLOTS; ++s)      /* what the alignment is for: a slot means one direction for the whole chunk */
            CHECK(d.kind[s] != CK_MIXED || ((d.sweepUniform >> s) & 1u), "a lateral slot with mixed offsets after the alignment");
        check_grid(m, p, 64, 6, 2, false);
        check_chunk_lists(m, p, one, 1, 0);
        check_probe_mask(m, p);
        const Plan id = plan_graph(m, false);      /* alignment off: the identity, and the same grid */
        CHECK(id.dslot.empty(), "aligned although off");
        check_slots_and_tables(m, id, false); check_chunk_descriptors(m, id); check_grid(m, id, 64, 6, 2, false);
        GridPlan g = p.g;
        CHECK(plan_strip_rows(one, m.N, m.ns, 1, 0, g) && g.ownLo == 0 && g.ownHi == 6, "rows %u..%u", g.ownLo, g.ownHi);
        CHECK(plan_pair_patches(g, one, 1, 0, 256, 6, true, 1.9, false, 0).bestW == 0 && plan_pair_patches(g, one, 1, 0, 256, 6, false, 1.9, false, 0).bestW == 6, "bestW");
        printf("ok box 64 x 6 x 2\n");

        /* a FreeDrainage node without an Up link is refused with its text, unless the node is another rank's */
        HostModel f = m; f.btype[5] = SF3D_BND_FREE_DRAINAGE;
        LinkTables t; char err[256] = {0};
        CHECK(plan_link_tables(f, p.dslot, 0, t, err, sizeof(err)) == SF3D_BOUNDARY_ERROR && std::string(err) == "FreeDrainage node without an Up link" && t.kind.empty(), "%s", err);
        Partition theirs; theirs.owner.assign(f.N, 1); f.presetPartition = &theirs; err[0] = 0;
        CHECK(plan_link_tables(f, p.dslot, 0, t, err, sizeof(err)) == SF3D_OK && err[0] == 0, "%s", err);
        printf("ok refusal\n");

        /* neither a box nor a masked grid: one lateral link retargeted two columns away */
        HostModel n = m;
        const uint32_t i = m.ns + 2 * 64 + 20;
        int s = 2; while (n.lto[s][i] != i + 1) ++s;
        n.lto[s][i] = i + 2;
        const Plan q = plan_graph(n);
        CHECK(q.g.node.empty() && q.g.chunk.empty() && q.g.idxMap.empty() && q.g.NX == 0 && q.g.NY == 0 && q.g.NZ == 0, "a partial description");
        check_slots_and_tables(n, q, false); check_chunk_descriptors(n, q);
        printf("ok neither\n");
    }
    {   /* box 128 x 8 x 3 in one rank and cut for two: 1 024 surface nodes cut at 512, between rows 3 and 4 */
        const HostModel m = box_model(128, 8, 3);
        CHECK(m.N == 3072, "%u nodes", m.N);
        const Plan p = plan_graph(m);
        check_slots_and_tables(m, p, false); check_chunk_descriptors(m, p); check_grid(m, p, 128, 8, 3, false);
        check_chunk_lists(m, p, one, 1, 0); check_probe_mask(m, p);
        for (int rank = 0; rank < 2; ++rank) {
            Partition part;
            CHECK(sf3d_compute_partition(m, rank, 2, part) == SF3D_OK && part.bounds[1] == 512, "partition");
            const ChunkLists c = check_chunk_lists(m, p, part, 2, rank);
            CHECK(c.ownedNodes == 1536 && c.nList == 24 && c.nListSurf == 8, "%u nodes in %u chunks", c.ownedNodes, c.nList);
            GridPlan g = p.g;
            CHECK(plan_strip_rows(part, m.N, m.ns, 2, rank, g) && g.ownLo == 4u * rank && g.ownHi == 4u * rank + 4 && g.node.size() == m.N, "rows %u..%u", g.ownLo, g.ownHi);
            for (uint32_t i = 0; i < m.N; ++i) { const uint32_t r = (i % m.ns) / 128; CHECK((part.owner[i] == rank) == (r >= g.ownLo && r < g.ownHi), "node %u", i); }
            EdgeRows e;
            CHECK(plan_edge_rows_direct(part, g, m.ns, 2, rank, e), "edge rows");
            const int side = rank == 0 ? 1 : 0, peer = 1 - rank;
            CHECK(e.edgePeer[side] == peer && e.edgePeer[1 - side] == -1, "peers %d %d", e.edgePeer[0], e.edgePeer[1]);
            const uint32_t rEdge = side == 0 ? g.ownLo : g.ownHi - 1, rHalo = side == 0 ? g.ownLo - 1 : g.ownHi;
            for (uint32_t l = 0; l < 3; ++l) for (uint32_t cc = 0; cc < 128; ++cc) {
                CHECK(part.send[peer].at(e.edgePut[side] + l * 128 + cc) == l * m.ns + rEdge * 128 + cc, "put base %u", e.edgePut[side]);
                CHECK(part.recv[peer].at(e.edgeGet[side] + l * 128 + cc) == l * m.ns + rHalo * 128 + cc, "get base %u", e.edgeGet[side]);
            }
            CHECK(plan_pair_patches(g, part, 2, rank, 256, 6, true, 1.9, false, 0).bestW == 0 && plan_pair_patches(g, part, 2, rank, 256, 6, false, 1.9, false, 0).bestW == 6, "bestW");
            /* a cut inside a row leaves no paired sweep, and no description */
            Partition mid = part; mid.owner[4 * 128 + 7] = (uint8_t)(1 - mid.owner[4 * 128 + 7]);
            GridPlan h = p.g;
            CHECK(!plan_strip_rows(mid, m.N, m.ns, 2, rank, h) && h.node.empty() && h.chunk.empty() && h.NX == 0 && h.NY == 0 && h.NZ == 0, "a strip cut inside a row");
        }
        GridPlan g = p.g;
        CHECK(plan_strip_rows(one, m.N, m.ns, 1, 0, g) && plan_pair_patches(g, one, 1, 0, 256, 6, true, 1.9, false, 0).bestW == 0, "bestW");
        printf("ok box 128 x 8 x 3\n");
    }
    {   /* box 192 x 6 x 2: the narrowest grid with chunks away from both row ends, where all 64 codes agree */
        const HostModel m = box_model(192, 6, 2);
        const Plan p = plan_graph(m);
        check_slots_and_tables(m, p, false); check_chunk_descriptors(m, p); check_grid(m, p, 192, 6, 2, false);
        uint32_t agree = 0;
        for (uint64_t code : p.g.chunk) agree += (uint32_t)(code >> 63);
        CHECK(agree > 0 && agree < p.g.chunk.size(), "%u chunks of %zu with one code", agree, p.g.chunk.size());
        printf("ok box 192 x 6 x 2\n");
    }
    {   /* a masked outline of 70 x 7 cells with a hole, columns 2 and 3 layers deep: the grid is padded to 128 columns, the last chunk is short */
        std::vector<std::vector<int32_t>> index;
        const HostModel m = masked_model(&index);
        CHECK(m.ns == 486 && m.N % 64 != 0 && m.N % m.ns != 0, "%u nodes, %u at the surface", m.N, m.ns);
        const Plan p = plan_graph(m);
        check_slots_and_tables(m, p, false); check_chunk_descriptors(m, p); check_grid(m, p, 128, 7, 3, true);
        for (uint32_t l = 0; l < 3; ++l) for (uint32_t r = 0; r < 7; ++r) for (uint32_t c = 0; c < 128; ++c)
            CHECK(p.g.idxMap[((size_t)l * 7 + r) * 128 + c] == (c < 70 ? index[l][(size_t)r * 70 + c] : -1), "idxMap at layer %u row %u column %u", l, r, c);
        check_chunk_lists(m, p, one, 1, 0); check_probe_mask(m, p);
        GridPlan g = p.g;
        CHECK(plan_strip_rows(one, m.N, m.ns, 1, 0, g) && g.ownLo == 0 && g.ownHi == 7, "rows");
        const PairPlan pp = plan_pair_patches(g, one, 1, 0, 256, 6, true, 1.9, false, 0);
        check_patches(g, pp, one, 1, 0);
        CHECK(pp.plist[0].size() == 4 && pp.bestW == 0 && plan_pair_patches(g, one, 1, 0, 256, 6, false, 1.9, false, 0).bestW == 6, "%zu patches, bestW %u", pp.plist[0].size(), pp.bestW);
        for (int rank = 0; rank < 2; ++rank) {      /* cut for two ranks (mid-row): the patches of a rank cover its columns */
            Partition part;
            CHECK(sf3d_compute_partition(m, rank, 2, part) == SF3D_OK && part.bounds[1] == 192, "partition");
            check_chunk_lists(m, p, part, 2, rank);
            GridPlan h = p.g;
            CHECK(plan_strip_rows(part, m.N, m.ns, 2, rank, h), "strip rows of a masked grid");
            check_patches(h, plan_pair_patches(h, part, 2, rank, 256, 6, true, 1.9, false, 0), part, 2, rank);
        }
        printf("ok masked 70 x 7\n");
    }
    /* the choice of W by the cost model on shapes large enough for it to choose (by hand, as in tests/test_plan_host.py): the C4 grid, and
     * one of eight strips of it with its two halo rows */
    CHECK(best_w(512, 512, 512, true) == 10 && best_w(512, 512, 512, false) == 10, "C4: W = %u", best_w(512, 512, 512, true));
    CHECK(best_w(512, 66, 64, true) == 0 && best_w(512, 66, 64, false) == 6, "a strip of C4: W = %u", best_w(512, 66, 64, false));
    printf("ok cost model\n");
    check_step_plan();
    printf("ok step plan\n");
    return 0;
}
