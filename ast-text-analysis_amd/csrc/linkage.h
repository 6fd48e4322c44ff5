// linkage.h -- complete and average linkage clusters on the device, built where the matrix lies (include/east_hip.h,
// "Clusters"; `east -j complete|average texts clusters`, `... keyphrases clusters`).
//
// Both linkages are REDUCIBLE: merging two clusters that are each other's strongest neighbour makes no third cluster more
// similar to the new one than it was to the stronger of the two.  So all reciprocal pairs of a round can be merged at the
// same time, and the dendrogram is the one the sequential algorithm finds; the tree takes a short series of rounds, not
// M - 1 dependent steps (the worst case, a plateau of equal weights, does take M - 1).
//
//   W = the upper triangle of S mirrored (lnk_copy_kernel: tile (ti, tj), ti <= tj, read row-wise once, written row-wise
//   twice, the mirror image turned in LDS; the first NaN -- average: the first value that is not finite -- is reported as
//   clu_symmetry_kernel reports its pair).  W is symmetric BYTE FOR BYTE from then on, so a kernel may read W[x][y] from
//   whichever row is convenient.  alive[v] = 1, size[v] = 1.
//   a round:
//   --lnk_best_kernel: clu_row_best (a wavefront a row, whole 512-byte pieces, CLU_UNROLL of them in flight) over the alive
//     rows, alive[] read beside the row; dead rows and dead columns are skipped--> nw[u], nn[u]
//   --lnk_pair_kernel, ONE workgroup, a thread a cluster: x and y = nn[x] are a pair when nn[y] == x and the weight reaches
//     the floor; every thread writes its OWN entries only (partner[x], alive[x], the new size[x]), and the larger end
//     records the merge in ITS slot of an M-slot list -- a representative dies once: no counter, no scan (clu_merge_kernel's
//     idiom)--> the pairs merged and the clusters left, 8 bytes read back
//   --lnk_update_kernel: a wavefront a row; only the rows of the representatives that merged go on.  Row u is rewritten
//     whole and coalesced from rows u and u' (for a column v that merged too: from their entries at v and v'); where v did
//     not merge, the same lane stores the value to W[v][u] as well -- the only entries of an unmerged row that change.  A
//     lane reads its own entry and entries of rows or columns that died in this round, which nobody writes: in place,
//     no second matrix.  O(pairs * M) entries a round.
//   --lnk_rank_kernel: clu_rank_kernel's counting against tiles of 256 slots in LDS, the key (weight, round, merge_a).
//
// LW is computed in ONE orientation, that of the pair (u, v) with u < v: first over v's columns, then over u's rows,
// whichever of the two rows the lane works for.  Comparisons, two products, a sum and a quotient of doubles (the build has
// -ffp-contract=off; the pragma below says so again): no atomic, the same bytes whatever the grid or the timing.
// The state and the frame of a build are clusters.h's; the build entry points, which take any linkage, are at the end of
// this file, behind linkage_build.
#pragma once
#include "clusters.h"

#define LNK_NO_FLOOR (-__builtin_inf())

// x belongs to the representative (n members before the round), y to its partner (np members)
__device__ __forceinline__ double lnk_lw(bool average, double x, double y, double n, double np)
{
#pragma clang fp contract(off)
    const double lo = (y < x) ? y : x;
    if (!average) return lo;
    const double hi = (y < x) ? x : y;
    const double px = n * x, py = np * y;
    const double r = (px + py) / (n + np);
    return r < lo ? lo : (r > hi ? hi : r);
}

// ---- the working copy, and the values the linkage does not take ------------------------------------------------------------
// Workgroup (ti, tj) of the NT x NT tiles of 64 x 64, ti <= tj (the others leave at once).  bad[workgroup] = the smallest
// a * M + b, a < b, of the tile whose S[a][b] is refused, or ~0 (clu_tile_min).  The diagonal gets S's own diagonal: nobody reads it.
__global__ __launch_bounds__(BLOCK) void lnk_copy_kernel(const double *__restrict__ S, double *__restrict__ W, u32 M, u32 NT, u32 average,
                                                         u64 *__restrict__ bad)
{
    __shared__ double turned[CLU_SYM_TILE * CLU_SYM_STRIDE];
    const u32 ti = blockIdx.x / NT, tj = blockIdx.x % NT;
    if (ti > tj) {                                                // (the same for the whole workgroup)
        if (threadIdx.x == 0u) bad[blockIdx.x] = ~0ull;
        return;
    }
    const u32 lane = lane_id(), wv = wave_id();
    const u32 r0 = ti * CLU_SYM_TILE, c0 = tj * CLU_SYM_TILE;
    u64 worst = ~0ull;
    for (u32 r = wv; r < CLU_SYM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = r0 + r, b = c0 + lane;
        const bool in = a < M && b < M;
        const double x = in ? S[(size_t)a * M + b] : 0.0;
        turned[r * CLU_SYM_STRIDE + lane] = x;
        if (in && a < b) {
            const bool refused = average ? !(x - x == 0.0) : x != x;      // (x - x: NaN for a NaN and for an infinity)
            const u64 at = (u64)a * M + b;
            if (refused && at < worst) worst = at;
        }
    }
    __syncthreads();
    for (u32 r = wv; r < CLU_SYM_TILE; r += WAVES_PER_BLOCK) {
        const double up = turned[r * CLU_SYM_STRIDE + lane], down = turned[lane * CLU_SYM_STRIDE + r];
        const u32 a = r0 + r, b = c0 + lane;
        if (a < M && b < M) W[(size_t)a * M + b] = (ti < tj || r <= lane) ? up : down;
        const u32 ma = c0 + r, mb = r0 + lane;                    // the mirror tile: rows c0 .., columns r0 ..
        if (ti < tj && ma < M && mb < M) W[(size_t)ma * M + mb] = down;
    }
    clu_tile_min(worst, lane, wv, bad);
}

// ---- the strongest neighbour of every alive cluster -----------------------------------------------------------------------
struct LnkPairIn {              // column j is a neighbour of cluster u: alive, and not u itself
    const u32 *__restrict__ alive;
    u32 u;
    __device__ __forceinline__ u32 word(u32 j) const { return alive[j]; }
    __device__ __forceinline__ double no_w() const { return 0.0; }
    __device__ __forceinline__ u32 no_word() const { return 0u; }
    __device__ __forceinline__ bool operator()(u32 j, double, u32 a) const { return a != 0u && j != u; }
};

__global__ __launch_bounds__(BLOCK) void lnk_best_kernel(const double *__restrict__ W, u32 M, const u32 *__restrict__ alive,
                                                         double *__restrict__ nw, u32 *__restrict__ nn)
{
    const u32 lane = lane_id();
    const u32 u = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (u >= M) return;                                           // (the same for the whole wavefront)
    if (!alive[u]) {
        if (lane == 0u) nn[u] = CLU_NONE;
        return;
    }
    const CluBest best = clu_row_best(W + (size_t)u * M, M, lane, LnkPairIn{alive, u});
    if (lane == 0u) { nw[u] = best.w; nn[u] = best.j; }
}

// ---- the reciprocal pairs: one workgroup ------------------------------------------------------------------------------------
// Thread x reads nn[] and nw[] of others and alive[] and size_in[] entries nobody writes here; it writes entries x only, and
// slot x of the merges when x is the end that dies.  info[0] = the pairs merged, info[1] = the clusters left.
__global__ __launch_bounds__(BLOCK) void lnk_pair_kernel(u32 M, u32 round, double floor, u32 *alive, const u32 *__restrict__ nn,
                                                         const double *__restrict__ nw, const u32 *__restrict__ size_in,
                                                         u32 *__restrict__ size_out, u32 *__restrict__ partner, u32 *__restrict__ ea,
                                                         u32 *__restrict__ eb, double *__restrict__ ew, u32 *__restrict__ ernd,
                                                         u32 *__restrict__ info)
{
    __shared__ u32 lds[2 * WAVES_PER_BLOCK];
    u32 pairs = 0, left = 0;
    for (u32 x = threadIdx.x; x < M; x += BLOCK) {
        u32 p = CLU_NONE, s = size_in[x];
        if (alive[x]) {
            const u32 y = nn[x];
            if (y != CLU_NONE && nn[y] == x) {
                const double w = nw[x < y ? x : y];               // (W[u][u'], u < u': the bytes the merge records)
                if (w >= floor) {
                    p = y;
                    if (x < y) {
                        s += size_in[y];
                        pairs++;
                    } else {
                        alive[x] = 0u;
                        ea[x] = y;
                        eb[x] = x;
                        ew[x] = w;
                        ernd[x] = round;
                    }
                }
            }
            left += (p == CLU_NONE || x < p) ? 1u : 0u;
        }
        partner[x] = p;
        size_out[x] = s;
    }
    pairs = wave_sum(pairs);
    left = wave_sum(left);
    if (lane_id() == 0u) { lds[wave_id()] = pairs; lds[WAVES_PER_BLOCK + wave_id()] = left; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        info[0] = lds[0] + lds[1] + lds[2] + lds[3];
        info[1] = lds[4] + lds[5] + lds[6] + lds[7];
    }
}

// ---- the entries that change ------------------------------------------------------------------------------------------------
// alive[] and partner[] as lnk_pair_kernel left them, size[] as it was BEFORE the round.  Row r goes on when r is alive and
// merged: it is the smaller end, rp = partner[r] > r died.  W is not restrict: the lane's own entry is read and written.
__global__ __launch_bounds__(BLOCK) void lnk_update_kernel(double *W, u32 M, u32 average, const u32 *__restrict__ alive,
                                                           const u32 *__restrict__ partner, const u32 *__restrict__ size)
{
    const u32 lane = lane_id();
    const u32 r = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (r >= M || !alive[r]) return;                              // (the same for the whole wavefront)
    const u32 rp = partner[r];
    if (rp == CLU_NONE) return;
    const double nr = (double)size[r], nrp = (double)size[rp];
    double *row = W + (size_t)r * M;
    const double *prow = W + (size_t)rp * M;
    for (u32 c = lane; c < M; c += 64u) {
        if (c == r || !alive[c]) continue;
        const u32 cp = partner[c];
        const double a = row[c], b = prow[c];                     // W[r][c], W[r'][c]
        double val;
        if (cp == CLU_NONE) {
            val = lnk_lw(average, a, b, nr, nrp);                 // (the same expression in both orientations)
        } else {
            const double nc = (double)size[c], ncp = (double)size[cp];
            const double a2 = row[cp], b2 = prow[cp];             // W[r][c'], W[r'][c']
            if (r < c)                                            // u = r, v = c: over v's columns, then over u's rows
                val = lnk_lw(average, lnk_lw(average, a, a2, nc, ncp), lnk_lw(average, b, b2, nc, ncp), nr, nrp);
            else                                                  // u = c, v = r: the same pair seen from row v
                val = lnk_lw(average, lnk_lw(average, a, b, nr, nrp), lnk_lw(average, a2, b2, nr, nrp), nc, ncp);
        }
        row[c] = val;
        if (cp == CLU_NONE) W[(size_t)c * M + r] = val;           // (a row that merged writes its own entry)
    }
}

// ---- the merges, strongest first ------------------------------------------------------------------------------------------
// Slot i of the M holds a merge when ea[i] != CLU_NONE.  A representative merges once a round, so (round, merge_a) is unique
// and a merge's place is its rank under (weight descending, round, merge_a): clu_rank_kernel's counting.
__global__ __launch_bounds__(BLOCK) void lnk_rank_kernel(u32 M, const u32 *__restrict__ ea, const u32 *__restrict__ eb,
                                                         const double *__restrict__ ew, const u32 *__restrict__ ernd,
                                                         int32_t *__restrict__ merge_a, int32_t *__restrict__ merge_b,
                                                         double *__restrict__ merge_w)
{
    __shared__ u64 lkey[BLOCK], lra[BLOCK];
    __shared__ u32 part[WAVES_PER_BLOCK][64];
    const u32 lane = lane_id(), wv = wave_id();
    const u32 i = blockIdx.x * 64u + lane;
    const u32 a = i < M ? ea[i] : CLU_NONE;
    const double w = a != CLU_NONE ? ew[i] : 0.0;
    const u64 my = a != CLU_NONE ? ordered_key(w) : 0ull, my_ra = a != CLU_NONE ? ((u64)ernd[i] << 32) | a : 0ull;
    u32 rank = 0;
    for (u32 j0 = 0; j0 < M; j0 += BLOCK) {
        const u32 j = j0 + threadIdx.x;
        const u32 ja = j < M ? ea[j] : CLU_NONE;
        __syncthreads();
        lkey[threadIdx.x] = ja != CLU_NONE ? ordered_key(ew[j]) : 0ull;
        lra[threadIdx.x] = ja != CLU_NONE ? ((u64)ernd[j] << 32) | ja : ~0ull;    // (no merge: in front of nothing)
        __syncthreads();
#pragma unroll 8
        for (u32 t = wv * 64u; t < wv * 64u + 64u; t++) {         // (every lane reads the same word: a broadcast)
            const u64 k = lkey[t], ra = lra[t];
            rank += (ra != ~0ull && (k > my || (k == my && ra < my_ra))) ? 1u : 0u;
        }
    }
    part[wv][lane] = rank;
    __syncthreads();
    if (wv == 0u && a != CLU_NONE) {
        rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        merge_a[rank] = (int32_t)a;
        merge_b[rank] = (int32_t)eb[i];
        merge_w[rank] = w;
    }
}

// ============================================================================================================ host ==
struct LinkageCopyGuard {                   // the working copy goes when the build ends, however it ends
    DevBuf &buf;
    ~LinkageCopyGuard() { buf.release(); }
};

// S: M x M doubles on the handle's device, symmetric (checked first when it is the caller's); complete or average.
static void linkage_build(east_hip_index *h, const double *S, u32 M, bool check, int32_t linkage, double floor, i64 *out)
{
    ClustersBuild b(h);
    ClustersState &g = b.g;
    if (M < 2) return b.close(M, 0, out);
    const bool average = linkage == EAST_HIP_LINKAGE_AVERAGE;
    if (check) clusters_check_symmetry(h, g, S, M);
    const u32 NT = clusters_tiles(M), tiles = NT * NT;
    LinkageCopyGuard guard{g.wcopy};
    const size_t copy_bytes = align256((size_t)M * M * 8) + align256((size_t)tiles * 8) + 256;
    // 10 arrays of 4 bytes a member, 3 of 8, the read-back words
    const size_t bytes = 10 * align256((size_t)M * 4) + 3 * align256((size_t)M * 8) + 2 * 256;
    if (!g.wcopy.try_ensure(copy_bytes, h->stream) || !g.work.try_ensure(bytes, h->stream)) {
        char msg[200];
        snprintf(msg, sizeof(msg), "clusters: the working copy of %u members needs %zu bytes, which the device does not have", M,
                 copy_bytes + bytes);
        east_throw(EAST_HIP_ERR_OOM, msg);
    }
    Arena wa = g.wcopy.arena();
    double *W = wa.alloc<double>((size_t)M * M);
    u64 *bad = wa.alloc<u64>(tiles);
    Ctx ctx = handle_ctx(h);
    LAUNCH(ctx, lnk_copy_kernel, tiles, S, W, M, NT, average ? 1u : 0u, bad);
    g.launches++;
    const u64 worst = clusters_first_bad(h, bad, tiles);
    if (worst != ~0ull) {
        char msg[200];
        snprintf(msg, sizeof(msg), "clusters: S[%llu][%llu] is %s: %s linkage takes no such similarity", (unsigned long long)(worst / M),
                 (unsigned long long)(worst % M), average ? "not finite" : "a NaN", average ? "average" : "complete");
        east_throw(EAST_HIP_ERR_INVALID, msg);
    }
    Arena a = g.work.arena();
    u32 *alive = a.alloc<u32>(M), *nn = a.alloc<u32>(M), *partner = a.alloc<u32>(M), *size0 = a.alloc<u32>(M), *size1 = a.alloc<u32>(M),
        *ea = a.alloc<u32>(M), *eb = a.alloc<u32>(M), *ernd = a.alloc<u32>(M);
    int32_t *ma = a.alloc<int32_t>(M), *mb = a.alloc<int32_t>(M);
    double *nw = a.alloc<double>(M), *ew = a.alloc<double>(M), *mw = a.alloc<double>(M);
    u32 *info = a.alloc<u32>(2);
    std::vector<u32> ones(M, 1u);
    HIP_CHECK(hipMemcpyAsync(alive, ones.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(size0, ones.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemsetAsync(ea, 0xFF, (size_t)M * 4, h->stream));
    const u32 wave_grid = ceil_div_u32(M, WAVES_PER_BLOCK);
    const double fl = floor != floor ? LNK_NO_FLOOR : floor;
    u32 host_info[2] = {0u, M};
    u32 *size_in = size0, *size_out = size1;
    // Three launches and one read-back a round.  The read-back stands between the pairing and the update, so a round that
    // finds no pair at the floor launches no update; the next round's pick queues behind the update without a wait.
    while (host_info[1] > 1u) {
        if (g.rounds >= (i64)M) east_throw(EAST_HIP_ERR_INTERNAL, "clusters: the rounds do not end");
        LAUNCH(ctx, lnk_best_kernel, wave_grid, (const double *)W, M, (const u32 *)alive, nw, nn);
        LAUNCH(ctx, lnk_pair_kernel, 1, M, (u32)g.rounds, fl, alive, (const u32 *)nn, (const double *)nw, (const u32 *)size_in, size_out,
               partner, ea, eb, ew, ernd, info);
        HIP_CHECK(hipMemcpyAsync(host_info, info, 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        g.launches += 2;
        if (!host_info[0]) break;                                 // no pair reaches the floor: that round merged nothing and is not counted
        LAUNCH(ctx, lnk_update_kernel, wave_grid, W, M, average ? 1u : 0u, (const u32 *)alive, (const u32 *)partner, (const u32 *)size_in);
        g.launches++;
        g.rounds++;
        std::swap(size_in, size_out);
    }
    const u32 F = M - host_info[1];
    if (F) {
        LAUNCH(ctx, lnk_rank_kernel, ceil_div_u32(M, 64), M, (const u32 *)ea, (const u32 *)eb, (const double *)ew, (const u32 *)ernd, ma, mb, mw);
        g.launches++;
        b.fetch_merges(F, ma, mb, mw);
    }
    b.close(M, F, out);                                           // (the timer finishes before the guard frees the copy the launches read)
}

// ---- the build entry points, whatever the linkage -------------------------------------------------------------------------
// Single linkage with a floor keeps the merges that reach it, a prefix of the list.
static void clusters_build_linkage(east_hip_index *h, const double *S, u32 M, bool check, int32_t linkage, double floor, i64 *out)
{
    if (linkage != EAST_HIP_LINKAGE_SINGLE) return linkage_build(h, S, M, check, linkage, floor, out);
    clusters_build(h, S, M, check, out);
    if (floor != floor) return;
    ClustersState &g = *consumer_peek<ClustersState>(h);
    size_t n = 0;
    while (n < g.merge_w.size() && g.merge_w[n] >= floor) n++;
    g.merge_a.resize(n);
    g.merge_b.resize(n);
    g.merge_w.resize(n);
    if (out) out[1] = (i64)n;
}

static void linkage_known(east_hip_index *h, int32_t linkage)
{
    if (linkage == EAST_HIP_LINKAGE_SINGLE || linkage == EAST_HIP_LINKAGE_COMPLETE || linkage == EAST_HIP_LINKAGE_AVERAGE) return;
    if (ClustersState *g = consumer_peek<ClustersState>(h)) g->withdraw();        // (a build that fails leaves no result)
    east_throw(EAST_HIP_ERR_INVALID, "clusters: unknown linkage (single = 0, complete = 1, average = 2)");
}

// The bodies of the build entry points; the two without a linkage are single linkage without a floor (a NaN).  What is
// refused of the source or the size comes before consumer_begin: the last result stays fetchable.
static void clusters_entry_resident(east_hip_index *h, int32_t source, int32_t linkage, double floor, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    linkage_known(h, linkage);
    const TableRef t = consumer_resident_square<ClustersState>(h, source, "clusters");
    clusters_build_linkage(h, t.p, t.K, false, linkage, floor, out);
}

static void clusters_entry_host(east_hip_index *h, const double *matrix, int32_t m, int32_t linkage, double floor, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    linkage_known(h, linkage);
    if (m < 0 || (u32)m >= CLU_MAX_M || (m > 0 && !matrix)) east_throw(EAST_HIP_ERR_INVALID, "clusters: null matrix or bad size");
    if (m == 0) {                                                 // (no members: nothing to upload, and no uploaded matrix left)
        use_device(h);
        consumer_begin<ClustersState>(h).table.withdraw();
        return clusters_build_linkage(h, nullptr, 0, false, linkage, floor, out);
    }
    const TableRef t = consumer_upload<ClustersState>(h, matrix, m, m, "clusters: null matrix or bad size", "the clusters' matrix", [] {});
    try {
        clusters_build_linkage(h, t.p, t.K, true, linkage, floor, out);
    } catch (...) {
        consumer_peek<ClustersState>(h)->table.withdraw();       // (a matrix that was refused is no source either)
        throw;
    }
}

extern "C" {

int east_hip_clusters_build_resident(east_hip_handle_t h, int32_t source, int64_t *out)
{
    return guarded([&] { clusters_entry_resident(h, source, EAST_HIP_LINKAGE_SINGLE, __builtin_nan(""), out); });
}

int east_hip_clusters_build_host(east_hip_handle_t h, const double *matrix, int32_t m, int64_t *out)
{
    return guarded([&] { clusters_entry_host(h, matrix, m, EAST_HIP_LINKAGE_SINGLE, __builtin_nan(""), out); });
}

int east_hip_clusters_build_resident_linkage(east_hip_handle_t h, int32_t source, int32_t linkage, double floor, int64_t *out)
{
    return guarded([&] { clusters_entry_resident(h, source, linkage, floor, out); });
}

int east_hip_clusters_build_host_linkage(east_hip_handle_t h, const double *matrix, int32_t m, int32_t linkage, double floor, int64_t *out)
{
    return guarded([&] { clusters_entry_host(h, matrix, m, linkage, floor, out); });
}

}  // extern "C"
