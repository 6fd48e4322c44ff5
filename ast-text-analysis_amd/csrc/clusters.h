// clusters.h -- single-linkage clusters on the device: the maximum spanning forest of a square matrix of similarities that
// is already there, and its cuts (include/east_hip.h, "Clusters"; `east texts clusters`, `east keyphrases clusters`;
// DESIGN.md 16).
//
// The pair {a, b}, a < b, is an edge when S[a][b] is not a NaN.  Edge e is STRONGER than f when w_e > w_f (-0.0 == +0.0),
// or the weights are equal and (a_e, b_e) < (a_f, b_f).  That is a strict total order, so the forest is unique; Boruvka's
// rounds find it: every component picks the strongest edge that leaves it, all picks belong to the forest.
//
//   comp[v] = v
//   a round:
//   --clu_best_kernel: a wavefront a row v, the row read once in whole 512-byte pieces, CLU_UNROLL of them requested
//     before the first comparison; comp[] comes out of the L2 (4 bytes a member against the matrix's 8).  Among the edges
//     of ONE member the stronger of two equal weights is the one with the smaller other end, whichever side of v it is
//     on, so a lane that meets its columns in ascending order keeps what it has unless w > best.  A NaN never wins, the
//     diagonal has v's own component.  Rows of a component that had no edge left in an earlier round are skipped--> bw[v], bj[v]
//   --clu_pick_kernel: a wavefront a component c (named by one of its members, its root): the members' best edges
//     compared as (w, lo, hi) triples, reduced across the lanes--> the edge and the component at its other end, tgt[c];
//     none: c is done for good (nothing leaves it now, so nothing ever will)
//   --clu_merge_kernel, ONE workgroup: c hooks under tgt[c]; two components that pick each other pick the SAME edge (it
//     leaves both, and each holds it strongest), the smaller root stays a root and the larger one records the edge; under
//     the strict order the picks have no other cycle.  A root that hooks stops being a root for good, so the edge goes to
//     slot c of a list of M slots: no counter, no scan.  Then pointer doubling from one array into the other,
//     a barrier between the passes, until a pass moves nothing -- ceil(log2 M) passes at most: a chain of M components
//     converges --, comp[v] = the root of comp[v],
//     and the roots and the roots not done are counted--> 8 bytes read back; the rounds end when at most one root is not done
//   --clu_rank_kernel: the slot of an edge in the result IS the number of edges stronger than it, counted against tiles of
//     256 slots in LDS (key = the order-preserving image of the double with the zeros folded, then (a, b));
//     the weight that comes back is S[a][b] read again, the upper triangle's own bytes.
//
// No atomic anywhere, only comparisons: two builds give the same bytes whatever the grid, the timing or the number of
// rounds.  Three launches a round and one at the end; an uploaded matrix is checked for symmetry in one tiled pass first
// (clu_symmetry_kernel: the tile and its mirror image both read row-wise, the mirror turned in LDS).
//
// The merges are fetched ONCE, at the end of the build, into the state: the cuts are a union-find over at most M - 1 merges
// on the host, and the matrix is not needed again.
//
// Complete and average linkage have their rounds in linkage.h, and the build entry points, which take any linkage, come
// behind them there.  What the three share is in here once: the row maximum (clu_row_best) and the tile minimum
// (clu_tile_min) under their kernels, the state, the frame of a build (ClustersBuild), clusters_first_bad and the cuts.
// lnk_rank_kernel is clu_rank_kernel's counting with another tie word, written out a second time: as one template over the
// slot the two compiled to other code, and clu_rank_kernel measured about 1 % slower in three forms of it.
#pragma once
#include "consumer.h"

#define CLU_UNROLL 8u                      // 512-byte pieces of a row requested before the first comparison
#define CLU_NONE 0xFFFFFFFFu
#define CLU_SYM_TILE 64u
#define CLU_SYM_STRIDE 65u                 // doubles from one row of the turned tile to the next (top.h: TOP_LDS_STRIDE)
#define CLU_MAX_M 0x7FFFFFF0u

// ---- the strongest entry of a row ------------------------------------------------------------------------------------------
struct CluBest {
    double w;
    u32 j;                                 // CLU_NONE: no column of the row may win
};

// A wavefront a row of M doubles, read once in whole 512-byte pieces with the members' words beside them, CLU_UNROLL of both
// requested before the first comparison.  In: word(j), member j's word; no_w() and no_word(), what a lane past the row's end
// holds; in(j, w, word): may column j win.  A lane meets its columns in ascending order, so it keeps what it has unless
// w > best; the lanes are reduced by (w, j), the smaller column of two equal weights.  Every lane returns the row's result.
template <class In> __device__ __forceinline__ CluBest clu_row_best(const double *__restrict__ row, u32 M, u32 lane, const In in)
{
    double best = 0.0;
    u32 best_j = CLU_NONE;
    for (u32 j0 = 0; j0 < M; j0 += 64u * CLU_UNROLL) {
        double w[CLU_UNROLL];
        u32 c[CLU_UNROLL];
#pragma unroll
        for (u32 i = 0; i < CLU_UNROLL; i++) {                    // (all loads requested before the first is used)
            const u32 j = j0 + i * 64u + lane;
            w[i] = j < M ? row[j] : in.no_w();
            c[i] = j < M ? in.word(j) : in.no_word();
        }
#pragma unroll
        for (u32 i = 0; i < CLU_UNROLL; i++) {
            const u32 j = j0 + i * 64u + lane;
            if (in(j, w[i], c[i]) && (best_j == CLU_NONE || w[i] > best)) { best = w[i]; best_j = j; }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ow = __shfl_xor(best, off, WAVE);
        const u32 oj = __shfl_xor(best_j, off, WAVE);
        if (oj != CLU_NONE && (best_j == CLU_NONE || ow > best || (ow == best && oj < best_j))) { best = ow; best_j = oj; }
    }
    return CluBest{best, best_j};
}

// ---- the strongest edge of every member ----------------------------------------------------------------------------------
struct CluEdgeIn {              // column j is an edge of a member of component cv: another component, and the weight no NaN
    const u32 *__restrict__ comp;
    u32 cv;
    __device__ __forceinline__ u32 word(u32 j) const { return comp[j]; }
    __device__ __forceinline__ double no_w() const { return __builtin_nan(""); }
    __device__ __forceinline__ u32 no_word() const { return cv; }
    __device__ __forceinline__ bool operator()(u32, double w, u32 c) const { return w == w && c != cv; }
};

__global__ __launch_bounds__(BLOCK) void clu_best_kernel(const double *__restrict__ S, u32 M, const u32 *__restrict__ comp,
                                                         const u32 *__restrict__ done, double *__restrict__ bw, u32 *__restrict__ bj)
{
    const u32 lane = lane_id();
    const u32 v = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (v >= M) return;                                           // (the same for the whole wavefront)
    const u32 cv = comp[v];
    if (done[cv]) {
        if (lane == 0u) bj[v] = CLU_NONE;
        return;
    }
    const CluBest best = clu_row_best(S + (size_t)v * M, M, lane, CluEdgeIn{comp, cv});
    if (lane == 0u) { bw[v] = best.w; bj[v] = best.j; }
}

// ---- the strongest edge of every component ---------------------------------------------------------------------------------
struct CluEdge {
    double w;
    u32 lo, hi, tgt;                       // lo = CLU_NONE: no edge
};

__device__ __forceinline__ bool clu_stronger(const CluEdge &e, const CluEdge &f)
{
    if (e.lo == CLU_NONE) return false;
    if (f.lo == CLU_NONE) return true;
    return e.w > f.w || (e.w == f.w && (e.lo < f.lo || (e.lo == f.lo && e.hi < f.hi)));
}

__global__ __launch_bounds__(BLOCK) void clu_pick_kernel(u32 M, const u32 *__restrict__ comp, const double *__restrict__ bw,
                                                         const u32 *__restrict__ bj, u32 *__restrict__ done, double *__restrict__ cw,
                                                         u32 *__restrict__ clo, u32 *__restrict__ chi, u32 *__restrict__ tgt)
{
    const u32 lane = lane_id();
    const u32 c = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (c >= M || comp[c] != c || done[c]) return;                // (the same for the whole wavefront: a wavefront a root)
    CluEdge best{0.0, CLU_NONE, CLU_NONE, CLU_NONE};
    for (u32 v = lane; v < M; v += 64u) {
        if (comp[v] != c) continue;
        const u32 j = bj[v];
        if (j == CLU_NONE) continue;
        const CluEdge e{bw[v], v < j ? v : j, v < j ? j : v, comp[j]};
        if (clu_stronger(e, best)) best = e;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        CluEdge o;
        o.w = __shfl_xor(best.w, off, WAVE);
        o.lo = __shfl_xor(best.lo, off, WAVE);
        o.hi = __shfl_xor(best.hi, off, WAVE);
        o.tgt = __shfl_xor(best.tgt, off, WAVE);
        if (clu_stronger(o, best)) best = o;
    }
    if (lane == 0u) {
        tgt[c] = best.tgt;
        if (best.lo == CLU_NONE) done[c] = 1u;
        else { cw[c] = best.w; clo[c] = best.lo; chi[c] = best.hi; }
    }
}

// ---- hooking, pointer doubling, the new labels: one workgroup -------------------------------------------------------------
// p0, p1: the parents of the roots, doubled from one into the other (a non-root is its own parent: nobody asks).  The
// arrays are written and read by this workgroup alone, a barrier between a pass that writes and the pass that reads.
// info[0] = roots, info[1] = roots that are not done.
__global__ __launch_bounds__(BLOCK) void clu_merge_kernel(u32 M, u32 *comp, const u32 *__restrict__ done, const double *__restrict__ cw,
                                                          const u32 *__restrict__ clo, const u32 *__restrict__ chi,
                                                          const u32 *__restrict__ tgt, u32 *p0, u32 *p1, u64 *__restrict__ ekey,
                                                          u32 *__restrict__ ea, u32 *__restrict__ eb, u32 *__restrict__ info)
{
    __shared__ u32 lds[2 * WAVES_PER_BLOCK];
    for (u32 c = threadIdx.x; c < M; c += BLOCK) {
        u32 p = c;
        if (comp[c] == c && !done[c]) {
            const u32 t = tgt[c];                                 // (a root that is not done has picked: t is another root, not done either)
            if (!(tgt[t] == c && c < t)) {
                p = t;
                ekey[c] = ordered_key(cw[c]);
                ea[c] = clo[c];
                eb[c] = chi[c];
            }
        }
        p0[c] = p;
    }
    __syncthreads();
    u32 *src = p0, *dst = p1;
    for (u32 reach = 1; reach < M; reach <<= 1) {                 // after the pass: the ancestor 2 reach up, or the root
        int moved = 0;
        for (u32 c = threadIdx.x; c < M; c += BLOCK) {
            const u32 p = src[c], pp = src[p];
            dst[c] = pp;
            moved |= pp != p;
        }
        const int more = __syncthreads_or(moved);                 // (the same answer in every thread)
        __syncthreads();                                          // (the pass's stores, for the next pass's loads)
        u32 *t = src; src = dst; dst = t;
        if (!more) break;                                         // every parent is a root: the usual end, after two or three passes
    }
    u32 roots = 0, live = 0;
    for (u32 v = threadIdx.x; v < M; v += BLOCK) {
        const u32 r = src[comp[v]];
        comp[v] = r;
        if (r == v) { roots++; live += done[v] ? 0u : 1u; }
    }
    roots = wave_sum(roots);
    live = wave_sum(live);
    if (lane_id() == 0u) { lds[wave_id()] = roots; lds[WAVES_PER_BLOCK + wave_id()] = live; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        info[0] = lds[0] + lds[1] + lds[2] + lds[3];
        info[1] = lds[4] + lds[5] + lds[6] + lds[7];
    }
}

// ---- the forest's edges, strongest first ----------------------------------------------------------------------------------
// Slot i of the M holds an edge when ea[i] != CLU_NONE.  (key, a, b) is unique, so an edge's place is its rank.  A workgroup
// ranks 64 slots, a lane a slot: the M slots pass through LDS in tiles of 256, every wavefront counts against a quarter of
// each tile, the four counts are added.
__global__ __launch_bounds__(BLOCK) void clu_rank_kernel(const double *__restrict__ S, u32 M, const u64 *__restrict__ ekey,
                                                         const u32 *__restrict__ ea, const u32 *__restrict__ eb,
                                                         int32_t *__restrict__ merge_a, int32_t *__restrict__ merge_b,
                                                         double *__restrict__ merge_w)
{
    __shared__ u64 lkey[BLOCK], lab[BLOCK];
    __shared__ u32 part[WAVES_PER_BLOCK][64];
    const u32 lane = lane_id(), wv = wave_id();
    const u32 i = blockIdx.x * 64u + lane;
    const u32 a = i < M ? ea[i] : CLU_NONE, b = i < M ? eb[i] : CLU_NONE;
    const u64 my = a != CLU_NONE ? ekey[i] : 0ull, my_ab = ((u64)a << 32) | b;
    u32 rank = 0;
    for (u32 j0 = 0; j0 < M; j0 += BLOCK) {
        const u32 j = j0 + threadIdx.x;
        const u32 ja = j < M ? ea[j] : CLU_NONE;
        __syncthreads();
        lkey[threadIdx.x] = ja != CLU_NONE ? ekey[j] : 0ull;
        lab[threadIdx.x] = ja != CLU_NONE ? ((u64)ja << 32) | eb[j] : ~0ull;      // (no edge: in front of nothing)
        __syncthreads();
#pragma unroll 8
        for (u32 t = wv * 64u; t < wv * 64u + 64u; t++) {         // (every lane reads the same word: a broadcast)
            const u64 k = lkey[t], ab = lab[t];
            rank += (ab != ~0ull && (k > my || (k == my && ab < my_ab))) ? 1u : 0u;
        }
    }
    part[wv][lane] = rank;
    __syncthreads();
    if (wv == 0u && a != CLU_NONE) {
        rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        merge_a[rank] = (int32_t)a;
        merge_b[rank] = (int32_t)b;
        merge_w[rank] = S[(size_t)a * M + b];
    }
}

// ---- the end of a pass over the NT x NT tiles of 64 x 64, a workgroup a tile ------------------------------------------------
// bad[workgroup] = the smallest `worst` of its threads: a * M + b of the tile's first pair that is refused, or ~0
__device__ __forceinline__ void clu_tile_min(u64 worst, u32 lane, u32 wv, u64 *__restrict__ bad)
{
    __shared__ u64 lds8[WAVES_PER_BLOCK];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(worst, off, WAVE);
        worst = o < worst ? o : worst;
    }
    if (lane == 0u) lds8[wv] = worst;
    __syncthreads();
    if (threadIdx.x == 0u) {
        u64 m = lds8[0];
        for (u32 k = 1; k < WAVES_PER_BLOCK; k++) m = lds8[k] < m ? lds8[k] : m;
        bad[blockIdx.x] = m;
    }
}

// ---- is an uploaded matrix symmetric? --------------------------------------------------------------------------------------
// Workgroup (ti, tj) of the NT x NT tiles, ti <= tj (the others leave at once): tile (ti, tj) against tile (tj, ti), both
// read row-wise, the second turned in LDS.  bad[workgroup] = the smallest a * M + b, a < b, of the tile with
// S[a][b] != S[b][a] and not both NaN, or ~0 (clu_tile_min); the host takes the smallest over the tiles.
__global__ __launch_bounds__(BLOCK) void clu_symmetry_kernel(const double *__restrict__ S, u32 M, u32 NT, u64 *__restrict__ bad)
{
    __shared__ double turned[CLU_SYM_TILE * CLU_SYM_STRIDE];
    const u32 ti = blockIdx.x / NT, tj = blockIdx.x % NT;
    if (ti > tj) {                                                // (the same for the whole workgroup: its mirror image does the work)
        if (threadIdx.x == 0u) bad[blockIdx.x] = ~0ull;
        return;
    }
    const u32 lane = lane_id(), wv = wave_id();
    const u32 r0 = ti * CLU_SYM_TILE, c0 = tj * CLU_SYM_TILE;
    for (u32 r = wv; r < CLU_SYM_TILE; r += WAVES_PER_BLOCK) {    // the mirror tile: rows c0 .., columns r0 ..
        const u32 a = c0 + r, b = r0 + lane;
        turned[lane * CLU_SYM_STRIDE + r] = a < M && b < M ? S[(size_t)a * M + b] : 0.0;
    }
    __syncthreads();
    u64 worst = ~0ull;
    for (u32 r = wv; r < CLU_SYM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = r0 + r, b = c0 + lane;
        if (a < M && b < M && a < b) {
            const double x = S[(size_t)a * M + b], y = turned[r * CLU_SYM_STRIDE + lane];
            const bool same = x == y || (x != x && y != y);
            const u64 at = (u64)a * M + b;
            if (!same && at < worst) worst = at;
        }
    }
    clu_tile_min(worst, lane, wv, bad);
}

// ============================================================================================================ host ==
// The clusters' device buffers belong to the handle and to nothing else; the result lives on the host.
struct ClustersState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_CLU;
    u32 M = 0;
    i64 rounds = 0, launches = 0;
    UploadedTable table;                    // a host matrix's copy (east_hip_clusters_build_host)
    DevBuf work;
    DevBuf wcopy;                           // the working copy of a complete or average linkage build, released after it (linkage.h)
    std::vector<int32_t> merge_a, merge_b;  // the merges, strongest first
    std::vector<double> merge_w;
    ClustersState() { bufs = {&table.buf, &work, &wcopy}; }
    ClustersState &clear_result()           // what a build leaves; the uploaded matrix, which it may be reading, stays
    {
        M = 0;
        rounds = launches = 0;
        merge_a.clear();
        merge_b.clear();
        merge_w.clear();
        return *this;
    }
    void clear() override { clear_result().table.withdraw(); }
};

// The frame of a build, whatever the linkage.  The opening: the last result withdrawn and cleared, the timer started.
struct ClustersBuild {
    east_hip_index *h;
    ClustersState &g;
    ConsumerTimer timer;
    explicit ClustersBuild(east_hip_index *h_) : h(h_), g(consumer_begin<ClustersState>(h_).clear_result()), timer(h_, g) {}
    void fetch_merges(u32 F, const int32_t *ma, const int32_t *mb, const double *mw)
    {
        g.merge_a.resize(F);
        g.merge_b.resize(F);
        g.merge_w.resize(F);
        HIP_CHECK(hipMemcpyAsync(g.merge_a.data(), ma, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(g.merge_b.data(), mb, (size_t)F * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(g.merge_w.data(), mw, (size_t)F * 8, hipMemcpyDeviceToHost, h->stream));
    }
    // The closing: the stream drained and timed, the result valid.
    void close(u32 M, u32 F, i64 *out)
    {
        timer.finish();
        g.M = M;
        g.valid = true;
        if (out) { out[0] = (i64)M; out[1] = (i64)F; out[2] = g.rounds; out[3] = g.launches; }
    }
};

// NT of a pass over the NT x NT tiles of M members, a workgroup a tile.
static u32 clusters_tiles(u32 M)
{
    const u32 NT = ceil_div_u32(M, CLU_SYM_TILE);
    if ((u64)NT * NT >= (u64)0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "clusters: more tiles than one launch takes");
    return NT;
}

// What such a pass found: the smallest of bad[tiles], a * M + b of the first refused pair in row-major order, or ~0.
static u64 clusters_first_bad(east_hip_index *h, const u64 *bad, u32 tiles)
{
    std::vector<u64> host(tiles);
    HIP_CHECK(hipMemcpyAsync(host.data(), bad, (size_t)tiles * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    return *std::min_element(host.begin(), host.end());
}

// An uploaded matrix: EAST_HIP_ERR_INVALID naming the first pair (in row-major order) that is not symmetric.
static void clusters_check_symmetry(east_hip_index *h, ClustersState &g, const double *S, u32 M)
{
    const u32 NT = clusters_tiles(M), tiles = NT * NT;
    g.work.ensure((size_t)tiles * 8 + 256, "the clusters' symmetry check", h->stream);
    u64 *bad = g.work.as<u64>();
    Ctx ctx = handle_ctx(h);
    LAUNCH(ctx, clu_symmetry_kernel, tiles, S, M, NT, bad);
    g.launches++;
    const u64 worst = clusters_first_bad(h, bad, tiles);
    if (worst != ~0ull) {
        char msg[200];
        snprintf(msg, sizeof(msg), "clusters: the matrix is not symmetric: S[%llu][%llu] differs from S[%llu][%llu]", (unsigned long long)(worst / M),
                 (unsigned long long)(worst % M), (unsigned long long)(worst % M), (unsigned long long)(worst / M));
        east_throw(EAST_HIP_ERR_INVALID, msg);
    }
}

// S: M x M doubles on the handle's device, symmetric (checked first when it is the caller's).
static void clusters_build(east_hip_index *h, const double *S, u32 M, bool check, i64 *out)
{
    ClustersBuild b(h);
    ClustersState &g = b.g;
    if (M < 2) return b.close(M, 0, out);
    if (check) clusters_check_symmetry(h, g, S, M);
    // 12 arrays of 4 bytes a member, 4 of 8, the read-back words
    const size_t bytes = 12 * align256((size_t)M * 4) + 4 * align256((size_t)M * 8) + 2 * 256;
    if (!g.work.try_ensure(bytes, h->stream)) {
        char msg[200];
        snprintf(msg, sizeof(msg), "clusters: the work arrays of %u members need %zu bytes, which the device does not have", M, bytes);
        east_throw(EAST_HIP_ERR_OOM, msg);
    }
    Arena a = g.work.arena();
    u32 *comp = a.alloc<u32>(M), *done = a.alloc<u32>(M), *bj = a.alloc<u32>(M), *clo = a.alloc<u32>(M), *chi = a.alloc<u32>(M),
        *tgt = a.alloc<u32>(M), *p0 = a.alloc<u32>(M), *p1 = a.alloc<u32>(M), *ea = a.alloc<u32>(M), *eb = a.alloc<u32>(M);
    int32_t *ma = a.alloc<int32_t>(M), *mb = a.alloc<int32_t>(M);
    double *bw = a.alloc<double>(M), *cw = a.alloc<double>(M), *mw = a.alloc<double>(M);
    u64 *ekey = a.alloc<u64>(M);
    u32 *info = a.alloc<u32>(2);
    std::vector<u32> ident(M);
    for (u32 v = 0; v < M; v++) ident[v] = v;
    HIP_CHECK(hipMemcpyAsync(comp, ident.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemsetAsync(done, 0, (size_t)M * 4, h->stream));
    HIP_CHECK(hipMemsetAsync(ea, 0xFF, (size_t)M * 4, h->stream));
    Ctx ctx = handle_ctx(h);
    const u32 wave_grid = ceil_div_u32(M, WAVES_PER_BLOCK);
    u32 host_info[2] = {M, M};
    // (a round at least halves the roots that are not done, and one more may find that those left have no edge)
    const i64 most = bit_width_u32(M) + 2;
    while (host_info[1] > 1u) {
        if (g.rounds >= most) east_throw(EAST_HIP_ERR_INTERNAL, "clusters: the rounds do not end");
        LAUNCH(ctx, clu_best_kernel, wave_grid, S, M, (const u32 *)comp, (const u32 *)done, bw, bj);
        LAUNCH(ctx, clu_pick_kernel, wave_grid, M, (const u32 *)comp, (const double *)bw, (const u32 *)bj, done, cw, clo, chi, tgt);
        LAUNCH(ctx, clu_merge_kernel, 1, M, comp, (const u32 *)done, (const double *)cw, (const u32 *)clo, (const u32 *)chi,
               (const u32 *)tgt, p0, p1, ekey, ea, eb, info);
        HIP_CHECK(hipMemcpyAsync(host_info, info, 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        g.rounds++;
        g.launches += 3;
    }
    const u32 F = M - host_info[0];
    if (F) {
        LAUNCH(ctx, clu_rank_kernel, ceil_div_u32(M, 64), S, M, (const u64 *)ekey, (const u32 *)ea, (const u32 *)eb, ma, mb, mw);
        g.launches++;
        b.fetch_merges(F, ma, mb, mw);
    }
    b.close(M, F, out);
}

// labels[v] = the smallest member of v's cluster after the first n_merges merges
static void clusters_cut(const ClustersState &g, size_t n_merges, int32_t *labels, i64 *out)
{
    std::vector<u32> parent(g.M);
    for (u32 v = 0; v < g.M; v++) parent[v] = v;
    auto find = [&](u32 v) {
        while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
        return v;
    };
    for (size_t i = 0; i < n_merges; i++) {
        const u32 a = find((u32)g.merge_a[i]), b = find((u32)g.merge_b[i]);
        if (a < b) parent[b] = a; else parent[a] = b;             // (the smaller root stays: a root is its cluster's smallest member)
    }
    if (labels)
        for (u32 v = 0; v < g.M; v++) labels[v] = (int32_t)find(v);
    if (out) { out[0] = (i64)g.M - (i64)n_merges; out[1] = (i64)n_merges; }
}

static const ClustersState &clusters_built(east_hip_index *h)
{
    return consumer_built<ClustersState>(h, "no clusters have been built on this handle");
}

extern "C" {

int east_hip_clusters_fetch(east_hip_handle_t h, int32_t *merge_a, int32_t *merge_b, double *merge_w)
{
    return guarded([&] {
        const ClustersState &g = clusters_built(h);
        const size_t F = g.merge_a.size();
        if (merge_a && F) memcpy(merge_a, g.merge_a.data(), F * 4);
        if (merge_b && F) memcpy(merge_b, g.merge_b.data(), F * 4);
        if (merge_w && F) memcpy(merge_w, g.merge_w.data(), F * 8);
    });
}

int east_hip_clusters_cut_threshold(east_hip_handle_t h, double t, int32_t *labels, int64_t *out)
{
    return guarded([&] {
        if (t != t) east_throw(EAST_HIP_ERR_INVALID, "clusters: the threshold is not a number");
        const ClustersState &g = clusters_built(h);
        size_t n = 0;
        while (n < g.merge_w.size() && g.merge_w[n] >= t) n++;    // (the merges are sorted by weight: a prefix)
        clusters_cut(g, n, labels, out);
    });
}

int east_hip_clusters_cut_count(east_hip_handle_t h, int32_t k, int32_t *labels, int64_t *out)
{
    return guarded([&] {
        if (k < 1) east_throw(EAST_HIP_ERR_INVALID, "clusters: the number of clusters must be at least 1");
        const ClustersState &g = clusters_built(h);
        const i64 want = (i64)g.M - (i64)k, F = (i64)g.merge_a.size();
        clusters_cut(g, (size_t)std::max<i64>(0, std::min(F, want)), labels, out);
    });
}

double east_hip_last_clusters_ms(east_hip_handle_t h) { return consumer_ms<ClustersState>(h); }

}  // extern "C"
