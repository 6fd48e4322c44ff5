// graph.h -- the keyphrase implication graph on the device, from a score table that is already there.
//
// Replaces the main loop of keyphrases_graph (reference east/applications.py:59-149): a keyphrase *occurs* in a text when
// its score reaches relevance_threshold, its *support* is the number of such texts, the nodes are the positions of the
// keyphrase list whose support reaches support_threshold, and for every ordered pair of nodes (A, B), A != B, in list
// order, an edge A -> B exists when float(shared) / max(support_A, 1) >= referral_confidence.
//
//   K x D doubles --ballot of (score >= threshold), 64 columns a wavefront--> bit rows, W = ceil(D / 64) words per position
//   --support = popcount, (double)support >= support_threshold, exclusive scan (scan.h)--> the kept rows, compacted in order
//   --tiles of 64 sources x 64 targets, both blocks' rows staged in LDS a slice of words at a time, shared =
//     sum popcount(a[w] & b[w]) in registers; the 64 lanes of a wavefront are 64 consecutive targets of one source, so the
//     ballot of the decision IS that source's ordered edge mask over the target block--> a count per (source, target block)
//   --exclusive scan of the counts in (source, target block) order = the reference's edge order--> the same tiles once
//     more, every edge written to its slot: (source position, target position, shared)
//
// Determinism: integer work, one IEEE division per decision, and no atomic anywhere -- an edge's slot is a prefix sum of
// counts, so two runs give the same bytes.  The decision is the division Python makes ((double)shared / (double)max(sup, 1)
// >= referral_confidence; the library is built with -ffp-contract=off and without fast-math, so the quotient is correctly
// rounded): 55 / 100 >= 0.55 holds in doubles where 55 >= 0.55 * 100 does not.  The one shortcut is exact: shared == 0
// gives the quotient +0.0, which reaches no positive threshold, so a wavefront whose 64 pairs share nothing skips it.
//
// The pair tiles run twice (count, fill) instead of keeping K^2 masks or K^2 counts of shared texts: the second pass leaves
// at once where the first one counted no edge for any of the tile's 64 sources, so a sparse graph pays for it where its
// edges are, and a dense one is bound by writing its edges either way.
//
// The host half is a consumer of the handle (consumer.h): it reads whichever table resolve_table names.
#pragma once
#include "consumer.h"

#define GR_TILE 64u                        // sources and targets of a workgroup's tile
#define GR_SRC_PER_WAVE (GR_TILE / WAVES_PER_BLOCK)
#define GR_MAX_SLICE 8                     // words of a bit row staged in LDS at a time

// ---- occurrence bits ---------------------------------------------------------------------------------------------------
// A wavefront per node position: 64 consecutive columns a step (one coalesced 512-byte load), the ballot of
// score >= threshold is the word (NaN compares false, -0.0 >= 0.0 is true: as numpy).  rows[p] = the table row of position
// p: a keyphrase listed twice reads the same row twice.  The words are written 64 at a time, a word per lane.
__global__ __launch_bounds__(BLOCK) void graph_bits_kernel(const double *__restrict__ table, u32 D, const u32 *__restrict__ rows,
                                                           u32 n, u32 W, double threshold, u64 *__restrict__ bits,
                                                           u32 *__restrict__ support)
{
    const u32 p = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (p >= n) return;
    const double *row = table + (size_t)rows[p] * D;
    u64 *out = bits + (size_t)p * W;
    const u32 lane = lane_id();
    u32 sup = 0;
    u64 mine = 0;
    for (u32 w0 = 0; w0 < W; w0 += 4u) {                  // (four loads requested before the first is used)
        double v[4];
#pragma unroll
        for (u32 k = 0; k < 4u; k++) {
            const u32 col = (w0 + k) * 64u + lane;
            v[k] = col < D ? row[col] : __builtin_nan("");
        }
#pragma unroll
        for (u32 k = 0; k < 4u; k++) {
            const u32 w = w0 + k;
            if (w < W) {                                  // (the same for the whole wavefront)
                const u64 word = __ballot(v[k] >= threshold);
                sup += (u32)__popcll(word);
                if ((w & 63u) == lane) mine = word;
                if ((w & 63u) == 63u || w + 1u == W) {
                    const u32 i = (w & ~63u) + lane;
                    if (i <= w) out[i] = mine;
                }
            }
        }
    }
    if (lane == 0) support[p] = sup;
}

// ---- node filter -------------------------------------------------------------------------------------------------------
// keep[p] = (double)support >= support_threshold (the CLI passes -p as a float); keep[n] = 0 for the scan
__global__ __launch_bounds__(BLOCK) void graph_keep_kernel(const u32 *__restrict__ support, u32 n, double support_threshold,
                                                           u32 *__restrict__ keep)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p > n) return;
    keep[p] = p < n && (double)support[p] >= support_threshold ? 1u : 0u;
}

// a wavefront per position: a kept one goes to slot keep_ex[p] -- its position, its support, its bit row
__global__ __launch_bounds__(BLOCK) void graph_compact_kernel(const u32 *__restrict__ keep_ex, const u32 *__restrict__ support,
                                                              const u64 *__restrict__ bits, u32 n, u32 W, u32 *__restrict__ kept,
                                                              u32 *__restrict__ csup, u64 *__restrict__ cbits)
{
    const u32 p = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (p >= n) return;
    const u32 j = keep_ex[p];
    if (keep_ex[p + 1u] == j) return;
    if (lane_id() == 0) { kept[j] = p; csup[j] = support[p]; }
    const u64 *src = bits + (size_t)p * W;
    u64 *dst = cbits + (size_t)j * W;
    for (u32 w = lane_id(); w < W; w += WAVE) dst[w] = src[w];
}

// ---- pairs -------------------------------------------------------------------------------------------------------------
// Workgroup (sb, tb): sources [64 sb, 64 sb + 64) x targets [64 tb, 64 tb + 64) of the M kept rows.  A wavefront takes 16
// of the sources; lane l is target 64 tb + l and keeps its slice of the target's words in registers, the source's words
// are LDS broadcasts.  Rows longer than SL words go a slice at a time, `shared` accumulating in registers.
// FILL == false: cnt[s * TB + tb] = edges of source s into target block tb.
// FILL == true: cnt holds the exclusive scan of those counts (M * TB + 1 entries, modulo 2^32: differences inside a row
// are exact, a row has fewer than 2^32 edges), row_base[s] the 64-bit number of edges in front of source s; every edge
// goes to row_base[s] + (cnt[s * TB + tb] - cnt[s * TB]) + its rank in the wavefront's mask.
template <int SL, bool FILL>
__global__ __launch_bounds__(BLOCK) void graph_pairs_kernel(const u64 *__restrict__ cbits, const u32 *__restrict__ csup,
                                                            const u32 *__restrict__ kept, u32 M, u32 W, u32 TB,
                                                            double referral_confidence, u32 *__restrict__ cnt,
                                                            const u64 *__restrict__ row_base, int32_t *__restrict__ e_src,
                                                            int32_t *__restrict__ e_dst, int32_t *__restrict__ e_shared)
{
    __shared__ u64 lds_s[GR_TILE * SL];
    __shared__ u64 lds_t[GR_TILE * (SL + 1)];             // (+ 1: lane l reads row l, the rows must not share their banks)
    const u32 tb = blockIdx.x % TB, sb = blockIdx.x / TB;
    const u32 lane = lane_id(), wv = wave_id();
    if (FILL) {                                           // a tile without an edge: nothing to write
        u32 c = 0;
        const u32 s = sb * GR_TILE + threadIdx.x;
        if (threadIdx.x < GR_TILE && s < M) {
            const size_t i = (size_t)s * TB + tb;
            c = cnt[i + 1u] - cnt[i];
        }
        if (!__syncthreads_or(c != 0u)) return;
    }
    u32 acc[GR_SRC_PER_WAVE];
#pragma unroll
    for (u32 s = 0; s < GR_SRC_PER_WAVE; s++) acc[s] = 0u;
    for (u32 w0 = 0; w0 < W; w0 += SL) {
        for (u32 i = threadIdx.x; i < GR_TILE * SL; i += BLOCK) {
            const u32 r = i / SL, w = i % SL;
            const bool in_row = w0 + w < W;
            const u32 srow = sb * GR_TILE + r, trow = tb * GR_TILE + r;
            lds_s[r * SL + w] = in_row && srow < M ? cbits[(size_t)srow * W + w0 + w] : 0ull;
            lds_t[r * (SL + 1) + w] = in_row && trow < M ? cbits[(size_t)trow * W + w0 + w] : 0ull;
        }
        __syncthreads();
        u64 b[SL];
#pragma unroll
        for (int w = 0; w < SL; w++) b[w] = lds_t[lane * (SL + 1) + w];
#pragma unroll
        for (u32 s = 0; s < GR_SRC_PER_WAVE; s++) {
#pragma unroll
            for (int w = 0; w < SL; w++) acc[s] += (u32)__popcll(lds_s[(wv * GR_SRC_PER_WAVE + s) * SL + w] & b[w]);
        }
        __syncthreads();
    }
    const u32 s0 = sb * GR_TILE + wv * GR_SRC_PER_WAVE, t = tb * GR_TILE + lane;
    const bool mine = lane < GR_SRC_PER_WAVE && s0 + lane < M;        // lane l < 16 also looks after source s0 + l
    const u32 my_sup = mine ? csup[s0 + lane] : 0u;
    u32 my_cnt = 0;
    u64 my_off = 0;
    int32_t my_id = 0;
    if (FILL) {
        if (mine) {
            const size_t i = (size_t)(s0 + lane) * TB;
            my_off = row_base[s0 + lane] + (u64)(u32)(cnt[i + tb] - cnt[i]);
        }
        if (t < M) my_id = (int32_t)kept[t];
    }
    const bool always = !(referral_confidence > 0.0);     // (also a NaN threshold: the comparison below is false for it)
#pragma unroll
    for (u32 s = 0; s < GR_SRC_PER_WAVE; s++) {
        const u32 src = s0 + s;
        const u32 sup = __shfl(my_sup, (int)s, WAVE);
        bool edge = false;
        if (acc[s] != 0u || always)
            edge = src < M && t < M && src != t && (double)acc[s] / (double)(sup > 1u ? sup : 1u) >= referral_confidence;
        const u64 mask = __ballot(edge);
        if (!FILL) {
            if (lane == s) my_cnt = (u32)__popcll(mask);
        } else {
            const u64 off = __shfl(my_off, (int)s, WAVE);
            if (edge) {
                const u64 o = off + (u64)__popcll(mask & (((u64)1 << lane) - 1ull));
                e_src[o] = (int32_t)kept[src];
                e_dst[o] = my_id;
                e_shared[o] = (int32_t)acc[s];
            }
        }
    }
    if (!FILL && mine) cnt[(size_t)(s0 + lane) * TB + tb] = my_cnt;
}

// ============================================================================================================ host ==
// The graph's device buffers belong to the handle and to nothing else: not the EASA arena, not the cosine buffers.
struct GraphState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_GRAPH;
    u32 n = 0, M = 0;                       // node positions, kept nodes
    i64 E = 0;                              // edges
    UploadedTable table;                    // a host table's copy (east_hip_graph_build_host)
    DevBuf nodes, pairs, edges;
    u32 *support = nullptr, *kept = nullptr;
    int32_t *e_src = nullptr, *e_dst = nullptr, *e_shared = nullptr;
    GraphState() { bufs = {&table.buf, &nodes, &pairs, &edges}; }
    void clear() override
    {
        n = M = 0;
        E = 0;
        table.withdraw();
    }
};

template <bool FILL>
static void graph_launch_pairs(Ctx &ctx, u32 grid, const u64 *cbits, const u32 *csup, const u32 *kept, u32 M, u32 W, u32 TB, double rc,
                               u32 *cnt, const u64 *row_base, int32_t *e_src, int32_t *e_dst, int32_t *e_shared)
{
    const char *name = FILL ? "graph_pairs_fill_kernel" : "graph_pairs_count_kernel";
#define GR_PAIRS(SL) LAUNCH_NAMED(ctx, name, (graph_pairs_kernel<SL, FILL>), grid, cbits, csup, kept, M, W, TB, rc, cnt, row_base, \
                                  e_src, e_dst, e_shared)
    if (W <= 1) GR_PAIRS(1);
    else if (W <= 2) GR_PAIRS(2);
    else if (W <= 4) GR_PAIRS(4);
    else GR_PAIRS(GR_MAX_SLICE);
#undef GR_PAIRS
}

static void graph_build(east_hip_index *h, TableRef t, const int32_t *rows, i64 n_pos, double relevance_threshold, double support_threshold,
                        double referral_confidence, i64 *out)
{
    if (n_pos < 0 || n_pos >= (i64)0x7FFFFFF0 || (n_pos > 0 && !rows)) east_throw(EAST_HIP_ERR_INVALID, "bad node positions");
    for (i64 p = 0; p < n_pos; p++)
        if (rows[p] < 0 || (u32)rows[p] >= t.K) east_throw(EAST_HIP_ERR_INVALID, "a node position names a row outside the score table");
    GraphState &g = consumer_begin<GraphState>(h);
    const u32 n = (u32)n_pos, D = t.D, W = ceil_div_u32(D, 64);
    g.n = n;
    g.M = 0;
    g.E = 0;
    Stats stats;
    Ctx ctx = handle_ctx(h, nullptr, &stats);
    ConsumerTimer timer(h, g);
    if (n) {
        const size_t n1 = (size_t)n + 1;
        g.nodes.ensure(n1 * 20 + (size_t)n * W * 8 + ((size_t)ceil_div_u32(n1, SCAN_TILE) + 1) * 8 + 16 * 256, "the keyphrase graph's node positions");
        Arena a = g.nodes.arena();
        ctx.arena = &a;
        g.support = a.alloc<u32>(n1);
        g.kept = a.alloc<u32>(n1);
        u32 *d_rows = a.alloc<u32>(n1), *keep = a.alloc<u32>(n1), *keep_ex = a.alloc<u32>(n1);
        u64 *bits = a.alloc<u64>((size_t)n * W);
        HIP_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        LAUNCH(ctx, graph_bits_kernel, ceil_div_u32(n, WAVES_PER_BLOCK), t.p, D, (const u32 *)d_rows, n, W, relevance_threshold, bits,
               g.support);
        LAUNCH(ctx, graph_keep_kernel, ceil_div_u32(n1, BLOCK), (const u32 *)g.support, n, support_threshold, keep);
        device_scan<ArrIn, false>(ctx, ArrIn{keep}, n + 1u, keep_ex);
        u32 M = 0;
        HIP_CHECK(hipMemcpyAsync(&M, keep_ex + n, 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        g.M = M;
        if (M) {
            const u32 TB = ceil_div_u32(M, GR_TILE), grid = TB * TB;
            const EmitCounts e = emit_counts(M, TB, "keyphrase graph: %u nodes are more than one device builds a graph of");
            g.pairs.ensure((size_t)M * W * 8 + (size_t)M * 4 + e.bytes, "the keyphrase graph's nodes");
            Arena b = g.pairs.arena();
            ctx.arena = &b;
            u64 *cbits = b.alloc<u64>((size_t)M * W);
            u32 *csup = b.alloc<u32>(M);
            LAUNCH(ctx, graph_compact_kernel, ceil_div_u32(n, WAVES_PER_BLOCK), (const u32 *)keep_ex, (const u32 *)g.support,
                   (const u64 *)bits, n, W, g.kept, csup, cbits);
            g.E = (i64)emit_count_scan_fill(
                ctx, e, false,
                [&](u32 *cnt) {
                    graph_launch_pairs<false>(ctx, grid, cbits, csup, g.kept, M, W, TB, referral_confidence, cnt, nullptr, nullptr, nullptr, nullptr);
                },
                [&](u64 E) {
                    const size_t eb = align256((size_t)E * 4);
                    g.edges.ensure(eb * 3, "the keyphrase graph's edges");
                    g.e_src = (int32_t *)g.edges.p;
                    g.e_dst = (int32_t *)(g.edges.p + eb);
                    g.e_shared = (int32_t *)(g.edges.p + 2 * eb);
                },
                [&](u32 *cnt, const u64 *row_base) {
                    graph_launch_pairs<true>(ctx, grid, cbits, csup, g.kept, M, W, TB, referral_confidence, cnt, row_base, g.e_src, g.e_dst,
                                             g.e_shared);
                });
        }
    }
    timer.finish();
    g.valid = true;
    if (out) { out[0] = g.M; out[1] = g.E; }
}

extern "C" {

int east_hip_graph_build_resident(east_hip_handle_t h, int32_t source, const int32_t *rows, int64_t n_positions,
                                  double relevance_threshold, double support_threshold, double referral_confidence, int64_t *out)
{
    return guarded([&] {
        graph_build(h, consumer_resident<GraphState>(h, source, "keyphrase graph"), rows, n_positions, relevance_threshold, support_threshold,
                    referral_confidence, out);
    });
}

int east_hip_graph_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs, const int32_t *rows,
                              int64_t n_positions, double relevance_threshold, double support_threshold, double referral_confidence,
                              int64_t *out)
{
    return guarded([&] {
        // (nothing to refuse before the upload: the rows are checked after it, the new table is the uploaded one)
        const TableRef t = consumer_upload<GraphState>(h, table, n_keyphrases, n_docs, "keyphrase graph: null or empty score table",
                                                       "the keyphrase graph's score table", [] {});
        graph_build(h, t, rows, n_positions, relevance_threshold, support_threshold, referral_confidence, out);
    });
}

int east_hip_graph_fetch(east_hip_handle_t h, int32_t *support, int32_t *kept, int32_t *edge_source, int32_t *edge_target,
                         int32_t *edge_shared)
{
    return guarded([&] {
        const GraphState &g = consumer_built<GraphState>(h, "no keyphrase graph has been built on this handle");
        const size_t eb = (size_t)g.E * 4;
        if (support && g.n) HIP_CHECK(hipMemcpyAsync(support, g.support, (size_t)g.n * 4, hipMemcpyDeviceToHost, h->stream));
        if (kept && g.M) HIP_CHECK(hipMemcpyAsync(kept, g.kept, (size_t)g.M * 4, hipMemcpyDeviceToHost, h->stream));
        if (edge_source && g.E) HIP_CHECK(hipMemcpyAsync(edge_source, g.e_src, eb, hipMemcpyDeviceToHost, h->stream));
        if (edge_target && g.E) HIP_CHECK(hipMemcpyAsync(edge_target, g.e_dst, eb, hipMemcpyDeviceToHost, h->stream));
        if (edge_shared && g.E) HIP_CHECK(hipMemcpyAsync(edge_shared, g.e_shared, eb, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

double east_hip_last_graph_ms(east_hip_handle_t h) { return consumer_ms<GraphState>(h); }

}  // extern "C"
