// bm25.h -- the Okapi BM25 relevance measure: a second score call of the cosine term index (cosine.h).
//
// Everything it reads lies in HBM once east_hip_cosine_build_texts[_v] has run: the postings of the current vector space
// in (unit, document) order, the document lengths n_d, the classes of east_hip_cosine_set_classes and the query look-up.
// It leaves its K x D table where a cosine score call leaves its own (CosState::table), so the graph, the ranking, the
// similarity and the clusters read it from EAST_HIP_GRAPH_SOURCE_COSINE as they read a cosine table.
//
//   idf_u = log1p((D - df_u + 0.5) / (df_u + 0.5))
//   w_ud  = idf_u * (c_ud * (k1 + 1)) / (c_ud + k1 * ((1 - b) + b * (n_d / avgdl))),  avgdl = (double)N / (double)D
//   score(k, d) = the sum of qtf_ku * w_ud over the distinct units of keyphrase k with a posting in d, in the order of
//                 their first occurrence in the keyphrase
//
// The library is built with -ffp-contract=off: every operation above is one IEEE rounding, in the order written.
//
// bm25_score_kernel writes every table element once and never reads the table: the accumulators of a strip of documents
// of one keyphrase live in LDS.  A group of threads -- a workgroup, or a wavefront where the collection is small -- zeroes
// them there, walks per distinct unit the part of its posting list that falls into the strip (post_doc ascends inside a
// unit: two binary searches), adds without an atomic (a document occurs once in a list) and stores the strip coalesced.
// The order of the additions of an element depends on the keyphrase alone: any grid and any strip give the same bytes.
//
// Included at the end of east_hip.hip, behind cosine.h.
#pragma once
#include "cosine.h"

#define BM25_LDS_DOCS 2048u                // accumulators a workgroup holds in LDS: 16 KiB -- eight workgroups a CU take 128 of its 160 KiB
#define BM25_WAVE_DOCS (BM25_LDS_DOCS / WAVES_PER_BLOCK)      // ... and a wavefront's share where a wavefront is the group
#define BM25_MAX_GRID (1u << 14)           // workgroups of a score launch at most: eight times what 256 CUs hold at once

// a thread per posting, streaming
__global__ __launch_bounds__(BLOCK) void bm25_weights_kernel(const u32 *__restrict__ post_doc, const u32 *__restrict__ post_unit,
                                                             const u32 *__restrict__ post_cnt, const u32 *__restrict__ unit_off,
                                                             const u32 *__restrict__ n_d, u32 P, u32 n_docs, double avgdl, double k1,
                                                             double b, double *__restrict__ w)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const u32 u = post_unit[p];
    const double df = (double)(unit_off[u + 1u] - unit_off[u]), c = (double)post_cnt[p];
    const double idf = log1p(((double)n_docs - df + 0.5) / (df + 0.5));
    w[p] = idf * (c * (k1 + 1.0)) / (c + k1 * ((1.0 - b) + b * ((double)n_d[post_doc[p]] / avgdl)));
}

// per query token: how often its unit occurs among the query's tokens where it is the first occurrence of that unit in its
// query, 0 elsewhere (cos_query_weights_kernel without the division)
__global__ __launch_bounds__(BLOCK) void bm25_query_kernel(const int32_t *__restrict__ q_ids, const u32 *__restrict__ q_off, u32 K,
                                                           u32 total, u32 n_units, double *__restrict__ qw)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    u32 lo = 0, hi = K;                                   // the query of token i: q_off[lo] <= i < q_off[lo + 1]
    while (hi - lo > 1u) { const u32 mid = (lo + hi) >> 1; if (q_off[mid] <= i) lo = mid; else hi = mid; }
    const int32_t id = q_ids[i];
    double v = 0.0;
    if (id >= 0 && (u32)id < n_units) {
        const u32 a = q_off[lo], e = q_off[lo + 1u];
        bool first = true;
        u32 c = 0;
        for (u32 x = a; x < e; x++) {
            if (q_ids[x] == id) { c++; if (x < i) first = false; }
        }
        if (first) v = (double)c;
    }
    qw[i] = v;
}

// the threads of a group have all passed: G == BLOCK the workgroup's barrier, G == WAVE the wavefront's own (its LDS
// operations complete in program order; the fences keep the compiler from moving them across)
template <int G> __device__ __forceinline__ void bm25_group_sync()
{
    if (G == BLOCK) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// A group of G threads per (keyphrase, strip of S documents), S <= BM25_LDS_DOCS / (BLOCK / G); item = k * n_strips + strip.
template <int G>
__global__ __launch_bounds__(BLOCK) void bm25_score_kernel(const int32_t *__restrict__ q_ids, const u32 *__restrict__ q_off,
                                                           const double *__restrict__ qw, u32 K, const u32 *__restrict__ unit_off,
                                                           const u32 *__restrict__ post_doc, const double *__restrict__ w, u32 n_docs,
                                                           u32 S, u32 n_strips, double *__restrict__ out)
{
    constexpr u32 GROUPS = BLOCK / G;
    __shared__ double lds[BM25_LDS_DOCS];
    double *acc = lds + (threadIdx.x / G) * (BM25_LDS_DOCS / GROUPS);
    const u32 t = threadIdx.x % G;
    const u64 items = (u64)K * n_strips;
    for (u64 item = (u64)blockIdx.x * GROUPS + threadIdx.x / G; item < items; item += (u64)gridDim.x * GROUPS) {
        const u32 k = (u32)(item / n_strips), d0 = (u32)(item % n_strips) * S, n = min(S, n_docs - d0);
        for (u32 i = t; i < n; i += G) acc[i] = 0.0;
        bm25_group_sync<G>();
        const u32 a = q_off[k], e = q_off[k + 1u];
        for (u32 i = a; i < e; i++) {
            const double q = qw[i];
            if (q == 0.0) continue;                       // (the same for every thread of the group)
            const u32 u = (u32)q_ids[i];
            u32 lo = unit_off[u], hi = unit_off[u + 1u];
            if (n_strips > 1u) {                          // the postings of the strip's documents [d0, d0 + n)
                lo += ascending_lower_bound(post_doc + lo, hi - lo, d0);
                hi = lo + ascending_lower_bound(post_doc + lo, hi - lo, d0 + n);
            }
            for (u32 p = lo + t; p < hi; p += G) acc[post_doc[p] - d0] += q * w[p];
            bm25_group_sync<G>();
        }
        double *row = out + (size_t)k * n_docs + d0;
        for (u32 i = t; i < n; i += G) row[i] = acc[i];
        bm25_group_sync<G>();                             // (the next item zeroes the accumulators)
    }
}

// ============================================================================================================ host ==
static void bm25_check_params(double k1, double b)
{
    if (!(k1 >= 0.0) || !std::isfinite(k1) || !(b >= 0.0 && b <= 1.0))
        east_throw(EAST_HIP_ERR_INVALID, "bm25: k1 must be finite and >= 0, b in [0, 1]");
}

// N = the sum of n_d, exact, summed on the device and read back once per build
static void bm25_total(Ctx &ctx, CosState &c)
{
    if (c.bm_total_valid) return;
    u32 *ex = ctx.arena->alloc<u32>((size_t)c.n_docs + 2);
    c.bm_N = c.n_docs ? device_scan_count(ctx, ArrIn{c.n_d}, c.n_docs, ex) : 0u;
    c.bm_avgdl = c.n_docs ? (double)c.bm_N / (double)c.n_docs : 0.0;
    c.bm_total_valid = true;
}

static void bm25_score(east_hip_index *h, const int32_t *q_ids, const i64 *q_offsets, i64 q_len, int32_t K, double k1, double b,
                       double *out)
{
    CosState &c = cos_built(h);
    if (K < 0 || (K > 0 && !q_offsets)) east_throw(EAST_HIP_ERR_INVALID, "bad score arguments");
    bm25_check_params(k1, b);
    if (K == 0) return;
    const char *bad_offsets = "q_offsets must start at 0 and end at q_len";
    if (q_offsets[K] != q_len || q_len < 0) east_throw(EAST_HIP_ERR_INVALID, bad_offsets);
    const std::vector<u32> off32 = ragged_offsets_u32(q_offsets, K, q_ids, bad_offsets, "q_offsets must not decrease");
    CosUnits &U = c.use_classes ? c.cls : c.terms;
    for (i64 i = 0; i < q_len; i++)
        if (q_ids[i] < -1 || (q_ids[i] >= 0 && (u32)q_ids[i] >= U.n_units))
            east_throw(EAST_HIP_ERR_INVALID, "a query id is neither -1 nor a unit of the vector space");
    c.table_valid = false;
    const u32 D = c.n_docs, total = (u32)q_len;
    const size_t b_ids = align256(((size_t)total + 1) * 4), b_off = align256(((size_t)K + 1) * 4),
                 b_qw = align256(((size_t)total + 1) * 8), table = (size_t)K * D * 8;
    c.score.ensure(b_ids + b_off + b_qw + table, "the cosine index");
    int32_t *d_ids = (int32_t *)c.score.p;
    u32 *d_off = (u32 *)(c.score.p + b_ids);
    double *d_qw = (double *)(c.score.p + b_ids + b_off), *d_out = (double *)(c.score.p + b_ids + b_off + b_qw);
    if (U.bm_weights.cap < ((size_t)U.P + 1) * 8) {
        U.bm_valid = false;
        U.bm_weights.ensure(((size_t)U.P + 1) * 8, "the cosine index");
    }
    double *w = (double *)U.bm_weights.p;
    Stats stats;
    Arena a = c.text.arena();             // (the build's first scratch, as cos_score takes it)
    Ctx ctx = handle_ctx(h, &a, &stats);
    const Knobs &knobs = ctx.knobs;
    ConsumerTimer timer(h, c);
    bm25_total(ctx, c);
    const bool make = !U.bm_valid || U.bm_k1 != k1 || U.bm_b != b;
    if (make) {
        U.bm_valid = false;
        if (U.P)
            LAUNCH(ctx, bm25_weights_kernel, ceil_div_u32(U.P, BLOCK), (const u32 *)U.post_doc, (const u32 *)U.post_unit,
                   (const u32 *)U.post_cnt, (const u32 *)U.unit_off, (const u32 *)c.n_d, U.P, D, c.bm_avgdl, k1, b, w);
    }
    if (total) HIP_CHECK(hipMemcpyAsync(d_ids, q_ids, (size_t)total * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (total)
        LAUNCH(ctx, bm25_query_kernel, ceil_div_u32(total, BLOCK), (const int32_t *)d_ids, (const u32 *)d_off, (u32)K, total,
               U.n_units, d_qw);
    // a wavefront per item where the whole collection fits a wavefront's accumulators, else a workgroup
    const bool wave = D <= BM25_WAVE_DOCS;
    const u32 cap = wave ? BM25_WAVE_DOCS : BM25_LDS_DOCS;
    const u32 S = knobs.bm25_strip > 0 ? std::min<u32>((u32)knobs.bm25_strip, cap) : cap;
    const u32 n_strips = std::max(1u, ceil_div_u32(D, S));
    const u64 items = (u64)K * n_strips;
    if (D) {
        if (wave)
            LAUNCH(ctx, bm25_score_kernel<WAVE>, (u32)std::min<u64>((items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, BM25_MAX_GRID),
                   (const int32_t *)d_ids, (const u32 *)d_off, (const double *)d_qw, (u32)K, (const u32 *)U.unit_off,
                   (const u32 *)U.post_doc, (const double *)w, D, S, n_strips, d_out);
        else
            LAUNCH(ctx, bm25_score_kernel<BLOCK>, (u32)std::min<u64>(items, BM25_MAX_GRID), (const int32_t *)d_ids,
                   (const u32 *)d_off, (const double *)d_qw, (u32)K, (const u32 *)U.unit_off, (const u32 *)U.post_doc,
                   (const double *)w, D, S, n_strips, d_out);
    }
    timer.stop();                           // (the time is the launches': the copy of the table is not in it)
    if (out && table) HIP_CHECK(hipMemcpyAsync(out, d_out, table, hipMemcpyDeviceToHost, h->stream));
    timer.finish();
    c.score_ms = c.ms;
    if (make) {
        U.bm_valid = true;
        U.bm_k1 = k1;
        U.bm_b = b;
        c.bm_made++;
    }
    c.table = d_out;
    c.table_K = (u32)K;
    c.table_valid = true;
}

extern "C" {

int east_hip_bm25_score_table(east_hip_handle_t h, const int32_t *q_ids, const int64_t *q_offsets, int64_t q_len,
                              int32_t n_keyphrases, double k1, double b, double *out)
{
    return guarded([&] { bm25_score(h, q_ids, q_offsets, q_len, n_keyphrases, k1, b, out); });
}

int east_hip_bm25_info(east_hip_handle_t h, double *out, int32_t cap)
{
    return guarded([&] {
        CosState &c = cos_built(h);
        if (!out || cap < 0) east_throw(EAST_HIP_ERR_INVALID, "bad info arguments");
        if (!c.bm_total_valid) {
            Stats stats;
            Arena a = c.text.arena();
            Ctx ctx = handle_ctx(h, &a, &stats);
            bm25_total(ctx, c);
        }
        const CosUnits &U = c.use_classes ? c.cls : c.terms;
        const double v[5] = {(double)c.bm_N, c.bm_avgdl, U.bm_valid ? U.bm_k1 : NAN, U.bm_valid ? U.bm_b : NAN, (double)c.bm_made};
        for (int i = 0; i < 5 && i < cap; i++) out[i] = v[i];
    });
}

int east_hip_debug_set_bm25_strip(int32_t documents)
{
    // documents of a strip of the score kernel at most (more than the accumulators hold is taken as what they hold); 0 or less: the default
    knobs_update([&](Knobs &k) { k.bm25_strip = documents > 0 ? documents : 0; });
    return EAST_HIP_OK;
}

}  // extern "C"
