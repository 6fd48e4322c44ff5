// score_host.h -- the host side of score.h: the resident keyphrases, the k-gram tables and the score walk.
#pragma once
#include "handle.h"
#include "score.h"

// The walk writes one fp64 per (keyphrase suffix, document); that scratch is bounded -- a table over a million
// one-line documents would need hundreds of GB -- and the documents are scored a stretch at a time.
static u32 score_doc_chunk(u32 n_q, u32 n_docs, size_t scratch_bytes)
{
    const size_t per_doc = (size_t)n_q * 8;
    const size_t fit = per_doc ? scratch_bytes / per_doc : n_docs;
    return (u32)std::min<size_t>(n_docs, std::max<size_t>(fit, 1));
}

// The score scratch for n_kp keyphrases of n_q suffixes in all, over n_docs documents scored `chunk` at a time.
static size_t keyphrase_scratch_bytes(u32 n_kp, u32 n_q, u32 n_docs, u32 chunk)
{
    return 256 + align256((size_t)n_q * 4) * 3 + align256(((size_t)n_kp + 1) * 4) * 3 + align256((size_t)n_q * chunk * 8) +
           align256((size_t)n_kp * n_docs * 8) * 2;
}

// The device half of setting keyphrases: the scratch is laid out for n_kp keyphrases of n_q suffixes, fill() queues on the
// handle's stream whatever writes q_raw (or q_code, with q_code_epoch), q_end, q_off[n_kp + 1] and -- n_blk > 0 -- q_blk[n_blk + 1]
// (score.h: score_walk_kernel, blk; n_blk == 0: a keyphrase is longer than a workgroup), from host arrays or from device
// arrays alike.  The caller waits for the stream where its sources are host memory.
template <class Fill>
static void set_keyphrases_device(east_hip_index *h, u32 n_kp, u32 n_q, u32 n_blk, const Knobs &kn, Fill fill)
{
    h->table_scored = false;
    h->kp.q_code_epoch = 0;
    h->kp.n_kp = h->kp.n_q = 0;                                  // (until the arrays are queued: a refused call leaves no keyphrases)
    const u32 chunk = score_doc_chunk(n_q, h->n_docs, kn.score_scratch_bytes);
    h->kp.buf.ensure(keyphrase_scratch_bytes(n_kp, n_q, h->n_docs, chunk), "the score scratch", h->stream);
    char *p = h->kp.buf.p + 256;                            // (the first bytes hold the probe counter of east_hip_score_probes)
    h->kp.q_raw = (u32 *)p;  p += align256((size_t)n_q * 4);
    h->kp.q_code = (u32 *)p; p += align256((size_t)n_q * 4);
    h->kp.q_end = (u32 *)p;  p += align256((size_t)n_q * 4);
    h->kp.q_off = (u32 *)p;  p += align256(((size_t)n_kp + 1) * 4);
    h->kp.group_off = (u32 *)p; p += align256(((size_t)n_kp + 1) * 4);      // synonym-expanded scoring: variants per keyphrase
    h->kp.q_blk = (u32 *)p;  p += align256(((size_t)n_kp + 1) * 4);
    h->kp.suffix = (double *)p; p += align256((size_t)n_q * chunk * 8);
    h->kp.table = (double *)p; p += align256((size_t)n_kp * h->n_docs * 8);
    h->kp.table_g = (double *)p;
    h->kp.n_blk = n_blk;
    fill();
    h->kp.n_kp = n_kp;
    h->kp.n_q = n_q;
    h->kp.score_chunk = chunk;
}

// The score walk's workgroups take whole keyphrases (score.h: score_walk_kernel, blk): consecutive keyphrases packed into
// stretches of at most BLOCK suffixes.  len(k) = the suffixes of keyphrase k.  blk comes back as the stretches' bounds
// (n_blk + 1 of them), or empty where a keyphrase is longer than a workgroup or the sums run in a kernel of their own.
template <class Len> static void pack_keyphrase_blocks(u32 n_kp, bool fused, Len len, std::vector<u32> &blk)
{
    blk.clear();
    if (!fused) return;
    blk.push_back(0);
    u32 used = 0;
    for (u32 k = 0; k < n_kp; k++) {
        const u64 l = len(k);
        if (l > BLOCK) { blk.clear(); return; }
        if (used + l > BLOCK) { blk.push_back(k); used = 0; }
        used += (u32)l;
    }
    blk.push_back(n_kp);
}

static void set_keyphrases(east_hip_index *h, const u32 *q_symbols, const i64 *q_offsets, int32_t n_kp)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
    if (n_kp < 1 || !q_symbols || !q_offsets) east_throw(EAST_HIP_ERR_INVALID, "no keyphrases");
    if (q_offsets[0] != 0) east_throw(EAST_HIP_ERR_INVALID, "q_offsets[0] must be 0");
    for (int32_t k = 0; k < n_kp; k++)
        if (q_offsets[k + 1] <= q_offsets[k])
            east_throw(EAST_HIP_ERR_INVALID, "empty keyphrase (the reference raises ZeroDivisionError, easa.py:134)");
    const i64 S = q_offsets[n_kp];
    if (S >= (i64)0x7FFFFFF0 || (i64)n_kp * h->n_docs >= ((i64)1 << 40))
        east_throw(EAST_HIP_ERR_INVALID, "keyphrase set too large");
    use_device(h);
    const u32 n_q = (u32)S;
    const Knobs kn = knobs_snapshot();
    std::vector<u32> end(n_q), off((size_t)n_kp + 1);
    for (int32_t k = 0; k < n_kp; k++) {
        off[k] = (u32)q_offsets[k];
        for (i64 i = q_offsets[k]; i < q_offsets[k + 1]; i++) end[i] = (u32)q_offsets[k + 1];
    }
    off[n_kp] = n_q;
    std::vector<u32> blk;
    pack_keyphrase_blocks((u32)n_kp, kn.score_fused, [&](u32 k) { return (u64)(q_offsets[k + 1] - q_offsets[k]); }, blk);
    set_keyphrases_device(h, (u32)n_kp, n_q, blk.empty() ? 0u : (u32)blk.size() - 1, kn, [&] {
        if (!blk.empty()) HIP_CHECK(hipMemcpyAsync(h->kp.q_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->kp.q_raw, q_symbols, (size_t)n_q * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->kp.q_end, end.data(), (size_t)n_q * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->kp.q_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

// device memory for n_docs rows of bins + 1 entries plus the fill's chunk scratch; false if it cannot be had
static bool kgram_reserve(east_hip_index *h, u64 bins, u32 n_docs)
{
    // (room for the pair layout: 8-byte entries of the last level + the table of the level above; the filled 4-byte
    // layout with its chunk scratch is smaller)
    const size_t chunks = (size_t)((bins + KGF_CHUNK - 1) / KGF_CHUNK);
    const size_t bytes = (2 * (size_t)(bins + 1) + (size_t)(bins / 2 + 2) + (size_t)(bins / 4 + 8) + 2 * chunks) * n_docs * 4 + 256;
    return h->kg.buf.try_ensure(bytes, h->stream);
}

// The tables the build marked (h->kg.marked), finished: a function of the index alone -- the marks and the document
// table, nothing of the caller's.  n_docs: the index's documents (a build in progress queues this behind its flags
// read-back, build.h, before h->n_docs is set).  false: nothing was marked, nothing queued
static bool kgram_finish_marked(east_hip_index *h, Ctx &ctx, u32 n_docs)
{
    if (h->kg.marked && h->kg.pairs) {
        // the pair layout: the last level stays as the build marked it (+ its end entries), the small table above it is filled
        const u32 bins3 = h->kg.bins / h->kg.A;
        LAUNCH(ctx, kgram_pairs_end_kernel, ceil_div_u32(n_docs, BLOCK), (const u32 *)h->doc_off, n_docs, h->kg.bins, h->kg.buf.as<u32>());
        LAUNCH(ctx, kgram_fill_kernel, n_docs, (const u32 *)h->doc_off, bins3, h->kg.kg3);
        // (levels 1 .. k - 2 as tables of their own: A + 1, A^2 + 1, ... entries per document)
        h->kg.up_stride = 0;
        u32 len = h->kg.A;
        for (int l = 1; l < h->kg.k - 1; l++) { h->kg.up_stride += len + 1; len *= h->kg.A; }
        if (h->kg.up_stride && h->kg.up)
            LAUNCH(ctx, kgram_upper_kernel, n_docs, (const u32 *)h->kg.kg3, bins3, h->kg.A, h->kg.k - 1, h->kg.up_stride, h->kg.up);
        return true;
    }
    if (h->kg.marked) {
        // the build left the bucket starts in the table: suffix minimum per document, in chunks
        const u32 bins = h->kg.bins, n_chunks = ceil_div_u32(bins, KGF_CHUNK);
        u32 *cmin = h->kg.buf.as<u32>() + (size_t)(bins + 1) * n_docs, *csuf = cmin + (size_t)n_chunks * n_docs;
        LAUNCH(ctx, kgram_chunk_min_kernel, dim3(n_chunks, n_docs), h->kg.buf.as<const u32>(), bins, n_chunks, cmin);
        LAUNCH(ctx, kgram_chunk_suffix_kernel, n_docs, (const u32 *)cmin, (const u32 *)h->doc_off, n_chunks, csuf);
        LAUNCH(ctx, kgram_chunk_fill_kernel, dim3(n_chunks, n_docs), (const u32 *)csuf, (const u32 *)h->doc_off, bins,
               n_chunks, h->kg.buf.as<u32>());
        return true;
    }
    return false;
}

// k-gram bucket tables of the current index (score.h); k = 0 when the alphabet is too wide
static void ensure_kgram(east_hip_index *h, Ctx &ctx)
{
    if (h->kg.built) return;
    if (kgram_finish_marked(h, ctx, h->n_docs)) {
        h->kg.built = true;
        return;
    }
    h->kg.k = 0;
    h->kg.pairs = false;
    h->kg.built = true;
    if (!h->use_s8 || h->n_docs > 65535) return;
    const u32 A = h->sigma_t + 2;
    int k = 0;
    u64 bins = 1;
    while (k < KGRAM_MAX_K && bins * A <= KGRAM_MAX_BINS && bins * A * 16 <= h->n / h->n_docs + 4096 &&
           (bins * A + 1) * h->n_docs * 4 <= ((u64)1 << 30)) {
        bins *= A;
        k++;
    }
    if (k == 0) return;
    const size_t bytes = (size_t)(bins + 1) * h->n_docs * 4;
    if (!kgram_reserve(h, bins, h->n_docs)) return;              // no table: plain binary search
    if ((u64)h->n / h->n_docs >= 256 * bins) {
        // long documents: every table entry by binary search on the suffix array
        LAUNCH(ctx, kgram_search_kernel, dim3(ceil_div_u32(bins + 1, BLOCK), h->n_docs), (const u32 *)h->sa,
               (const uint8_t *)h->s8, (const u32 *)h->doc_off, k, A, (u32)bins, h->kg.buf.as<u32>());
    } else {
        HIP_CHECK(hipMemsetAsync(h->kg.buf.p, 0xFF, bytes, h->stream));
        i64 longest = 0;
        for (u32 d = 0; d < h->n_docs; d++) longest = std::max(longest, h->h_doc_off[d + 1] - h->h_doc_off[d]);
        if (h->n_docs > 1)
            LAUNCH_NAMED(ctx, "kgram_mark_kernel", kgram_mark_tiled_kernel,
                         dim3(ceil_div_u32((u64)longest + 3, BLOCK * 4), h->n_docs), (const u32 *)h->lcp, (const u32 *)h->sa,
                         (const uint8_t *)h->s8, (const u32 *)h->doc_off, h->n_docs, h->n, k, A, (u32)bins, h->kg.buf.as<u32>());
        else
            LAUNCH(ctx, kgram_mark_kernel, dim3(ceil_div_u32((u64)longest, BLOCK), h->n_docs), (const u32 *)h->lcp,
                   (const u32 *)h->sa, (const uint8_t *)h->s8, (const u32 *)h->doc_off, h->n_docs, h->n, k, A, (u32)bins,
                   h->kg.buf.as<u32>());
        LAUNCH(ctx, kgram_fill_kernel, h->n_docs, (const u32 *)h->doc_off, (u32)bins, h->kg.buf.as<u32>());
    }
    h->kg.k = k;
    h->kg.A = A;
    h->kg.bins = (u32)bins;
}

#define SCORE_DIRECT_OUT_MAX ((u64)1 << 18)     // scores (2 MiB): up to here east_hip_score_resident's block is written by the kernels

// queues the score kernels; result in h->kp.table (K x D) / h->kp.suffix (D x S), and -- table_out != nullptr, device memory --
// in the caller's block as well: the kernels write every score to both
static void score_resident(east_hip_index *h, int normalized, unsigned long long *probe_count = nullptr,
                           double *suffix_host = nullptr, double *table_out = nullptr)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
    if (!h->kp.n_kp) east_throw(EAST_HIP_ERR_INVALID, "no keyphrases set");
    use_device(h);
    Ctx ctx = handle_ctx(h);
    HIP_CHECK(hipEventRecord(h->ev0, h->stream));
    ensure_kgram(h, ctx);
    if (h->kp.q_code_epoch != h->map_epoch) {               // (the same keyphrases under the same code map: q_code stands)
        LAUNCH(ctx, query_map_kernel, ceil_div_u32(h->kp.n_q, BLOCK), (const u32 *)h->kp.q_raw, h->kp.n_q,
               (const u32 *)h->code_map, (const u32 *)h->hi_bits, (const u32 *)h->hi_rank,
               h->sigma_hi ? h->sigma_t - h->sigma_hi + 1u : 0u, h->kp.q_code);
        h->kp.q_code_epoch = h->map_epoch;
    }
    KgTables kt;
    kt.kg = h->kg.buf.as<u32>(); kt.kg3 = h->kg.kg3; kt.k = h->kg.k; kt.pairs = h->kg.k > 0 && h->kg.pairs; kt.A = h->kg.A; kt.bins = h->kg.bins;
    if (kt.pairs && h->kg.up_stride && h->kg.up) {
        kt.up = h->kg.up;
        kt.up_stride = h->kg.up_stride;
        static const bool up_lds_off = getenv("EAST_HIP_SCORE_UP_LDS") && atoi(getenv("EAST_HIP_SCORE_UP_LDS")) == 0;   // (A/B timing)
        kt.up_lds = !up_lds_off && h->kg.up_stride <= KG_UP_LDS_WORDS;
    }
    if (kt.k > 0) kt.finish();
    kt.endgame = ctx.knobs.score_endgame;
    // whole keyphrases per workgroup, summed in the walk (no per-suffix results unless the caller wants them: then the
    // documents go a stretch at a time, as far as the scratch reaches); otherwise per-suffix results + the reduction kernel
    const bool fused = h->kp.n_blk > 0;
    u32 chunk = h->kp.score_chunk;
    if (fused && !suffix_host) {
        // (no scratch to bound the stretch -- the grid does: a launch of at most Knobs::score_grid_blocks workgroups, far below
        // HIP's limit of 2^32 threads per grid dimension; many short documents times thousands of keyphrases go a stretch
        // of documents at a time, a multiple of 8 for the XCD-aware order)
        const u64 fit = ctx.knobs.score_grid_blocks / h->kp.n_blk;
        chunk = (u32)std::min<u64>(h->n_docs, fit >= 8 ? fit & ~(u64)7 : std::max<u64>(fit, 1));
    }
    for (u32 first = 0; first < h->n_docs; first += chunk) {
        const u32 count = std::min(chunk, h->n_docs - first);
        const int xcd_order = count >= 64;                // see score_walk_kernel
        const u32 per_doc = fused ? h->kp.n_blk : ceil_div_u32(h->kp.n_q, BLOCK);
        const u64 walk_grid64 = (u64)(xcd_order ? 8u * ceil_div_u32(count, 8) : count) * per_doc;
        if (walk_grid64 >= ((u64)1 << 24)) east_throw(EAST_HIP_ERR_INVALID, "keyphrase set too large for one score launch");
        const u32 walk_grid = (u32)walk_grid64;
        double *suffix = fused && !suffix_host ? (double *)nullptr : h->kp.suffix;
        const u32 *blk = fused ? (const u32 *)h->kp.q_blk : (const u32 *)nullptr;
        if (h->use_s8)
            LAUNCH_NAMED(ctx, "score_walk_kernel", (score_walk_kernel<uint8_t>), walk_grid, (const uint8_t *)h->s8,
                         (const u32 *)h->sa, (const u32 *)h->doc_off, (const u32 *)h->n_strings, h->n_docs,
                         (const u32 *)h->kp.q_code, (const u32 *)h->kp.q_end, h->kp.n_q, normalized, kt, xcd_order, first, count, suffix,
                         probe_count, blk, h->kp.n_blk, (const u32 *)h->kp.q_off, h->kp.table, fused ? table_out : (double *)nullptr);
        else
            LAUNCH_NAMED(ctx, "score_walk_kernel", (score_walk_kernel<u32>), walk_grid, (const u32 *)h->s,
                         (const u32 *)h->sa, (const u32 *)h->doc_off, (const u32 *)h->n_strings, h->n_docs,
                         (const u32 *)h->kp.q_code, (const u32 *)h->kp.q_end, h->kp.n_q, normalized, kt, xcd_order, first, count, suffix,
                         probe_count, blk, h->kp.n_blk, (const u32 *)h->kp.q_off, h->kp.table, fused ? table_out : (double *)nullptr);
        if (!fused)
            LAUNCH(ctx, score_reduce_kernel, ceil_div_u32((u64)h->kp.n_kp * count, BLOCK), (const double *)h->kp.suffix,
                   (const u32 *)h->kp.q_off, h->kp.n_kp, h->n_docs, h->kp.n_q, first, count, h->kp.table, table_out);
        if (suffix_host)                                  // the per-suffix results of this stretch of documents (D x S, row-major)
            HIP_CHECK(hipMemcpyAsync(suffix_host + (size_t)first * h->kp.n_q, h->kp.suffix, (size_t)count * h->kp.n_q * 8,
                                     hipMemcpyDeviceToHost, h->stream));
    }
    HIP_CHECK(hipEventRecord(h->ev1, h->stream));
    h->table_scored = true;
}
