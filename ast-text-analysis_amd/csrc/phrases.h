// phrases.h -- keyphrase candidates out of the indexed texts themselves: the repeated phrases of one to eight words of the
// cosine term index's collection, counted exactly, the redundant ones removed, the rest ranked (include/east_hip.h,
// "Phrase extraction"; `east keyphrases extract`).
//
// The index keeps the token sequence (cosine.h: tok_term, tok_doc -- the term of every kept token, COS_NONE for a stopword,
// and its document).  The n-grams are NAMED level by level, the way prefix doubling names suffixes; nothing is hashed:
//
//   level 1: the positions whose token is a word; key = the term id
//   level n: the positions whose (n-1)-gram survived and whose n-th token is a word of the same text;
//            key = id_{n-1}[j] << bit_width(V - 1) | tok_term[j + n - 1], value = j, compacted by a scan
//   --stable radix sort over exactly those bits (the positions went in ascending)--> runs of equal keys = the distinct
//   n-grams; inside a run the positions ascend: the head is the first occurrence, and the documents never decrease
//   --per run: count = its length, texts = 1 + the steps of tok_doc inside it (a flag scan), first = the head's position;
//     a run SURVIVES with count >= min_count (no extension of a phrase is more frequent than the phrase) and gets a dense
//     id, scattered to its members' positions (id_n, COS_NONE elsewhere)
//   --closedness: the head j of a surviving run R of level n marks the (n-1)-grams at j and at j + 1 OPEN when their count
//     is R's -- a plain store of 1; there is no atomic in this file
//   --emission of level n - 1 (its marks are final now): a flag per position that is the head of a surviving, closed run
//     with texts >= min_texts, a scan over the positions, the candidate (n, count, texts, first) to its slot: the list is
//     in (n, first) order
//   candidates --one stable sort by max_score - count * n--> the contract's order; the first N are gathered; their text by
//   count, scan and fill, a wavefront a phrase (as cos_term_text_kernel).
//
// A level is 5 launches of this file (keys, runs, stats + id scatter + marks, emission flags, emission), one fill, the
// sort's passes and 5 scans, and 2 read-backs: the survivors; the candidates of the level below with the next level's
// domain.  Level max_words + 1 is never built; a level without a survivor ends the build.  The naming half of a level --
// keys, sort, runs, survivors, ids -- is phr_level_step, which the shingle overlap (overlap.h) runs too.
//
// Memory: 112 bytes a kept token of work arrays, 16 bytes a candidate, the result.  Buffers of this consumer's own.
#pragma once
#include "consumer.h"
#include "cosine.h"
#include "radix_sort.h"
#include "scan.h"

#define PHR_MAX_WORDS 8

// ---- the domain of a level ------------------------------------------------------------------------------------------------
// 1 where the n-gram at position j is to be named: its (n-1)-gram survived (id_prev; level 1: the token is a word), its
// last token lies in the same text and is a word.  An input of the scan: it reads rows, no gather.
struct PhrDomainIn {
    const u32 *tok_term, *tok_doc, *id_prev;
    u32 n, T;
    __device__ __forceinline__ u32 operator()(u32 j) const
    {
        if (n == 1u) return tok_term[j] != COS_NONE ? 1u : 0u;
        const u32 e = j + n - 1u;
        if (e >= T) return 0u;
        return id_prev[j] != COS_NONE && tok_doc[e] == tok_doc[j] && tok_term[e] != COS_NONE ? 1u : 0u;
    }
};

// dex = exclusive scan of the domain: every position of the domain to its slot, in ascending order
__global__ __launch_bounds__(BLOCK) void phr_keys_kernel(PhrDomainIn dom, const u32 *__restrict__ dex, int term_bits,
                                                         u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= dom.T || !dom(j)) return;
    const u32 slot = dex[j];
    keys[slot] = dom.n == 1u ? (u64)dom.tok_term[j] : ((u64)dom.id_prev[j] << term_bits) | dom.tok_term[j + dom.n - 1u];
    vals[slot] = j;
}

// ---- runs of equal keys ---------------------------------------------------------------------------------------------------
// ri = inclusive scan of the run heads over the sorted keys.  Per run its first sorted position (and n behind the last
// run); per sorted position whether the document steps from the member in front of it inside the run.
__global__ __launch_bounds__(BLOCK) void phr_runs_kernel(const u32 *__restrict__ ri, const u32 *__restrict__ svals,
                                                         const u32 *__restrict__ tok_doc, u32 n, u32 *__restrict__ run_start,
                                                         u32 *__restrict__ tflag)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r1 = ri[i];
    const bool head = i == 0u || ri[i - 1u] != r1;
    if (head) run_start[r1 - 1u] = i;
    if (i + 1u == n) run_start[r1] = n;
    tflag[i] = !head && tok_doc[svals[i]] != tok_doc[svals[i - 1u]] ? 1u : 0u;
}

// 1 at the head of a run that survives (count >= min_count): its exclusive scan numbers the survivors
struct PhrSurvIn {
    const u32 *ri, *run_start;
    u32 min_count;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        const u32 r1 = ri[i];
        if (i > 0u && ri[i - 1u] == r1) return 0u;
        return run_start[r1] - i >= min_count ? 1u : 0u;
    }
};

// the statistics of a level's surviving n-grams (by dense id) and, of the level below, their counts and open marks
struct PhrLevel {
    u32 *id, *count, *texts, *first, *open;
};

// One pass over the sorted pairs: every member of a surviving run takes the run's id to its position; the head writes the
// run's statistics and marks the two (n-1)-grams it extends open where their count is its own.  sx = the survivors' scan,
// tx = the exclusive scan of tflag (with its total behind).  below.id == nullptr: level 1.
__global__ __launch_bounds__(BLOCK) void phr_stats_kernel(const u32 *__restrict__ ri, const u32 *__restrict__ run_start,
                                                          const u32 *__restrict__ sx, const u32 *__restrict__ tx,
                                                          const u32 *__restrict__ svals, u32 n, u32 min_count, PhrLevel cur,
                                                          PhrLevel below, u32 n_below)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r = ri[i] - 1u, a = run_start[r], e = run_start[r + 1u], cnt = e - a;
    if (cnt < min_count) return;
    const u32 id = sx[a], j = svals[i];
    cur.id[j] = id;
    if (i != a) return;
    cur.count[id] = cnt;
    cur.texts[id] = 1u + tx[e] - tx[a];
    cur.first[id] = j;
    cur.open[id] = 0u;
    if (!below.id) return;
    const u32 p = below.id[j], q = below.id[j + 1u];     // (both survived: they occur at least cnt times)
    if (p < n_below && below.count[p] == cnt) below.open[p] = 1u;
    if (q < n_below && below.count[q] == cnt) below.open[q] = 1u;
}

// ---- emission -------------------------------------------------------------------------------------------------------------
// eflag[j] = position j is the head of a surviving, closed n-gram with texts >= min_texts (a gather: an array)
__global__ __launch_bounds__(BLOCK) void phr_emit_flags_kernel(PhrLevel lv, u32 T, u32 min_texts, u32 *__restrict__ eflag)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= T) return;
    const u32 id = lv.id[j];
    eflag[j] = id != COS_NONE && lv.first[id] == j && !lv.open[id] && lv.texts[id] >= min_texts ? 1u : 0u;
}

// a candidate: (words, count, texts, first); eex = exclusive scan of eflag, base = the candidates of the levels below
__global__ __launch_bounds__(BLOCK) void phr_emit_kernel(PhrLevel lv, const u32 *__restrict__ eflag, const u32 *__restrict__ eex, u32 T,
                                                         u32 words, u32 base, uint4 *__restrict__ cand)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= T || !eflag[j]) return;
    const u32 id = lv.id[j];
    cand[base + eex[j]] = make_uint4(words, lv.count[id], lv.texts[id], j);
}

// ---- order, cut, text -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void phr_score_keys_kernel(const uint4 *__restrict__ cand, u32 C, u64 max_score, u64 *__restrict__ keys,
                                                               u32 *__restrict__ vals)
{
    const u32 c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= C) return;
    keys[c] = max_score - (u64)cand[c].x * cand[c].y;
    vals[c] = c;
}

struct PhrOut {
    int32_t *words, *count, *texts, *first, *first_text;
    u32 *tlen;
};

// the r-th phrase of the order; tlen = the code points of its text (the words' and a space between two)
__global__ __launch_bounds__(BLOCK) void phr_gather_kernel(const u32 *__restrict__ order, const uint4 *__restrict__ cand, u32 R,
                                                           const u32 *__restrict__ tok_term, const u32 *__restrict__ tok_doc,
                                                           const u32 *__restrict__ term_len, PhrOut o)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= R) return;
    const uint4 c = cand[order ? order[r] : r];
    o.words[r] = (int32_t)c.x;
    o.count[r] = (int32_t)c.y;
    o.texts[r] = (int32_t)c.z;
    o.first[r] = (int32_t)c.w;
    o.first_text[r] = (int32_t)tok_doc[c.w];
    u32 len = c.x - 1u;
    for (u32 w = 0; w < c.x; w++) len += term_len[tok_term[c.w + w]];
    o.tlen[r] = len;
}

// a wavefront per phrase: its term ids, and its words' code points joined by one U+0020
__global__ __launch_bounds__(BLOCK) void phr_text_kernel(const int32_t *__restrict__ words, const int32_t *__restrict__ first, u32 R,
                                                         const u32 *__restrict__ ids_off, const u32 *__restrict__ text_off,
                                                         const u32 *__restrict__ tok_term, const u32 *__restrict__ term_off,
                                                         const u32 *__restrict__ term_len, const u32 *__restrict__ tcp,
                                                         int32_t *__restrict__ term_ids, u32 *__restrict__ text)
{
    const u32 r = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (r >= R) return;
    const u32 nw = (u32)words[r], j = (u32)first[r], lane = lane_id();
    if (lane < nw) term_ids[ids_off[r] + lane] = (int32_t)tok_term[j + lane];
    u32 pos = text_off[r];
    for (u32 w = 0; w < nw; w++) {
        const u32 t = tok_term[j + w], len = term_len[t];
        const u32 *s = tcp + term_off[t];
        for (u32 i = lane; i < len; i += WAVE) text[pos + i] = s[i];
        pos += len;
        if (w + 1u < nw) {
            if (lane == 0u) text[pos] = 0x20u;
            pos++;
        }
    }
}

// ============================================================================================================ host ==
struct PhraseState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_PHR;
    DevBuf work, cand, out, text;           // the levels' arrays and the sorts; the candidates; the result's rows; its ids and text
    u32 returned = 0, n_ids = 0, n_cps = 0;
    i64 candidates = 0;
    int levels = 0;
    i64 domain[PHR_MAX_WORDS] = {0}, survivors[PHR_MAX_WORDS] = {0};
    PhrOut o = {};
    u32 *ids_off = nullptr, *text_off = nullptr, *text_cps = nullptr;
    int32_t *term_ids = nullptr;
    PhraseState()
    {
        bufs = {&work, &cand, &out, &text};
        keep_bytes = (size_t)64 << 20;
    }
    void clear() override
    {
        returned = n_ids = n_cps = 0;
        candidates = 0;
        levels = 0;
        for (int i = 0; i < PHR_MAX_WORDS; i++) domain[i] = survivors[i] = 0;
    }
};

struct PhraseParams {
    int32_t min_words, max_words, min_count, min_texts;
    i64 N;
};

// room for `bytes` with the first `used` bytes kept (the candidates of the levels below)
static void phr_grow_keep(DevBuf &b, size_t bytes, size_t used, hipStream_t stream)
{
    if (bytes <= b.cap) return;
    const size_t want = std::max(bytes, b.cap * 2);
    void *q = nullptr;
    HIP_CHECK(hipStreamSynchronize(stream));
    if (hipMalloc(&q, want) != hipSuccess) {
        (void)hipGetLastError();
        east_throw(EAST_HIP_ERR_OOM, "hipMalloc of " + std::to_string(want) + " bytes for the phrase candidates failed");
    }
    if (used) {
        HIP_CHECK(hipMemcpyAsync(q, b.p, used, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    b.release();
    b.p = (char *)q;
    b.cap = want;
}

static inline int phr_bit_width64(u64 x) { int b = 0; while (x) { b++; x >>= 1; } return b; }

// ---- one level ------------------------------------------------------------------------------------------------------------
// The arrays a level works in (the caller's arena): the domain's scan, the sort's two pairs, and over the sorted pairs the
// run numbers, the runs' starts, the text steps and their scan, the survivors' scan.
struct PhrWork {
    u32 *dex = nullptr;
    SortBufs<u64> sb = {};
    u32 *ri = nullptr, *run_start = nullptr, *tflag = nullptr, *tx = nullptr, *sx = nullptr;
    int term_bits = 0;
};

struct PhrStep {
    u32 surv;       // the runs that survive (0 with stats == false)
    int r;          // the sort's buffers that hold the sorted pairs
};

// Level din.n of the naming, shared by the phrases and the shingle overlap (overlap.h): W.dex = the exclusive scan of the
// domain `din` with `dom` positions in it; n_below = the survivors of the level below.  Keys, the stable sort over exactly
// the needed bits, the runs and their text steps (ri, run_start, tflag, tx).  stats: the survivors with min_count get
// their dense ids at their members' positions (L.id, COS_NONE elsewhere) and their statistics, and mark the level below
// (B; B.id == nullptr: level 1); without, the level is named only and L is not touched.
static PhrStep phr_level_step(Ctx &ctx, const PhrDomainIn &din, u32 dom, u32 n_below, u32 min_count, PhrWork &W, PhrLevel L, PhrLevel B,
                              bool stats)
{
    const u32 T = din.T, n = din.n;
    PhrStep st{0u, 0};
    if (stats && T) HIP_CHECK(hipMemsetAsync(L.id, 0xFF, (size_t)T * 4, ctx.stream));
    if (!dom) return st;
    LAUNCH(ctx, phr_keys_kernel, ceil_div_u32(T, BLOCK), din, (const u32 *)W.dex, W.term_bits, W.sb.keys[0], W.sb.vals[0]);
    const int bits = std::max(1, n == 1u ? W.term_bits : bit_width_u32(n_below - 1u) + W.term_bits);
    st.r = radix_sort_pairs<u64>(ctx, W.sb, dom, bits);
    const u32 *sv = W.sb.vals[st.r];
    const u32 grid_D = ceil_div_u32(dom, BLOCK);
    device_scan<RunHeadIn<u64>, true>(ctx, RunHeadIn<u64>{W.sb.keys[st.r], 0}, dom, W.ri);
    LAUNCH(ctx, phr_runs_kernel, grid_D, (const u32 *)W.ri, sv, din.tok_doc, dom, W.run_start, W.tflag);
    device_scan_with_total(ctx, ArrIn{W.tflag}, dom, W.tx);
    if (!stats) return st;
    st.surv = device_scan_count(ctx, PhrSurvIn{W.ri, W.run_start, min_count}, dom, W.sx);
    if (st.surv)
        LAUNCH(ctx, phr_stats_kernel, grid_D, (const u32 *)W.ri, (const u32 *)W.run_start, (const u32 *)W.sx, (const u32 *)W.tx, sv, dom,
               min_count, L, B, n_below);
    return st;
}

static void phrases_check(const PhraseParams &pp, const i64 *out)
{
    if (pp.max_words < 1 || pp.max_words > PHR_MAX_WORDS) east_throw(EAST_HIP_ERR_INVALID, "phrases: max_words must lie in 1 .. 8");
    if (pp.min_words < 1 || pp.min_words > pp.max_words) east_throw(EAST_HIP_ERR_INVALID, "phrases: min_words must lie in 1 .. max_words");
    if (pp.min_count < 1) east_throw(EAST_HIP_ERR_INVALID, "phrases: min_count must be at least 1");
    if (pp.min_texts < 1) east_throw(EAST_HIP_ERR_INVALID, "phrases: min_texts must be at least 1");
    if (pp.N < 0) east_throw(EAST_HIP_ERR_INVALID, "phrases: N must not be negative (0 keeps every candidate)");
    if (!out) east_throw(EAST_HIP_ERR_INVALID, "phrases: out is null");
}

static void phrases_build(east_hip_index *h, const PhraseParams &pp, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    phrases_check(pp, out);
    CosState *cp = consumer_peek<CosState>(h);
    if (!cp || !cp->valid) east_throw(EAST_HIP_ERR_NOT_BUILT, "phrases: no cosine index has been built on this handle");
    use_device(h);
    const CosState &c = *cp;
    PhraseState &g = consumer_begin<PhraseState>(h);        // (every refusal lies above: an earlier result stays until here)
    g.clear();
    const u32 T = c.n_kept, V = c.V;
    const u32 *tok_term = c.tok_term, *tok_doc = c.tok_doc;
    const size_t K1 = (size_t)T + 2;
    // (a kept token: seven arrays over the positions, the sort's two pairs of 12 bytes, five arrays over the sorted pairs,
    // two levels of four statistics -- 104 bytes -- and 8 to spare for the sort's and the scans' scratch)
    g.work.ensure(K1 * 112 + ((size_t)4 << 20), "the phrases", h->stream);
    Arena a = g.work.arena();
    Stats stats;
    Ctx ctx = handle_ctx(h, &a, &stats);
    ConsumerTimer timer(h, g);
    PhrLevel lv[2];
    for (PhrLevel &l : lv) {
        l.id = a.alloc<u32>(K1);
        l.count = a.alloc<u32>(K1);
        l.texts = a.alloc<u32>(K1);
        l.first = a.alloc<u32>(K1);
        l.open = a.alloc<u32>(K1);
    }
    u32 *dex = a.alloc<u32>(K1), *eflag[2], *eex[2];
    for (int k = 0; k < 2; k++) { eflag[k] = a.alloc<u32>(K1); eex[k] = a.alloc<u32>(K1); }
    PhrWork W;
    W.dex = dex;
    W.sb = sort_bufs_alloc<u64>(a, K1);
    W.ri = a.alloc<u32>(K1);
    W.run_start = a.alloc<u32>(K1);
    W.tflag = a.alloc<u32>(K1);
    W.tx = a.alloc<u32>(K1);
    W.sx = a.alloc<u32>(K1);
    W.term_bits = bit_width_u32(V ? V - 1u : 0u);
    const u32 grid_T = ceil_div_u32(T, BLOCK);

    int cur = 0;
    u32 dom = 0, n_below = 0;
    u64 C = 0;
    PhrDomainIn din{tok_term, tok_doc, nullptr, 1u, T};
    if (T) dom = device_scan_count(ctx, din, T, dex);
    for (u32 n = 1; n <= (u32)pp.max_words; n++) {
        const PhrLevel L = lv[cur], B = n > 1u ? lv[cur ^ 1] : PhrLevel{nullptr, nullptr, nullptr, nullptr, nullptr};
        g.levels = (int)n;
        g.domain[n - 1] = dom;
        const u32 surv = phr_level_step(ctx, din, dom, n_below, (u32)pp.min_count, W, L, B, true).surv;
        g.survivors[n - 1] = surv;
        const bool last = n == (u32)pp.max_words || surv == 0;
        // the level below is final now (its marks are in); this level is where nothing follows it
        const bool emit_below = n > 1u && n - 1u >= (u32)pp.min_words, emit_cur = last && surv && n >= (u32)pp.min_words;
        if (emit_below) {
            LAUNCH(ctx, phr_emit_flags_kernel, grid_T, B, T, (u32)pp.min_texts, eflag[0]);
            device_scan_with_total(ctx, ArrIn{eflag[0]}, T, eex[0]);
        }
        if (emit_cur) {
            LAUNCH(ctx, phr_emit_flags_kernel, grid_T, L, T, (u32)pp.min_texts, eflag[1]);
            device_scan_with_total(ctx, ArrIn{eflag[1]}, T, eex[1]);
        }
        if (!last) {
            din = PhrDomainIn{tok_term, tok_doc, L.id, n + 1u, T};
            device_scan_with_total(ctx, din, T, dex);
        }
        u32 c_below = 0, c_cur = 0, dom_next = 0;
        if (emit_below || emit_cur || !last) {
            if (emit_below) HIP_CHECK(hipMemcpyAsync(&c_below, eex[0] + T, 4, hipMemcpyDeviceToHost, h->stream));
            if (emit_cur) HIP_CHECK(hipMemcpyAsync(&c_cur, eex[1] + T, 4, hipMemcpyDeviceToHost, h->stream));
            if (!last) HIP_CHECK(hipMemcpyAsync(&dom_next, dex + T, 4, hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        if ((u64)C + c_below + c_cur >= (u64)0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "phrases: 2^31 - 16 candidates or more");
        if (c_below + c_cur) phr_grow_keep(g.cand, (size_t)(C + c_below + c_cur) * 16, (size_t)C * 16, h->stream);
        if (c_below) LAUNCH(ctx, phr_emit_kernel, grid_T, B, (const u32 *)eflag[0], (const u32 *)eex[0], T, n - 1u, (u32)C, g.cand.as<uint4>());
        C += c_below;
        if (c_cur) LAUNCH(ctx, phr_emit_kernel, grid_T, L, (const u32 *)eflag[1], (const u32 *)eex[1], T, n, (u32)C, g.cand.as<uint4>());
        C += c_cur;
        if (last) break;
        n_below = surv;
        dom = dom_next;
        cur ^= 1;
    }

    // ---- the order: score descending; the stable sort keeps (words, first) among equal scores
    const u32 R = pp.N > 0 ? (u32)std::min<u64>((u64)pp.N, C) : (u32)C;
    const u32 *order = nullptr;
    Arena a2;
    if (C > 1 && R) {
        HIP_CHECK(hipStreamSynchronize(h->stream));           // (the level arrays are done with)
        g.work.ensure(((size_t)C + 2) * 28 + ((size_t)4 << 20), "the phrases", h->stream);
        a2 = g.work.arena();
        ctx.arena = &a2;
        SortBufs<u64> cs = sort_bufs_alloc<u64>(a2, (size_t)C + 1);
        const u64 max_score = (u64)T * (u64)pp.max_words;     // (count <= T, words <= max_words)
        LAUNCH(ctx, phr_score_keys_kernel, ceil_div_u32(C, BLOCK), (const uint4 *)g.cand.as<uint4>(), (u32)C, max_score, cs.keys[0], cs.vals[0]);
        const int r = radix_sort_pairs<u64>(ctx, cs, (u32)C, std::max(1, phr_bit_width64(max_score)));
        order = cs.vals[r];
    }
    // ---- the first R: rows, then ids and text by count, scan and fill
    const size_t R1 = (size_t)R + 2;
    g.out.ensure(R1 * 32 + 16 * 256, "the phrases", h->stream);
    Arena ao = g.out.arena();
    g.o.words = ao.alloc<int32_t>(R1);
    g.o.count = ao.alloc<int32_t>(R1);
    g.o.texts = ao.alloc<int32_t>(R1);
    g.o.first = ao.alloc<int32_t>(R1);
    g.o.first_text = ao.alloc<int32_t>(R1);
    g.o.tlen = ao.alloc<u32>(R1);
    g.ids_off = ao.alloc<u32>(R1);
    g.text_off = ao.alloc<u32>(R1);
    u32 n_ids = 0, n_cps = 0;
    if (R) {
        LAUNCH(ctx, phr_gather_kernel, ceil_div_u32(R, BLOCK), order, (const uint4 *)g.cand.as<uint4>(), R, tok_term, tok_doc,
               (const u32 *)c.term_len, g.o);
        Arena as = g.work.arena();                            // (the scans' scratch: behind the candidate sort, which is queued)
        if (order) as = a2;
        ctx.arena = &as;
        device_scan_with_total(ctx, ArrIn{(const u32 *)g.o.words}, R, g.ids_off);
        device_scan_with_total(ctx, ArrIn{(const u32 *)g.o.tlen}, R, g.text_off);
        device_read_words(ctx, {{&n_ids, g.ids_off + R}, {&n_cps, g.text_off + R}});
    } else {
        HIP_CHECK(hipMemsetAsync(g.ids_off, 0, 4, h->stream));
        HIP_CHECK(hipMemsetAsync(g.text_off, 0, 4, h->stream));
    }
    g.text.ensure(align256(((size_t)n_ids + 1) * 4) + align256(((size_t)n_cps + 1) * 4) + 256, "the phrases", h->stream);
    Arena at = g.text.arena();
    g.term_ids = at.alloc<int32_t>((size_t)n_ids + 1);
    g.text_cps = at.alloc<u32>((size_t)n_cps + 1);
    if (R)
        LAUNCH(ctx, phr_text_kernel, ceil_div_u32(R, WAVES_PER_BLOCK), (const int32_t *)g.o.words, (const int32_t *)g.o.first, R,
               (const u32 *)g.ids_off, (const u32 *)g.text_off, tok_term, (const u32 *)c.term_off, (const u32 *)c.term_len,
               (const u32 *)c.tcp, g.term_ids, g.text_cps);
    timer.finish();
    g.returned = R;
    g.candidates = (i64)C;
    g.n_ids = n_ids;
    g.n_cps = n_cps;
    g.valid = true;
    out[0] = R;
    out[1] = (i64)C;
    out[2] = n_cps;
    out[3] = g.levels;
}

static void phrases_fetch(east_hip_index *h, int32_t *words, int32_t *count, int32_t *texts, int32_t *first, int32_t *first_text,
                          int32_t *term_ids, i64 *text_off, u32 *text)
{
    PhraseState &g = consumer_built<PhraseState>(h, "no phrases have been extracted on this handle");
    const size_t R = g.returned;
    const struct { int32_t *dst; const int32_t *src; } rows[5] = {
        {words, g.o.words}, {count, g.o.count}, {texts, g.o.texts}, {first, g.o.first}, {first_text, g.o.first_text}};
    for (const auto &r : rows)
        if (r.dst && R) HIP_CHECK(hipMemcpyAsync(r.dst, r.src, R * 4, hipMemcpyDeviceToHost, h->stream));
    if (term_ids && g.n_ids) HIP_CHECK(hipMemcpyAsync(term_ids, g.term_ids, (size_t)g.n_ids * 4, hipMemcpyDeviceToHost, h->stream));
    if (text && g.n_cps) HIP_CHECK(hipMemcpyAsync(text, g.text_cps, (size_t)g.n_cps * 4, hipMemcpyDeviceToHost, h->stream));
    std::vector<u32> off;
    if (text_off) {
        off.resize(R + 1);
        HIP_CHECK(hipMemcpyAsync(off.data(), g.text_off, (R + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (text_off)
        for (size_t r = 0; r <= R; r++) text_off[r] = off[r];
}

extern "C" {

int east_hip_phrases_build(east_hip_handle_t h, int32_t min_words, int32_t max_words, int32_t min_count, int32_t min_texts, int64_t N,
                           int64_t *out)
{
    return guarded([&] { phrases_build(h, PhraseParams{min_words, max_words, min_count, min_texts, N}, out); });
}

int east_hip_phrases_fetch(east_hip_handle_t h, int32_t *words, int32_t *count, int32_t *texts, int32_t *first, int32_t *first_text,
                           int32_t *term_ids, int64_t *text_off, uint32_t *text)
{
    return guarded([&] { phrases_fetch(h, words, count, texts, first, first_text, term_ids, text_off, text); });
}

int east_hip_phrases_levels(east_hip_handle_t h, int64_t *domain, int64_t *survivors)
{
    return guarded([&] {
        const PhraseState &g = consumer_built<PhraseState>(h, "no phrases have been extracted on this handle");
        for (int i = 0; i < PHR_MAX_WORDS; i++) {
            if (domain) domain[i] = g.domain[i];
            if (survivors) survivors[i] = g.survivors[i];
        }
    });
}

double east_hip_last_phrases_ms(east_hip_handle_t h) { return consumer_ms<PhraseState>(h); }

}  // extern "C"
