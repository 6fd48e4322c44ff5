// passages.h -- the shared passages of pairs of indexed texts: for an ordered pair (a, b) the maximal runs of shingle
// positions of a whose w-word shingle occurs in b, ranked (include/east_hip.h, "Shared passages"; `east texts passages`;
// DESIGN.md 21).  Integers only; nothing floating point and no atomic in this file.
//
//   tok_term, tok_doc --ovl_names_postings (overlap.h): levels 1 .. w, the shared runs as dense units, their postings-->
//     pos_unit[T] = the unit of the shingle at every position (COS_NONE outside a shared run or outside the domain);
//     p_doc[P], p_pos[P] = the postings in (unit, text) order, p_pos the smallest position of the unit in that text;
//     unit_off[U + 1]; text_start[D + 1]
//   pairs --a scan over ceil(len_a / 64)--> row_off: a pair's ROW is one bit a position of a, in 64-bit words of its own
//   --pas_match_kernel: a wavefront a word, a lane a position, one ballot, one 8-byte store--> the bit words
//   --heads and tails of the runs by shifts with the neighbouring word of the SAME row, three popcount scans--> the shared
//     starts and the covered words per pair (differences at the row bounds), and a number for every run: the k-th head and
//     the k-th tail are one passage, words = tail - head + w; nobody walks a run
//   --a scan over words >= min_words, ONE stable radix sort by pair << bits | (T + w - words)--> the contract's order; the
//     place inside the pair is the rank minus the pair's first rank, per_pair cuts there; a scan over the pairs' returned
//     counts gives pair_off; `at` = p_pos of the posting (unit at start, text b)
//
// Membership, "does b hold unit u", has two routes behind east_hip_debug_set_passages_route, each the other's differential
// partner: 1 searches b in the unit's own ascending text list p_doc[unit_off[u] .. unit_off[u + 1]); 2 searches u in b's
// ascending unit list du[doc_off[b] .. doc_off[b + 1]) -- the overlap's operands, one more stable sort by text.
//
// Memory: 128 bytes a kept token of work arrays while the levels run; 4 bytes a position and 12 a posting that stay (28 a
// posting more on route 2); 36 bytes a pair; 24 bytes a bit word; 16 bytes a run and 24 a passage that passes the filter;
// 12 a passage returned.  Buffers of this consumer's own: a build disturbs neither the overlap matrix nor the phrases.
#pragma once
#include "consumer.h"
#include "cosine.h"
#include "overlap.h"
#include "phrases.h"

#define PAS_DEFAULT_ROUTE 1                        // what route 0 means ("Measured")
#define PAS_MAX_PAIRS ((i64)1 << 24)
#define PAS_MAX_BIT_WORDS (1u << 25)               // below 2^31 bits over all rows: every count of them fits 32 bits
#define PAS_MATCH_GRID 16384u                      // workgroups of the match kernel at most: a wavefront then takes several words

// ---- the index: units and postings by position ------------------------------------------------------------------------------
// Over the sorted pairs of level w (as ovl_postings_kernel): every member of a SHARED run takes the run's unit to its
// position (pos_unit: 0xFF bytes before); a posting takes its position to its slot.
__global__ __launch_bounds__(BLOCK) void pas_units_kernel(OvlPostIn post, const u32 *__restrict__ ux, const u32 *__restrict__ px,
                                                          const u32 *__restrict__ svals, u32 n, u32 *__restrict__ pos_unit,
                                                          u32 *__restrict__ p_pos)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r = post.ri[i] - 1u, a = post.run_start[r], e = post.run_start[r + 1u];
    if (post.tx[e] == post.tx[a]) return;                   // (one text holds the whole run)
    const u32 j = svals[i];
    pos_unit[j] = ux[a];
    if (i == a || post.tflag[i]) p_pos[px[i]] = j;
}

// ---- rows -------------------------------------------------------------------------------------------------------------------
struct PasRowWordsIn {      // the 64-bit words of a pair's row: an input of the scan
    const u32 *pair_a, *text_start;
    __device__ __forceinline__ u32 operator()(u32 p) const
    {
        const u32 a = pair_a[p];
        return (text_start[a + 1u] - text_start[a] + 63u) >> 6;
    }
};

// word_pair[wd] = the pair whose row holds word wd: the last pair whose row_off is <= wd (pairs without a word own none)
__global__ __launch_bounds__(BLOCK) void pas_word_pair_kernel(const u32 *__restrict__ row_off, u32 n_pairs, u32 W, u32 *__restrict__ word_pair)
{
    const u32 wd = blockIdx.x * BLOCK + threadIdx.x;
    if (wd >= W) return;
    u32 lo = 0, hi = n_pairs;                               // the first pair whose row_off is > wd
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (row_off[mid] <= wd) lo = mid + 1u; else hi = mid;
    }
    word_pair[wd] = lo - 1u;                                // (row_off[0] = 0 <= wd: lo >= 1)
}

// ---- the match --------------------------------------------------------------------------------------------------------------
struct PasIndex {
    const u32 *text_start, *pos_unit;
    const u32 *unit_off, *p_doc;        // route 1: per unit its texts, ascending
    const u32 *doc_off, *du;            // route 2: per text its units, ascending
};

// A wavefront takes word wd = 64 consecutive positions of one pair's row; the pair, its texts and their bounds are the same
// for the whole wavefront and are read through the scalar unit (readfirstlane makes wd uniform for the compiler).  A lane
// reads the unit at its position and asks whether b holds it; the ballot is the word; lane 0 stores its 8 bytes.  Every
// word is written exactly once, bits behind the text's end are 0.
template <int ROUTE>
__global__ __launch_bounds__(BLOCK) void pas_match_kernel(PasIndex ix, const u32 *__restrict__ pair_a, const u32 *__restrict__ pair_b,
                                                          const u32 *__restrict__ row_off, const u32 *__restrict__ word_pair, u32 W,
                                                          u64 *__restrict__ words)
{
    const u32 lane = lane_id(), stride = gridDim.x * WAVES_PER_BLOCK;
    for (u32 wv = blockIdx.x * WAVES_PER_BLOCK + wave_id(); wv < W; wv += stride) {
        const u32 wd = __builtin_amdgcn_readfirstlane(wv);
        const u32 p = word_pair[wd], a = pair_a[p], b = pair_b[p];
        const u32 end = ix.text_start[a + 1u];
        const u32 j = ix.text_start[a] + (wd - row_off[p]) * 64u + lane;
        bool hit = false;
        if (j < end) {
            const u32 u = ix.pos_unit[j];
            if (u != COS_NONE) {
                u32 lo, hi, v;
                const u32 *list;
                if (ROUTE == 1) { list = ix.p_doc; lo = ix.unit_off[u]; hi = ix.unit_off[u + 1u]; v = b; }
                else { list = ix.du; lo = ix.doc_off[b]; hi = ix.doc_off[b + 1u]; v = u; }
                const u32 behind = hi;
                while (lo < hi) {                             // the first entry that is >= v
                    const u32 mid = lo + ((hi - lo) >> 1);
                    if (list[mid] < v) lo = mid + 1u; else hi = mid;
                }
                hit = lo < behind && list[lo] == v;
            }
        }
        const u64 f = __ballot(hit);
        if (lane == 0u) words[wd] = f;
    }
}

// ---- runs from words --------------------------------------------------------------------------------------------------------
// prev / next = the neighbouring words of the SAME row, 0 at the row's first and last word: no carry between rows.
__device__ __forceinline__ u64 pas_heads(u64 f, u64 prev) { return f & ~((f << 1) | (prev >> 63)); }
__device__ __forceinline__ u64 pas_tails(u64 f, u64 next) { return f & ~((f >> 1) | (next << 63)); }
// the positions of this word inside a shingle that starts at a shared start: the starts' bits smeared w - 1 places upward,
// with the bits that the previous word's starts push over the boundary
__device__ __forceinline__ u64 pas_cover(u64 f, u64 prev, u32 w)
{
    u64 c = f;
    for (u32 s = 1; s < w; s++) c |= (f << s) | (prev >> (64u - s));
    return c;
}

struct PasRows {
    const u64 *words;
    const u32 *word_pair, *row_off;
    __device__ __forceinline__ u64 prev(u32 wd) const { return wd > row_off[word_pair[wd]] ? words[wd - 1u] : 0ull; }
    __device__ __forceinline__ u64 next(u32 wd) const { return wd + 1u < row_off[word_pair[wd] + 1u] ? words[wd + 1u] : 0ull; }
};

struct PasStartsIn {        // inputs of the scans over the words
    const u64 *words;
    __device__ __forceinline__ u32 operator()(u32 wd) const { return (u32)__popcll(words[wd]); }
};
struct PasCoverIn {
    PasRows rows;
    u32 w;
    __device__ __forceinline__ u32 operator()(u32 wd) const
    {
        const u64 f = rows.words[wd];
        if (w == 1u) return (u32)__popcll(f);
        return (u32)__popcll(pas_cover(f, rows.prev(wd), w));
    }
};
struct PasHeadsIn {
    PasRows rows;
    __device__ __forceinline__ u32 operator()(u32 wd) const
    {
        const u64 f = rows.words[wd];
        return f ? (u32)__popcll(pas_heads(f, rows.prev(wd))) : 0u;
    }
};

// hx = the exclusive scan of the heads' popcounts (with its total).  The heads in front of a word number its heads; its
// tails are numbered by the same scan less the one run that is open at the word's lower boundary: heads and tails are
// equal in number and order, the q-th head and the q-th tail are one passage.
__global__ __launch_bounds__(BLOCK) void pas_runs_kernel(PasRows rows, const u32 *__restrict__ hx, const u32 *__restrict__ pair_a,
                                                         const u32 *__restrict__ text_start, u32 W, u32 *__restrict__ q_head,
                                                         u32 *__restrict__ q_tail, u32 *__restrict__ q_pair)
{
    const u32 wd = blockIdx.x * BLOCK + threadIdx.x;
    if (wd >= W) return;
    const u64 f = rows.words[wd];
    if (!f) return;
    const u64 prev = rows.prev(wd), next = rows.next(wd);
    const u32 p = rows.word_pair[wd];
    const u32 base = text_start[pair_a[p]] + (wd - rows.row_off[p]) * 64u;
    u32 q = hx[wd];
    for (u64 m = pas_heads(f, prev); m; m &= m - 1ull, q++) {
        q_head[q] = base + (u32)__builtin_ctzll(m);
        q_pair[q] = p;
    }
    q = hx[wd] - (u32)((prev >> 63) & f & 1ull);
    for (u64 m = pas_tails(f, next); m; m &= m - 1ull, q++) q_tail[q] = base + (u32)__builtin_ctzll(m);
}

// ---- filter, order, cut -----------------------------------------------------------------------------------------------------
struct PasKeepIn {          // 1 where run q is a passage of min_words words or more: an input of the scan
    const u32 *q_head, *q_tail;
    u32 w, min_words;
    __device__ __forceinline__ u32 operator()(u32 q) const { return q_tail[q] - q_head[q] + w >= min_words ? 1u : 0u; }
};

// the kept runs in (pair, start) order: key = pair << bits | (max_words - words), value = the run
__global__ __launch_bounds__(BLOCK) void pas_keys_kernel(PasKeepIn keep, const u32 *__restrict__ kx, const u32 *__restrict__ q_pair, u32 Q,
                                                         u32 max_words, int bits, u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= Q || !keep(q)) return;
    const u32 c = kx[q];
    keys[c] = ((u64)q_pair[q] << bits) | (u64)(max_words - (keep.q_tail[q] - keep.q_head[q] + keep.w));
    vals[c] = q;
}

struct PasPairOut {
    int32_t *starts, *covered, *found;
    u32 *keep_off, *ret;    // the pair's first rank among the kept runs; the passages returned for it
};

// per pair: differences of the scans at the row's bounds (sx: shared starts, cx: covered, hx: runs, kx: kept runs)
__global__ __launch_bounds__(BLOCK) void pas_pairs_kernel(const u32 *__restrict__ row_off, const u32 *__restrict__ sx, const u32 *__restrict__ cx,
                                                          const u32 *__restrict__ hx, const u32 *__restrict__ kx, u32 n_pairs, u32 per_pair,
                                                          PasPairOut o)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    const u32 r0 = row_off[p], r1 = row_off[p + 1u];
    o.starts[p] = (int32_t)(sx[r1] - sx[r0]);
    o.covered[p] = (int32_t)(cx[r1] - cx[r0]);
    const u32 k0 = kx[hx[r0]], found = kx[hx[r1]] - k0;
    o.found[p] = (int32_t)found;
    o.keep_off[p] = k0;
    o.ret[p] = per_pair ? min(found, per_pair) : found;
}

// rank r of the order -> its place behind pair_off, when per_pair keeps it; at = the smallest position in b of the shingle
// at the passage's start: the posting (unit, b) exists, b holds the unit
__global__ __launch_bounds__(BLOCK) void pas_gather_kernel(const u32 *__restrict__ order, u32 C, const u32 *__restrict__ q_head,
                                                           const u32 *__restrict__ q_tail, const u32 *__restrict__ q_pair,
                                                           const u32 *__restrict__ keep_off, const u32 *__restrict__ pair_off,
                                                           const u32 *__restrict__ pair_b, u32 per_pair, u32 w, PasIndex ix,
                                                           const u32 *__restrict__ p_pos, int32_t *__restrict__ start,
                                                           int32_t *__restrict__ words, int32_t *__restrict__ at)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= C) return;
    const u32 q = order[r], p = q_pair[q], slot = r - keep_off[p];
    if (per_pair && slot >= per_pair) return;
    const u32 o = pair_off[p] + slot, j = q_head[q], u = ix.pos_unit[j], b = pair_b[p];
    u32 lo = ix.unit_off[u], hi = ix.unit_off[u + 1u];
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (ix.p_doc[mid] < b) lo = mid + 1u; else hi = mid;
    }
    start[o] = (int32_t)j;
    words[o] = (int32_t)(q_tail[q] - j + w);
    at[o] = (int32_t)p_pos[lo];
}

// ============================================================================================================ host ==
struct PassagesState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_PAS;
    DevBuf work, idx, pairs, rows, runs, cut, out;  // the levels' arrays; units and postings; per pair; per bit word; per run; the order; the result
    hipEvent_t ev_a = nullptr, ev_b = nullptr;      // behind the names and postings; behind the match kernel
    u32 D = 0, n_pairs = 0, returned = 0;
    float ms_names = -1.f, ms_match = -1.f, ms_rest = -1.f;
    const u32 *text_start = nullptr, *pair_off = nullptr;
    PasPairOut po = {};
    int32_t *start = nullptr, *words = nullptr, *at = nullptr;
    PassagesState() { bufs = {&work, &idx, &pairs, &rows, &runs, &cut, &out}; }
    ~PassagesState() override
    {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
    void clear() override
    {
        D = n_pairs = returned = 0;
        ms_names = ms_match = ms_rest = -1.f;
    }
};

struct PassageParams {
    int32_t words, min_words, per_pair;
    const int32_t *pair_a, *pair_b;
    i64 n_pairs;
};

static void passages_build(east_hip_index *h, const PassageParams &pp, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (pp.words < 1 || pp.words > PHR_MAX_WORDS) east_throw(EAST_HIP_ERR_INVALID, "passages: words must lie in 1 .. 8");
    if (pp.min_words < pp.words) east_throw(EAST_HIP_ERR_INVALID, "passages: min_words must not be below words");
    if (pp.per_pair < 0) east_throw(EAST_HIP_ERR_INVALID, "passages: per_pair must not be negative (0 keeps every passage)");
    if (pp.n_pairs < 0 || pp.n_pairs > PAS_MAX_PAIRS) east_throw(EAST_HIP_ERR_INVALID, "passages: the number of pairs must lie in 0 .. 2^24");
    if (pp.n_pairs > 0 && (!pp.pair_a || !pp.pair_b)) east_throw(EAST_HIP_ERR_INVALID, "passages: the pairs are null");
    if (!out) east_throw(EAST_HIP_ERR_INVALID, "passages: out is null");
    CosState *cp = consumer_peek<CosState>(h);
    if (!cp || !cp->valid) east_throw(EAST_HIP_ERR_NOT_BUILT, "passages: no cosine index has been built on this handle");
    const CosState &c = *cp;
    const u32 T = c.n_kept, D = c.n_docs, w = (u32)pp.words, n_pairs = (u32)pp.n_pairs;
    if (D < 1) east_throw(EAST_HIP_ERR_INVALID, "passages: the index holds no text");
    if (T >= 0x7FFFFFF0u - PHR_MAX_WORDS) east_throw(EAST_HIP_ERR_INVALID, "passages: a text may have 2^31 or more shingle positions");
    for (u32 p = 0; p < n_pairs; p++) {
        const int32_t a = pp.pair_a[p], b = pp.pair_b[p];
        if (a < 0 || b < 0 || (u32)a >= D || (u32)b >= D)
            east_throw(EAST_HIP_ERR_INVALID, "passages: pair " + std::to_string(p) + " names a text outside 0 .. " + std::to_string(D - 1u));
        if (a == b) east_throw(EAST_HIP_ERR_INVALID, "passages: pair " + std::to_string(p) + " pairs text " + std::to_string(a) + " with itself");
    }
    use_device(h);
    PassagesState &g = consumer_begin<PassagesState>(h);     // (every refusal of an argument lies above: an earlier result stays until here)
    g.clear();
    const std::string of = std::to_string(n_pairs) + " pairs of " + std::to_string(D) + " texts";
    auto pas_oom = [&](const char *what, double bytes) { consumer_oom("passages", what, of, bytes); };
    const Knobs kn = knobs_snapshot();
    const int route = kn.passages_route == 0 ? PAS_DEFAULT_ROUTE : kn.passages_route;
    const u32 *tok_doc = c.tok_doc;
    const size_t K1 = (size_t)T + 2, D2 = (size_t)D + 2, N2 = (size_t)n_pairs + 2;
    // (a kept token: overlap_build's arrays but three of the sizes')
    const size_t work_bytes = K1 * 128 + ((size_t)4 << 20);
    if (!g.work.try_ensure(work_bytes, h->stream)) pas_oom("the levels' arrays", (double)work_bytes);
    Arena a = g.work.arena();
    Stats stats;
    Ctx ctx = handle_ctx(h, &a, &stats);
    ConsumerTimer timer(h, g);
    if (!g.ev_a) HIP_CHECK(hipEventCreate(&g.ev_a));
    if (!g.ev_b) HIP_CHECK(hipEventCreate(&g.ev_b));
    i64 launches = 0;

    // ---- 1. names and postings: pos_unit, the postings in (unit, text) order with their positions, unit_off, text_start
    u32 *first = a.alloc<u32>(K1);
    u32 *pos_unit = nullptr, *text_start = nullptr, *p_doc = nullptr, *p_unit = nullptr, *p_pos = nullptr, *unit_off = nullptr, *doc_off = nullptr;
    Arena ia;
    SortBufs<u32> sb = {};
    const OvlNames nm = ovl_names_postings(ctx, a, c, w, [&](u32 U, u32 P) {
        const size_t P1 = (size_t)P + 2;
        const size_t idx_bytes = align256(K1 * 4) + 2 * align256(D2 * 4) + 3 * align256(P1 * 4) + align256(((size_t)U + 2) * 4) +
                                 (route == 2 ? 4 * align256(P1 * 4) + P1 / 2 + ((size_t)4 << 20) : 0) + 4096;
        if (!g.idx.try_ensure(idx_bytes, h->stream)) pas_oom("the units and the postings", (double)idx_bytes);
        ia = g.idx.arena();
        pos_unit = ia.alloc<u32>(K1);
        text_start = ia.alloc<u32>(D2);
        doc_off = ia.alloc<u32>(D2);
        p_doc = ia.alloc<u32>(P1);
        p_unit = ia.alloc<u32>(P1);
        p_pos = ia.alloc<u32>(P1);
        unit_off = ia.alloc<u32>((size_t)U + 2);
        if (route == 2) sb = sort_bufs_alloc<u32>(ia, P1);
        return OvlPostingRoom{first, p_doc, p_unit};
    });
    const u32 U = nm.U, P = nm.P;
    launches += nm.named ? 1 : 0;
    HIP_CHECK(hipMemsetAsync(pos_unit, 0xFF, K1 * 4, h->stream));
    if (U) {
        LAUNCH(ctx, pas_units_kernel, ceil_div_u32(nm.dom, BLOCK), nm.post, (const u32 *)nm.ux, (const u32 *)nm.px, (const u32 *)nm.W.sb.vals[nm.sr], nm.dom,
               pos_unit, p_pos);
        launches++;
    }
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)U + 1, BLOCK), (const u32 *)p_unit, P, U, unit_off);
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)D + 1, BLOCK), tok_doc, T, D, text_start);
    launches += 2;
    PasIndex ix{text_start, pos_unit, unit_off, p_doc, nullptr, nullptr};
    if (route == 2 && U) {                                   // the overlap's operands: per text its units ascending
        HIP_CHECK(hipMemcpyAsync(sb.keys[0], p_doc, (size_t)P * 4, hipMemcpyDeviceToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(sb.vals[0], p_unit, (size_t)P * 4, hipMemcpyDeviceToDevice, h->stream));
        ctx.arena = &ia;
        const int r = radix_sort_pairs<u32>(ctx, sb, P, bit_width_u32(D - 1u));
        LAUNCH(ctx, ovl_doc_off_kernel, ceil_div_u32(D + 1u, BLOCK), (const u32 *)sb.keys[r], P, D, doc_off);
        launches++;
        ix.doc_off = doc_off;
        ix.du = sb.vals[r];
    }

    // ---- 2. rows: the pairs up, a row's words by a scan over the pairs
    const size_t pairs_bytes = 9 * align256(N2 * 4) + N2 / 256 + ((size_t)1 << 20);
    if (!g.pairs.try_ensure(pairs_bytes, h->stream)) pas_oom("the pairs", (double)pairs_bytes);
    Arena pa = g.pairs.arena();
    u32 *pair_a = pa.alloc<u32>(N2), *pair_b = pa.alloc<u32>(N2), *row_off = pa.alloc<u32>(N2), *pair_off = pa.alloc<u32>(N2);
    PasPairOut po;
    po.starts = pa.alloc<int32_t>(N2);
    po.covered = pa.alloc<int32_t>(N2);
    po.found = pa.alloc<int32_t>(N2);
    po.keep_off = pa.alloc<u32>(N2);
    po.ret = pa.alloc<u32>(N2);
    ctx.arena = &pa;
    if (n_pairs) {
        HIP_CHECK(hipMemcpyAsync(pair_a, pp.pair_a, (size_t)n_pairs * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(pair_b, pp.pair_b, (size_t)n_pairs * 4, hipMemcpyHostToDevice, h->stream));
    }
    device_scan_with_total(ctx, PasRowWordsIn{pair_a, text_start}, n_pairs, row_off);
    u32 W = 0;
    std::vector<u32> ts((size_t)D + 1);
    HIP_CHECK(hipMemcpyAsync(ts.data(), text_start, ((size_t)D + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    device_read_words(ctx, {{&W, row_off + n_pairs}});      // (and: the pairs have left the caller's arrays)
    u64 all_words = 0;                                        // (the scan's sum is one modulo 2^32: the bound is tested on the exact one)
    for (u32 p = 0; p < n_pairs; p++) all_words += (u64)((ts[(size_t)pp.pair_a[p] + 1] - ts[(size_t)pp.pair_a[p]] + 63u) >> 6);
    if (all_words >= PAS_MAX_BIT_WORDS) east_throw(EAST_HIP_ERR_INVALID, "passages: the pairs' rows take 2^25 bit words or more");
    HIP_CHECK(hipEventRecord(g.ev_a, h->stream));

    // ---- 3. the match
    const size_t W1 = (size_t)W + 2;
    const size_t rows_bytes = align256(W1 * 8) + 4 * align256(W1 * 4) + W1 / 256 + ((size_t)1 << 20);
    if (!g.rows.try_ensure(rows_bytes, h->stream)) pas_oom("the bit words", (double)rows_bytes);
    Arena ra = g.rows.arena();
    u64 *words = ra.alloc<u64>(W1);
    u32 *word_pair = ra.alloc<u32>(W1), *sx = ra.alloc<u32>(W1), *cx = ra.alloc<u32>(W1), *hx = ra.alloc<u32>(W1);
    ctx.arena = &ra;
    if (W) {
        LAUNCH(ctx, pas_word_pair_kernel, ceil_div_u32(W, BLOCK), (const u32 *)row_off, n_pairs, W, word_pair);
        const u32 grid = std::min(ceil_div_u32(W, WAVES_PER_BLOCK), PAS_MATCH_GRID);
        if (route == 2 && U)
            LAUNCH(ctx, pas_match_kernel<2>, grid, ix, (const u32 *)pair_a, (const u32 *)pair_b, (const u32 *)row_off, (const u32 *)word_pair, W, words);
        else
            LAUNCH(ctx, pas_match_kernel<1>, grid, ix, (const u32 *)pair_a, (const u32 *)pair_b, (const u32 *)row_off, (const u32 *)word_pair, W, words);
        launches += 2;
    }
    HIP_CHECK(hipEventRecord(g.ev_b, h->stream));

    // ---- 4. runs from words: three scans, the runs' heads and tails to their numbers
    const PasRows rows{words, word_pair, row_off};
    device_scan_with_total(ctx, PasStartsIn{words}, W, sx);
    device_scan_with_total(ctx, PasCoverIn{rows, w}, W, cx);
    device_scan_with_total(ctx, PasHeadsIn{rows}, W, hx);
    u32 n_starts = 0, Q = 0;
    device_read_words(ctx, {{&n_starts, sx + W}, {&Q, hx + W}});
    const size_t Q1 = (size_t)Q + 2;
    const size_t runs_bytes = 4 * align256(Q1 * 4) + Q1 / 256 + ((size_t)1 << 20);
    if (!g.runs.try_ensure(runs_bytes, h->stream)) pas_oom("the runs", (double)runs_bytes);
    Arena qa = g.runs.arena();
    u32 *q_head = qa.alloc<u32>(Q1), *q_tail = qa.alloc<u32>(Q1), *q_pair = qa.alloc<u32>(Q1), *kx = qa.alloc<u32>(Q1);
    ctx.arena = &qa;
    if (Q) {
        LAUNCH(ctx, pas_runs_kernel, ceil_div_u32(W, BLOCK), rows, (const u32 *)hx, (const u32 *)pair_a, (const u32 *)text_start, W, q_head, q_tail, q_pair);
        launches++;
    }

    // ---- 5. filter, order, cut
    const PasKeepIn keep{q_head, q_tail, w, (u32)pp.min_words};
    u32 C = device_scan_count(ctx, keep, Q, kx);
    if (n_pairs) {
        LAUNCH(ctx, pas_pairs_kernel, ceil_div_u32(n_pairs, BLOCK), (const u32 *)row_off, (const u32 *)sx, (const u32 *)cx, (const u32 *)hx, (const u32 *)kx,
               n_pairs, (u32)pp.per_pair, po);
        launches++;
    }
    ctx.arena = &pa;
    device_scan_with_total(ctx, ArrIn{po.ret}, n_pairs, pair_off);
    u32 R = 0;
    device_read_words(ctx, {{&R, pair_off + n_pairs}});
    const size_t R1 = (size_t)R + 2;
    if (!g.out.try_ensure(3 * align256(R1 * 4) + 256, h->stream)) pas_oom("the passages", 3.0 * (double)R1 * 4.0);
    Arena oa = g.out.arena();
    g.start = oa.alloc<int32_t>(R1);
    g.words = oa.alloc<int32_t>(R1);
    g.at = oa.alloc<int32_t>(R1);
    if (C) {
        const size_t C1 = (size_t)C + 2;
        const size_t cut_bytes = 2 * align256(C1 * 8) + 2 * align256(C1 * 4) + C1 / 2 + ((size_t)4 << 20);
        if (!g.cut.try_ensure(cut_bytes, h->stream)) pas_oom("the order of the passages", (double)cut_bytes);
        Arena ca = g.cut.arena();
        ctx.arena = &ca;
        SortBufs<u64> cs = sort_bufs_alloc<u64>(ca, C1);
        const u32 max_words = T + w;                          // (a passage lies inside a text)
        const int wbits = std::max(1, bit_width_u32(max_words)), pbits = bit_width_u32(n_pairs - 1u);
        LAUNCH(ctx, pas_keys_kernel, ceil_div_u32(Q, BLOCK), keep, (const u32 *)kx, (const u32 *)q_pair, Q, max_words, wbits, cs.keys[0], cs.vals[0]);
        const int r = radix_sort_pairs<u64>(ctx, cs, C, wbits + pbits);
        LAUNCH(ctx, pas_gather_kernel, ceil_div_u32(C, BLOCK), (const u32 *)cs.vals[r], C, (const u32 *)q_head, (const u32 *)q_tail, (const u32 *)q_pair,
               (const u32 *)po.keep_off, (const u32 *)pair_off, (const u32 *)pair_b, (u32)pp.per_pair, w, ix, (const u32 *)p_pos, g.start, g.words, g.at);
        launches += 2;
    }
    timer.finish();
    HIP_CHECK(hipEventElapsedTime(&g.ms_names, g.ev0, g.ev_a));
    HIP_CHECK(hipEventElapsedTime(&g.ms_match, g.ev_a, g.ev_b));
    HIP_CHECK(hipEventElapsedTime(&g.ms_rest, g.ev_b, g.ev1));
    g.D = D;
    g.n_pairs = n_pairs;
    g.returned = R;
    g.text_start = text_start;
    g.pair_off = pair_off;
    g.po = po;
    g.valid = true;
    out[0] = (i64)D; out[1] = (i64)T; out[2] = (i64)n_pairs; out[3] = (i64)U; out[4] = (i64)P; out[5] = (i64)W;
    out[6] = (i64)n_starts; out[7] = (i64)Q; out[8] = (i64)R; out[9] = launches; out[10] = (i64)route;
    out[11] = (i64)nm.levels;
}

static void passages_fetch(east_hip_index *h, i64 *pair_off, int32_t *starts, int32_t *covered, int32_t *found, int32_t *start, int32_t *words,
                           int32_t *at, int32_t *text_start)
{
    PassagesState &g = consumer_built<PassagesState>(h, "no passages have been built on this handle");
    const size_t n = g.n_pairs, R = g.returned;
    const struct { int32_t *dst; const void *src; size_t count; } rows[7] = {
        {starts, g.po.starts, n}, {covered, g.po.covered, n}, {found, g.po.found, n}, {start, g.start, R}, {words, g.words, R}, {at, g.at, R},
        {text_start, g.text_start, (size_t)g.D + 1}};
    for (const auto &r : rows)
        if (r.dst && r.count) HIP_CHECK(hipMemcpyAsync(r.dst, r.src, r.count * 4, hipMemcpyDeviceToHost, h->stream));
    std::vector<u32> off;
    if (pair_off) {
        off.resize(n + 1);
        HIP_CHECK(hipMemcpyAsync(off.data(), g.pair_off, (n + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (pair_off)
        for (size_t p = 0; p <= n; p++) pair_off[p] = off[p];
}

extern "C" {

int east_hip_passages_build(east_hip_handle_t h, int32_t words, int32_t min_words, int32_t per_pair, const int32_t *pair_a,
                            const int32_t *pair_b, int64_t n_pairs, int64_t *out)
{
    return guarded([&] { passages_build(h, PassageParams{words, min_words, per_pair, pair_a, pair_b, n_pairs}, out); });
}

int east_hip_passages_fetch(east_hip_handle_t h, int64_t *pair_off, int32_t *starts, int32_t *covered, int32_t *found, int32_t *start,
                            int32_t *words, int32_t *at, int32_t *text_start)
{
    return guarded([&] { passages_fetch(h, pair_off, starts, covered, found, start, words, at, text_start); });
}

double east_hip_last_passages_ms(east_hip_handle_t h) { return consumer_ms<PassagesState>(h); }

int east_hip_passages_phases(east_hip_handle_t h, double *ms)
{
    return guarded([&] {
        const PassagesState &g = consumer_built<PassagesState>(h, "no passages have been built on this handle");
        if (!ms) east_throw(EAST_HIP_ERR_INVALID, "passages: ms is null");
        ms[0] = (double)g.ms_names;
        ms[1] = (double)g.ms_match;
        ms[2] = (double)g.ms_rest;
    });
}

int east_hip_debug_set_passages_route(int route)
{
    // 0: the default (PAS_DEFAULT_ROUTE); 1: b in the unit's text list; 2: the unit in b's unit list
    if (route < 0 || route > 2) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.passages_route = route; });
    return EAST_HIP_OK;
}

}  // extern "C"
