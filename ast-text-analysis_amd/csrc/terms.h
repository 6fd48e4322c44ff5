// terms.h -- the characteristic terms of texts and of groups of texts: per group the units of the cosine index's vector
// space with the largest mean normalised weight (include/east_hip.h, "Characteristic terms"; `east texts terms`;
// DESIGN.md 19).
//
// The index holds the postings (unit, document, count) in (unit, document) order, their place in document order and, per
// weighting, the weight x of every posting and the norm of every document (cosine.h).  The result is a group-by-sum of the
// sparse D x units matrix of x / norm over arbitrary groups of its rows, and a top-N over the ragged rows of that sum:
//
//   postings --cost_scatter_kernel (cosine_texts.h)--> per document its units ascending (du) and its weights (dw)
//   --terms_keys_kernel: a thread a posting in document order--> key = group << unit bits | unit, value = the posting's
//     place, q = x / norm
//   --stable radix sort over exactly bit_width(G - 1) + bit_width(units - 1) bits (left out under the identity grouping:
//     the keys ascend as they are)--> runs of equal keys = the entries (group, unit); inside a run the places ascend, and
//     with them the texts: that is the order of the sum
//   --terms_runs_kernel: the head of a run adds it left to right in one accumulator that starts from the first addend, divides
//     by the group's members and writes (group, unit, value, texts)
//   --ascending_offsets_kernel--> the entries of every group; a scan of texts >= min_texts compacts the entries that pass:
//     the SEGMENTS, (group, unit) ascending
//   --the pre-selection (below)--> the candidates of every segment
//   --stable radix sort by the complement of the value's 63 bits below the sign (positive doubles order as their bit
//     patterns), then a stable sort by the group--> per group its candidates by value descending, unit ascending among
//     equal values
//   --terms_gather_kernel: the first min(n, length) of every segment into [G, n]
//
// The pre-selection.  The digest of a value is 12 bits that never decrease with it: 4095 - min((VALUE_TOP - bits) >> 48,
// 4095), VALUE_TOP the bits of 1.0: sixteen steps an octave below 1.0 over 256 octaves.  A workgroup takes a fixed tile of TERMS_TILE compacted entries
// and walks the segments that meet it.  A segment of at most n entries needs no boundary (0: all of it).  A longer one that
// lies inside the tile is counted into a histogram in LDS (integer counts), whose sums from the top down give the
// BOUNDARY: the highest digest at or above which at least n entries lie.  A segment that runs over a tile's end leaves the
// counts of its piece in the tile's own two rows of `partial` -- row 0 the piece of the segment that came in over the
// tile's front, row 1 the piece of the one that leaves over its end --, and terms_bound_long_kernel, a workgroup per tile
// in which such a segment starts, adds the pieces in tile order and finds the boundary the same way.  No two workgroups
// write one word; there is no atomic on global memory.  Only entries at or above their segment's boundary reach the sort:
// every entry of the final n is among them, and so is every entry of the boundary's bin, so a tie at the cut is decided by
// the sort, by unit id.  east_hip_debug_set_terms_select(1) sends every entry through the sort: the same bytes.
//
// Order of the sums: fixed by the collection and the grouping alone.  No floating-point atomic; nothing depends on timing.
//
// Memory: 96 bytes a posting of work arrays, 20 bytes an entry and 20 bytes a place of the result, buffers of this
// consumer's own.
#pragma once
#include "consumer.h"
#include "cosine.h"
#include "cosine_texts.h"
#include "radix_sort.h"
#include "scan.h"

#define TERMS_MAX_N 1024                           // the ranking's own limit (top.h: TOP_MAX_N)
#define TERMS_TILE 4096u                           // compacted entries of a histogram tile
#define TERMS_BINS 4096u                           // digests
#define TERMS_BINS_PER_THREAD (TERMS_BINS / BLOCK)
#define TERMS_VALUE_TOP 0x3FF0000000000000ull      // the bit pattern of 1.0: no value lies above it
#define TERMS_VALUE_BITS 63                        // the bits of a positive double below the sign
static_assert(TERMS_BINS % BLOCK == 0, "a thread owns whole bins");

// the sort key of a value: ascending keys are descending values (any positive double)
__device__ __forceinline__ u64 terms_value_key(double v) { return 0x7FFFFFFFFFFFFFFFull - (u64)__double_as_longlong(v); }
// (the values lie in (0, 1]: the digest spends its bins below 1.0; anything above would share the top bin)
__device__ __forceinline__ u32 terms_digest(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    const u64 t = b < TERMS_VALUE_TOP ? (TERMS_VALUE_TOP - b) >> 48 : 0ull;
    return TERMS_BINS - 1u - (u32)(t < (u64)(TERMS_BINS - 1u) ? t : (u64)(TERMS_BINS - 1u));
}

// ---- keys -------------------------------------------------------------------------------------------------------------------
// Thread = place i in document order: its document by binary search in doc_off.  group == nullptr: group[d] = d.
__global__ __launch_bounds__(BLOCK) void terms_keys_kernel(const u32 *__restrict__ du, const double *__restrict__ dw,
                                                           const u32 *__restrict__ doc_off, u32 D, u32 P,
                                                           const double *__restrict__ norm, const u32 *__restrict__ group,
                                                           int unit_bits, u64 *__restrict__ keys, u32 *__restrict__ vals,
                                                           double *__restrict__ q)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    u32 lo = 0, hi = D;                                           // the last d with doc_off[d] <= i
    while (hi - lo > 1u) { const u32 mid = lo + ((hi - lo) >> 1); if (doc_off[mid] <= i) lo = mid; else hi = mid; }
    const u32 g = group ? group[lo] : lo;
    keys[i] = ((u64)g << unit_bits) | du[i];
    vals[i] = i;
    q[i] = dw[i] / norm[lo];
}

// ---- runs -------------------------------------------------------------------------------------------------------------------
// ri = inclusive scan of the run heads over the sorted keys.  The head of run r adds its members' quotients left to right.
__global__ __launch_bounds__(BLOCK) void terms_runs_kernel(const u64 *__restrict__ skeys, const u32 *__restrict__ svals,
                                                           const u32 *__restrict__ ri, const double *__restrict__ q, u32 P,
                                                           int unit_bits, const u32 *__restrict__ members,
                                                           u32 *__restrict__ e_group, u32 *__restrict__ e_unit,
                                                           double *__restrict__ e_value, u32 *__restrict__ e_texts)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const u32 r1 = ri[i];
    if (i > 0u && ri[i - 1u] == r1) return;
    const u64 key = skeys[i];
    double s = q[svals[i]];
    u32 e = i + 1u;
    for (; e < P && skeys[e] == key; e++) s += q[svals[e]];
    const u32 g = (u32)(key >> unit_bits), r = r1 - 1u;
    e_group[r] = g;
    e_unit[r] = (u32)(key & (((u64)1 << unit_bits) - 1ull));
    e_value[r] = s / (double)members[g];
    e_texts[r] = e - i;
}

// ---- segments ---------------------------------------------------------------------------------------------------------------
// 1 where an entry passes min_texts: an input of the scan
struct TermsPassIn {
    const u32 *e_texts;
    u32 min_texts;
    __device__ __forceinline__ u32 operator()(u32 e) const { return e_texts[e] >= min_texts ? 1u : 0u; }
};

// px = exclusive scan of the pass flags (with the total behind): the passing entries to their slots, and the segments'
// offsets soff[g] = px[goff[g]] for g = 0 .. G
__global__ __launch_bounds__(BLOCK) void terms_compact_kernel(const u32 *__restrict__ px, u32 E, const u32 *__restrict__ e_group,
                                                              const double *__restrict__ e_value, u32 *__restrict__ c_ent,
                                                              u32 *__restrict__ c_group, double *__restrict__ c_value)
{
    const u32 e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E || px[e + 1u] == px[e]) return;
    const u32 slot = px[e];
    c_ent[slot] = e;
    c_group[slot] = e_group[e];
    c_value[slot] = e_value[e];
}

__global__ __launch_bounds__(BLOCK) void terms_seg_offsets_kernel(const u32 *__restrict__ px, const u32 *__restrict__ goff, u32 G,
                                                                  u32 *__restrict__ soff)
{
    const u32 g = blockIdx.x * BLOCK + threadIdx.x;
    if (g <= G) soff[g] = px[goff[g]];
}

// ---- the pre-selection ------------------------------------------------------------------------------------------------------
// hist: TERMS_BINS counts in LDS.  The highest digest at or above which at least `need` entries lie (need >= 1 and at most
// the counts' sum): thread t owns the TERMS_BINS_PER_THREAD bins below TERMS_BINS - t * TERMS_BINS_PER_THREAD, so the
// exclusive sum over the threads is the count above its bins; exactly one thread finds the bin, and writes it.
__device__ __forceinline__ void terms_boundary(const u32 *hist, u32 need, u32 *lds4, u32 *bound)
{
    const u32 top = TERMS_BINS - threadIdx.x * TERMS_BINS_PER_THREAD;      // (one above this thread's highest bin)
    u32 own = 0;
#pragma unroll
    for (u32 k = 1; k <= TERMS_BINS_PER_THREAD; k++) own += hist[top - k];
    u32 total = 0;
    u32 above = block_exclusive_sum(own, lds4, total);
    if (above < need && above + own >= need) {
        for (u32 k = 1; k <= TERMS_BINS_PER_THREAD; k++) {
            above += hist[top - k];
            if (above >= need) { *bound = top - k; break; }
        }
    }
}

// Workgroup = tile t of the compacted entries [t TILE, min(F, (t + 1) TILE)).  bound[] was zeroed: all of a segment.
__global__ __launch_bounds__(BLOCK) void terms_hist_kernel(const double *__restrict__ c_value, const u32 *__restrict__ soff, u32 G,
                                                           u32 F, u32 n, u32 *__restrict__ bound, u32 *__restrict__ partial)
{
    __shared__ u32 hist[TERMS_BINS];
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    const u32 t0 = blockIdx.x * TERMS_TILE, t1 = min(F, t0 + TERMS_TILE);
    u32 lo = 0, hi = G;                                           // the last g with soff[g] <= t0: the segment that holds t0
    while (hi - lo > 1u) { const u32 mid = lo + ((hi - lo) >> 1); if (soff[mid] <= t0) lo = mid; else hi = mid; }
    for (u32 g = lo; g < G; g++) {                                // (the same for every thread of the workgroup)
        const u32 a = soff[g], e = soff[g + 1u];
        if (a >= t1) break;
        if (e - a <= n) continue;                                 // (also an empty segment)
        const u32 pa = max(a, t0), pe = min(e, t1);
        __syncthreads();                                          // (the histogram of the segment before has been read)
        for (u32 b = threadIdx.x; b < TERMS_BINS; b += BLOCK) hist[b] = 0u;
        __syncthreads();
        for (u32 i = pa + threadIdx.x; i < pe; i += BLOCK) atomicAdd(&hist[terms_digest(c_value[i])], 1u);
        syncthreads_after_lds_atomics();
        if (a >= t0 && e <= t1) {
            terms_boundary(hist, n, lds4, bound + g);
        } else {
            u32 *row = partial + ((size_t)blockIdx.x * 2u + (a < t0 ? 0u : 1u)) * TERMS_BINS;
            for (u32 b = threadIdx.x; b < TERMS_BINS; b += BLOCK) row[b] = hist[b];
        }
    }
}

// Workgroup = tile t: the segment that holds the tile's last entry, where it starts in the tile and runs on behind it.  Its
// pieces: row 1 of tile t, row 0 of every tile behind up to the one that holds its last entry.
__global__ __launch_bounds__(BLOCK) void terms_bound_long_kernel(const u32 *__restrict__ partial, const u32 *__restrict__ soff, u32 G,
                                                                 u32 F, u32 n, u32 *__restrict__ bound)
{
    __shared__ u32 hist[TERMS_BINS];
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    const u32 t0 = blockIdx.x * TERMS_TILE, t1 = t0 + TERMS_TILE;
    if (t1 >= F) return;                                          // (the last tile: nothing runs on behind it)
    const u32 last = t1 - 1u;
    u32 lo = 0, hi = G;                                           // the last g with soff[g] <= last
    while (hi - lo > 1u) { const u32 mid = lo + ((hi - lo) >> 1); if (soff[mid] <= last) lo = mid; else hi = mid; }
    const u32 a = soff[lo], e = soff[lo + 1u];
    if (a < t0 || e <= t1 || e - a <= n) return;                  // (it came in over the front; it ends here; all of it is taken)
    const u32 tiles_behind = (e - 1u) / TERMS_TILE - blockIdx.x;
    // (a thread's sixteen bins lie BLOCK apart: every load is a coalesced row, and the sixteen of a tile -- four tiles' with
    // the unrolling -- are in flight together; a segment of two million entries is five hundred tiles)
    u32 c[TERMS_BINS_PER_THREAD];
#pragma unroll
    for (u32 j = 0; j < TERMS_BINS_PER_THREAD; j++) c[j] = partial[((size_t)blockIdx.x * 2u + 1u) * TERMS_BINS + j * BLOCK + threadIdx.x];
#pragma unroll 4
    for (u32 k = 1; k <= tiles_behind; k++) {
        const u32 *row = partial + ((size_t)(blockIdx.x + k) * 2u) * TERMS_BINS + threadIdx.x;
#pragma unroll
        for (u32 j = 0; j < TERMS_BINS_PER_THREAD; j++) c[j] += row[j * BLOCK];
    }
#pragma unroll
    for (u32 j = 0; j < TERMS_BINS_PER_THREAD; j++) hist[j * BLOCK + threadIdx.x] = c[j];
    __syncthreads();
    terms_boundary(hist, n, lds4, bound + lo);
}

// 1 where a compacted entry reaches the sort
struct TermsSelectIn {
    const double *c_value;
    const u32 *c_group, *bound;
    __device__ __forceinline__ u32 operator()(u32 i) const { return terms_digest(c_value[i]) >= bound[c_group[i]] ? 1u : 0u; }
};

// sx = exclusive scan of the selection (nullptr: every entry, to its own slot)
__global__ __launch_bounds__(BLOCK) void terms_value_keys_kernel(const double *__restrict__ c_value, const u32 *__restrict__ sx, u32 F,
                                                                 u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= F) return;
    u32 slot = i;
    if (sx) {
        if (sx[i + 1u] == sx[i]) return;
        slot = sx[i];
    }
    keys[slot] = terms_value_key(c_value[i]);
    vals[slot] = i;
}

// the candidates in value order: the group of each as the key of the second sort
__global__ __launch_bounds__(BLOCK) void terms_group_keys_kernel(const u32 *__restrict__ order, const u32 *__restrict__ c_group, u32 S,
                                                                 u32 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= S) return;
    const u32 c = order[i];
    keys[i] = c_group[c];
    vals[i] = c;
}

// ---- the result -------------------------------------------------------------------------------------------------------------
struct TermsOut {
    int32_t *count, *unit, *texts, *df;
    double *value;
};

// Thread (g, r): place r of group g.  cand_off[g]: where the candidates of g start in `order` (the compacted entries by
// group, value descending, unit ascending); behind count[g] = min(n, the segment's length): -1 and NaN (top.h's result).
__global__ __launch_bounds__(BLOCK) void terms_gather_kernel(const u32 *__restrict__ order, const u32 *__restrict__ cand_off, u32 S,
                                                             const u32 *__restrict__ soff, const u32 *__restrict__ c_ent,
                                                             const u32 *__restrict__ e_unit, const double *__restrict__ e_value,
                                                             const u32 *__restrict__ e_texts, const u32 *__restrict__ unit_off,
                                                             u32 G, u32 n, TermsOut o)
{
    const u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (gid >= (u64)G * n) return;
    const u32 g = (u32)(gid / n), r = (u32)(gid % n);
    const u32 cnt = min(n, soff[g + 1u] - soff[g]);
    if (r == 0u) o.count[g] = (int32_t)cnt;
    int32_t unit = -1, texts = -1, df = -1;
    double value = __builtin_nan("");
    const u32 at = cand_off[g] + r;
    if (r < cnt && at < S) {                                      // (at < S: the selection holds at least cnt of the segment)
        const u32 e = c_ent[order[at]], u = e_unit[e];
        unit = (int32_t)u;
        value = e_value[e];
        texts = (int32_t)e_texts[e];
        df = (int32_t)(unit_off[u + 1u] - unit_off[u]);
    }
    o.unit[gid] = unit;
    o.value[gid] = value;
    o.texts[gid] = texts;
    o.df[gid] = df;
}

// ============================================================================================================ host ==
// The buffers belong to the handle and to nothing else: not the cosine index's, the EASA arena or another consumer's.
struct TermsState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_TERMS;
    DevBuf work, ent, out;                  // the build's arrays; the entries (the vectors); the ranked result
    u32 G = 0, n = 0, E = 0;
    u32 *goff = nullptr, *e_group = nullptr, *e_unit = nullptr, *e_texts = nullptr;
    double *e_value = nullptr;
    TermsOut o = {};
    std::vector<int32_t> members;
    TermsState()
    {
        bufs = {&work, &ent, &out};
        keep_bytes = (size_t)64 << 20;
    }
    void clear() override
    {
        G = n = E = 0;
        members.clear();
    }
};

struct TermsParams {
    int32_t weighting;
    const int32_t *group;
    int32_t n_groups, n, min_texts;
};

// the launches of device_scan over len elements (scan.h): one a tile, two up to SCAN_RAW_TILES tiles, the sums' own scan above
static i64 terms_scan_launches(u32 len)
{
    const u32 nb = ceil_div_u32(len, SCAN_TILE);
    return nb <= 1 ? 1 : nb <= SCAN_RAW_TILES ? 2 : 2 + terms_scan_launches(nb);
}

static void terms_build(east_hip_index *h, const TermsParams &tp, i64 *out)
{
    const char *who = "characteristic terms";
    CosState &c = cos_built(h);                                 // (a null handle; no index)
    if (tp.weighting < 0 || tp.weighting > 1) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: unknown weighting");
    if (tp.n < 1 || tp.n > TERMS_MAX_N) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: n must be 1 .. 1024");
    if (tp.min_texts < 1) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: min_texts must be at least 1");
    CosUnits &U = c.use_classes ? c.cls : c.terms;
    const u32 D = c.n_docs, P = U.P, n_units = U.n_units, n = (u32)tp.n;
    if (D < 1) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: the index holds no text");
    if (tp.n_groups < 1) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: n_groups must be at least 1");
    if (!tp.group && (u32)tp.n_groups != D)
        east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: without a grouping n_groups must be the number of texts, " + std::to_string(D) +
                                             ", not " + std::to_string(tp.n_groups));
    const u32 G = (u32)tp.n_groups;
    std::vector<int32_t> members((size_t)G, tp.group ? 0 : 1);
    if (tp.group)
        for (u32 d = 0; d < D; d++) {
            if (tp.group[d] < 0 || tp.group[d] >= tp.n_groups)
                east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: group[" + std::to_string(d) + "] = " + std::to_string(tp.group[d]) +
                                                     " lies outside 0 .. " + std::to_string(tp.n_groups - 1));
            members[(size_t)tp.group[d]]++;
        }
    if ((u64)G * n >= (u64)0x7FFFFFF0u * BLOCK) east_throw(EAST_HIP_ERR_INVALID, "characteristic terms: more places than one launch takes");
    const int unit_bits = bit_width_u32(n_units ? n_units - 1u : 0u), group_bits = bit_width_u32(G - 1u);
    const Knobs kn = knobs_snapshot();
    const bool select = kn.terms_select == 0;
    TermsState &g = consumer_begin<TermsState>(h);             // (every refusal lies above: an earlier result stays until here)
    g.clear();
    const std::string texts = std::to_string(D) + " texts in " + std::to_string(G) + " groups";
    auto oom = [&](const char *what, double bytes) { consumer_oom(who, what, texts, bytes); };

    // ---- room: the result, and the work arrays of both halves of the build (an entry is a posting at most)
    const size_t P1 = (size_t)P + 2, G1 = (size_t)G + 2, places = (size_t)G * n;
    const size_t out_bytes = align256(G1 * 4) + 3 * align256((places + 1) * 4) + align256((places + 1) * 8) + 256;
    const size_t tiles = ceil_div_u32(P1, TERMS_TILE) + 1;
    const size_t work_bytes = P1 * 96 + G1 * 24 + align256(tiles * 2 * TERMS_BINS * 4) + ((size_t)8 << 20);
    if (!g.out.try_ensure(out_bytes, h->stream)) oom("the ranked terms", (double)out_bytes);
    if (!g.work.try_ensure(work_bytes, h->stream)) oom("the work arrays", (double)work_bytes);
    Arena ao = g.out.arena();
    g.o.count = ao.alloc<int32_t>(G1);
    g.o.unit = ao.alloc<int32_t>(places + 1);
    g.o.texts = ao.alloc<int32_t>(places + 1);
    g.o.df = ao.alloc<int32_t>(places + 1);
    g.o.value = ao.alloc<double>(places + 1);
    double *w = nullptr, *norm = nullptr;
    cos_weight_ptrs(U, D, tp.weighting, &w, &norm);
    Arena a = g.work.arena();
    Stats stats;
    Ctx ctx = handle_ctx(h, &a, &stats);
    i64 launches = 0, scans = 0;
    auto scan_launches = terms_scan_launches;

    // ---- the grouping and its members
    u32 *d_group = tp.group ? a.alloc<u32>(D) : nullptr, *d_members = a.alloc<u32>(G);
    if (tp.group) HIP_CHECK(hipMemcpyAsync(d_group, tp.group, (size_t)D * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_members, members.data(), (size_t)G * 4, hipMemcpyHostToDevice, h->stream));
    u32 *goff = a.alloc<u32>(G1), *soff = a.alloc<u32>(G1), *cand_off = a.alloc<u32>(G1), *bound = a.alloc<u32>(G1);
    const size_t stage = a.mark();

    ConsumerTimer timer(h, g);
    cos_make_weights(ctx, c, U, tp.weighting, w, norm);
    if (!U.w_valid[tp.weighting]) launches += P ? 2 : 1;

    // ---- operands, keys, the grouping sort, runs
    u32 E = 0;
    bool skipped = !tp.group;
    i64 passes = 0;
    if (P) {
        u32 *du = a.alloc<u32>(P1), *ri = a.alloc<u32>(P1);
        double *dw = a.alloc<double>(P1), *q = a.alloc<double>(P1);
        SortBufs<u64> sb = sort_bufs_alloc<u64>(a, P1);
        LAUNCH(ctx, cost_scatter_kernel, ceil_div_u32(P, BLOCK), (const u32 *)U.post_unit, (const double *)w, (const u32 *)U.inv_perm, P, du, dw);
        LAUNCH(ctx, terms_keys_kernel, ceil_div_u32(P, BLOCK), (const u32 *)du, (const double *)dw, (const u32 *)U.doc_off, D, P,
               (const double *)norm, (const u32 *)d_group, unit_bits, sb.keys[0], sb.vals[0], q);
        launches += 2;
        int r = 0;
        if (tp.group) {
            r = radix_sort_pairs<u64>(ctx, sb, P, std::max(1, group_bits + unit_bits));
            passes += stats.radix_passes;
        }
        device_scan<RunHeadIn<u64>, true>(ctx, RunHeadIn<u64>{sb.keys[r], 0}, P, ri);
        scans += scan_launches(P);
        device_read_words(ctx, {{&E, ri + (P - 1u)}});
        const size_t ent_bytes = 3 * align256(((size_t)E + 1) * 4) + align256(((size_t)E + 1) * 8) + align256(G1 * 4) + 256;
        if (!g.ent.try_ensure(ent_bytes, h->stream)) oom("the entries", (double)ent_bytes);
        Arena ae = g.ent.arena();
        g.e_group = ae.alloc<u32>((size_t)E + 1);
        g.e_unit = ae.alloc<u32>((size_t)E + 1);
        g.e_texts = ae.alloc<u32>((size_t)E + 1);
        g.e_value = ae.alloc<double>((size_t)E + 1);
        g.goff = ae.alloc<u32>(G1);
        LAUNCH(ctx, terms_runs_kernel, ceil_div_u32(P, BLOCK), (const u64 *)sb.keys[r], (const u32 *)sb.vals[r], (const u32 *)ri,
               (const double *)q, P, unit_bits, (const u32 *)d_members, g.e_group, g.e_unit, g.e_value, g.e_texts);
        launches++;
    } else {
        if (!g.ent.try_ensure(align256(G1 * 4) + 5 * 256, h->stream)) oom("the entries", (double)G1 * 4);
        Arena ae = g.ent.arena();
        g.e_group = ae.alloc<u32>(1);
        g.e_unit = ae.alloc<u32>(1);
        g.e_texts = ae.alloc<u32>(1);
        g.e_value = ae.alloc<double>(1);
        g.goff = ae.alloc<u32>(G1);
    }
    // (the entries of group v are [goff[v], goff[v + 1]): e_group ascends)
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)G + 1, BLOCK), (const u32 *)g.e_group, E, G, goff);
    launches++;
    HIP_CHECK(hipMemcpyAsync(g.goff, goff, ((size_t)G + 1) * 4, hipMemcpyDeviceToDevice, h->stream));
    a.release(stage);                                             // (the postings' arrays are done with once the queue reaches here)

    // ---- the segments: the entries that pass min_texts, compacted
    u32 F = 0, S = 0;
    const u32 *order = nullptr;
    i64 sort_passes = 0;
    if (E) {
        const size_t E1 = (size_t)E + 2;
        u32 *px = a.alloc<u32>(E1), *c_ent = a.alloc<u32>(E1), *c_group = a.alloc<u32>(E1);
        double *c_value = a.alloc<double>(E1);
        F = device_scan_count(ctx, TermsPassIn{g.e_texts, (u32)tp.min_texts}, E, px);
        scans += scan_launches(E + 1u);
        LAUNCH(ctx, terms_compact_kernel, ceil_div_u32(E, BLOCK), (const u32 *)px, E, (const u32 *)g.e_group, (const double *)g.e_value,
               c_ent, c_group, c_value);
        LAUNCH(ctx, terms_seg_offsets_kernel, ceil_div_u32((u64)G + 1, BLOCK), (const u32 *)px, (const u32 *)goff, G, soff);
        launches += 2;
        if (F) {
            // ---- the pre-selection
            u32 *sx = nullptr;
            S = F;
            if (select) {
                const u32 NT = ceil_div_u32(F, TERMS_TILE);
                u32 *partial = a.alloc<u32>((size_t)NT * 2 * TERMS_BINS);
                sx = a.alloc<u32>((size_t)F + 2);
                HIP_CHECK(hipMemsetAsync(bound, 0, (size_t)G * 4, h->stream));
                LAUNCH(ctx, terms_hist_kernel, NT, (const double *)c_value, (const u32 *)soff, G, F, n, bound, partial);
                LAUNCH(ctx, terms_bound_long_kernel, NT, (const u32 *)partial, (const u32 *)soff, G, F, n, bound);
                launches += 2;
                S = device_scan_count(ctx, TermsSelectIn{c_value, c_group, bound}, F, sx);
                scans += scan_launches(F + 1u);
            }
            // ---- by value, then by group: both sorts are stable, and the entries went in by (group, unit)
            SortBufs<u64> vs = sort_bufs_alloc<u64>(a, (size_t)S + 2);
            SortBufs<u32> gs = sort_bufs_alloc<u32>(a, (size_t)S + 2);
            LAUNCH(ctx, terms_value_keys_kernel, ceil_div_u32(F, BLOCK), (const double *)c_value, (const u32 *)sx, F, vs.keys[0], vs.vals[0]);
            const i64 before = stats.radix_passes;
            const int r = radix_sort_pairs<u64>(ctx, vs, S, TERMS_VALUE_BITS);
            LAUNCH(ctx, terms_group_keys_kernel, ceil_div_u32(S, BLOCK), (const u32 *)vs.vals[r], (const u32 *)c_group, S, gs.keys[0], gs.vals[0]);
            const int r2 = radix_sort_pairs<u32>(ctx, gs, S, group_bits);
            sort_passes = stats.radix_passes - before;
            launches += 2;
            order = gs.vals[r2];
            LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)G + 1, BLOCK), (const u32 *)gs.keys[r2], S, G, cand_off);
            launches++;
        }
        LAUNCH(ctx, terms_gather_kernel, ceil_div_u32((u64)G * n, BLOCK), order, (const u32 *)cand_off, S, (const u32 *)soff, (const u32 *)c_ent,
               (const u32 *)g.e_unit, (const double *)g.e_value, (const u32 *)g.e_texts, (const u32 *)U.unit_off, G, n, g.o);
        launches++;
    } else {                                                      // no posting at all: every place is empty
        HIP_CHECK(hipMemsetAsync(g.o.count, 0, (size_t)G * 4, h->stream));
        HIP_CHECK(hipMemsetAsync(g.o.unit, 0xFF, places * 4, h->stream));
        HIP_CHECK(hipMemsetAsync(g.o.texts, 0xFF, places * 4, h->stream));
        HIP_CHECK(hipMemsetAsync(g.o.df, 0xFF, places * 4, h->stream));
        HIP_CHECK(hipMemsetAsync(g.o.value, 0xFF, places * 8, h->stream));      // (every bit set: a NaN)
    }
    timer.finish();
    U.w_valid[tp.weighting] = true;
    g.G = G;
    g.n = n;
    g.E = E;
    g.members = std::move(members);
    g.valid = true;
    passes += sort_passes;
    if (out) {
        out[0] = (i64)D; out[1] = (i64)G; out[2] = (i64)n_units; out[3] = (i64)P; out[4] = (i64)E;
        out[5] = (i64)F; out[6] = (i64)S; out[7] = passes; out[8] = launches + scans + 3 * passes; out[9] = skipped ? 1 : 0;
    }
}

static void terms_fetch(east_hip_index *h, int32_t *members, int32_t *count, int32_t *unit, double *value, int32_t *texts, int32_t *df)
{
    TermsState &g = consumer_built<TermsState>(h, "no characteristic terms have been built on this handle");
    const size_t places = (size_t)g.G * g.n;
    if (members) std::copy(g.members.begin(), g.members.end(), members);
    if (count) HIP_CHECK(hipMemcpyAsync(count, g.o.count, (size_t)g.G * 4, hipMemcpyDeviceToHost, h->stream));
    if (unit) HIP_CHECK(hipMemcpyAsync(unit, g.o.unit, places * 4, hipMemcpyDeviceToHost, h->stream));
    if (value) HIP_CHECK(hipMemcpyAsync(value, g.o.value, places * 8, hipMemcpyDeviceToHost, h->stream));
    if (texts) HIP_CHECK(hipMemcpyAsync(texts, g.o.texts, places * 4, hipMemcpyDeviceToHost, h->stream));
    if (df) HIP_CHECK(hipMemcpyAsync(df, g.o.df, places * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

static void terms_fetch_vectors(east_hip_index *h, i64 *offsets, int32_t *unit, double *value, int32_t *texts)
{
    TermsState &g = consumer_built<TermsState>(h, "no characteristic terms have been built on this handle");
    const size_t E = g.E;
    std::vector<u32> off;
    if (offsets) {
        off.resize((size_t)g.G + 1);
        HIP_CHECK(hipMemcpyAsync(off.data(), g.goff, off.size() * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (unit && E) HIP_CHECK(hipMemcpyAsync(unit, g.e_unit, E * 4, hipMemcpyDeviceToHost, h->stream));
    if (value && E) HIP_CHECK(hipMemcpyAsync(value, g.e_value, E * 8, hipMemcpyDeviceToHost, h->stream));
    if (texts && E) HIP_CHECK(hipMemcpyAsync(texts, g.e_texts, E * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (offsets)
        for (size_t v = 0; v < off.size(); v++) offsets[v] = off[v];
}

extern "C" {

int east_hip_terms_build(east_hip_handle_t h, int32_t weighting, const int32_t *group, int32_t n_groups, int32_t n, int32_t min_texts,
                         int64_t *out)
{
    return guarded([&] { terms_build(h, TermsParams{weighting, group, n_groups, n, min_texts}, out); });
}

int east_hip_terms_fetch(east_hip_handle_t h, int32_t *members, int32_t *count, int32_t *unit, double *value, int32_t *texts, int32_t *df)
{
    return guarded([&] { terms_fetch(h, members, count, unit, value, texts, df); });
}

int east_hip_terms_fetch_vectors(east_hip_handle_t h, int64_t *offsets, int32_t *unit, double *value, int32_t *texts)
{
    return guarded([&] { terms_fetch_vectors(h, offsets, unit, value, texts); });
}

double east_hip_last_terms_ms(east_hip_handle_t h) { return consumer_ms<TermsState>(h); }

int east_hip_debug_set_terms_select(int mode)
{
    // 0: the pre-selection in front of the final sort (the default); 1: none, every entry that passes min_texts is sorted
    if (mode != 0 && mode != 1) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.terms_select = mode; });
    return EAST_HIP_OK;
}

}  // extern "C"
