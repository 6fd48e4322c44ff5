// synonyms.h -- Lin's similarity of words from dependency triples, on the device: the arithmetic half of the reference's
// SynonymExtractor (east/synonyms/synonyms.py:116-169).  The half in front of it (:52-88), which turns text into triples with
// a closed parser, is not here: the host hands over the raw triples (w1, r, w2) as interned ids.
//
//   3 x N ids + the table r -> r' --emit every triple and its inverse (w2, r', w1), each one 64-bit key--> 2N keys
//   --radix_sort.h--> equal keys form a run: one distinct triple t, its length the frequency f(t)
//   --scan.h over "differs from the key in front" (whole key / the key without w2)--> the number of every distinct triple
//     and of its group (w1, r); F_w1r = sum of f^2 over a group, F_r = sum of f^2 over a relation (64-bit integer sums:
//     synonyms.py:129-131 add frequencies[t] once per OCCURRENCE of t); F_rw2(r, w2) = F_w1r(w2, r') is looked up in the
//     group of the inverse triple, which is always in the list
//   --q = (double)f * F_r / F_w1r / F_rw2, exactly these three IEEE operations (-ffp-contract=off); kept iff q > 1.0,
//     I = log(q)--> CSR rows: row = w1, column = the feature (r, w2) ascending (the sort order), row sums in that order
//   --tiles of 16 sources x 256 targets of the candidate list, the sources' rows staged in LDS as sorted (feature, value)
//     lists a chunk at a time; a lane is a target, walks its row once per chunk and looks every entry up in the 16 staged
//     lists by binary search; the numerator of a pair grows in ascending feature order--> a count per (source, target
//     tile)
//   --exclusive scan in (source, target tile) order--> the same tiles once more: (a, b, similarity) of every pair with
//     similarity > threshold, sources in list order, a source's targets in list order
//
// Key layout: w1 << 38 | r << 26 | w2 -- SY_WORD_BITS = 26 bits a word id, SY_REL_BITS = 12 bits a relation id.  More words
// or relations than that are refused (EAST_HIP_ERR_INVALID).
//
// Determinism: the only atomics are 64-bit INTEGER additions (the marginals; integer addition is associative, so their
// order changes nothing).  Every floating-point sum runs in one fixed order and no atomic decides a slot: a pair's slot is
// a prefix sum of counts, as graph.h writes its edges.  Two builds and pair passes of one input give the same bytes.
// The one shortcut is exact: two rows without a common feature have numerator 0, similarity 0.0, which exceeds no
// threshold >= 0 (negative thresholds are refused), so such a pair costs no division.
//
// The host half is a consumer of the handle (consumer.h); its pair list comes out of the frame's count-scan-fill driver.
#pragma once
#include "consumer.h"
#include "radix_sort.h"
#include <math.h>

#define SY_WORD_BITS 26
#define SY_REL_BITS 12
#define SY_FEAT_BITS (SY_WORD_BITS + SY_REL_BITS)
#define SY_WORD_MASK ((1ull << SY_WORD_BITS) - 1ull)
#define SY_REL_MASK ((1ull << SY_REL_BITS) - 1ull)
#define SY_FEAT_MASK ((1ull << SY_FEAT_BITS) - 1ull)
#define SY_SRC 16u                         // sources of a workgroup's tile (their rows in LDS)
#define SY_TGT BLOCK                       // targets of a tile: one a lane
#define SY_MAX_CHUNK 128u                  // entries of a source row staged at a time: 16 x 128 x 16 bytes = 32 KiB (+ the tile's bookkeeping: four workgroups a CU)
#define SY_MAX_CANDIDATES (1u << 20)       // (C * ceil(C / 256) counts must fit 32 bits: a little less than 2^20 in fact)

__device__ __forceinline__ u64 syn_key(u32 w1, u32 r, u32 w2) { return ((u64)w1 << SY_FEAT_BITS) | ((u64)r << SY_WORD_BITS) | (u64)w2; }

// ---- counts ------------------------------------------------------------------------------------------------------------
// synonyms.py:74-86: every raw triple and its inverse
__global__ __launch_bounds__(BLOCK) void syn_emit_kernel(const int32_t *__restrict__ w1, const int32_t *__restrict__ rel,
                                                         const int32_t *__restrict__ w2, const int32_t *__restrict__ inv, u32 N,
                                                         u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const u32 a = (u32)w1[i], r = (u32)rel[i], b = (u32)w2[i];
    keys[2u * i] = syn_key(a, r, b);
    keys[2u * i + 1u] = syn_key(b, (u32)inv[r], a);
    vals[2u * i] = 2u * i;
    vals[2u * i + 1u] = 2u * i + 1u;
}

// d_inc / g_inc: inclusive sums of the heads (RunHeadIn, scan.h) of distinct triples / of groups (w1, r).  The head of run d writes the run's
// key, where it starts and its group; the head of a group writes the group's key (w1 << 12 | r).  d_pos[D] = M.
__global__ __launch_bounds__(BLOCK) void syn_runs_kernel(const u64 *__restrict__ keys, const u32 *__restrict__ d_inc,
                                                         const u32 *__restrict__ g_inc, u32 M, u64 *__restrict__ d_key,
                                                         u32 *__restrict__ d_pos, u32 *__restrict__ d_gid, u64 *__restrict__ g_key)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= M) return;
    const u64 k = keys[i];
    const u64 prev = i ? keys[i - 1u] : ~k;
    if (k != prev) {
        const u32 d = d_inc[i] - 1u, g = g_inc[i] - 1u;
        d_key[d] = k;
        d_pos[d] = i;
        d_gid[d] = g;
        if (i == 0u || (k >> SY_WORD_BITS) != (prev >> SY_WORD_BITS)) g_key[g] = k >> SY_WORD_BITS;
    }
    if (i == M - 1u) d_pos[d_inc[i]] = M;
}

// F_w1r[g] += f^2 over the distinct triples of group g, F_r[r] += f^2 over those of relation r (both zeroed by the host).
// The groups are runs of consecutive d: a wavefront adds up each run it holds by shuffles and the run's first lane adds the
// sum once; the relations are counted in LDS first.  Integer additions only: their order changes nothing.
__global__ __launch_bounds__(BLOCK) void syn_marginals_kernel(const u64 *__restrict__ d_key, const u32 *__restrict__ d_pos,
                                                              const u32 *__restrict__ d_gid, u32 D, u32 R,
                                                              unsigned long long *__restrict__ F_w1r,
                                                              unsigned long long *__restrict__ F_r)
{
    __shared__ unsigned long long lds_r[1u << SY_REL_BITS];
    for (u32 r = threadIdx.x; r < R; r += BLOCK) lds_r[r] = 0ull;
    __syncthreads();
    const u32 lane = lane_id();
    for (u32 base = blockIdx.x * BLOCK; base < D; base += gridDim.x * BLOCK) {      // (the same trip count for the whole workgroup)
        const u32 d = base + threadIdx.x;
        const bool live = d < D;
        u64 x = 0;
        u32 g = 0xFFFFFFFFu;
        if (live) {
            const u64 f = (u64)(d_pos[d + 1u] - d_pos[d]);
            x = f * f;
            g = d_gid[d];
            atomicAdd(&lds_r[(u32)(d_key[d] >> SY_WORD_BITS) & (u32)SY_REL_MASK], (unsigned long long)x);
        }
        const u32 g_prev = __shfl_up(g, 1, WAVE);
        const bool head = live && (lane == 0u || g_prev != g);
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {      // segmented sum towards the run's first lane
            const u64 y = __shfl_down(x, off, WAVE);
            const u32 gy = __shfl_down(g, off, WAVE);
            if (lane + (u32)off < (u32)WAVE && gy == g) x += y;
        }
        if (head) atomicAdd(&F_w1r[g], (unsigned long long)x);
    }
    syncthreads_after_lds_atomics();
    for (u32 r = threadIdx.x; r < R; r += BLOCK)
        if (lds_r[r]) atomicAdd(&F_r[r], lds_r[r]);
}

// ---- features ----------------------------------------------------------------------------------------------------------
// synonyms.py:126-132 for every distinct triple: q with the reference's three operations in its order, kept iff q > 1.0
// (what `I > 0` decides, without the logarithm), I = log(q).
__global__ __launch_bounds__(BLOCK) void syn_features_kernel(const u64 *__restrict__ d_key, const u32 *__restrict__ d_pos,
                                                             const u32 *__restrict__ d_gid, const u64 *__restrict__ g_key, u32 G,
                                                             const unsigned long long *__restrict__ F_w1r,
                                                             const unsigned long long *__restrict__ F_r,
                                                             const int32_t *__restrict__ inv, u32 D, u32 *__restrict__ keep,
                                                             double *__restrict__ value)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= D) return;
    const u64 k = d_key[d];
    const u32 r = (u32)(k >> SY_WORD_BITS) & (u32)SY_REL_MASK, w2 = (u32)(k & SY_WORD_MASK);
    const u64 inverse_group = ((u64)w2 << SY_REL_BITS) | (u64)(u32)inv[r];       // F_rw2(r, w2) = F_w1r(w2, r')
    u32 lo = 0, hi = G;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (g_key[mid] < inverse_group) lo = mid + 1u; else hi = mid;
    }
    const u64 f_rw2 = lo < G && g_key[lo] == inverse_group ? F_w1r[lo] : 0ull;    // (always found: the inverse of every triple is listed)
    const double f = (double)(d_pos[d + 1u] - d_pos[d]);
    const double q = f * (double)F_r[r] / (double)F_w1r[d_gid[d]] / (double)f_rw2;
    const bool kept = f_rw2 != 0ull && q > 1.0;
    keep[d] = kept ? 1u : 0u;
    value[d] = kept ? log(q) : 0.0;
}

__global__ __launch_bounds__(BLOCK) void syn_compact_kernel(const u64 *__restrict__ d_key, const u32 *__restrict__ keep_ex,
                                                            const double *__restrict__ value, u32 D, u64 *__restrict__ feat,
                                                            double *__restrict__ val, u32 *__restrict__ row_of)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= D) return;
    const u32 j = keep_ex[d];
    if (keep_ex[d + 1u] == j) return;
    const u64 k = d_key[d];
    feat[j] = k & SY_FEAT_MASK;
    val[j] = value[d];
    row_of[j] = (u32)(k >> SY_FEAT_BITS);
}

// the divisor's half of a word (synonyms.py:147-148), added in ascending column order
__global__ __launch_bounds__(BLOCK) void syn_row_sum_kernel(const u32 *__restrict__ row_off, const double *__restrict__ val, u32 W,
                                                            double *__restrict__ row_sum)
{
    const u32 w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= W) return;
    double s = 0.0;
    for (u32 p = row_off[w], e = row_off[w + 1u]; p < e; p++) s += val[p];
    row_sum[w] = s;
}

// ---- look-ups ----------------------------------------------------------------------------------------------------------
// synonyms.py:144-152 for a list of pairs of words: a thread merges the two rows, the numerator in ascending column order
__global__ __launch_bounds__(BLOCK) void syn_similarity_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ b, u32 n,
                                                               const u32 *__restrict__ row_off, const u64 *__restrict__ feat,
                                                               const double *__restrict__ val, const double *__restrict__ row_sum,
                                                               double *__restrict__ out)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 wa = (u32)a[i], wb = (u32)b[i];
    u32 p = row_off[wa], q = row_off[wb];
    const u32 pe = row_off[wa + 1u], qe = row_off[wb + 1u];
    double num = 0.0;
    while (p < pe && q < qe) {
        const u64 fa = feat[p], fb = feat[q];
        if (fa == fb) num += val[p] + val[q];
        p += fa <= fb ? 1u : 0u;
        q += fb <= fa ? 1u : 0u;
    }
    const double den = row_sum[wa] + row_sum[wb];
    out[i] = den != 0.0 ? num / den : 0.0;
}

// ---- all pairs ---------------------------------------------------------------------------------------------------------
// Workgroup (sb, tb): sources [16 sb, 16 sb + 16) x targets [256 tb, 256 tb + 256) of the C candidates; the pairs are those
// with source index < target index, so a tile whose last target is no later than its first source leaves at once.  The
// sources' rows lie in LDS, L entries each at a time (L <= SY_MAX_CHUNK; the test knob makes it small).  Lane l of the
// workgroup is target 256 tb + l: for every chunk it walks its own row once and looks each entry up in the 16 staged lists
// (a range check against the list's ends, then a binary search), adding I(source, .) + I(target, .) on a hit.  Chunks ascend
// and so does the walk: the numerator of a pair is added in ascending column order.
// FILL == false: cnt[s * TB + tb] = pairs of source s in target tile tb (the words of tiles that left early stay zero).
// FILL == true: cnt holds the exclusive scan of those counts (modulo 2^32: differences inside a source's row are exact),
// row_base[s] the 64-bit number of pairs in front of source s; a pair goes to row_base[s] + (cnt[s * TB + tb] - cnt[s * TB])
// + the pairs of s in the wavefronts in front of this one + its rank in this wavefront's mask.
template <bool FILL>
__global__ __launch_bounds__(BLOCK) void syn_pairs_kernel(const u32 *__restrict__ cand, u32 C, const u32 *__restrict__ row_off,
                                                          const u64 *__restrict__ feat, const double *__restrict__ val,
                                                          const double *__restrict__ row_sum, u32 L, u32 TB, double threshold,
                                                          u32 *__restrict__ cnt, const u64 *__restrict__ row_base,
                                                          int32_t *__restrict__ out_a, int32_t *__restrict__ out_b,
                                                          double *__restrict__ out_sim)
{
    __shared__ u64 lds_f[SY_SRC * SY_MAX_CHUNK];
    __shared__ double lds_v[SY_SRC * SY_MAX_CHUNK];
    __shared__ u32 lds_beg[SY_SRC], lds_len[SY_SRC], lds_word[SY_SRC];
    __shared__ double lds_sum[SY_SRC];
    __shared__ u32 lds_cnt[WAVES_PER_BLOCK][SY_SRC];
    const u32 tb = blockIdx.x % TB, sb = blockIdx.x / TB;
    const u32 s0 = sb * SY_SRC, t0 = tb * SY_TGT;
    if (t0 + SY_TGT <= s0 + 1u) return;                   // no target behind the first source
    const u32 lane = lane_id(), wv = wave_id();
    if (FILL) {                                           // a tile without a pair: nothing to write
        u32 c = 0;
        const u32 s = s0 + threadIdx.x;
        if (threadIdx.x < SY_SRC && s < C) {
            const size_t i = (size_t)s * TB + tb;
            c = cnt[i + 1u] - cnt[i];
        }
        if (!__syncthreads_or(c != 0u)) return;
    }
    if (threadIdx.x < SY_SRC) {
        const u32 s = s0 + threadIdx.x;
        u32 b = 0, e = 0, w = 0;
        double sum = 0.0;
        if (s < C) { w = cand[s]; b = row_off[w]; e = row_off[w + 1u]; sum = row_sum[w]; }
        lds_beg[threadIdx.x] = b;
        lds_len[threadIdx.x] = e - b;
        lds_word[threadIdx.x] = w;
        lds_sum[threadIdx.x] = sum;
    }
    __syncthreads();
    u32 max_len = 0;
#pragma unroll
    for (u32 s = 0; s < SY_SRC; s++) max_len = max(max_len, lds_len[s]);
    const u32 t = t0 + threadIdx.x;
    u32 tw = 0, t_beg = 0, t_end = 0;
    double t_sum = 0.0;
    if (t < C) { tw = cand[t]; t_beg = row_off[tw]; t_end = row_off[tw + 1u]; t_sum = row_sum[tw]; }
    double acc[SY_SRC];
    u32 shared = 0;                                       // bit s: source s and this target have a feature in common
#pragma unroll
    for (u32 s = 0; s < SY_SRC; s++) acc[s] = 0.0;
    for (u32 c0 = 0; c0 < max_len; c0 += L) {             // (max_len, L: the same for the whole workgroup)
        for (u32 i = threadIdx.x; i < SY_SRC * L; i += BLOCK) {
            const u32 s = i / L, e = i % L;
            if (c0 + e < lds_len[s]) {
                const u32 p = lds_beg[s] + c0 + e;
                lds_f[s * SY_MAX_CHUNK + e] = feat[p];
                lds_v[s * SY_MAX_CHUNK + e] = val[p];
            }
        }
        __syncthreads();
        for (u32 p = t_beg; p < t_end; p++) {
            const u64 tf = feat[p];
            const double tv = val[p];
#pragma unroll
            for (u32 s = 0; s < SY_SRC; s++) {
                const u32 len = lds_len[s];
                if (len <= c0) continue;                  // (the same for the whole workgroup)
                const u32 n = min(L, len - c0);
                const u64 *list = lds_f + s * SY_MAX_CHUNK;
                if (tf < list[0] || tf > list[n - 1u]) continue;
                u32 lo = 0, hi = n;
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if (list[mid] < tf) lo = mid + 1u; else hi = mid;
                }
                if (list[lo] == tf) {                     // (lo < n: tf <= list[n - 1])
                    acc[s] += lds_v[s * SY_MAX_CHUNK + lo] + tv;
                    shared |= 1u << s;
                }
            }
        }
        __syncthreads();
    }
    // synonyms.py:145-152, :162: one IEEE division, strict comparison; acc[s] becomes the similarity
    u32 hits = 0;
#pragma unroll
    for (u32 s = 0; s < SY_SRC; s++) {
        const u32 src = s0 + s;
        double sim = 0.0;
        if (((shared >> s) & 1u) && src < t && t < C) {   // (src < t < C: both are candidates)
            const double den = lds_sum[s] + t_sum;
            sim = den != 0.0 ? acc[s] / den : 0.0;
        }
        acc[s] = sim;
        const bool hit = sim > threshold;
        const u64 mask = __ballot(hit);
        if (hit) hits |= 1u << s;
        if (lane == s) lds_cnt[wv][s] = (u32)__popcll(mask);
    }
    __syncthreads();
    if (!FILL) {
        if (threadIdx.x < SY_SRC && s0 + threadIdx.x < C) {
            u32 c = 0;
#pragma unroll
            for (u32 w = 0; w < WAVES_PER_BLOCK; w++) c += lds_cnt[w][threadIdx.x];
            cnt[(size_t)(s0 + threadIdx.x) * TB + tb] = c;
        }
        return;
    }
#pragma unroll
    for (u32 s = 0; s < SY_SRC; s++) {
        const bool hit = (hits >> s) & 1u;
        const u64 mask = __ballot(hit);
        if (!mask) continue;
        const size_t i = (size_t)(s0 + s) * TB;           // (a hit: s0 + s < C)
        u64 off = row_base[s0 + s] + (u64)(u32)(cnt[i + tb] - cnt[i]);
        for (u32 w = 0; w < wv; w++) off += lds_cnt[w][s];
        if (hit) {
            const u64 o = off + (u64)__popcll(mask & (((u64)1 << lane) - 1ull));
            out_a[o] = (int32_t)lds_word[s];
            out_b[o] = (int32_t)tw;
            out_sim[o] = acc[s];
        }
    }
}

// ============================================================================================================ host ==
// The synonyms' device buffers belong to the handle and to nothing else: not the EASA arena, the cosine buffers or the graph.
struct SynState : Consumer {             // valid: the feature rows; ms: the last build or pair pass
    static constexpr int SLOT = east_hip_index::SLOT_SYN;
    bool pairs_valid = false;
    i64 n_raw = 0, n_distinct = 0, n_features = 0, longest_row = 0, n_pairs = 0;
    u32 W = 0, R = 0;
    DevBuf work, csr, pairs, out;           // build scratch; the CSR rows; candidates + counts; the pair list
    u32 *row_off = nullptr;
    u64 *feat = nullptr;
    double *val = nullptr, *row_sum = nullptr;
    int32_t *o_a = nullptr, *o_b = nullptr;
    double *o_sim = nullptr;
    SynState() { bufs = {&work, &csr, &pairs, &out}; }
    void clear() override
    {
        pairs_valid = false;
        n_raw = n_distinct = n_features = longest_row = n_pairs = 0;
        W = R = 0;
    }
};

static SynState &syn_built(east_hip_index *h) { return consumer_built<SynState>(h, "no synonym features have been built on this handle"); }

static void syn_build(east_hip_index *h, const int32_t *w1, const int32_t *rel, const int32_t *w2, i64 n_triples, const int32_t *inv,
                      i64 n_words, i64 n_relations)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (!w1 || !rel || !w2 || !inv || n_triples < 1 || n_triples >= ((i64)1 << 30))
        east_throw(EAST_HIP_ERR_INVALID, "synonyms: null argument, no triples or 2^30 of them and more");
    if (n_words < 1 || n_words > ((i64)1 << SY_WORD_BITS) || n_relations < 1 || n_relations > ((i64)1 << SY_REL_BITS))
        east_throw(EAST_HIP_ERR_INVALID, "synonyms: at most 2^26 words and 2^12 relations fit the 64-bit triple key");
    for (i64 r = 0; r < n_relations; r++)
        if (inv[r] < 0 || inv[r] >= n_relations || inv[inv[r]] != r)
            east_throw(EAST_HIP_ERR_INVALID, "synonyms: the inverse-relation table is not an involution of the relation ids");
    for (i64 i = 0; i < n_triples; i++)
        if (w1[i] < 0 || w1[i] >= n_words || w2[i] < 0 || w2[i] >= n_words || rel[i] < 0 || rel[i] >= n_relations)
            east_throw(EAST_HIP_ERR_INVALID, "synonyms: a triple names a word or a relation outside the given counts");
    use_device(h);
    SynState &g = consumer_begin<SynState>(h);
    g.pairs_valid = false;
    const u32 N = (u32)n_triples, M = 2u * N, W = (u32)n_words, R = (u32)n_relations;
    Stats stats;
    Ctx ctx = handle_ctx(h, nullptr, &stats);
    g.work.ensure((size_t)M * 84 + (size_t)N * 12 + (size_t)R * 12 + (size_t)M / 2 + ((size_t)4 << 20), "the synonyms' triples", h->stream);
    Arena a = g.work.arena();
    ctx.arena = &a;
    ConsumerTimer timer(h, g);
    int32_t *d_w1 = a.alloc<int32_t>(N), *d_rel = a.alloc<int32_t>(N), *d_w2 = a.alloc<int32_t>(N), *d_inv = a.alloc<int32_t>(R);
    HIP_CHECK(hipMemcpyAsync(d_w1, w1, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_rel, rel, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_w2, w2, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_inv, inv, (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
    SortBufs<u64> sb = sort_bufs_alloc<u64>(a, M);
    LAUNCH(ctx, syn_emit_kernel, ceil_div_u32(N, BLOCK), (const int32_t *)d_w1, (const int32_t *)d_rel, (const int32_t *)d_w2,
           (const int32_t *)d_inv, N, sb.keys[0], sb.vals[0]);
    const int sorted = radix_sort_pairs<u64>(ctx, sb, M, SY_FEAT_BITS + std::max(1, bit_width_u32(W - 1u)));
    const u64 *keys = sb.keys[sorted];
    u32 *d_inc = a.alloc<u32>(M), *g_inc = a.alloc<u32>(M);
    device_scan<RunHeadIn<u64>, true>(ctx, RunHeadIn<u64>{keys, 0}, M, d_inc);
    device_scan<RunHeadIn<u64>, true>(ctx, RunHeadIn<u64>{keys, SY_WORD_BITS}, M, g_inc);
    u32 D = 0, G = 0;
    device_read_words(ctx, {{&D, d_inc + (M - 1u)}, {&G, g_inc + (M - 1u)}});
    u64 *d_key = a.alloc<u64>(D), *g_key = a.alloc<u64>(G);
    u32 *d_pos = a.alloc<u32>((size_t)D + 1), *d_gid = a.alloc<u32>(D);
    unsigned long long *F_w1r = a.alloc<unsigned long long>(G), *F_r = a.alloc<unsigned long long>(R);
    u32 *keep = a.alloc<u32>(D), *keep_ex = a.alloc<u32>((size_t)D + 1);
    double *value = a.alloc<double>(D);
    LAUNCH(ctx, syn_runs_kernel, ceil_div_u32(M, BLOCK), keys, (const u32 *)d_inc, (const u32 *)g_inc, M, d_key, d_pos, d_gid, g_key);
    HIP_CHECK(hipMemsetAsync(F_w1r, 0, (size_t)G * 8, h->stream));
    HIP_CHECK(hipMemsetAsync(F_r, 0, (size_t)R * 8, h->stream));
    LAUNCH(ctx, syn_marginals_kernel, std::min<u32>(ceil_div_u32(D, BLOCK), 2048u), (const u64 *)d_key, (const u32 *)d_pos,
           (const u32 *)d_gid, D, R, F_w1r, F_r);
    LAUNCH(ctx, syn_features_kernel, ceil_div_u32(D, BLOCK), (const u64 *)d_key, (const u32 *)d_pos, (const u32 *)d_gid,
           (const u64 *)g_key, G, (const unsigned long long *)F_w1r, (const unsigned long long *)F_r, (const int32_t *)d_inv, D, keep,
           value);
    const u32 F = device_scan_count(ctx, ArrIn{keep}, D, keep_ex);
    const size_t al = 256;
    g.csr.ensure(((size_t)W + 1) * 4 + (size_t)F * 16 + (size_t)W * 8 + 8 * al, "the synonyms' feature rows", h->stream);
    Arena c = g.csr.arena();
    g.row_off = c.alloc<u32>((size_t)W + 1);
    g.feat = c.alloc<u64>(std::max<u32>(F, 1u));
    g.val = c.alloc<double>(std::max<u32>(F, 1u));
    g.row_sum = c.alloc<double>(W);
    u32 *row_of = a.alloc<u32>(std::max<u32>(F, 1u));
    LAUNCH(ctx, syn_compact_kernel, ceil_div_u32(D, BLOCK), (const u64 *)d_key, (const u32 *)keep_ex, (const double *)value, D, g.feat,
           g.val, row_of);
    // (row_of ascends: the kept entries of word w are [row_off[w], row_off[w + 1]))
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)W + 1, BLOCK), (const u32 *)row_of, F, W, g.row_off);
    LAUNCH(ctx, syn_row_sum_kernel, ceil_div_u32(W, BLOCK), (const u32 *)g.row_off, (const double *)g.val, W, g.row_sum);
    std::vector<u32> off((size_t)W + 1);
    HIP_CHECK(hipMemcpyAsync(off.data(), g.row_off, ((size_t)W + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    timer.finish();
    u32 longest = 0;
    for (u32 w = 0; w < W; w++) longest = std::max(longest, off[w + 1] - off[w]);
    g.n_raw = N;
    g.n_distinct = D;
    g.n_features = F;
    g.longest_row = longest;
    g.W = W;
    g.R = R;
    g.n_pairs = 0;
    g.valid = true;
}

template <bool FILL>
static void syn_launch_pairs(Ctx &ctx, u32 grid, const SynState &g, const u32 *cand, u32 C, u32 L, u32 TB, double threshold, u32 *cnt,
                             const u64 *row_base, int32_t *o_a, int32_t *o_b, double *o_sim)
{
    LAUNCH_NAMED(ctx, FILL ? "syn_pairs_fill_kernel" : "syn_pairs_count_kernel", (syn_pairs_kernel<FILL>), grid, cand, C,
                 (const u32 *)g.row_off, (const u64 *)g.feat, (const double *)g.val, (const double *)g.row_sum, L, TB, threshold, cnt,
                 row_base, o_a, o_b, o_sim);
}

static void syn_pairs(east_hip_index *h, const int32_t *candidates, i64 n_candidates, double threshold, i64 *n_pairs)
{
    SynState &g = syn_built(h);
    if (n_candidates < 0 || n_candidates > (i64)SY_MAX_CANDIDATES || (n_candidates > 0 && !candidates))
        east_throw(EAST_HIP_ERR_INVALID, "synonyms: null candidates, or more than 2^20 of them");
    if (!(threshold >= 0.0)) east_throw(EAST_HIP_ERR_INVALID, "synonyms: the threshold is negative or not a number");
    {
        std::vector<bool> seen(g.W, false);
        for (i64 i = 0; i < n_candidates; i++) {
            if (candidates[i] < 0 || (u32)candidates[i] >= g.W) east_throw(EAST_HIP_ERR_INVALID, "synonyms: a candidate is not a word id");
            if (seen[candidates[i]]) east_throw(EAST_HIP_ERR_INVALID, "synonyms: a candidate is listed twice");
            seen[candidates[i]] = true;
        }
    }
    use_device(h);
    g.pairs_valid = false;
    g.ms = -1.f;
    g.n_pairs = 0;
    const u32 C = (u32)n_candidates;
    Stats stats;
    Ctx ctx = handle_ctx(h, nullptr, &stats);
    const u32 L = (u32)std::min<int>(std::max(ctx.knobs.syn_chunk, 1), (int)SY_MAX_CHUNK);
    ConsumerTimer timer(h, g);
    if (C >= 2u) {
        const u32 TB = ceil_div_u32(C, SY_TGT), grid = ceil_div_u32(C, SY_SRC) * TB;
        const EmitCounts e = emit_counts(C, TB, "synonyms: more candidates than one pair pass counts");
        g.pairs.ensure((size_t)C * 4 + e.bytes, "the synonyms' pair counts", h->stream);
        Arena b = g.pairs.arena();
        ctx.arena = &b;
        u32 *cand = b.alloc<u32>(C);
        HIP_CHECK(hipMemcpyAsync(cand, candidates, (size_t)C * 4, hipMemcpyHostToDevice, h->stream));
        g.n_pairs = (i64)emit_count_scan_fill(
            ctx, e, true,                                     // (the tiles that leave early write no count)
            [&](u32 *cnt) { syn_launch_pairs<false>(ctx, grid, g, cand, C, L, TB, threshold, cnt, nullptr, nullptr, nullptr, nullptr); },
            [&](u64 E) {
                const size_t ib = align256((size_t)E * 4), db = align256((size_t)E * 8);
                g.out.ensure(2 * ib + db, "the synonym pairs", h->stream);
                g.o_a = (int32_t *)g.out.p;
                g.o_b = (int32_t *)(g.out.p + ib);
                g.o_sim = (double *)(g.out.p + 2 * ib);
            },
            [&](u32 *cnt, const u64 *row_base) {
                syn_launch_pairs<true>(ctx, grid, g, cand, C, L, TB, threshold, cnt, row_base, g.o_a, g.o_b, g.o_sim);
            });
    }
    timer.finish();
    g.pairs_valid = true;
    if (n_pairs) *n_pairs = g.n_pairs;
}

extern "C" {

int east_hip_synonyms_build(east_hip_handle_t h, const int32_t *w1, const int32_t *relation, const int32_t *w2, int64_t n_triples,
                            const int32_t *inverse_relation, int32_t n_words, int32_t n_relations)
{
    return guarded([&] { syn_build(h, w1, relation, w2, n_triples, inverse_relation, n_words, n_relations); });
}

int east_hip_synonyms_info(east_hip_handle_t h, int64_t *out, int32_t cap)
{
    if (!h || !out) return EAST_HIP_ERR_INVALID;
    return guarded([&] {
        SynState &g = syn_built(h);
        const int64_t v[6] = {g.n_raw, g.n_distinct, (int64_t)g.W, (int64_t)g.R, g.n_features, g.longest_row};
        for (int i = 0; i < 6 && i < cap; i++) out[i] = v[i];
    });
}

int east_hip_synonyms_get_rows(east_hip_handle_t h, int64_t *offsets, int32_t *relation, int32_t *word, double *value,
                               double *row_sum)
{
    return guarded([&] {
        SynState &g = syn_built(h);
        use_device(h);
        const size_t F = (size_t)g.n_features;
        std::vector<u32> off(offsets ? (size_t)g.W + 1 : 0);
        std::vector<u64> feat(relation || word ? F : 0);
        if (offsets) HIP_CHECK(hipMemcpyAsync(off.data(), g.row_off, ((size_t)g.W + 1) * 4, hipMemcpyDeviceToHost, h->stream));
        if (!feat.empty()) HIP_CHECK(hipMemcpyAsync(feat.data(), g.feat, F * 8, hipMemcpyDeviceToHost, h->stream));
        if (value && F) HIP_CHECK(hipMemcpyAsync(value, g.val, F * 8, hipMemcpyDeviceToHost, h->stream));
        if (row_sum) HIP_CHECK(hipMemcpyAsync(row_sum, g.row_sum, (size_t)g.W * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < off.size(); i++) offsets[i] = (int64_t)off[i];
        for (size_t i = 0; i < feat.size(); i++) {
            if (relation) relation[i] = (int32_t)(feat[i] >> SY_WORD_BITS);
            if (word) word[i] = (int32_t)(feat[i] & SY_WORD_MASK);
        }
    });
}

int east_hip_synonyms_similarity(east_hip_handle_t h, const int32_t *a, const int32_t *b, int64_t n_pairs, double *out)
{
    return guarded([&] {
        SynState &g = syn_built(h);
        if (n_pairs < 0 || n_pairs >= (i64)0x7FFFFFF0 || (n_pairs > 0 && (!a || !b || !out)))
            east_throw(EAST_HIP_ERR_INVALID, "synonyms: null argument or too many pairs");
        for (i64 i = 0; i < n_pairs; i++)
            if (a[i] < 0 || (u32)a[i] >= g.W || b[i] < 0 || (u32)b[i] >= g.W) east_throw(EAST_HIP_ERR_INVALID, "synonyms: a pair names no word id");
        if (!n_pairs) return;
        use_device(h);
        const u32 n = (u32)n_pairs;
        // (the pair pass's buffer: a look-up withdraws the counts of the last pair pass, not its fetched list)
        g.pairs.ensure((size_t)n * 16 + 4 * 256, "the synonyms' look-ups", h->stream);
        Arena ar = g.pairs.arena();
        int32_t *d_a = ar.alloc<int32_t>(n), *d_b = ar.alloc<int32_t>(n);
        double *d_out = ar.alloc<double>(n);
        Ctx ctx = handle_ctx(h);
        HIP_CHECK(hipMemcpyAsync(d_a, a, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(d_b, b, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        LAUNCH(ctx, syn_similarity_kernel, ceil_div_u32(n, BLOCK), (const int32_t *)d_a, (const int32_t *)d_b, n, (const u32 *)g.row_off,
               (const u64 *)g.feat, (const double *)g.val, (const double *)g.row_sum, d_out);
        HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int east_hip_synonyms_pairs(east_hip_handle_t h, const int32_t *candidates, int32_t n_candidates, double threshold, int64_t *n_pairs)
{
    return guarded([&] { syn_pairs(h, candidates, n_candidates, threshold, n_pairs); });
}

int east_hip_synonyms_fetch(east_hip_handle_t h, int32_t *a, int32_t *b, double *similarity)
{
    return guarded([&] {
        SynState &g = syn_built(h);
        if (!g.pairs_valid) east_throw(EAST_HIP_ERR_NOT_BUILT, "no synonym pairs have been computed on this handle");
        use_device(h);
        const size_t E = (size_t)g.n_pairs;
        if (a && E) HIP_CHECK(hipMemcpyAsync(a, g.o_a, E * 4, hipMemcpyDeviceToHost, h->stream));
        if (b && E) HIP_CHECK(hipMemcpyAsync(b, g.o_b, E * 4, hipMemcpyDeviceToHost, h->stream));
        if (similarity && E) HIP_CHECK(hipMemcpyAsync(similarity, g.o_sim, E * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

double east_hip_last_synonyms_ms(east_hip_handle_t h) { return consumer_ms<SynState>(h); }

int east_hip_debug_set_synonyms_chunk(int entries)
{
    // row entries of a source staged in LDS at a time by the pair kernel: 1 .. SY_MAX_CHUNK (128); 0 or less: the default (128)
    knobs_update([&](Knobs &k) { k.syn_chunk = entries > 0 ? std::min(entries, (int)SY_MAX_CHUNK) : (int)SY_MAX_CHUNK; });
    return EAST_HIP_OK;
}

}  // extern "C"
