// window_sort.h -- the key generators and kernels of the window sort over all suffixes (construction A of
// dc3.h's header) and of the level-0 machinery it shares with DC3's sample sort on the byte stream:
//
//   WindowSrc / KeyNeqWindowIn   w-symbol window keys (generated inside the first radix pass) and the
//                                naming predicate on the sorted keys
//   lvl0_place_kernel            one pass that places every untied suffix and every small tie group,
//                                with the LCP entries (one document)
//   lvl0_finish_kernel           the same fused with the sort's last digit
//   refinement rounds            large tie groups: compacted domains keyed by (group, next window),
//                                prefix doubling for long repeats, direct endgame on small domains
// The host drivers of all of the above (dc3_level0_bytes, window_suffix_sort) live in level0.h.
#pragma once
#include "common.h"
#include "radix_sort.h"
#include "scan.h"
#include "ht_code.h"
#include <math.h>
#include <algorithm>

__device__ __forceinline__ u32 dc3_sample_pos(u32 t, u32 n0)
{
    return t < n0 ? 3u * t + 1u : 3u * (t - n0) + 2u;
}

// Level 0 on the byte stream runs either over the DC3 sample (element t = sample number, n0 > 0)
// or over ALL suffixes (n0 == 0: element t = text position), see window_suffix_sort.
__device__ __forceinline__ u32 lvl0_pos(u32 t, u32 n0) { return n0 ? dc3_sample_pos(t, n0) : t; }
#include "lds_group_sort.h"
#include "persist_rounds.h"
// (the test knobs of this file live in Ctx::knobs -- common.h: Knobs)
struct FusedAbort {};           // the fused finish met a repeat too long to order directly: the level is redone with the full sort

#define RESOLVE_MAX_LEN 2048            // longest direct comparison of two suffixes (symbols)

// ---- window keys -------------------------------------------------------------------------------
// A suffix is keyed by its first w symbols (w >= 3, w*bits <= 64), packed at `bits` per symbol.
// Level 0 of an EASA build: every symbol >= the terminator class is a unique string terminator,
// ordered by its position in the corpus.  All terminators share the code term_first in the key
// and the symbols behind the first terminator are dropped; suffixes are enumerated in text order,
// so the STABLE sort leaves equal keys in position order = terminator order, and a key holding a
// terminator is unique.  For DC3's sample (n0 > 0) any order-preserving name over a window that
// covers the triple keeps DC3 correct -- comparing (name(i), name(i+3), ...) still walks the two
// suffixes left to right.
// The key bits left over below the w full symbols (`spare`) take the top bits of symbol w+1:
// still order-preserving, and it thins the ties out further for free.
// Several documents in one shard (all-suffix mode): the document number sits ABOVE the window in the key,
// so one sort yields every document's own suffix array side by side -- no partition afterwards --
// and the window only has to tell the suffixes of ONE document apart.
struct DocKey {
    const u32 *doc_off = nullptr;   // n_docs + 1 offsets into the shard (device)
    u32 n_docs = 1;
    int bits = 0;                   // bit_width(n_docs - 1); 0 = one document
    const u32 *tile_doc = nullptr;  // document of position t << DOC_TILE_SHIFT (filled by dc3_level0_bytes)
    const u32 *h_doc_off = nullptr; // the offsets on the host (nullptr in a sizing run)
    // Segmented sort (radix_sort.h: RsSeg; set by window_suffix_sort): every pass keeps the documents in their own ranges,
    // the keys hold NO document number (bits = 0 then) -- 6-8 more bits of text in the same passes.  What told the
    // documents apart in the keys still holds at the seams: a document's last ranks are its terminator-first suffixes
    // (the terminator class is the largest code), and a key that holds a terminator never ties.
    RsSeg seg;
};
#define DOC_TILE_SHIFT 12

// The score walk's k-gram bucket tables (score.h) can be read off the sorted window keys for free: rank j
// opens a bucket of its document iff the leading k symbol fields (or the document number) of its key
// differ from the key before -- exactly "k-gram class code differs", terminator class and the zeroes
// behind it included.  The placement pass writes those entries (kg[d][code] = rank inside the document;
// the table was preset to 0xFFFFFFFF), the score side only has to run the suffix-minimum fill.
// pairs (k >= 2): the table of the last level holds 8-byte entries {rank, text position of the suffix at that rank} and
// stays UNFILLED (empty buckets keep 0xFFFFFFFF; the walk of score.h looks for a bucket's end among the next entries),
// and the levels above it get a table of their own, kg3 (k - 1 symbols, 4-byte entries, filled on the score side: it is
// A times smaller).  A walk that arrives in a bucket of ONE suffix -- most do -- then has that suffix's position with
// the entry it read anyway, instead of behind a dependent read of the suffix array; the position is only ever used for
// such buckets, whose suffix is untied and therefore final when the mark is written.
struct KgMark {
    u32 *kg = nullptr;              // n_docs rows of bins + 1 entries
    int k = 0;                      // on entry: the largest k the table has room for; on return: the k marked (<= w)
    u32 A = 0, bins = 0;            // alphabet of the class codes (sigma_text + 2), A^k
    const u32 *doc_off = nullptr;
    u32 n_docs = 1;
    u32 *kg3 = nullptr;             // pairs: n_docs rows of bins / A + 1 entries
    int pairs = 0;
    int by_rank = 0;                // segmented sort: the keys hold no document number -- the document comes from the rank
};

// the document of rank j (documents side by side: d with doc_off[d] <= j < doc_off[d + 1])
__device__ __forceinline__ u32 doc_of_rank(const u32 *__restrict__ doc_off, u32 n_docs, u32 j)
{
    u32 lo = 0, hi = n_docs;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (doc_off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// Segmented first-level sort: the sorted keys are sorted inside every document's range of ranks only -- "an equal key
// `limit` places away means more than `limit` equal keys around this one" holds inside a document, and the kernels that
// use it ask for the bounds of the document a rank lies in (d0: the document of a rank at or in front of j, found once
// per workgroup).  n_docs = 0: one range, [0, m).
struct SegRanks {
    const u32 *doc_off = nullptr;
    u32 n_docs = 0;
};
// (the document of the stretch's first rank and its range of ranks, staged in LDS by the workgroup: nearly every rank of
// the stretch lies in it, and the question costs two LDS reads instead of two global loads)
struct DocHint {
    u32 d0, lo, hi;
};
__device__ __forceinline__ void seg_doc_bounds(const SegRanks &sr, const DocHint &h, u32 j, u32 &lo, u32 &hi)
{
    if (j < h.hi) { lo = h.lo; hi = h.hi; return; }
    u32 d = h.d0 + 1u;
    while (d + 1 < sr.n_docs && j >= sr.doc_off[d + 1]) d++;
    lo = sr.doc_off[d];
    hi = sr.doc_off[d + 1];
}
__device__ __forceinline__ DocHint doc_hint_of_rank(const u32 *__restrict__ doc_off, u32 n_docs, u32 j)
{
    const u32 d = doc_of_rank(doc_off, n_docs, j);
    return DocHint{d, doc_off[d], doc_off[d + 1]};
}

// rank j (key k, the key before it kp, its suffix v) opens a k-gram bucket of its document?  Then write the mark(s).
// (hint, by_rank only: the document of the first rank of the workgroup's stretch)
// (SEG: 0 / 1 = km.by_rank known at compile time, 2 = read at run time)
template <class K, int SEG = 2>
__device__ __forceinline__ void kg_mark_key(const KgMark &km, int w, int b, int spare, u32 j, K k, K kp, u32 v,
                                            const DocHint &hint = DocHint{0u, 0u, 0u})
{
    const int top = spare + (w - km.k) * b;
    const bool same = j != 0 && (K)(k >> top) == (K)(kp >> top);
    u32 d = 0, dlo = 0;
    bool by_rank = true;
    if (SEG == 1 || (SEG == 2 && km.by_rank)) {
        // equal class codes: the same bucket -- unless this is the first rank of a document; the key before it is then the
        // last of the document before, terminator first, and so is this one
        if (same && ((u32)(k >> (spare + (w - 1) * b)) & ((1u << b) - 1u)) != km.A - 1u) return;
        d = hint.d0;
        dlo = hint.lo;
        if (j >= hint.hi) {                             // (a seam inside the stretch)
            d++;
            while (d + 1 < km.n_docs && j >= km.doc_off[d + 1]) d++;
            dlo = km.doc_off[d];
        }
        if (same && j != dlo) return;
    } else {
        if (same) return;
        d = km.n_docs > 1 ? (u32)(k >> (w * b + spare)) : 0u;   // (one document: no bits above the window)
        by_rank = false;
    }
    u32 code = 0;
    for (int q = 0; q < km.k; q++) code = code * km.A + ((u32)(k >> (spare + (w - 1 - q) * b)) & ((1u << b) - 1u));
    if (code >= km.bins) return;                        // (only in a speculative build that assumed the wrong alphabet)
    // (read here, behind the code: measured -- 0.45 against 0.42 ms for the 64 MiB finish; one document starts at rank 0)
    if (!by_rank) dlo = km.n_docs > 1 ? km.doc_off[d] : 0u;
    const u32 jl = j - dlo;
    if (!km.pairs) { km.kg[(size_t)d * (km.bins + 1) + code] = jl; return; }
    reinterpret_cast<uint2 *>(km.kg)[(size_t)d * (km.bins + 1) + code] = uint2{jl, v};
    const int top3 = top + b;                           // the level above: k - 1 symbols
    if (j == 0 || jl == 0 || (K)(k >> top3) != (K)(kp >> top3)) km.kg3[(size_t)d * (km.bins / km.A + 1) + code / km.A] = jl;
}

__global__ __launch_bounds__(BLOCK) void doc_tiles_kernel(const u32 *__restrict__ doc_off, u32 n_docs, u32 n_tiles,
                                                          u32 *__restrict__ tile_doc)
{
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_tiles) return;
    const u32 p = t << DOC_TILE_SHIFT;
    u32 lo = 0, hi = n_docs;                    // last d with doc_off[d] <= p
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (doc_off[mid] <= p) lo = mid; else hi = mid;
    }
    tile_doc[t] = lo;
}

template <class K> struct WindowSrc {          // the (window key, element) pairs, generated by the first radix pass
    static constexpr int MODE = 1;             // (element by element: DC3's sample, n0 > 0)
    const uint8_t *s8;
    u32 n0;
    int w, b, spare;
    u32 term_first;
    DocKey docs;
    __device__ __forceinline__ K key(u32 u) const
    {
        K key = window(u);
        if (docs.bits) {                            // (all-suffix mode: u is the text position)
            // the document of the 4096-position tile's first position, then a step forward where a
            // document boundary falls inside the tile (two loads, the same for nearly every lane)
            u32 lo = docs.tile_doc[u >> DOC_TILE_SHIFT];
            while (lo + 1 < docs.n_docs && docs.doc_off[lo + 1] <= u) lo++;
            key |= (K)lo << (w * b + spare);
        }
        return key;
    }
    __device__ __forceinline__ K window(u32 u) const
    {
        const u32 p = n0 ? 3u * (u >> 1) + 1u + (u & 1u) : u;     // text order either way (the sort is stable)
        u64 lo8, hi8;                               // w <= 12 symbols: two unaligned 8-byte loads
        __builtin_memcpy(&lo8, s8 + p, 8);
        __builtin_memcpy(&hi8, s8 + p + 8, 8);
        K key = 0;
        bool ended = false;
        for (int i = 0; i < w; i++) {
            const u32 byte = (u32)((i < 8 ? lo8 >> (8 * i) : hi8 >> (8 * (i - 8))) & 0xFFu);
            const u32 x = ended ? 0u : byte;
            ended = ended || x == 0xFFu;
            key = (key << b) | (K)(x == 0xFFu ? term_first : x);
        }
        if (spare > 0) {
            const u32 byte = (u32)((w < 8 ? lo8 >> (8 * w) : hi8 >> (8 * (w - 8))) & 0xFFu);
            const u32 x = ended ? 0u : (byte == 0xFFu ? term_first : byte);
            key = (key << spare) | (K)(x >> (b - spare));
        }
        return key;
    }
    __device__ __forceinline__ u32 val(u32 u) const { return n0 ? ((u & 1u) ? n0 + (u >> 1) : (u >> 1)) : u; }
    // the low 8 bits of key(u) alone -- all the first pass's histogram needs: only the last one or two
    // symbols of the window (and the partial one) are decoded; where the first terminator sits comes from a
    // zero-byte test on the loaded bytes
    __device__ __forceinline__ u32 low_digit(u32 u) const
    {
        const u32 p = n0 ? 3u * (u >> 1) + 1u + (u & 1u) : u;
        u64 lo8, hi8;
        __builtin_memcpy(&lo8, s8 + p, 8);
        __builtin_memcpy(&hi8, s8 + p + 8, 8);
        const u64 zl = ~lo8, zh = ~hi8;                 // zero byte <=> 0xFF
        const u64 tl = (zl - 0x0101010101010101ull) & ~zl & 0x8080808080808080ull;
        const u64 th = (zh - 0x0101010101010101ull) & ~zh & 0x8080808080808080ull;
        const int tpos = tl ? __builtin_ctzll(tl) >> 3 : (th ? 8 + (__builtin_ctzll(th) >> 3) : 16);
        const int m = (8 - spare + b - 1) / b < w ? (8 - spare + b - 1) / b : w;     // full symbols reaching into the low byte
        u32 acc = 0;
        for (int i = w - m; i < w; i++) {
            const u32 byte = (u32)((i < 8 ? lo8 >> (8 * i) : hi8 >> (8 * (i - 8))) & 0xFFu);
            const u32 x = i > tpos ? 0u : byte;
            acc = (acc << b) | (x == 0xFFu ? term_first : x);
        }
        if (spare > 0) {
            const u32 byte = (u32)((w < 8 ? lo8 >> (8 * w) : hi8 >> (8 * (w - 8))) & 0xFFu);
            const u32 x = w > tpos ? 0u : (byte == 0xFFu ? term_first : byte);
            acc = (acc << spare) | (x >> (b - spare));
        }
        return acc & 255u;
    }
};

// The same keys for ALL suffixes in text order (n0 == 0, element u = text position u), a tile at a time:
// a thread takes 8 consecutive positions, loads their 21 bytes once (three aligned 8-byte loads) and
// rolls the keys out from right to left --
//     key(q) = code(x[q]) on top of [ the fields of key(q + 1) moved down one place ],   all zero behind a terminator
// -- so that a key costs a dozen integer operations instead of its own two unaligned loads and a loop
// over its symbols, and the truncation at the first terminator comes with the recurrence.  The radix
// sort's first pass calls fill_tile (keys into LDS, no round trip through HBM) and hist_tile (digit
// histogram of a tile).
#define TW_RUN 8
template <class K> struct TextWindowGen {
    static constexpr int MODE = 2;
    const uint8_t *s8;                          // byte stream; readable (any content) up to 24 bytes behind the last symbol
    u32 n;
    int w, b, spare;
    u32 term_first;
    DocKey docs;

    __device__ __forceinline__ void prepare() const {}
    // keys of the positions p0 .. p0 + 7 from x = the bytes s8[p0 .. p0 + 24)
    template <int RUN = TW_RUN>
    __device__ __forceinline__ void keys_of_run(const u32 (&x)[6], K (&out)[RUN]) const
    {
        const int top = spare + (w - 1) * b;
        const K fmask = ((K)1 << b) - 1;
        K key = 0;
#pragma unroll
        for (int q = RUN + 12; q >= 0; q--) {
            if (q > RUN + w) continue;          // (uniform: the run starts w + 1 symbols to the right, from zero)
            const u32 c = (x[q >> 2] >> ((q & 3) * 8)) & 0xFFu;
            const bool term = c == 0xFFu;
            const K body = key >> spare;        // the w full fields of key(q + 1)
            const K rest = (K)((body >> b) << spare) | (K)((body & fmask) >> (b - spare));
            key = ((K)(term ? term_first : c) << top) | (term ? (K)0 : rest);
            if (q < RUN) out[q] = key;
        }
    }
    __device__ __forceinline__ void load_run(u32 p0, u32 (&x)[6]) const
    {
        // (p0 is a multiple of 8 where the tiles start at multiples of RS_TILE; a document's own tiles start anywhere)
        uint2 a, c, e;
        __builtin_memcpy(&a, s8 + p0, 8);
        __builtin_memcpy(&c, s8 + p0 + 8, 8);
        __builtin_memcpy(&e, s8 + p0 + 16, 8);
        x[0] = a.x; x[1] = a.y; x[2] = c.x; x[3] = c.y; x[4] = e.x; x[5] = e.y;
    }
    // the document number on top of the keys of a run (several documents per shard)
    __device__ __forceinline__ void add_docs(u32 p0, K (&out)[TW_RUN]) const
    {
        u32 lo = docs.tile_doc[p0 >> DOC_TILE_SHIFT];
        const int at = w * b + spare;
        // (the document of the run's first position; inside the run the next document's offset is compared against, one
        // load per run instead of one per position -- a run of 8 positions crosses a document border once in 10^5 runs)
        while (lo + 1 < docs.n_docs && docs.doc_off[lo + 1] <= p0) lo++;
        u32 next_off = lo + 1 < docs.n_docs ? docs.doc_off[lo + 1] : 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < TW_RUN; q++) {
            while (p0 + q >= next_off) {
                lo++;
                next_off = lo + 1 < docs.n_docs ? docs.doc_off[lo + 1] : 0xFFFFFFFFu;
            }
            out[q] |= (K)lo << at;
        }
    }
    __device__ __forceinline__ void fill_tile(K *s_keys, u32 tile_base, u32 tile_count) const
    {
        if (!docs.bits) {
            // no document number to add: runs of RS_IPT = 4 positions, so that every thread of the scatter workgroup rolls
            // one out (a run of 8 costs 8 + w + 1 steps of the recurrence and leaves half of the threads idle; one of 4
            // costs 4 + w + 1 steps on all of them)
            constexpr int HALF = TW_RUN / 2;
            for (u32 r = threadIdx.x; r < (u32)RS_TILE / HALF; r += RS_THREADS) {
                if (r * HALF >= tile_count) break;
                u32 x[6];
                K k[HALF];
                load_run(tile_base + r * HALF, x);
                keys_of_run<HALF>(x, k);
                if constexpr (sizeof(K) == 4) *reinterpret_cast<uint4 *>(&s_keys[r * HALF]) = uint4{(u32)k[0], (u32)k[1], (u32)k[2], (u32)k[3]};
                else {
#pragma unroll
                    for (int q = 0; q < HALF; q++) s_keys[r * HALF + q] = k[q];
                }
            }
            return;
        }
        for (u32 r = threadIdx.x; r < (u32)RS_TILE / TW_RUN; r += RS_THREADS) {
            if (r * TW_RUN >= tile_count) break;
            u32 x[6];
            K k[TW_RUN];
            load_run(tile_base + r * TW_RUN, x);
            keys_of_run(x, k);
            if (docs.bits) add_docs(tile_base + r * TW_RUN, k);
#pragma unroll
            for (int q = 0; q < TW_RUN; q++) s_keys[r * TW_RUN + q] = k[q];
        }
    }
    // digit histogram of the positions [e0, e1) of a tile, by ONE wave
    template <bool CHECK = true> __device__ __forceinline__ void hist_tile(u32 *mine, u32 e0, u32 e1, int shift, u32 mask) const
    {
        const bool need_docs = docs.bits && w * b + spare < shift + 12;     // (a digit only sees the document number of short windows)
        for (u32 p0 = e0 + lane_id() * TW_RUN; p0 < e1; p0 += WAVE * TW_RUN) {
            u32 x[6];
            K k[TW_RUN];
            load_run(p0, x);
            keys_of_run(x, k);
            if (need_docs) add_docs(p0, k);
#pragma unroll
            for (int q = 0; q < TW_RUN; q++)
                if (p0 + q < e1) radix_hist_add<CHECK>(mine, (u32)(k[q] >> shift) & mask);
        }
    }
};

static_assert(TW_RUN == RS_GEN_RUN, "presence_remap_hist_kernel rolls out the same runs");
// the counts of presence_remap_hist_kernel stand for this generator's first pass: the same bytes, the same window
template <class K> static inline bool rs_first_hist_counted_for(const RsFirstHist &p, const TextWindowGen<K> &g)
{
    return !g.docs.bits && !g.docs.seg.n_docs && p.s8 == g.s8 && p.n == g.n && p.key_bytes == (int)sizeof(K) && p.w == g.w &&
           p.b == g.b && p.spare == g.spare && p.term_first == g.term_first;
}

// The same for keys of VARIABLE-LENGTH code words (ht_code.h): the key of position q is the first `sb` bits of the coded
// suffix -- stream(q) = code(x[q]) on top of stream(q + 1) moved down by its length, nothing behind a terminator's code
// word --, under the document number.  Code words have at least HT_MIN_LEN = 3 bits, so 16 symbols fill the HT_MAX_STREAM =
// 48 stream bits a key may carry: the run of 8 positions is rolled out of its 24 loaded bytes from the right.  enc[] (byte -> code << 8 | length) is staged in
// LDS by prepare(), which the two kernels of the first radix pass call once, workgroup-wide.
__device__ __forceinline__ u32 *ht_enc_lds()
{
    __shared__ u32 t[256];
    return t;
}
static_assert(HT_MAX_STREAM / HT_MIN_LEN <= 16, "HtWindowGen looks 16 symbols ahead: a key must not hold more");
template <class K> struct HtWindowGen {
    static constexpr int MODE = 2;
    const uint8_t *s8;                          // byte stream; readable (any content) up to 24 bytes behind the last symbol
    u32 n;
    int sb;                                     // stream bits of a key (key bits below the document number)
    const u32 *enc;
    DocKey docs;

    __device__ __forceinline__ void prepare() const
    {
        u32 *t = ht_enc_lds();
        for (u32 i = threadIdx.x; i < 256u; i += blockDim.x) t[i] = enc[i];
        __syncthreads();
    }
    __device__ __forceinline__ void keys_of_run(const u32 (&x)[6], K (&out)[TW_RUN]) const
    {
        const u32 *t = ht_enc_lds();
        K st = 0;
#pragma unroll
        for (int q = 23; q >= 0; q--) {
            const u32 c = (x[q >> 2] >> ((q & 3) * 8)) & 0xFFu;
            const u32 e = t[c];
            const int len = (int)(e & 0xFFu);
            const K rest = c == 0xFFu ? (K)0 : (K)(st >> len);
            st = ((K)(e >> 8) << (sb - len)) | rest;
            if (q < TW_RUN) out[q] = st;
        }
    }
    __device__ __forceinline__ void load_run(u32 p0, u32 (&x)[6]) const
    {
        // (p0 is a multiple of 8 where the tiles start at multiples of RS_TILE; a document's own tiles start anywhere)
        uint2 a, c, e;
        __builtin_memcpy(&a, s8 + p0, 8);
        __builtin_memcpy(&c, s8 + p0 + 8, 8);
        __builtin_memcpy(&e, s8 + p0 + 16, 8);
        x[0] = a.x; x[1] = a.y; x[2] = c.x; x[3] = c.y; x[4] = e.x; x[5] = e.y;
    }
    __device__ __forceinline__ void add_docs(u32 p0, K (&out)[TW_RUN]) const
    {
        u32 lo = docs.tile_doc[p0 >> DOC_TILE_SHIFT];
        while (lo + 1 < docs.n_docs && docs.doc_off[lo + 1] <= p0) lo++;
        u32 next_off = lo + 1 < docs.n_docs ? docs.doc_off[lo + 1] : 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < TW_RUN; q++) {
            while (p0 + q >= next_off) {
                lo++;
                next_off = lo + 1 < docs.n_docs ? docs.doc_off[lo + 1] : 0xFFFFFFFFu;
            }
            out[q] |= (K)lo << sb;
        }
    }
    __device__ __forceinline__ void fill_tile(K *s_keys, u32 tile_base, u32 tile_count) const
    {
        for (u32 r = threadIdx.x; r < (u32)RS_TILE / TW_RUN; r += RS_THREADS) {
            if (r * TW_RUN >= tile_count) break;
            u32 x[6];
            K k[TW_RUN];
            load_run(tile_base + r * TW_RUN, x);
            keys_of_run(x, k);
            if (docs.bits) add_docs(tile_base + r * TW_RUN, k);
#pragma unroll
            for (int q = 0; q < TW_RUN; q++) s_keys[r * TW_RUN + q] = k[q];
        }
    }
    template <bool CHECK = true> __device__ __forceinline__ void hist_tile(u32 *mine, u32 e0, u32 e1, int shift, u32 mask) const
    {
        const bool need_docs = docs.bits && sb < shift + 12;
        for (u32 p0 = e0 + lane_id() * TW_RUN; p0 < e1; p0 += WAVE * TW_RUN) {
            u32 x[6];
            K k[TW_RUN];
            load_run(p0, x);
            keys_of_run(x, k);
            if (need_docs) add_docs(p0, k);
#pragma unroll
            for (int q = 0; q < TW_RUN; q++)
                if (p0 + q < e1) radix_hist_add<CHECK>(mine, (u32)(k[q] >> shift) & mask);
        }
    }
};

// Layout of a window key of `used` = w * bits + document bits: whole radix passes are paid for anyway, so
// the key is filled up to a whole number of digits (of the width the sort will pick) with the top bits of
// one more symbol.  Returns the spare bits taken from symbol w + 1.
static int lvl0_spare_bits(int used, int key_bits, int bt, int w)
{
    const int total = std::min(radix_pass_count(used) * RS_DB, key_bits);
    return w < 12 ? std::min(total - used, bt - 1) : 0;
}

// ht_sb != 0: the keys hold variable-length code words (HtWindowGen): ht_sb stream bits under the document number,
// ht_dec = the decode table (global memory; kernels that read many keys stage it in LDS), ht_wmin = the whole symbols
// every key without a terminator holds at least.
template <class K> struct KeyNeqWindowIn {
    static constexpr bool HAS_KEYS = true;
    const K *keys;
    K rep_t, ones, highs;       // terminator code / 1 / top bit replicated into every full-symbol field
    int ht_sb = 0, ht_wmin = 0;
    const uint16_t *ht_dec = nullptr;
    // the coded stream of a key, left-aligned (the document number shifted out at the top)
    __device__ __forceinline__ K ht_stream(K k) const
    {
        return ht_sb >= (int)sizeof(K) * 8 ? k : (K)(k << ((int)sizeof(K) * 8 - ht_sb));
    }
    // bits the streams of k and kp have in common (ht_sb if the keys are equal; -1: different documents)
    __device__ __forceinline__ int ht_common_bits(K k, K kp) const
    {
        const K d = k ^ kp;
        if (!d) return ht_sb;
        int hb;
        if constexpr (sizeof(K) == 4) hb = 31 - __clz((u32)d); else hb = 63 - __clzll((u64)d);
        return hb >= ht_sb ? -1 : ht_sb - 1 - hb;
    }
    // what the key k holds; common = the symbols it shares with kp (the LCP of the two suffixes, if the keys differ);
    // tb: see HtScan::top
    template <class Table> __device__ __forceinline__ HtScan ht_read(K k, K kp, const Table &dec, int tb = 0) const
    {
        const int cb = ht_common_bits(k, kp);
        return ht_scan<K>(ht_stream(k), ht_sb, dec, cb < 0 ? 0 : cb, tb);
    }
    // "does any of the w full symbols equal the terminator code": xor turns such a field into zero,
    // then the zero-field test (x - ones) & ~x & highs (exact for "any field is zero")
    static KeyNeqWindowIn make(const K *keys, int w, int b, int spare, u32 term_first)
    {
        KeyNeqWindowIn f{keys, 0, 0, 0};
        for (int j = 0; j < w; j++) {
            f.rep_t |= (K)term_first << (spare + j * b);
            f.ones |= (K)1 << (spare + j * b);
            f.highs |= (K)1 << (spare + j * b + b - 1);
        }
        return f;
    }
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        const K k = keys[i];
        if (ht_sb) return (i == 0 || k != keys[i - 1] || ht_read(k, k, ht_dec).term) ? 1u : 0u;
        const K x = k ^ rep_t;
        const bool has_term = ((x - ones) & ~x & highs) != 0;
        return (i == 0 || has_term || k != keys[i - 1]) ? 1u : 0u;
    }
};

// s12[t] = name of sample t; also clears the three pad words behind s12.
__global__ __launch_bounds__(BLOCK) void dc3_scatter_names_kernel(const u32 *__restrict__ vals,
                                                                  const u32 *__restrict__ names,
                                                                  u32 n02, u32 *__restrict__ s12)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n02) s12[vals[i]] = names[i];
    if (i < 3) s12[n02 + i] = 0;
}

// ---- step 2c: refinement of tied names (level 0, byte stream) ---------------------------------
// Natural-language text repeats words and phrases, so half of the suffixes can share their
// w-symbol name.  The tied ones are worked off in rounds, each on the compacted list of what is
// still tied (`domain`: elem[] = the suffixes in their current order, flag[] = 1 where a group of
// equal names starts, slot[] = where each sits in the global order):
//   * small groups (<= REFINE_SMALL_GROUP) are ordered directly on the text, for good;
//   * the members of larger groups are keyed by (group, the NEXT window of symbols) and radix
//     sorted -- the groups stay where they are, their members get ordered by the next symbols --
//     and what is still tied afterwards forms the next, smaller domain.
// A few rounds cover a whole 3-word string.  Long repeats (the domain shrinks slowly): in all-suffix
// mode the rounds switch to prefix doubling (further down) and finish in O(log n) rounds; in DC3's
// sample mode they stop when the domain stalls -- the refined names still are valid DC3 names
// (order-preserving over a window that covers the triple) and feed the recursion.
#ifndef REFINE_SMALL_GROUP
#define REFINE_SMALL_GROUP 6
#endif
#define REFINE_MAX_ROUNDS 32
#define REFINE_ENDGAME_DOMAIN 262144     // domains this small: groups up to REFINE_ENDGAME_GROUP are ordered directly,
#define REFINE_ENDGAME_GROUP 128         // with comparisons of at most REFINE_ENDGAME_LEN symbols (longer: give up)
#define REFINE_ENDGAME_LEN 256
#define REFINE_DOUBLING_LEN 64           // direct comparisons of small groups in prefix-doubling rounds once long repeats are known
#define REFINE_SMALL_INPUT 65536          // inputs this small use the endgame limits from the placement pass on

struct BitIn {                                  // one flag per element, 64 to a word (written by wave ballots)
    const u64 *bits;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (u32)(bits[i >> 6] >> (i & 63u)) & 1u; }
};

// The rank of a set bit among the set bits -- where a kept element goes when the domain is compacted -- from
// the number of set bits in front of its word (an exclusive scan over the WORDS, 1/64 of the elements).
struct PopIn {
    const u64 *bits;
    u32 n_words;
    __device__ __forceinline__ u32 operator()(u32 w) const { return w < n_words ? (u32)__popcll(bits[w]) : 0u; }
};
struct BitRank {
    const u64 *bits;
    const u32 *word_prefix;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        return word_prefix[i >> 6] + (u32)__popcll(bits[i >> 6] & (((u64)1 << (i & 63u)) - 1ull));
    }
};

struct FlagArrIn {                              // the naming predicate of a compacted domain
    static constexpr bool HAS_KEYS = false;
    const u32 *flags;
    __device__ __forceinline__ u32 operator()(u32 i) const { return flags[i]; }
};

// LCP of sorted neighbours from their window keys k (the later one) and kp alone: the leading symbol
// fields the two keys have in common, cut at the first terminator field (equal terminator codes
// are two DIFFERENT terminators).  Returns w with whole = true when the full windows agree and hold
// no terminator -- only then does the text have to be read, from offset w on.
template <class K>
__device__ __forceinline__ u32 lvl0_lcp_of_key_pair(const KeyNeqWindowIn<K> &f, int w, int b, int spare, K k, K kp,
                                                    bool &whole)
{
    if (f.ht_sb) {
        const HtScan r = f.ht_read(k, kp, f.ht_dec);
        whole = k == kp && !r.term;
        return r.common;
    }
    // (the field of a bit position without a division per rank: x / b = (x * ceil(2^16 / b)) >> 16 for the positions of a
    // key, x < 64; the reciprocal is the same for every rank -- uniform, computed once)
    const u32 inv_b = (65536u + (u32)b - 1u) / (u32)b;
    const u64 d = (u64)(k ^ kp);
    u32 mism = (u32)w;                                   // leading symbol fields in common
    if (d) {
        const int hb = 63 - __builtin_clzll(d);
        if (hb >= spare + w * b) mism = 0;              // (different documents: the entry is reset by lcp_doc_starts)
        else if (hb >= spare) mism = (u32)w - 1u - (((u32)(hb - spare) * inv_b) >> 16);
    }
    const K x = k ^ f.rep_t;
    const u64 tz = (u64)((K)(x - f.ones) & ~x & f.highs);    // at most one field holds the terminator code
    const u32 term = tz ? (u32)w - 1u - (((u32)(__builtin_ctzll(tz) - spare) * inv_b) >> 16) : (u32)w;
    const u32 h = mism < term ? mism : term;
    whole = h == (u32)w && d == 0;
    return h;
}

template <class K>
__device__ __forceinline__ u32 lvl0_lcp_of_keys(const KeyNeqWindowIn<K> &f, int w, int b, int spare, u32 r, bool &whole)
{
    return lvl0_lcp_of_key_pair(f, w, b, spare, f.keys[r], f.keys[r - 1], whole);
}

// A tied element j of a domain (elem[], naming predicate `starts`, slot[] or identity): if its group
// of equal names is small (<= REFINE_SMALL_GROUP), its rank inside the group is found by comparing
// the suffixes themselves from offset `depth` on, 8 symbols per step, and it is placed for good:
// order_g, names_g (sample mode) and -- keyed first domain, one document -- its LCP entry, which is
// the longest common prefix with a smaller member found on the way, or comes from the keys for the
// first of the group (lcp_first).  Returns 1 when the group is large: left to the radix round.
// A comparison longer than max_len (a long repeat inside a SMALL group: duplicated passages) cannot be
// decided here.  The optimistic pass (mode 0) only raises `fail`; the host then restores the domain
// and repeats the pass in two steps, so that all members of a group act alike: mode 1 marks the
// groups that hold such a pair (bit of the group's first position in `bad`), mode 2 leaves those
// groups to the rounds -- as if they were large -- and places the others.
struct LongRepeats {
    u32 *bad = nullptr;
    int mode = 0;
};

// The first 8 symbols behind the common depth of the tied elements of a workgroup's stretch, gathered ONCE per
// element into LDS: a member of a group of g then ranks itself with g - 1 LDS reads instead of 2 (g - 1) text gathers
// (only pairs that agree on all 8 symbols go on reading the text).
struct NextSymbols {
    const u64 *k2 = nullptr;        // k2[x - first] for the domain positions first .. first + count - 1 (valid for tied ones)
    u32 first = 0, count = 0;
};

// The keys and elements of a workgroup's stretch of the sorted domain (plus PLACE_HALO to either side), staged in
// LDS by the placement pass: the tied elements look for the bounds of their groups and for the other members
// there instead of through a dozen scattered global loads each (phase 2 of the pass was bound by those).
// Outside the staged range both fall back to the arrays.
#define PLACE_HALO 8
template <class K> struct TileStarts {
    KeyNeqWindowIn<K> f;
    const K *kt;                    // kt[i - first] = keys[i] for first <= i < first + count
    u32 first, count;
    const u32 *tbits = nullptr;     // variable-length keys: bit (i - first + tskip) = "the key at i holds a terminator" (staged range)
    u32 tskip = 0;
    __device__ __forceinline__ K key(u32 i) const { return i - first < count ? kt[i - first] : f.keys[i]; }
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        if (i == 0) return 1u;
        const K k = key(i);
        if (k != key(i - 1)) return 1u;
        if (f.ht_sb) {
            if (i - first < count) return (tbits[(i - first + tskip) >> 5] >> ((i - first + tskip) & 31u)) & 1u;
            return f.ht_read(k, k, f.ht_dec).term ? 1u : 0u;
        }
        const K x = k ^ f.rep_t;
        return ((x - f.ones) & ~x & f.highs) != 0 ? 1u : 0u;
    }
};
struct TileElems {
    const u32 *g, *t;               // t[i - first] = g[i] for first <= i < first + count
    u32 first, count;
    __device__ __forceinline__ u32 operator[](u32 i) const { return i - first < count ? t[i - first] : g[i]; }
};

template <class Starts, class LcpFirst, class Elem = const u32 *>
__device__ __forceinline__ u32 lvl0_place_tied(u32 j, const Elem &elem, const Starts &starts,
                                               const u32 *__restrict__ slot, u32 m, const uint8_t *__restrict__ s8,
                                               u32 n0, u32 depth, u32 *__restrict__ order_g,
                                               u32 *__restrict__ names_g, u32 *__restrict__ lcp_g, LcpFirst lcp_first,
                                               u32 *__restrict__ fail, u32 limit = REFINE_SMALL_GROUP,
                                               u32 max_len = RESOLVE_MAX_LEN, u32 *__restrict__ name_of = nullptr,
                                               LongRepeats lr = LongRepeats(), NextSymbols ns = NextSymbols())
{
    const bool first = slot == nullptr;
    const u32 e = elem[j];
    u32 a = j, bnd = j + 1;
    while (a > 0 && !starts(a) && j - a <= limit) a--;
    while (bnd < m && !starts(bnd) && bnd - j <= limit) bnd++;
    if (bnd - a > limit || (lr.mode == 2 && ((lr.bad[a >> 5] >> (a & 31u)) & 1u))) {
        if (first && lr.mode != 1) { order_g[j] = e; if (names_g) names_g[j] = starts(j); }
        return 1;
    }
    const u32 p = lvl0_pos(e, n0);
    const bool cached = ns.k2 && j - ns.first < ns.count;
    const u64 u0 = cached ? ns.k2[j - ns.first] : 0;
    u32 r = 0, best = 0;                                // best: longest common prefix with a smaller member
    for (u32 x = a; x < bnd; x++) {
        if (x == j) continue;
        const u32 p2 = lvl0_pos(elem[x], n0);
        bool decided = false, less = false;             // less: suffix p2 < suffix p
        u32 h = depth;
        for (; h < depth + max_len && !decided; h += 8) {
            const bool first_step = h == depth && cached && x - ns.first < ns.count;
            const u64 u = first_step ? u0 : load_u64_unaligned(s8 + p + h);
            const u64 v = first_step ? ns.k2[x - ns.first] : load_u64_unaligned(s8 + p2 + h);
            const u64 d = u ^ v, z = ~u;
            const u64 tz = (z - 0x0101010101010101ull) & ~z & 0x8080808080808080ull;
            const u32 mism = d ? (u32)__builtin_ctzll(d) >> 3 : 8u;
            const u32 term = tz ? (u32)__builtin_ctzll(tz) >> 3 : 8u;
            if (term < mism) { less = p2 < p; decided = true; h += term; break; }     // both end in (different) terminators
            if (mism < 8u) { less = ((v >> (8 * mism)) & 0xFFu) < ((u >> (8 * mism)) & 0xFFu); decided = true; h += mism; break; }
        }
        if (!decided) {
            if (lr.mode == 1) atomicOr(&lr.bad[a >> 5], 1u << (a & 31u));
            else atomicOr(fail, 1u);                    // (mode 0: the host restores the domain and repeats the pass)
            return 0;
        }
        if (less) { r++; best = h > best ? h : best; }
    }
    if (lr.mode == 1) return 0;                         // (marking only)
    const u32 at = a + r;                               // final place inside the domain
    const u32 at_g = first ? at : slot[at];
    order_g[at_g] = e;
    if (names_g) names_g[first ? j : slot[j]] = 1;
    if (name_of) name_of[p] = at_g;                     // (prefix doubling: a placed suffix is named by its exact position)
    // (its LCP entry: with a smaller member of the group, or -- the first of a group of the keyed first domain -- from
    // the keys; the first of a group of a later domain keeps the entry it got when its group split off, see
    // dc3_refine_writeback_kernel)
    if (lcp_g) {
        if (r > 0) lcp_g[at_g] = best;
        else if (first) lcp_g[at_g] = lcp_first(at);
    }
    return 0;
}

// four consecutive keys with 16-byte loads (p: 16-byte aligned)
template <class K> __device__ __forceinline__ void fin_load4(const K *p, K (&out)[5])
{
    if constexpr (sizeof(K) == 4) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else {
        const uint4 q0 = reinterpret_cast<const uint4 *>(p)[0], q1 = reinterpret_cast<const uint4 *>(p)[1];
        out[0] = ((u64)q0.y << 32) | q0.x; out[1] = ((u64)q0.w << 32) | q0.z;
        out[2] = ((u64)q1.y << 32) | q1.x; out[3] = ((u64)q1.w << 32) | q1.z;
    }
}

struct NoLcp {
    __device__ __forceinline__ u32 operator()(u32) const { return 0u; }
};

// First domain = the whole sorted input, 4 consecutive elements per thread (16-byte loads and
// stores).  A suffix whose key differs from both neighbours' (or holds a terminator) is final:
// suffix array entry, name flag (sample mode) and LCP entry (lcp_g: all-suffix mode, one document;
// from the two keys, no text is read) are written at once; tied ones go through lvl0_place_tied.
// keep[]: one bit per element, set for members of large groups; block_keep: their number per workgroup.
#define PLACE_IPT 4
// HT: the keys hold variable-length code words (KeyNeqWindowIn::ht_sb): the decode table is staged in LDS, every thread
// reads its keys once with it (terminator inside? whole symbols? symbols shared with the key before = the LCP entry),
// and a tied suffix is compared with the other members of its group from the depth its own key holds (`w` is then the
// least number of symbols any key holds).
template <class K, bool ENDGAME_LIMITS, bool OPTIMISTIC, bool HT = false>  // (OPTIMISTIC: the first attempt, LongRepeats mode 0 folded in)
__global__ __launch_bounds__(BLOCK) void lvl0_place_kernel(KeyNeqWindowIn<K> f, const u32 *__restrict__ vals, u32 m,
                                                          const uint8_t *__restrict__ s8, u32 n0, int w, int b,
                                                          int spare, u32 *__restrict__ order_g,
                                                          u32 *__restrict__ names_g, u32 *__restrict__ lcp_g,
                                                          u64 *__restrict__ keep, u32 *__restrict__ block_keep,
                                                          u32 *__restrict__ fail, LongRepeats lr_arg, KgMark km,
                                                          uint8_t *__restrict__ xdep0 = nullptr, SegRanks sr = SegRanks(),
                                                          u32 *__restrict__ spec_keep = nullptr)      // (as FinishArgs::spec_keep)
{
    const LongRepeats lr = OPTIMISTIC ? LongRepeats() : lr_arg;
    constexpr u32 limit = ENDGAME_LIMITS ? REFINE_ENDGAME_GROUP : REFINE_SMALL_GROUP;
    constexpr u32 max_len = ENDGAME_LIMITS ? REFINE_ENDGAME_LEN : RESOLVE_MAX_LEN;
    __shared__ u32 keep_bits[BLOCK * PLACE_IPT / 32];
    __shared__ u32 work[BLOCK * PLACE_IPT];             // the tied elements of this workgroup's stretch
    __shared__ u64 next8[BLOCK * PLACE_IPT];            // their next 8 symbols (NextSymbols)
    __shared__ __attribute__((aligned(16))) K key_tile[BLOCK * PLACE_IPT + 2 * PLACE_HALO];   // TileStarts
    __shared__ __attribute__((aligned(16))) u32 val_tile[BLOCK * PLACE_IPT + 2 * PLACE_HALO];  // TileElems
    __shared__ u32 n_keep, n_work;
    constexpr int TB_WORDS = (BLOCK * PLACE_IPT + 2 * PLACE_HALO + 31) / 32 + 1;
    __shared__ __attribute__((aligned(16))) uint16_t dec_lds[HT ? HT_DEC_SIZE : 8];  // the decode table
    __shared__ u32 term_bits[HT ? TB_WORDS : 1];        // by staged index: the key holds a terminator
    __shared__ uint8_t dep_tile[HT ? BLOCK * PLACE_IPT : 1];   // whole symbols of the stretch's keys
    __shared__ DocHint kg_hint;                         // (segmented sort) the document of the stretch's first rank
    if (threadIdx.x < BLOCK * PLACE_IPT / 32) keep_bits[threadIdx.x] = 0;
    if (threadIdx.x == 0) { n_keep = 0; n_work = 0; }
    if constexpr (HT) {
        // (the table's 8 KiB with two 16-byte loads per thread: a loop of 2-byte copies was sixteen loads in four round trips)
        static_assert(HT_DEC_SIZE == BLOCK * 16, "two 16-byte loads per thread");
        const uint4 *src = reinterpret_cast<const uint4 *>(f.ht_dec) + threadIdx.x * 2u;
        const uint4 d0 = src[0], d1 = src[1];
        uint4 *dst = reinterpret_cast<uint4 *>(dec_lds) + threadIdx.x * 2u;
        dst[0] = d0; dst[1] = d1;
        if (threadIdx.x < TB_WORDS) term_bits[threadIdx.x] = 0;
    }
    // (every load of the prologue is requested in front of the first barrier: behind it -- as this was written until round 5
    // -- the halo's loads and then the stretch's each waited a round trip of their own, after thread 0's search for the
    // stretch's document, which now runs while they are in flight)
    const u32 j0 = (blockIdx.x * BLOCK + threadIdx.x) * PLACE_IPT;
    u32 my_keep = 0;                                    // suffixes this thread left to the rounds
    // PLACE_HALO entries to either side of the stretch (threads 0 .. 2*PLACE_HALO-1, one each)
    const u32 stretch0 = blockIdx.x * (BLOCK * PLACE_IPT);
    const bool halo_left = threadIdx.x < PLACE_HALO;
    const u32 halo_q = halo_left ? threadIdx.x : threadIdx.x - PLACE_HALO;
    const u64 halo_g = halo_left ? (u64)stretch0 + halo_q - PLACE_HALO : (u64)stretch0 + BLOCK * PLACE_IPT + halo_q;    // (wraps below 0: skipped)
    const bool has_halo = threadIdx.x < 2 * PLACE_HALO && (!halo_left || stretch0 >= PLACE_HALO) && halo_g < (u64)m + 8;
    // (unconditional loads -- a lane with nothing to fetch reads entry 0 --: behind a branch the compiler waits for each load
    // where the branch ends, one round trip per load)
    const u64 halo_at = has_halo ? halo_g : 0u;
    const K halo_k = f.keys[halo_at];
    const u32 halo_v = vals[halo_at];
    K k[PLACE_IPT + 2];
    u32 v[PLACE_IPT];
    u32 work_mask = 0;                                  // bit e: rank j0 + e goes to phase 2
    {
        // keys j0 .. j0+3 and their elements: 16-byte loads (the arrays carry 8 spare entries behind m: whole groups of 4);
        // the keys to either side (j0-1, j0+4) come out of the staged tile behind the barrier -- variable-length keys read
        // them before it (the walk over the five keys), from the array
        const u32 jl = j0 < m ? j0 : 0u;
        K k4[5];
        fin_load4<K>(f.keys + jl, k4);
#pragma unroll
        for (int e = 0; e < PLACE_IPT; e++) k[e + 1] = k4[e];
        const uint4 q = *reinterpret_cast<const uint4 *>(vals + jl);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        if constexpr (HT) {
            k[0] = jl > 0 ? f.keys[jl - 1] : (K)0;
            k[PLACE_IPT + 1] = f.keys[jl + PLACE_IPT];
        }
    }
    if (threadIdx.x == 0)
        kg_hint = sr.n_docs ? doc_hint_of_rank(sr.doc_off, sr.n_docs, blockIdx.x * (BLOCK * PLACE_IPT)) : DocHint{0u, 0u, 0u};
    __syncthreads();
    if (has_halo) {
        const u32 at = halo_left ? halo_q : PLACE_HALO + BLOCK * PLACE_IPT + halo_q;
        key_tile[at] = halo_k;
        val_tile[at] = halo_v;
        if constexpr (HT)
            if (halo_g < m && f.ht_read(halo_k, halo_k, dec_lds).term) atomicOr(&term_bits[at >> 5], 1u << (at & 31u));
    }
    if (j0 < m) {
        const u32 at0 = PLACE_HALO + threadIdx.x * PLACE_IPT;
        if constexpr (sizeof(K) == 4) *reinterpret_cast<uint4 *>(&key_tile[at0]) = uint4{(u32)k[1], (u32)k[2], (u32)k[3], (u32)k[4]};
        else {
#pragma unroll
            for (int e = 0; e < PLACE_IPT; e++) key_tile[at0 + e] = k[e + 1];
        }
        *reinterpret_cast<uint4 *>(&val_tile[at0]) = uint4{v[0], v[1], v[2], v[3]};
    }
    HtScan sc[PLACE_IPT + 1];                           // (HT) what the thread's keys hold; [PLACE_IPT]: the key behind them
    if constexpr (HT) {
        if (j0 < m) {
            u32 tb = 0;
            HtWalk<K> walk;                             // (one walk over the five keys: see HtWalk)
#pragma unroll
            for (int e = 0; e <= PLACE_IPT; e++) {
                int cb = f.ht_common_bits(k[e + 1], k[e]);
                cb = cb < 0 ? 0 : cb;
                if (e > 0) walk.inherit(cb);
                // (the whole key only where the rank may be tied; else the boundaries its own and the next LCP entry need)
                const bool all = k[e + 1] == k[e] || (e < PLACE_IPT && k[e + 2] == k[e + 1]);
                int cbn = e < PLACE_IPT ? f.ht_common_bits(k[e + 2], k[e + 1]) : 0;
                cbn = cbn < 0 ? 0 : cbn;
                walk.extend(f.ht_stream(k[e + 1]), f.ht_sb, dec_lds, all ? f.ht_sb : (cb > cbn ? cb : cbn));
                sc[e] = walk.result(cb, 0);
                if (e < PLACE_IPT) {
                    if (sc[e].term && j0 + e < m) tb |= 1u << e;
                    dep_tile[threadIdx.x * PLACE_IPT + e] = (uint8_t)sc[e].whole;
                }
            }
            // (per rank: what its key holds beyond the least any key does -- the extra depth of its tie group, should the
            // rounds get it; j0 is a multiple of 4 and the array is padded: one 4-byte store)
            if (xdep0) {
                u32 x4 = 0;
#pragma unroll
                for (int e = 0; e < PLACE_IPT; e++) {
                    const u32 x = sc[e].whole > (u32)f.ht_wmin ? sc[e].whole - (u32)f.ht_wmin : 0u;
                    x4 |= (x > 255u ? 255u : x) << (8 * e);
                }
                *reinterpret_cast<u32 *>(xdep0 + j0) = x4;
            }
            const u32 at0 = PLACE_HALO + threadIdx.x * PLACE_IPT;
            if (tb) {
                atomicOr(&term_bits[at0 >> 5], tb << (at0 & 31u));
                if ((at0 & 31u) + PLACE_IPT > 32u) atomicOr(&term_bits[(at0 >> 5) + 1], tb >> (32u - (at0 & 31u)));
            }
        }
    }
    __syncthreads();                                    // (the staged keys: the test for large groups reads them `limit` places away)
    const DocHint hint = kg_hint;
    if (j0 < m) {
        if constexpr (!HT) {
            // (the first stretch has no left halo: rank 0 has no key before it)
            k[0] = j0 > 0 ? key_tile[PLACE_HALO + threadIdx.x * PLACE_IPT - 1] : (K)0;
            k[PLACE_IPT + 1] = key_tile[PLACE_HALO + threadIdx.x * PLACE_IPT + PLACE_IPT];
        }
        bool start[PLACE_IPT + 1];
#pragma unroll
        for (int e = 0; e <= PLACE_IPT; e++) {
            bool has_term;
            if constexpr (HT) has_term = sc[e].term;
            else {
                const K x = k[e + 1] ^ f.rep_t;
                has_term = ((x - f.ones) & ~x & f.highs) != 0;
            }
            start[e] = j0 + e == 0 || j0 + e >= m || has_term || k[e + 1] != k[e];
        }
        if (OPTIMISTIC && km.kg) {                      // k-gram bucket starts, read off the keys (see KgMark)
#pragma unroll
            for (int e = 0; e < PLACE_IPT; e++)
                if (j0 + e < m) kg_mark_key<K>(km, w, b, spare, j0 + e, k[e + 1], k[e], v[e], hint);
        }
        // every rank: final (its key differs from both neighbours'), a member of a large group (sorted keys: an equal key
        // `limit` places away means more than `limit` equal keys around it -- natural-language text: half of the suffixes;
        // flagged without the exact bounds), or one for phase 2
        u32 fin_mask = 0, large_mask = 0;
#pragma unroll
        for (int e = 0; e < PLACE_IPT; e++) {
            const u32 j = j0 + e;
            if (j >= m) break;
            if (start[e] && start[e + 1]) fin_mask |= 1u << e;
#ifdef PLACE_DIAG_NOLARGEREAD
            else if (k[e] == k[e + 1] && k[e + 2] == k[e + 1]) large_mask |= 1u << e;
#else
            else if (k[e] == k[e + 1] && k[e + 2] == k[e + 1]) {                   // (tied on both sides: worth two more reads)
                bool big;
                u32 dlo = 0, dhi = m;                                              // (the sorted range the rank lies in)
                if (sr.n_docs) seg_doc_bounds(sr, hint, j, dlo, dhi);
                if constexpr (limit <= PLACE_HALO) {                               // (out of the staged keys)
                    const u32 at = PLACE_HALO + threadIdx.x * PLACE_IPT + e;
                    big = (j >= dlo + limit && key_tile[at - limit] == k[e + 1]) || (j + limit < dhi && key_tile[at + limit] == k[e + 1]);
                } else {
                    big = (j >= dlo + limit && f.keys[j - limit] == k[e + 1]) || (j + limit < dhi && f.keys[j + limit] == k[e + 1]);
                }
                if (big) large_mask |= 1u << e;
            }
#endif
        }
        if (large_mask) {
            const u32 local0 = threadIdx.x * PLACE_IPT;                           // (a thread's four bits lie in one word)
            atomicOr(&keep_bits[local0 >> 5], large_mask << (local0 & 31u));
            my_keep += (u32)__popc(large_mask);
        }
        if ((fin_mask | large_mask) == (1u << PLACE_IPT) - 1u) {
            // 16-byte stores.  (The LCP entry of a member of a large group that is not the group's first rank is whatever
            // the two keys say -- the rounds write every such entry when its group splits or is ordered; the first rank's
            // entry is the right one already.)
            *reinterpret_cast<uint4 *>(order_g + j0) = uint4{v[0], v[1], v[2], v[3]};
            if (names_g)
                *reinterpret_cast<uint4 *>(names_g + j0) = uint4{(fin_mask & 1u) ? 1u : (u32)start[0], (fin_mask & 2u) ? 1u : (u32)start[1],
                                                                 (fin_mask & 4u) ? 1u : (u32)start[2], (fin_mask & 8u) ? 1u : (u32)start[3]};
            if (lcp_g) {
                u32 h[PLACE_IPT];
#pragma unroll
                for (int e = 0; e < PLACE_IPT; e++) {
                    bool whole;
                    if constexpr (HT) h[e] = j0 + e > 0 ? sc[e].common : 0u;
                    else h[e] = j0 + e > 0 ? lvl0_lcp_of_key_pair(f, w, b, spare, k[e + 1], k[e], whole) : 0u;
                }
                *reinterpret_cast<uint4 *>(lcp_g + j0) = uint4{h[0], h[1], h[2], h[3]};
            }
        } else {
#pragma unroll
            for (int e = 0; e < PLACE_IPT; e++) {
                const u32 j = j0 + e;
                if (j >= m) break;
                if ((fin_mask >> e) & 1u) {
                    order_g[j] = v[e];
                    if (names_g) names_g[j] = 1;
                    if (lcp_g) {
                        bool whole;
                        if constexpr (HT) lcp_g[j] = j > 0 ? sc[e].common : 0u;
                        else lcp_g[j] = j > 0 ? lvl0_lcp_of_key_pair(f, w, b, spare, k[e + 1], k[e], whole) : 0u;
                    }
                } else if ((large_mask >> e) & 1u) {
                    order_g[j] = v[e];
                    if (names_g) names_g[j] = start[e];
                } else {
                    work_mask |= 1u << e;                // phase 2
                }
            }
        }
    }
    {   // the work list: one LDS atomic per wavefront (natural-language text sends half of the ranks there)
        const u32 wc = (u32)__popc(work_mask);
        const u32 inc = wave_inclusive_sum(wc);
        u32 wbase = 0;
        if (lane_id() == 63u && inc) wbase = atomicAdd(&n_work, inc);
        wbase = __shfl(wbase, 63, WAVE) + inc - wc;
#pragma unroll
        for (int e = 0; e < PLACE_IPT; e++)
            if ((work_mask >> e) & 1u) work[wbase++] = j0 + e;
    }
    __syncthreads();
    // phase 2: the tied elements, one per thread, so that their text gathers run side by side
    // instead of one after the other inside the thread that met them.  First every one of them fetches the 8
    // symbols behind the window once (NextSymbols), then they rank themselves inside their groups.
#ifdef PLACE_DIAG_NOPHASE2
    const u32 todo = 0;
#else
    const u32 todo = n_work;
#endif
    const u32 stretch = blockIdx.x * (BLOCK * PLACE_IPT);
    for (u32 i = threadIdx.x; i < todo; i += BLOCK) {
        const u32 j = work[i];
        const u32 dep = HT ? (u32)dep_tile[j - stretch] : (u32)w;       // (the members of a group hold the same key)
        next8[j - stretch] = load_u64_unaligned(s8 + lvl0_pos(val_tile[PLACE_HALO + j - stretch], n0) + dep);
    }
    __syncthreads();
    const NextSymbols ns{next8, stretch, (u32)(BLOCK * PLACE_IPT)};
    // the staged range: the stretch and PLACE_HALO to either side, as far as it exists
    const u32 t_first = stretch >= PLACE_HALO ? stretch - PLACE_HALO : stretch;
    const u32 t_skip = stretch >= PLACE_HALO ? 0u : (u32)PLACE_HALO;               // (no left halo in the first stretch)
    const u64 t_end = std::min<u64>((u64)stretch + BLOCK * PLACE_IPT + PLACE_HALO, (u64)m + 8);
    const u32 t_count = (u32)(t_end - t_first);
    const TileStarts<K> tstarts{f, key_tile + t_skip, t_first, t_count, HT ? term_bits : (const u32 *)nullptr, t_skip};
    const TileElems telems{vals, val_tile + t_skip, t_first, t_count};
    for (u32 i = threadIdx.x; i < todo; i += BLOCK) {
        const u32 j = work[i];
        auto lcp_first = [&](u32 at) -> u32 {
            bool whole;
            if constexpr (HT) return at > 0 ? f.ht_read(tstarts.key(at), tstarts.key(at - 1), dec_lds).common : 0u;
            else return at > 0 ? lvl0_lcp_of_key_pair(f, w, b, spare, tstarts.key(at), tstarts.key(at - 1), whole) : 0u;
        };
        const u32 dep = HT ? (u32)dep_tile[j - stretch] : (u32)w;
        if (lvl0_place_tied(j, telems, tstarts, (const u32 *)nullptr, m, s8, n0, dep, order_g, names_g, lcp_g, lcp_first, fail,
                            limit, max_len, (u32 *)nullptr, lr, ns)) {
            const u32 local = j - blockIdx.x * (BLOCK * PLACE_IPT);
            atomicOr(&keep_bits[local >> 5], 1u << (local & 31u));
            my_keep++;
        }
    }
    // (the count: one LDS atomic per wavefront -- natural-language text keeps hundreds of suffixes per stretch, and as
    // many adds to one word queue up behind one another)
    my_keep = wave_sum(my_keep);
    if (lane_id() == 0 && my_keep) atomicAdd(&n_keep, my_keep);
    __syncthreads();
    // (entries m.. are 0: the exclusive scan over m + 1 entries yields the total)
    if (threadIdx.x < BLOCK * PLACE_IPT / 64)
        keep[(size_t)blockIdx.x * (BLOCK * PLACE_IPT / 64) + threadIdx.x] =
            ((u64)keep_bits[2 * threadIdx.x + 1] << 32) | keep_bits[2 * threadIdx.x];
    if (threadIdx.x == 0) {
        block_keep[blockIdx.x] = n_keep;
        if (spec_keep && n_keep) spec_keep[0] = 1u;
    }
}

// ---- the fused end of the sort: last digit + placement in one pass ---------------------------------
// The global LSD passes stop above the low `L` key bits: the pairs arrive sorted (stably) by the TOP part of
// their keys -- document number, the leading symbols -- with the suffixes of a *bucket* (equal top part)
// still in text order.  A window wide enough to tell most suffixes apart leaves a handful of suffixes per
// bucket, so the last digit is not worth a trip through HBM: a workgroup stages a stretch of FIN_CHUNK
// pairs (+ FIN_G to either side) in LDS, every member of a bucket of at most FIN_G suffixes finds its rank
// inside the bucket by counting the members with smaller low bits (equal ones: text order, the sort stays
// stable), the pairs are permuted inside LDS, and the placement logic of lvl0_place_kernel runs on the
// staged, now fully sorted keys -- suffix array, LCP entries, k-gram bucket starts, direct ordering of the
// small tie groups.  One global radix pass (20 B per suffix) and the re-read of the sorted pairs are gone.
//   * A bucket belongs to the workgroup in whose stretch it STARTS (it may run up to FIN_G - 1 positions
//     into the next stretch; the neighbour sees from its own halo that the bucket is not its own).
//   * The LCP entry of a bucket's first rank only depends on the top parts of the two keys (they differ
//     there), so any member of the bucket in front serves as "the key before".
//   * A bucket of more than FIN_G suffixes whose top part holds a terminator is constant -- the fields
//     behind a terminator are zero --: equal keys in text order, final as they stand.
//   * Any other bucket of more than FIN_G suffixes (skewed text) is handed to the refinement rounds as
//     ONE tie group: its members agree on the symbols that lie wholly inside the top part, and that
//     number of symbols is the depth the rounds start from (dc3_level0_bytes: depth0).  Large groups of
//     equal FULL keys join them at the same depth (they agree on more, which does no harm).
#define FIN_IPT 4
#define FIN_CHUNK (BLOCK * FIN_IPT)
// FIN_G = the largest bucket ordered here; the kernel exists for 64 (the default) and 32 (a smaller halo: 3 % less to
// stage, for inputs whose buckets are expected to hold at most ten suffixes)
template <int G> struct FinGeom {
    static constexpr int LEFT = G + 4;                  // staged entries in front of the stretch (>= G + 1; a multiple of 4: a thread's four flags share a word)
    static constexpr int RIGHT = G + 4;                 // ... behind it (>= G + 1)
    static constexpr int STAGE = LEFT + FIN_CHUNK + RIGHT;
    static constexpr int WORDS = (STAGE + 31) / 32 + 1;
    static constexpr int SCAN_WORDS = (G + 4 + 31) / 32 + 1;
};

template <class K> struct FinishArgs {
    const K *keys;
    const u32 *vals;
    u32 m;
    const uint8_t *s8;
    int w, b, spare, low_bits;
    u32 inv_b;                              // ceil(2^16 / b): (x * inv_b) >> 16 = x / b for the bit positions of a key
    K rep_t, ones, highs;                   // KeyNeqWindowIn's constants over all w symbol fields
    K top_mask;                             // the bits of the fields that lie wholly inside the top part
    int kg_top;                             // 1: the k-gram class code reaches below the top part (marks inside a handed-over bucket would be missed)
    u32 *order_g, *lcp_g;
    u64 *keep, *gstart;                     // one bit per rank (zeroed; OR-ed into): left to the rounds / first of its group
    u32 *block_keep, *fail, *kg_bad;
    u32 *spec_keep = nullptr;               // != nullptr (a speculative build that expects no rounds): set to 1 by every workgroup that keeps a suffix
    KgMark km;
    // variable-length code words in the keys (ht_code.h; ht_sb = 0: fixed-width fields): stream bits, the least whole
    // symbols the TOP part of a key holds (the depth the rounds start from), the decode table, and per rank handed to the
    // rounds what its group shares beyond that depth
    int ht_sb = 0, ht_wmin = 0;
    const uint16_t *ht_dec = nullptr;
    uint8_t *xdep0 = nullptr;
    // (segmented sort: km.by_rank, with km.doc_off / km.n_docs = the documents' ranges of ranks -- set whether or not
    // k-gram marks are written)
};

// highest set bit of fl[] in [lo, i] / lowest in [i, hi]; -1 if none (the ranges span at most G + 4 bits)
template <class GE> __device__ __forceinline__ int fin_prev_bit(const u32 *fl, int i, int lo)
{
    int found = -1;
    int wi = i >> 5;
    u32 word = fl[wi] & (0xFFFFFFFFu >> (31 - (i & 31)));
#pragma unroll
    for (int step = 0; step < GE::SCAN_WORDS; step++) {
        if (found < 0 && word) found = (wi << 5) + 31 - __clz(word);
        if (found < 0 && wi > 0) { wi--; word = fl[wi]; } else word = 0;
    }
    return found >= lo ? found : -1;
}
template <class GE> __device__ __forceinline__ int fin_next_bit(const u32 *fl, int i, int hi)
{
    int found = -1;
    int wi = i >> 5;
    u32 word = fl[wi] & (0xFFFFFFFFu << (i & 31));
#pragma unroll
    for (int step = 0; step < GE::SCAN_WORDS; step++) {
        if (found < 0 && word) found = (wi << 5) + __ffs(word) - 1;
        if (found < 0 && wi + 1 < GE::WORDS) { wi++; word = fl[wi]; } else word = 0;
    }
    return found >= 0 && found <= hi ? found : -1;
}

// lvl0_lcp_of_key_pair without the divisions by the symbol width
template <class K>
__device__ __forceinline__ u32 fin_lcp_of_key_pair(const FinishArgs<K> &a, K k, K kp)
{
    const int w = a.w, b = a.b, spare = a.spare;
    const K d = k ^ kp;
    u32 mism = (u32)w;
    if (d) {
        int hb;
        if constexpr (sizeof(K) == 4) hb = 31 - __clz((u32)d); else hb = 63 - __clzll((u64)d);
        if (hb >= spare + w * b) mism = 0;              // (different documents: the entry is reset by lcp_doc_starts)
        else if (hb >= spare) mism = (u32)w - 1u - (((u32)(hb - spare) * a.inv_b) >> 16);
    }
    const K x = k ^ a.rep_t;
    const K tz = (K)(x - a.ones) & ~x & a.highs;        // at most one field holds the terminator code
    u32 term = (u32)w;
    if (tz) {
        int lb;
        if constexpr (sizeof(K) == 4) lb = __ffs((u32)tz) - 1; else lb = __ffsll((unsigned long long)tz) - 1;
        term = (u32)w - 1u - (((u32)(lb - spare) * a.inv_b) >> 16);
    }
    return mism < term ? mism : term;
}

// lvl0_place_tied for the fused finish: a member of a group of equal keys ranks itself inside the group by comparing
// the suffixes from offset w on and is placed for good (suffix array, LCP entry).  The group lies inside its bucket,
// so everything touched is staged (staged indices throughout); next4[] holds the 4 symbols behind the window of every
// tied pair (enough to tell nearly all of them apart; longer comparisons go on reading the text, 8 symbols a step).
// Returns 1 when the group has more than `limit` members (left to the rounds).
// (dec8 / depth_i: variable-length keys -- the decode table in LDS and the whole symbols the member's key holds: the depth
// the comparisons start from.  A tied member's key holds no terminator, and the members of its group hold the same key.)
template <class K>
__device__ __forceinline__ u32 fin_place_tied(const FinishArgs<K> &a, int i, const K *kt, const u32 *vt, const u32 *next4,
                                              u32 base, u32 limit, u32 max_len, const uint8_t *dec8 = nullptr, u32 depth_i = 0)
{
    auto starts = [&](int x) -> bool {
        if (base + (u32)x == 0) return true;
        const K k = kt[x], xx = k ^ a.rep_t;
        if (a.ht_sb) return k != kt[x - 1];
        return ((K)(xx - a.ones) & ~xx & a.highs) != 0 || k != kt[x - 1];
    };
    int lo = i, hi = i + 1;
    while (!starts(lo) && (u32)(i - lo) <= limit) lo--;
    while (base + (u32)hi < a.m && !starts(hi) && (u32)(hi - i) <= limit) hi++;
    if ((u32)(hi - lo) > limit) return 1;
    const uint8_t *s8 = a.s8;
    const u32 depth = a.ht_sb ? depth_i : (u32)a.w, p = vt[i];
    const u32 u0 = next4[i];
    u32 r = 0, best = 0;                                // best: longest common prefix with a smaller member
    for (int x = lo; x < hi; x++) {
        if (x == i) continue;
        const u32 p2 = vt[x];
        bool decided = false, less = false;             // less: suffix p2 < suffix p
        u32 h = depth;
        {
            const u32 v0 = next4[x];
            const u32 d = u0 ^ v0, z = ~u0;
            const u32 tz = (z - 0x01010101u) & ~z & 0x80808080u;
            const u32 mism = d ? (u32)(__ffs(d) - 1) >> 3 : 4u;
            const u32 term = tz ? (u32)(__ffs(tz) - 1) >> 3 : 4u;
            if (term < mism) { less = p2 < p; decided = true; h += term; }        // both end in (different) terminators
            else if (mism < 4u) { less = ((v0 >> (8 * mism)) & 0xFFu) < ((u0 >> (8 * mism)) & 0xFFu); decided = true; h += mism; }
            else h += 4;
        }
        for (; h < depth + max_len && !decided; h += 8) {
            const u64 u = load_u64_unaligned(s8 + p + h), v = load_u64_unaligned(s8 + p2 + h);
            const u64 d = u ^ v, z = ~u;
            const u64 tz = (z - 0x0101010101010101ull) & ~z & 0x8080808080808080ull;
            const u32 mism = d ? (u32)__builtin_ctzll(d) >> 3 : 8u;
            const u32 term = tz ? (u32)__builtin_ctzll(tz) >> 3 : 8u;
            if (term < mism) { less = p2 < p; decided = true; h += term; break; }
            if (mism < 8u) { less = ((v >> (8 * mism)) & 0xFFu) < ((u >> (8 * mism)) & 0xFFu); decided = true; h += mism; break; }
        }
        if (!decided) { atomicOr(a.fail, 1u); return 0; }   // (a repeat too long to compare: the host redoes the level with the full sort)
        if (less) { r++; best = h > best ? h : best; }
    }
    const int at = lo + (int)r;
    const u32 at_g = base + (u32)at;
    a.order_g[at_g] = p;
    if (a.lcp_g) {
        u32 h = best;
        if (r == 0) {
            if (at_g == 0) h = 0;
            else if (a.ht_sb) {
                const KeyNeqWindowIn<K> hf{nullptr, 0, 0, 0, a.ht_sb, a.ht_wmin, a.ht_dec};
                h = hf.ht_read(kt[at], kt[at - 1], dec8).common;
            } else h = fin_lcp_of_key_pair(a, kt[at], kt[at - 1]);
        }
        a.lcp_g[at_g] = h;
    }
    return 0;
}

template <class K, bool ENDGAME_LIMITS, int FIN_G, bool HT = false, bool SEG = false>
__global__ __launch_bounds__(BLOCK) void lvl0_finish_kernel(FinishArgs<K> a)
{
    using GE = FinGeom<FIN_G>;
    constexpr int FIN_LEFT = GE::LEFT, FIN_STAGE = GE::STAGE, FIN_WORDS = GE::WORDS;
    constexpr u32 limit = ENDGAME_LIMITS ? (REFINE_ENDGAME_GROUP < FIN_G ? REFINE_ENDGAME_GROUP : FIN_G) : REFINE_SMALL_GROUP;
    constexpr u32 max_len = ENDGAME_LIMITS ? REFINE_ENDGAME_LEN : RESOLVE_MAX_LEN;
    constexpr int HELD = FIN_IPT + 1;                   // a thread holds 4 pairs of the stretch and (threads 0 .. FIN_G) one of the right halo
    constexpr int G = FIN_G;
    __shared__ __attribute__((aligned(16))) K kt[FIN_STAGE];
    __shared__ __attribute__((aligned(16))) u32 vt[FIN_STAGE];
    __shared__ u32 next4[FIN_STAGE];                    // the 4 symbols behind the window of the tied pairs; before: comp
    __shared__ uint16_t work[FIN_CHUNK + FIN_G];
    __shared__ u32 fl[FIN_WORDS];                       // bucket starts, by staged index
    __shared__ u32 keep_bits[FIN_WORDS], gs_bits[FIN_WORDS];
    __shared__ u32 n_keep, n_work;
    __shared__ DocHint kg_hint;                         // (segmented sort) the document of the stretch's first rank
    __shared__ __attribute__((aligned(16))) uint8_t dec8[HT ? HT_DEC_SIZE : 16];   // variable-length keys: the decode table (length, terminator bit)
    __shared__ uint8_t wdep[HT ? FIN_CHUNK + FIN_G : 1];   // ... the whole symbols of the tied members' keys, by work list index
    const KeyNeqWindowIn<K> hf{a.keys, a.rep_t, a.ones, a.highs, a.ht_sb, a.ht_wmin, a.ht_dec};
    u32 *comp = next4;                                  // (bucket start, low key bits, staged index) of every pair; next4 is used after the ranking
    const u32 m = a.m;
    const u32 c0 = blockIdx.x * FIN_CHUNK;
    const u32 base = c0 - FIN_LEFT;                     // global rank of staged entry 0 (wraps in the first stretch: such ranks test as > m)
    const int L = a.low_bits;
    const u32 tid = threadIdx.x;
    if (tid < FIN_WORDS) { fl[tid] = 0; keep_bits[tid] = 0; gs_bits[tid] = 0; }
    if (tid == 0) {
        n_keep = 0; n_work = 0;
        if constexpr (SEG) kg_hint = doc_hint_of_rank(a.km.doc_off, a.km.n_docs, c0);
    }
    // ---- stage the pairs ---------------------------------------------------------------------------
    K key[HELD];
    u32 val[HELD];
    const int i0 = (int)(FIN_LEFT + tid * FIN_IPT);     // staged index of the thread's first pair
    const int ih = (int)(FIN_LEFT + FIN_CHUNK + tid);   // ... of its right-halo pair (threads 0 .. FIN_G)
    const u32 j0 = c0 + tid * FIN_IPT;
    u32 valid = 0;                                      // bit e: the held pair e exists (rank < m)
    {
        if (j0 + FIN_IPT <= m) {                        // (16-byte loads)
            fin_load4<K>(a.keys + j0, key);
            const uint4 q = *reinterpret_cast<const uint4 *>(a.vals + j0);
            val[0] = q.x; val[1] = q.y; val[2] = q.z; val[3] = q.w;
            valid = 15u;
        } else {
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++) {
                const bool ok = j0 + e < m;
                key[e] = ok ? a.keys[j0 + e] : (K)0;
                val[e] = ok ? a.vals[j0 + e] : 0u;
                valid |= ok ? 1u << e : 0u;
            }
        }
        // (every load of the prologue is requested before the first one is used: with the staging of the stretch in between,
        // the halo loads waited for the stretch's and for each other -- three round trips where one does)
        key[FIN_IPT] = 0; val[FIN_IPT] = 0;
        if (tid <= (u32)G) {
            const u32 jr = c0 + FIN_CHUNK + tid;        // right halo
            if (jr < m) { key[FIN_IPT] = a.keys[jr]; val[FIN_IPT] = a.vals[jr]; valid |= 16u; }
        }
        K key_l = 0;
        u32 val_l = 0;
        if (tid < (u32)FIN_LEFT) {                      // left halo (never moved)
            const u32 jl = base + tid;
            if (jl < m) { key_l = a.keys[jl]; val_l = a.vals[jl]; }
        }
        if constexpr (HT) {
            // (the low bytes of the table's 4 096 16-bit entries, a thread's sixteen with two 16-byte loads -- requested with
            // the pairs; a loop of 2-byte loads at the top of the kernel was four round trips in front of them)
            static_assert(HT_DEC_SIZE == BLOCK * 16, "two 16-byte loads per thread");
            const uint4 *src = reinterpret_cast<const uint4 *>(a.ht_dec) + tid * 2u;
            const uint4 d0 = src[0], d1 = src[1];
            auto lows = [](u32 x, u32 y) { return (x & 0xFFu) | ((x >> 8) & 0xFF00u) | ((y & 0xFFu) << 16) | ((y << 8) & 0xFF000000u); };
            *reinterpret_cast<uint4 *>(&dec8[tid * 16u]) = uint4{lows(d0.x, d0.y), lows(d0.z, d0.w), lows(d1.x, d1.y), lows(d1.z, d1.w)};
        }
        if constexpr (sizeof(K) == 4) *reinterpret_cast<uint4 *>(&kt[i0]) = uint4{(u32)key[0], (u32)key[1], (u32)key[2], (u32)key[3]};
        else {
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++) kt[i0 + e] = key[e];
        }
        *reinterpret_cast<uint4 *>(&vt[i0]) = uint4{val[0], val[1], val[2], val[3]};
        if (tid <= (u32)G) { kt[ih] = key[FIN_IPT]; vt[ih] = val[FIN_IPT]; }
        if (tid < (u32)FIN_LEFT) { kt[tid] = key_l; vt[tid] = val_l; }
    }
    __syncthreads();
    // ---- bucket starts: the top part differs from the rank before (rank 0 and rank m count as starts) ----
    u32 myfl = 0;                                       // bit e: the held pair e starts a bucket
    {
        K prev = kt[i0 - 1];
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++) {
            const u32 j = j0 + e;
            if (j <= m && (j == 0 || j == m || (K)(key[e] >> L) != (K)(prev >> L))) myfl |= 1u << e;
            prev = key[e];
        }
        if (myfl) atomicOr(&fl[i0 >> 5], myfl << (i0 & 31));
        if (tid <= (u32)G) {
            const u32 j = base + (u32)ih;
            if (j <= m && (j == m || (K)(key[FIN_IPT] >> L) != (K)(kt[ih - 1] >> L))) { myfl |= 16u; atomicOr(&fl[ih >> 5], 1u << (ih & 31)); }
        }
        if (tid >= 1 && tid < (u32)FIN_LEFT) {
            const u32 j = base + tid;
            if (j <= m && (j == 0 || j == m || (K)(kt[tid] >> L) != (K)(kt[tid - 1] >> L))) atomicOr(&fl[tid >> 5], 1u << (tid & 31));
        }
    }
    __syncthreads();
    // ---- every held pair: its bucket [s, en) ----------------------------------------------------------------
    // own: a bucket of at most FIN_G pairs that starts in this workgroup's stretch (it is ordered here);
    // hot: a pair of the stretch in a larger bucket.  Everything else belongs to a neighbour.
    int s[HELD], en[HELD];
    u32 own = 0, hot = 0;
    {
        int run = (myfl & 1u) ? i0 : fin_prev_bit<GE>(fl, i0, i0 - G + 1);
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++) {
            if (e > 0 && ((myfl >> e) & 1u)) run = i0 + e;
            s[e] = run >= i0 + e - G + 1 ? run : -1;
        }
        int nxt = fin_next_bit<GE>(fl, i0 + FIN_IPT, i0 + FIN_IPT - 1 + G);
#pragma unroll
        for (int e = FIN_IPT - 1; e >= 0; e--) {
            en[e] = nxt;
            if ((myfl >> e) & 1u) nxt = i0 + e;
        }
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++) {
            if (!((valid >> e) & 1u)) continue;
            if (s[e] < 0 || en[e] < 0 || en[e] - s[e] > G) hot |= 1u << e;
            else if (s[e] >= (int)FIN_LEFT) own |= 1u << e;         // (s < FIN_LEFT: the bucket of the workgroup before)
        }
        s[FIN_IPT] = en[FIN_IPT] = -1;
        if (valid & 16u) {
            const int sh = (myfl & 16u) ? ih : fin_prev_bit<GE>(fl, ih, ih - G + 1);
            if (sh >= (int)FIN_LEFT && sh < (int)(FIN_LEFT + FIN_CHUNK)) {
                const int eh = fin_next_bit<GE>(fl, ih + 1, sh + G);
                if (eh >= 0) { s[FIN_IPT] = sh; en[FIN_IPT] = eh; own |= 16u; }
            }
        }
    }
    const u32 lowmask = (1u << L) - 1u;
    u32 ck[HELD];
#pragma unroll
    for (int e = 0; e < HELD; e++) {
        const int i = e < FIN_IPT ? i0 + e : ih;
        ck[e] = ((u32)s[e] << 19) | (((u32)key[e] & lowmask) << 11) | (u32)i;
        if ((own >> e) & 1u) comp[i] = ck[e];
    }
    __syncthreads();
    // ---- ranks: the pairs of the stretch [lo, hi) that cover this thread's buckets, counted once for all four ----
    // (comp orders the pairs by bucket first: dest = lo + the number of pairs in [lo, hi) below this one)
    int dest[HELD];
    {
        int lo = FIN_STAGE, hi = 0;
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++)
            if ((own >> e) & 1u) { lo = s[e] < lo ? s[e] : lo; hi = en[e] > hi ? en[e] : hi; }
        u32 c0_ = 0, c1_ = 0, c2_ = 0, c3_ = 0;
#ifndef FIN_DIAG_NORANK
        int x = lo;
        for (; x + 1 < hi; x += 2) {                    // (two pairs per step: one ds_read2)
            const u32 ca = comp[x], cb = comp[x + 1];
            c0_ += (ca < ck[0] ? 1u : 0u) + (cb < ck[0] ? 1u : 0u);
            c1_ += (ca < ck[1] ? 1u : 0u) + (cb < ck[1] ? 1u : 0u);
            c2_ += (ca < ck[2] ? 1u : 0u) + (cb < ck[2] ? 1u : 0u);
            c3_ += (ca < ck[3] ? 1u : 0u) + (cb < ck[3] ? 1u : 0u);
        }
        if (x < hi) {
            const u32 c = comp[x];
            c0_ += c < ck[0] ? 1u : 0u;
            c1_ += c < ck[1] ? 1u : 0u;
            c2_ += c < ck[2] ? 1u : 0u;
            c3_ += c < ck[3] ? 1u : 0u;
        }
#else
        c0_ = (u32)(i0 - lo); c1_ = c0_ + 1; c2_ = c0_ + 2; c3_ = c0_ + 3;
#endif
        dest[0] = lo + (int)c0_; dest[1] = lo + (int)c1_; dest[2] = lo + (int)c2_; dest[3] = lo + (int)c3_;
        dest[FIN_IPT] = -1;
        if (own & 16u) {
            u32 c = 0;
            for (int x = s[FIN_IPT]; x < en[FIN_IPT]; x++) c += comp[x] < ck[FIN_IPT] ? 1u : 0u;
            dest[FIN_IPT] = s[FIN_IPT] + (int)c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < HELD; e++)
        if ((own >> e) & 1u) { kt[dest[e]] = key[e]; vt[dest[e]] = val[e]; }
    __syncthreads();
    // ---- placement on the staged, sorted keys ----------------------------------------------------------
    const DocHint hint = SEG ? kg_hint : DocHint{0u, 0u, 0u};
    const KeyNeqWindowIn<K> f{a.keys, a.rep_t, a.ones, a.highs};   // (keys / vals: never read -- everything the tie code touches is staged; a null pointer here crashes hipcc 7.2)
    const int w = a.w, b = a.b, spare = a.spare;
    u32 my_keep = 0;                                    // suffixes this thread left to the rounds (summed per wavefront at the end)
    auto kg_mark = [&](u32 j, K k, K kp, u32 v) {       // k-gram bucket starts, read off the keys (see KgMark)
        kg_mark_key<K, SEG ? 1 : 0>(a.km, w, b, spare, j, k, kp, v, hint);
    };
    // rank `base + i` (one of this workgroup's): returns true when it is final here (suffix and LCP entry in sa_o / lcp_o,
    // to be stored by the caller); a rank handed to the rounds or a member of a small tie group is dealt with inside
    // (sc: variable-length keys -- what the key holds, as far as this rank needs it: the symbols shared with the key before
    // always, the rest where the rank is in a hot bucket or tied with a neighbour)
    auto place_one = [&](int i, bool is_hot, bool first, K k, K kp, K kn, u32 v, u32 &sa_o, u32 &lcp_o, const HtScan &sc) -> bool {
        const u32 j = base + (u32)i;
        sa_o = v;
        if constexpr (HT) lcp_o = j > 0 ? sc.common : 0u;
        else lcp_o = j > 0 ? fin_lcp_of_key_pair(a, k, kp) : 0u;
        // (a rank left to the rounds: what its group shares beyond the depth the rounds start from)
        auto note_depth = [&](u32 shared) {
            if constexpr (HT) a.xdep0[j] = (uint8_t)(shared > (u32)a.ht_wmin ? (shared - (u32)a.ht_wmin > 255u ? 255u : shared - (u32)a.ht_wmin) : 0u);
        };
        if (is_hot) {
            if (a.km.kg && first) kg_mark(j, k, kp, v);
            bool constant;
            if constexpr (HT) constant = sc.term_top;
            else {
                const K xt = k ^ (a.rep_t & a.top_mask);
                constant = ((K)(xt - (a.ones & a.top_mask)) & ~xt & (a.highs & a.top_mask)) != 0;
            }
            if (constant) return true;                  // a constant bucket: final as it stands
            note_depth(sc.top);
            // (handed to the rounds: the suffix goes to its rank as it is, with the caller's 16-byte stores; the LCP entry is
            // the right one for the group's first rank, and the rounds write every other one when the group splits)
            atomicOr(&keep_bits[i >> 5], 1u << (i & 31));
            my_keep++;
            if (first) atomicOr(&gs_bits[i >> 5], 1u << (i & 31));
            if (a.kg_top && a.km.kg) *a.kg_bad = 1u;
            return true;
        }
        if (a.km.kg) kg_mark(j, k, kp, v);
        bool st, st_next = j + 1 >= m;
        if constexpr (HT) {
            st = j == 0 || sc.term || k != kp;
            st_next = st_next || kn != k || sc.term;    // (an equal key holds a terminator exactly if this one does)
        } else {
            const K x = k ^ f.rep_t;
            st = j == 0 || ((K)(x - f.ones) & ~x & f.highs) != 0 || k != kp;
            if (!st_next) {
                const K xn = kn ^ f.rep_t;
                st_next = ((K)(xn - f.ones) & ~xn & f.highs) != 0 || kn != k;
            }
        }
        if (st && st_next) return true;
        // tied: a group of equal keys inside this bucket (all of it is staged).  More than `limit` equal keys around
        // this one (an equal key `limit` places away -- equal keys share their bucket, so that place is sorted too):
        // a large group, left to the rounds without the exact bounds.
        bool big = false;
        {
            const int lo = i - (int)limit, hi = i + (int)limit;
            u32 dlo = 0, dhi = m;                       // (the sorted range the rank lies in)
            if constexpr (SEG) seg_doc_bounds(SegRanks{a.km.doc_off, a.km.n_docs}, hint, j, dlo, dhi);
            if (lo >= 1 && j >= dlo + limit) big = kt[lo] == k;
            if (!big && hi <= (int)(FIN_LEFT + FIN_CHUNK + FIN_G) && j + limit < dhi) big = kt[hi] == k;   // (staged up to there)
        }
        if (big) {
            atomicOr(&keep_bits[i >> 5], 1u << (i & 31));
            my_keep++;
            if (st) atomicOr(&gs_bits[i >> 5], 1u << (i & 31));
            note_depth(sc.whole);
            return true;                                // (as above: stored by the caller)
        }
        const u32 wi = atomicAdd(&n_work, 1u);
        work[wi] = (uint16_t)i;
        if constexpr (HT) wdep[wi] = (uint8_t)sc.whole;
        return false;
    };
    {
        u32 sa4[FIN_IPT], lc4[FIN_IPT];
        u32 fin = 0;
        const u32 todo4 = (own | hot) & 15u;
        // the sorted keys of the thread's four ranks and of the two next to them, the suffixes: 16-byte LDS reads
        K kq[FIN_IPT + 2];
        u32 vq[FIN_IPT];
        kq[0] = j0 > 0 ? kt[i0 - 1] : (K)0;
        if constexpr (sizeof(K) == 4) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&kt[i0]);
            kq[1] = q.x; kq[2] = q.y; kq[3] = q.z; kq[4] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++) kq[e + 1] = kt[i0 + e];
        }
        kq[FIN_IPT + 1] = kt[i0 + FIN_IPT];
        {
            const uint4 q = *reinterpret_cast<const uint4 *>(&vt[i0]);
            vq[0] = q.x; vq[1] = q.y; vq[2] = q.z; vq[3] = q.w;
        }
#ifndef FIN_DIAG_NOPLACE
        // variable-length keys: the four keys are read in one walk (HtWalk) -- the boundaries inside the bits a key shares
        // with the one before are inherited, the rest is decoded only as far as it is needed
        HtScan sc4[FIN_IPT];
        if constexpr (HT) {
            HtWalk<K> walk;
            const int tb = a.ht_sb - L;
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++) {
                const K k = kq[e + 1];
                int cb = hf.ht_common_bits(k, kq[e]);
                const int cb_next = hf.ht_common_bits(kq[e + 2], k);
                if (e == 0) cb = cb < 0 ? 0 : cb; else { cb = cb < 0 ? 0 : cb; walk.inherit(cb); }
                const bool all = ((hot >> e) & 1u) || k == kq[e] || kq[e + 2] == k;       // a hot bucket, or tied with a neighbour
                const int need = all ? a.ht_sb : (cb > cb_next ? cb : cb_next);
                walk.extend(hf.ht_stream(k), a.ht_sb, dec8, need);
                sc4[e] = walk.result(cb, tb);
            }
        } else {
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++) sc4[e] = HtScan{0u, 0u, 0u, false, false};
        }
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++)
            if (((todo4 >> e) & 1u) &&
                place_one(i0 + e, (hot >> e) & 1u, (myfl >> e) & 1u, kq[e + 1], kq[e], kq[e + 2], vq[e], sa4[e], lc4[e], sc4[e]))
                fin |= 1u << e;
#else
#pragma unroll
        for (int e = 0; e < FIN_IPT; e++) { sa4[e] = vq[e]; lc4[e] = (u32)kq[e + 1] ^ (u32)kq[e]; }
        fin = todo4;
#endif
        if (fin == 15u) {
            *reinterpret_cast<uint4 *>(a.order_g + j0) = uint4{sa4[0], sa4[1], sa4[2], sa4[3]};
            if (a.lcp_g) *reinterpret_cast<uint4 *>(a.lcp_g + j0) = uint4{lc4[0], lc4[1], lc4[2], lc4[3]};
        } else {
#pragma unroll
            for (int e = 0; e < FIN_IPT; e++)
                if ((fin >> e) & 1u) {
                    a.order_g[j0 + e] = sa4[e];
                    if (a.lcp_g) a.lcp_g[j0 + e] = lc4[e];
                }
        }
        if (own & 16u) {                                // the overhang of the last bucket that starts in the stretch
            u32 sa1, lc1;
            HtScan sc1{0u, 0u, 0u, false, false};
            if constexpr (HT) sc1 = hf.ht_read(kt[ih], kt[ih - 1], dec8, a.ht_sb - L);
            if (place_one(ih, false, false, kt[ih], kt[ih - 1], kt[ih + 1], vt[ih], sa1, lc1, sc1)) {
                a.order_g[base + (u32)ih] = sa1;
                if (a.lcp_g) a.lcp_g[base + (u32)ih] = lc1;
            }
        }
    }
    __syncthreads();
    // phase 2: the members of small tie groups, one per thread (as in lvl0_place_kernel)
    const u32 todo = n_work;
    for (u32 q = tid; q < todo; q += BLOCK) {
        const u32 i = work[q];
        u32 x4;
        __builtin_memcpy(&x4, a.s8 + vt[i] + (HT ? (u32)wdep[q] : (u32)w), 4);
        next4[i] = x4;
    }
    __syncthreads();
    for (u32 q = tid; q < todo; q += BLOCK) {
        const int i = (int)work[q];
        if (fin_place_tied(a, i, kt, vt, next4, base, limit, max_len, HT ? dec8 : (const uint8_t *)nullptr, HT ? (u32)wdep[q] : 0u)) {
            const u32 j = base + (u32)i;
            a.order_g[j] = vt[i];
            atomicOr(&keep_bits[i >> 5], 1u << (i & 31));
            my_keep++;
            if constexpr (HT) {
                const u32 shared = (u32)wdep[q];
                a.xdep0[j] = (uint8_t)(shared > (u32)a.ht_wmin ? (shared - (u32)a.ht_wmin > 255u ? 255u : shared - (u32)a.ht_wmin) : 0u);
            }
            const K k = kt[i], x = k ^ a.rep_t;
            const bool has_term = HT ? false : ((K)(x - a.ones) & ~x & a.highs) != 0;       // (a tied key holds none)
            if (j == 0 || has_term || k != kt[i - 1]) {     // the first of its group
                atomicOr(&gs_bits[i >> 5], 1u << (i & 31));
                if (a.lcp_g) {
                    if constexpr (HT) a.lcp_g[j] = j > 0 ? hf.ht_read(k, kt[i - 1], dec8).common : 0u;
                    else a.lcp_g[j] = j > 0 ? fin_lcp_of_key_pair(a, k, kt[i - 1]) : 0u;
                }
            }
        }
    }
    my_keep = wave_sum(my_keep);
    if (lane_id() == 0 && my_keep) atomicAdd(&n_keep, my_keep);
    __syncthreads();
    // the bits of the ranks [c0, c0 + FIN_CHUNK + FIN_G): OR-ed into the global words (the overhang shares its words with
    // the next workgroup); nearly all of them are zero
    if (tid < (FIN_CHUNK + FIN_G + 31) / 32) {
        // staged index FIN_LEFT + 32 t .. + 31  ->  global bit c0 + 32 t ..
        const u32 ib = FIN_LEFT + 32u * tid;
        const u32 sh = ib & 31u, wi = ib >> 5;
        u32 kb = keep_bits[wi] >> sh, gb = gs_bits[wi] >> sh;
        if (sh) { kb |= keep_bits[wi + 1] << (32u - sh); gb |= gs_bits[wi + 1] << (32u - sh); }
        const u32 bit0 = c0 + 32u * tid;
        if (kb) atomicOr(reinterpret_cast<u32 *>(a.keep) + (bit0 >> 5), kb);
        if (gb) atomicOr(reinterpret_cast<u32 *>(a.gstart) + (bit0 >> 5), gb);
    }
    if (tid == 0) {
        a.block_keep[blockIdx.x] = n_keep;
        if (a.spec_keep && n_keep) a.spec_keep[0] = 1u;
    }
}

// group starts kept as one bit per rank (the fused finish): the naming predicate of the first compaction
struct BitStarts {
    static constexpr bool HAS_KEYS = false;
    const u64 *bits;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (u32)(bits[i >> 6] >> (i & 63u)) & 1u; }
};

// LCP entries by comparing the two suffixes from their first symbol (same cap rule as lcp8_kernel)
// ... of a LIST of ranks: the members of the groups that were still open when the rounds went over to prefix doubling
// (their slots, kept when that round compacted its domain) -- a few per cent of all ranks, no pass over the others
__global__ __launch_bounds__(BLOCK) void lvl0_lcp_text_list_kernel(const uint8_t *__restrict__ s8, const u32 *__restrict__ sa,
                                                                   const u32 *__restrict__ ranks, u32 count,
                                                                   u32 *__restrict__ lcp, u32 *__restrict__ capped,
                                                                   LcpBudget budget, bool hinted = false)
{
    // hinted (the persistent rounds, persist_rounds.h): lcp[r] holds what the two suffixes are known to share -- the depth
    // of the round in which they came apart --, and the comparison starts there
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    const u32 r = ranks[t];
    if (r == 0) { lcp[0] = 0; return; }
    const u32 h0 = hinted ? lcp[r] : 0u;
    // (a pair known to share LCP_SOFT_CAP symbols or more goes straight to the finishing pass, whose comparisons run a
    // wavefront wide: one thread walking 10 000 symbols is 300 dependent round trips -- 0.3 ms that a small build waits for)
    if (hinted) budget.per_slot = 0;                    // (... and none of them goes deeper than that here)
    const u32 h = h0 >= LCP_SOFT_CAP ? (LCP_PARTIAL_BIT | h0) : lcp_bytes_capped(s8, sa[r - 1], sa[r], h0, budget);
    if (h & LCP_PARTIAL_BIT) raise_flag(capped);
    lcp[r] = h;
}

// A later, compacted domain of m elements (slot[] = where each sits in the global order): untied
// elements already have their place (written by the previous round's write-back); small groups are
// placed by lvl0_place_tied; members of large groups are marked in keep[] (one bit each).
__global__ __launch_bounds__(BLOCK) void dc3_refine_classify_kernel(const u32 *__restrict__ elem, FlagArrIn starts,
                                                                    const u32 *__restrict__ slot, u32 m,
                                                                    const uint8_t *__restrict__ s8, u32 n0, u32 depth,
                                                                    u32 *__restrict__ order_g, u32 *__restrict__ names_g,
                                                                    u64 *__restrict__ keep, u32 *__restrict__ fail,
                                                                    u32 limit, u32 max_len, u32 *__restrict__ name_of,
                                                                    LongRepeats lr, u32 *__restrict__ lcp_g,
                                                                    const uint2 *__restrict__ only_rest = nullptr,
                                                                    const uint8_t *__restrict__ xdep = nullptr)
{
    // (as in the placement pass: every tied element of the workgroup's stretch fetches the 8 symbols behind the common
    // depth once, and the members of a group rank themselves against those instead of gathering each other's text)
    // only_rest != nullptr: the in-LDS round classified its own tiles (lds_group_sort.h: LgClassify) -- only the positions
    // the global sort took are looked at, and the keep bits are OR-ed into words the host has zeroed
    __shared__ u64 next8[BLOCK];
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    u32 my_keep = 0;
    const bool mine = !only_rest || LgUncovered{only_rest, m}(j);       // (a group lies wholly inside or outside the tiles)
    const bool tied = mine && j < m && ((j > 0 && !starts(j)) || (j + 1 < m && !starts(j + 1)));
    if (tied && xdep) depth += (u32)xdep[j];            // (the members of a group share it)
    // (limit 1: nothing is compared -- deep doubling rounds --, so nothing is fetched: the gather was 0.5 ms of a 0.73 ms launch
    // over 16 M elements)
    if (tied && limit > 1u) next8[threadIdx.x] = load_u64_unaligned(s8 + lvl0_pos(elem[j], n0) + depth);
    __syncthreads();
    if (tied)
        my_keep = lvl0_place_tied(j, elem, starts, slot, m, s8, n0, depth, order_g, names_g, lcp_g, NoLcp(), fail, limit, max_len,
                                  name_of, lr, NextSymbols{next8, blockIdx.x * BLOCK, (u32)BLOCK});
    // keep[]: one bit per element (entries m.. of the last word are 0: the exclusive scan over m + 1 yields the total)
    const u64 bal = __ballot(my_keep != 0);
    if (lane_id() == 0) {
        if (!only_rest) keep[j >> 6] = bal;
        else if (bal) atomicOr((unsigned long long *)&keep[j >> 6], (unsigned long long)bal);
    }
}

// A repeat too long for the direct ordering leaves its group half written: put the whole domain back
// the way it was before the classify pass (elem[] and the domain's predicate are untouched by it).
template <class Starts>
__global__ __launch_bounds__(BLOCK) void dc3_refine_restore_kernel(const u32 *__restrict__ elem, Starts starts,
                                                                   const u32 *__restrict__ slot, u32 m,
                                                                   u32 *__restrict__ order_g, u32 *__restrict__ names_g)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const u32 g = slot ? slot[j] : j;
    order_g[g] = elem[j];
    if (names_g) names_g[g] = starts(j);
}

// the members of large groups, compacted: the radix round's input.  Four consecutive domain positions per thread: their
// keep bits come out of one word, and a thread none of whose positions is kept (half of them, in natural-language text)
// is done after a single load.
#define COMPACT_IPT 4
template <class Starts>
__global__ __launch_bounds__(BLOCK) void dc3_refine_compact_kernel(const u32 *__restrict__ elem, Starts starts,
                                                                   const u32 *__restrict__ slot, BitIn keep,
                                                                   BitRank idx, u32 m,
                                                                   u32 *__restrict__ slot_out, u32 *__restrict__ elem_out,
                                                                   u32 *__restrict__ group_start,
                                                                   u32 *__restrict__ lcp_g = nullptr, int w = 0, int b = 0,
                                                                   int spare = 0, const uint8_t *__restrict__ xdep_in = nullptr,
                                                                   uint8_t *__restrict__ xdep_out = nullptr)
{
    // xdep (variable-length first-level keys): what the group of a position shares BEYOND the rounds' common depth --
    // first domain: written per rank by the placement pass (the whole symbols of the key less the least any key holds);
    // later domains: copied along
    const u32 j0 = (blockIdx.x * BLOCK + threadIdx.x) * COMPACT_IPT;
    if (j0 >= m) return;
    const u64 word = keep.bits[j0 >> 6];
    const u32 nib = (u32)(word >> (j0 & 63u)) & ((1u << COMPACT_IPT) - 1u);
    if (!nib) return;
    // (the rank of the first kept position among the kept ones; the others follow)
    u32 k = idx.word_prefix[j0 >> 6] + (u32)__popcll(word & (((u64)1 << (j0 & 63u)) - 1ull));
    // (what the four positions need is read for all four before any of it is used: one wait instead of one per kept
    // position -- the lines are the same ones)
    u32 st4[COMPACT_IPT], el4[COMPACT_IPT], sl4[COMPACT_IPT];
#pragma unroll
    for (int e = 0; e < COMPACT_IPT; e++) {
        const u32 j = j0 + e < m ? j0 + e : j0;
        st4[e] = starts(j);
        el4[e] = elem[j];
        sl4[e] = slot ? slot[j] : j;
    }
#pragma unroll
    for (int e = 0; e < COMPACT_IPT; e++) {
        const u32 j = j0 + e;
        if (j >= m || !((nib >> e) & 1u)) continue;
        const u32 st = st4[e];
        slot_out[k] = sl4[e];
        elem_out[k] = el4[e];
        group_start[k] = st;
        if (xdep_out) xdep_out[k] = xdep_in ? xdep_in[j] : (uint8_t)0;
        if constexpr (Starts::HAS_KEYS) {
            // the keyed first domain: the first rank of a group left to the rounds gets its LCP entry here, from the
            // two keys -- whichever member ends up there
            if (lcp_g && st) {
                bool whole;
                lcp_g[j] = j > 0 ? lvl0_lcp_of_keys(starts, w, b, spare, j, whole) : 0u;
            }
        }
        k++;
    }
}

// key = (dense group number << w2*b) | next window of w2 symbols at offset `depth`
__global__ __launch_bounds__(BLOCK) void dc3_refine_keys_kernel(const uint8_t *__restrict__ s8,
                                                                const u32 *__restrict__ elems,
                                                                const u32 *__restrict__ group, u32 n_tied, u32 n0,
                                                                u32 depth, int w2, int b, u32 term_first,
                                                                u64 *__restrict__ keys, u32 *__restrict__ vals,
                                                                const uint8_t *__restrict__ xdep = nullptr,
                                                                const u32 *__restrict__ full_idx = nullptr)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_tied) return;
    const u32 p = lvl0_pos(elems[j], n0) + depth + (xdep ? (u32)xdep[full_idx ? full_idx[j] : j] : 0u);
    u64 lo8, hi8;
    __builtin_memcpy(&lo8, s8 + p, 8);
    __builtin_memcpy(&hi8, s8 + p + 8, 8);
    u64 key = group[j];
    bool ended = false;
    for (int i = 0; i < w2; i++) {
        const u32 byte = (u32)((i < 8 ? lo8 >> (8 * i) : hi8 >> (8 * (i - 8))) & 0xFFu);
        const u32 x = ended ? 0u : byte;
        ended = ended || x == 0xFFu;
        key = (key << b) | (u64)(x == 0xFFu ? term_first : x);
    }
    keys[j] = key;
    vals[j] = elems[j];                 // (the suffix itself travels with its key: no look-up after the sort)
}

// ---- prefix doubling for long repeats (all-suffix mode) ------------------------------------------
// A domain that shrinks slowly holds long repeats (boilerplate, runs of one character): symbol
// windows would take 6-12 symbols off per round.  Then every suffix gets a NAME -- the global
// position where its group of equal prefixes starts, its own position once it is placed -- kept in
// name_of[text position], and a round keys the members of a group by the name of the suffix `depth`
// symbols further on (Manber-Myers / Larsson-Sadakane): names order suffixes by at least `depth`
// symbols, so every round doubles the depth and the rounds are bounded by log2(n).
__global__ __launch_bounds__(BLOCK) void dc3_names_init_kernel(const u32 *__restrict__ order_g, u32 n,
                                                               u32 *__restrict__ name_of)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) name_of[order_g[i]] = i;
}

// start_slot[k] = global position of the first member of the domain's k-th group (inc = inclusive scan of flag)
__global__ __launch_bounds__(BLOCK) void dc3_group_starts_kernel(const u32 *__restrict__ flag, const u32 *__restrict__ inc,
                                                                 const u32 *__restrict__ slot, u32 m,
                                                                 u32 *__restrict__ start_slot)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r < m && flag[r]) start_slot[inc[r] - 1u] = slot[r];
}

// (only_kept: members of groups that were just placed for good keep their exact position as name)
__global__ __launch_bounds__(BLOCK) void dc3_names_update_kernel(const u32 *__restrict__ elem, const u32 *__restrict__ inc,
                                                                 const u32 *__restrict__ start_slot, u32 m,
                                                                 const u64 *__restrict__ only_kept,
                                                                 u32 *__restrict__ name_of)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= m) return;
    if (only_kept && !((only_kept[r >> 6] >> (r & 63u)) & 1u)) return;
    name_of[elem[r]] = start_slot[inc[r] - 1u];
}

// key = (dense group number << 32) | name of the suffix `depth` symbols further on
__global__ __launch_bounds__(BLOCK) void dc3_double_keys_kernel(const u32 *__restrict__ name_of,
                                                                const u32 *__restrict__ elems,
                                                                const u32 *__restrict__ group, u32 m, u32 depth, int name_bits,
                                                                u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    keys[j] = ((u64)group[j] << name_bits) | (u64)name_of[elems[j] + depth];      // (a name is a rank: bit_width(n) bits, not 32 -- a pass less)
    vals[j] = elems[j];                 // (the suffix itself travels with its key: no look-up after the sort)
}

// after the sort: the slots of the domain receive their members in refined order (globally and as
// the next domain's elem[]), and the naming predicate is updated
__global__ __launch_bounds__(BLOCK) void dc3_refine_writeback_kernel(const u64 *__restrict__ keys,
                                                                     const u32 *__restrict__ vals,
                                                                     const u32 *__restrict__ slots,
                                                                     const u32 *__restrict__ elems, u32 n_tied,
                                                                     u64 rep_t, u64 ones, u64 highs,
                                                                     u32 *__restrict__ order_g, u32 *__restrict__ names_g,
                                                                     u32 *__restrict__ elem_out, u32 *__restrict__ flag_out,
                                                                     u32 *__restrict__ lcp_g = nullptr, u32 depth = 0,
                                                                     int w2 = 0, int b = 0,
                                                                     const u32 *__restrict__ full_idx = nullptr,
                                                                     const uint8_t *__restrict__ xdep = nullptr)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_tied) return;
    const u64 k = keys[r], kp = r ? keys[r - 1] : 0;
    const u64 x = k ^ rep_t;
    const u64 tz = (x - ones) & ~x & highs;
    const bool has_term = tz != 0;                              // a terminator inside the window: unique
    // (full_idx: the sorted pairs are the compacted rest of a domain; groups keep their stretches, so the r-th of
    // them belongs where the r-th of the rest came from)
    const u32 at = full_idx ? full_idx[r] : r;
    const u32 slot = slots[at], e = vals[r];
    const u32 f = (r == 0 || has_term || k != kp) ? 1u : 0u;
    order_g[slot] = e;
    if (names_g) names_g[slot] = f;
    elem_out[at] = e;
    flag_out[at] = f;
    // symbol windows: where a group splits, the LCP entry of the rank that starts the new group is what the two
    // windows have in common behind the `depth` symbols the group shares (cut at a terminator: two equal terminator
    // codes are different terminators) -- final whichever members end up at the seam.  The first rank of the old
    // group keeps the entry it has.
    const int gshift = w2 * b;
    if (lcp_g && f && r > 0 && (k >> gshift) == (kp >> gshift)) {
        const u64 d = (k ^ kp) & (((u64)1 << gshift) - 1u);
        const u32 inv_b = (65536u + (u32)b - 1u) / (u32)b;   // (uniform: x / b = (x * inv_b) >> 16 for bit positions below 64)
        const u32 mism = d ? (u32)w2 - 1u - (((u32)(63 - __builtin_clzll(d)) * inv_b) >> 16) : (u32)w2;
        const u32 term = tz ? (u32)w2 - 1u - (((u32)__builtin_ctzll(tz) * inv_b) >> 16) : (u32)w2;
        lcp_g[slot] = depth + (xdep ? (u32)xdep[at] : 0u) + (mism < term ? mism : term);
    }
}

// one bit per rank: the slots of the kept members of a domain
__global__ __launch_bounds__(BLOCK) void lvl0_mark_slots_kernel(const u32 *__restrict__ slot, BitIn keep, u32 m,
                                                                u32 *__restrict__ mask)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m || !keep(j)) return;
    const u32 s = slot ? slot[j] : j;
    atomicOr(&mask[s >> 5], 1u << (s & 31u));
}

// what the placement pass left undone, next to the other flags (speculative build: read at the very end):
// the sum of its workgroups' counts (out[] was zeroed with the build's flag words; a few workgroups add into it)
#define SPEC_COUNT_TILE (BLOCK * 16)
__global__ __launch_bounds__(BLOCK) void spec_counts_kernel(const u32 *__restrict__ block_keep, u32 gp,
                                                            const u32 *__restrict__ fail, u32 *__restrict__ out)
{
    __shared__ u32 lds[WAVES_PER_BLOCK];
    const u32 base = blockIdx.x * SPEC_COUNT_TILE;
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const u32 i = base + j * BLOCK + threadIdx.x;
        if (i < gp) sum += block_keep[i];
    }
    sum = wave_sum(sum);
    if (lane_id() == 0) lds[wave_id()] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 t = lds[0] + lds[1] + lds[2] + lds[3];
        if (t) atomicAdd(&out[0], t);
        if (blockIdx.x == 0) out[1] = *fail;
    }
}

// Several stretches of device memory set to a value each in ONE launch (the k-gram marks' table, the keep bits and the
// group-start bits in front of the first placement pass: a fill launch each cost a launch-sized gap on the build's one
// stream).  Regions of whole words that start at multiples of 16 bytes; a workgroup belongs to one region and a thread
// stores four 16-byte groups.
#define CLEAR_MAX_REGIONS 4
#define CLEAR_BLOCK_WORDS (BLOCK * 16u)
struct ClearRegions {
    u32 *p[CLEAR_MAX_REGIONS];
    u32 words[CLEAR_MAX_REGIONS], value[CLEAR_MAX_REGIONS], first_block[CLEAR_MAX_REGIONS + 1];
    int count = 0;
};
__global__ __launch_bounds__(BLOCK) void clear_regions_kernel(ClearRegions r)
{
    int k = 0;
    while (k + 1 < r.count && blockIdx.x >= r.first_block[k + 1]) k++;
    u32 *p = r.p[k];
    const u32 words = r.words[k], v = r.value[k];
    const u32 w0 = (blockIdx.x - r.first_block[k]) * CLEAR_BLOCK_WORDS;
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        const u32 i = w0 + (j * BLOCK + threadIdx.x) * 4u;
        if (i + 4u <= words) *reinterpret_cast<uint4 *>(p + i) = uint4{v, v, v, v};
        else
            for (u32 q = i; q < words; q++) p[q] = v;
    }
}
