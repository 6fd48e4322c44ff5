// alphabet.h -- the kernels in front of the suffix sort: which code points the corpus holds, their dense codes, the
// byte / u32 symbol stream the build sorts, the planning sample and the checks of the caller's document layout.
#pragma once
#include "common.h"

#define TEXT_SYMBOLS EAST_HIP_TERMINATOR_START      // 0x0A00 = 2560 possible text code points
#define PRESENT_WORDS (TEXT_SYMBOLS / 32)           // 80
#define TERM_TAG EAST_HIP_TERMINATOR_TAG            // tagged encoding: bit 31 marks a terminator, text is any code point
#define HI_SYMBOLS (0x110000u - TEXT_SYMBOLS)       // text code points at or above the reference's terminator base
#define HI_WORDS (HI_SYMBOLS / 32u)                 // 34736

// ------------------------------------------------------------ prep kernels --
// (vec: the caller's symbol array is 16-byte aligned, as every allocation is; a misaligned view of a
// larger buffer takes the symbol-by-symbol path)
__global__ __launch_bounds__(BLOCK) void presence_kernel(const u32 *__restrict__ sym, u32 n, int vec,
                                                         u32 *__restrict__ present)
{
    __shared__ u32 bits[PRESENT_WORDS];
    if (threadIdx.x < PRESENT_WORDS) bits[threadIdx.x] = 0;
    __syncthreads();
    // a plain LDS read filters the (overwhelmingly common) already-set case; a stale read only
    // costs a redundant atomic
    auto mark = [&](u32 c) {
        if (c < TEXT_SYMBOLS && !(((volatile u32 *)bits)[c >> 5] & (1u << (c & 31u))))
            atomicOr(&bits[c >> 5], 1u << (c & 31u));
    };
    const u32 stride = gridDim.x * BLOCK;
    const u32 n4 = vec ? n >> 2 : 0u;                      // four symbols per 16-byte load, four loads in flight
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    for (; i + 3u * stride < n4; i += 4u * stride) {
        const uint4 a = reinterpret_cast<const uint4 *>(sym)[i], b = reinterpret_cast<const uint4 *>(sym)[i + stride];
        const uint4 c = reinterpret_cast<const uint4 *>(sym)[i + 2u * stride], d = reinterpret_cast<const uint4 *>(sym)[i + 3u * stride];
        mark(a.x); mark(a.y); mark(a.z); mark(a.w);
        mark(b.x); mark(b.y); mark(b.z); mark(b.w);
        mark(c.x); mark(c.y); mark(c.z); mark(c.w);
        mark(d.x); mark(d.y); mark(d.z); mark(d.w);
    }
    for (; i < n4; i += stride) {
        const uint4 c = reinterpret_cast<const uint4 *>(sym)[i];
        mark(c.x); mark(c.y); mark(c.z); mark(c.w);
    }
    for (u32 i = (n4 << 2) + blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) mark(sym[i]);
    __syncthreads();
    if (threadIdx.x < PRESENT_WORDS && bits[threadIdx.x]) atomicOr(&present[threadIdx.x], bits[threadIdx.x]);
}

// Dense codes of the text alphabet from the presence bitmap: code point c -> its rank (1 ..) among the code
// points present, 0 if absent; flags[FLAG_SIGMA] = their number.  One workgroup, ten code points per thread.
// `assumed` != NONE: the host went ahead with that alphabet size (speculative build); a different one is recorded in
// flags[FLAG_STATUS].
#define FLAG_CAPPED 0
#define FLAG_STATUS 1
#define FLAG_SIGMA 2
#define FLAG_KEEP 3              // a boolean: a speculative build that expected no rounds left suffixes in large groups (set by the placement's workgroups)
#define FLAG_FAIL 4              // ... and its placement gave up on a long repeat, where that is not FLAG_PLACE_FAIL itself (spec_counts_kernel)
#define FLAG_SIGMA_HI 5
#define FLAG_PLACE_FAIL 6        // the placement pass's "a repeat too long to order directly" (window_sort.h: fail), zeroed with the flags
#define FLAG_KG_BAD 7            // the fused finish could not mark every k-gram bucket start (Ctx::kg_bad)
#define FLAG_SAMPLE 8             // 17 words: sample_prefix_kernel's counts (dup2, dup4 for l = 1 .. 8) and the sample size
#define FLAG_ANN_LISTED 25        // the ranks ann_wide_kernel decided: one add per run of tiles (the next build's block order, build.h)
#define FLAG_WORDS 32
#define STATUS_NO_TERMINATOR 1u
#define STATUS_N_STRINGS 2u
#define STATUS_SIGMA_GUESS 4u
#define STATUS_BAD_SYMBOL 8u
// guess: the code map (TEXT_SYMBOLS words) and the presence bitmap (PRESENT_WORDS words) of the handle's last build,
// kept outside the arena.  A speculative build has already turned the symbols into bytes with that map
// (presence_remap_kernel); `check` then compares the bitmaps -- any difference, and the bytes are wrong: STATUS_SIGMA_GUESS --,
// and in any case the guess is replaced by what this build found.
__device__ __forceinline__ void codemap_block(const u32 *__restrict__ present, u32 assumed, u32 *__restrict__ code_map,
                                              u32 *__restrict__ flags, u32 *__restrict__ guess, int check)
{
    if (guess && threadIdx.x < PRESENT_WORDS) {
        u32 *gp = guess + TEXT_SYMBOLS;
        if (check && gp[threadIdx.x] != present[threadIdx.x]) atomicOr(&flags[FLAG_STATUS], STATUS_SIGMA_GUESS);
        gp[threadIdx.x] = present[threadIdx.x];
    }
    static_assert(TEXT_SYMBOLS == BLOCK * 10, "ten code points per thread");
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    const u32 c0 = threadIdx.x * 10u;
    u32 bits = 0, cnt = 0;
#pragma unroll
    for (u32 i = 0; i < 10; i++) {
        const u32 b = (present[(c0 + i) >> 5] >> ((c0 + i) & 31u)) & 1u;
        bits |= b << i;
        cnt += b;
    }
    u32 total;
    u32 run = block_exclusive_sum(cnt, lds4, total);
#pragma unroll
    for (u32 i = 0; i < 10; i++) {
        const u32 code = ((bits >> i) & 1u) ? ++run : 0u;
        code_map[c0 + i] = code;
        if (guess) guess[c0 + i] = code;
    }
    if (threadIdx.x == 0) {
        flags[FLAG_SIGMA] = total;
        u32 st = 0;
        if (assumed != 0xFFFFFFFFu && assumed != total) st |= STATUS_SIGMA_GUESS;
        if (st) atomicOr(&flags[FLAG_STATUS], st);
    }
}

// The code map and, in the same launch, the check that every document ends in a terminator (memory safety: it stops every
// suffix comparison).  Every workgroup looks at its BLOCK documents and ORs what it finds straight into the status flag --
// nothing crosses workgroups --, and workgroup 0 makes the code map besides.
__global__ __launch_bounds__(BLOCK) void validate_codemap_kernel(const u32 *__restrict__ sym, const u32 *__restrict__ doc_off,
                                                                 u32 n_docs, u32 tagged, const u32 *__restrict__ present,
                                                                 u32 assumed, u32 *__restrict__ code_map,
                                                                 u32 *__restrict__ flags, u32 *__restrict__ guess, int check)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d < n_docs) {
        const u32 c = sym[doc_off[d + 1] - 1];
        if (tagged ? !(c >> 31) : c < TEXT_SYMBOLS) atomicOr(&flags[FLAG_STATUS], STATUS_NO_TERMINATOR);
    }
    if (blockIdx.x == 0) codemap_block(present, assumed, code_map, flags, guess, check);
}

// Planning sample ("The plan of a first build"): SAMPLE_N consecutive suffixes of the raw symbol stream;
// for every prefix length l = 1 .. SAMPLE_MAX_L, how many of them share their first l symbols (no terminator among
// them) with at least one / at least three others of the sample.  Natural-language text repeats words within a few
// thousand characters, random text does not: the host takes the window width and the fused finish from these counts
// in the same build, no history needed.  One workgroup per prefix length; counts by hashing into a table of 16-bit
// counters in LDS, twice with different hashes, the smaller count taken (count-min).
#define SAMPLE_N 8192
#define SAMPLE_MAX_L 8
#define SAMPLE_SLOTS 16384
#define SAMPLE_THREADS 1024
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_prefix_kernel(const u32 *__restrict__ sym, u32 n, u32 pos0, u32 count,
                                                                       u32 *__restrict__ out)
{
    constexpr int PER = SAMPLE_N / SAMPLE_THREADS;
    __shared__ uint16_t s16[SAMPLE_N + SAMPLE_MAX_L];   // the symbols; 0xFFFF = a terminator (or the end of the stream)
    __shared__ u32 tab[SAMPLE_SLOTS / 2];               // 16-bit counters, two to a word
    __shared__ u32 acc[2 * SAMPLE_MAX_L];
    for (u32 i = threadIdx.x; i < SAMPLE_N + SAMPLE_MAX_L; i += SAMPLE_THREADS) {
        const u32 p = pos0 + i;
        const u32 c = p < n ? sym[p] : 0xFFFFFFFFu;
        s16[i] = c < TEXT_SYMBOLS ? (uint16_t)c : (uint16_t)0xFFFFu;
    }
    if (threadIdx.x < 2 * SAMPLE_MAX_L) acc[threadIdx.x] = 0;
    {
        const int l = (int)blockIdx.x + 1;              // one workgroup per prefix length, side by side
        u32 first_count[PER];
        u32 d2 = 0, d4 = 0;
        for (int variant = 0; variant < 2; variant++) {
            __syncthreads();
            for (u32 i = threadIdx.x; i < SAMPLE_SLOTS / 2; i += SAMPLE_THREADS) tab[i] = 0;
            __syncthreads();
            u32 slot[PER];
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const u32 p = threadIdx.x + SAMPLE_THREADS * q;
                u32 h = 0x811C9DC5u;
                bool ok = p < count;
                for (int t = 0; t < l; t++) {
                    const u32 c = s16[p + t];
                    ok = ok && c != 0xFFFFu;
                    h = (h ^ c) * 0x01000193u;
                }
                h ^= h >> 15;
                h *= variant ? 0x9E3779B1u : 0x85EBCA6Bu;
                slot[q] = ok ? h >> 18 : 0xFFFFFFFFu;   // 14 bits
                if (ok) atomicAdd(&tab[slot[q] >> 1], 1u << (16u * (slot[q] & 1u)));
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const u32 c = slot[q] != 0xFFFFFFFFu ? (tab[slot[q] >> 1] >> (16u * (slot[q] & 1u))) & 0xFFFFu : 0u;
                if (variant == 0) first_count[q] = c;
                else {
                    const u32 both = c < first_count[q] ? c : first_count[q];
                    d2 += both >= 2u ? 1u : 0u;
                    d4 += both >= 4u ? 1u : 0u;
                }
            }
        }
        d2 = wave_sum(d2);
        d4 = wave_sum(d4);
        if (lane_id() == 0) { atomicAdd(&acc[2 * (l - 1)], d2); atomicAdd(&acc[2 * (l - 1) + 1], d4); }
    }
    __syncthreads();
    if (threadIdx.x < 2) out[2 * blockIdx.x + threadIdx.x] = acc[2 * blockIdx.x + threadIdx.x];
    if (threadIdx.x == 0 && blockIdx.x == 0) out[2 * SAMPLE_MAX_L] = count;
}

// Speculative build: presence bitmap AND byte stream in one pass over the symbols, the bytes through the code map of
// the handle's last build (guess; validate_codemap_kernel finds out whether that was right).  16-byte aligned input only.
__global__ __launch_bounds__(BLOCK) void presence_remap_kernel(const u32 *__restrict__ sym, u32 n,
                                                               const u32 *__restrict__ guess, u32 *__restrict__ present,
                                                               uint8_t *__restrict__ s8)
{
    __shared__ u32 bits[PRESENT_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t map8[TEXT_SYMBOLS];
    if (threadIdx.x < PRESENT_WORDS) bits[threadIdx.x] = 0;
    {
        // (the code map's 2 560 words with 16-byte loads, all of a thread's requested before the first is used -- own
        // allocation, 256-byte aligned --: a loop of one word per step was ten round trips in front of the first symbol)
        static_assert(TEXT_SYMBOLS % 4 == 0, "whole 16-byte groups");
        constexpr u32 GROUPS = TEXT_SYMBOLS / 4, ROUNDS = (GROUPS + BLOCK - 1) / BLOCK;
        uint4 q[ROUNDS];
#pragma unroll
        for (u32 r = 0; r < ROUNDS; r++) {
            const u32 g = threadIdx.x + r * BLOCK;
            q[r] = reinterpret_cast<const uint4 *>(guess)[g < GROUPS ? g : 0u];
        }
#pragma unroll
        for (u32 r = 0; r < ROUNDS; r++) {
            const u32 g = threadIdx.x + r * BLOCK;
            if (g < GROUPS)
                reinterpret_cast<u32 *>(map8)[g] = (q[r].x & 0xFFu) | ((q[r].y & 0xFFu) << 8) | ((q[r].z & 0xFFu) << 16) | ((q[r].w & 0xFFu) << 24);
        }
    }
    __syncthreads();
    auto code = [&](u32 c) -> u32 {
        if (c >= TEXT_SYMBOLS) return 0xFFu;
        if (!(((volatile u32 *)bits)[c >> 5] & (1u << (c & 31u)))) atomicOr(&bits[c >> 5], 1u << (c & 31u));
        return map8[c];
    };
    auto word = [&](const uint4 q) -> u32 { return code(q.x) | (code(q.y) << 8) | (code(q.z) << 16) | (code(q.w) << 24); };
    const u32 stride = gridDim.x * BLOCK, n4 = n >> 2;
    u32 *out = reinterpret_cast<u32 *>(s8);
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    for (; i + 3u * stride < n4; i += 4u * stride) {       // four 16-byte loads in flight
        const uint4 a = reinterpret_cast<const uint4 *>(sym)[i], b = reinterpret_cast<const uint4 *>(sym)[i + stride];
        const uint4 c = reinterpret_cast<const uint4 *>(sym)[i + 2u * stride], d = reinterpret_cast<const uint4 *>(sym)[i + 3u * stride];
        out[i] = word(a);
        out[i + stride] = word(b);
        out[i + 2u * stride] = word(c);
        out[i + 3u * stride] = word(d);
    }
    for (; i < n4; i += stride) out[i] = word(reinterpret_cast<const uint4 *>(sym)[i]);
    if (blockIdx.x == 0 && threadIdx.x < 20u) {            // the last n % 4 symbols and the 16 pad bytes
        const u32 j = (n4 << 2) + threadIdx.x;
        if (j < n) s8[j] = (uint8_t)code(sym[j]);
        else if (j < n + 16u) s8[j] = 0;
    }
    __syncthreads();
    if (threadIdx.x < PRESENT_WORDS && bits[threadIdx.x]) atomicOr(&present[threadIdx.x], bits[threadIdx.x]);
}

struct TermIn {                                 // 1 at terminators; defined on [0, n]
    const u32 *sym;
    u32 n;
    u32 tagged;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        return (i < n && (tagged ? sym[i] >> 31 : (u32)(sym[i] >= TEXT_SYMBOLS))) ? 1u : 0u;
    }
};

// ---- tagged encoding: text code points at or above U+0A00 ------------------------------------------
// (a stream whose terminators carry EAST_HIP_TERMINATOR_TAG may hold any code point as text; the kernels above
// and below read such a stream unchanged as long as no text symbol reaches U+0A00 -- a tagged terminator is
// ">= U+0A00" --, and that is found out here)
// (the whole bitmap -- 136 KiB -- lives in the workgroup's LDS: a plain LDS read filters the bits that are set, which
// in CJK text is every symbol after the first few thousand; one 1024-thread workgroup per CU, grid-stride, and only
// the words a workgroup has touched go to the global bitmap)
#define PRESENCE_HI_THREADS 1024
__global__ __launch_bounds__(PRESENCE_HI_THREADS) void presence_hi_kernel(const u32 *__restrict__ sym, u32 n,
                                                                          u32 *__restrict__ hi_bits, u32 *__restrict__ status)
{
    __shared__ u32 bits[HI_WORDS];
    for (u32 w = threadIdx.x; w < HI_WORDS; w += PRESENCE_HI_THREADS) bits[w] = 0;
    __syncthreads();
    const u32 stride = gridDim.x * PRESENCE_HI_THREADS;
    for (u32 i = blockIdx.x * PRESENCE_HI_THREADS + threadIdx.x; i < n; i += stride) {
        const u32 c = sym[i];
        if (c < TEXT_SYMBOLS || (c >> 31)) continue;
        if (c >= 0x110000u) { atomicOr(status, STATUS_BAD_SYMBOL); continue; }
        const u32 k = c - TEXT_SYMBOLS;
        if (!(((volatile u32 *)bits)[k >> 5] & (1u << (k & 31u)))) atomicOr(&bits[k >> 5], 1u << (k & 31u));
    }
    __syncthreads();
    for (u32 w = threadIdx.x; w < HI_WORDS; w += PRESENCE_HI_THREADS)
        if (bits[w]) atomicOr(&hi_bits[w], bits[w]);
}

// hi_rank[w] = code points present below word w of the bitmap; flags[FLAG_SIGMA_HI] = their number.  One workgroup.
__global__ __launch_bounds__(BLOCK) void hi_rank_kernel(const u32 *__restrict__ hi_bits, u32 *__restrict__ hi_rank,
                                                        u32 *__restrict__ flags)
{
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    const u32 per = (HI_WORDS + BLOCK - 1) / BLOCK;
    const u32 w0 = threadIdx.x * per, w1 = w0 + per < HI_WORDS ? w0 + per : HI_WORDS;
    u32 cnt = 0;
    for (u32 w = w0; w < w1; w++) cnt += __popc(hi_bits[w]);
    u32 total;
    u32 run = block_exclusive_sum(cnt, lds4, total);
    for (u32 w = w0; w < w1; w++) { hi_rank[w] = run; run += __popc(hi_bits[w]); }
    if (threadIdx.x == 0) flags[FLAG_SIGMA_HI] = total;
}

__device__ __forceinline__ u32 hi_rank_of(const u32 *__restrict__ hi_bits, const u32 *__restrict__ hi_rank, u32 k)
{
    return hi_rank[k >> 5] + __popc(hi_bits[k >> 5] & ((1u << (k & 31u)) - 1u));
}

// dense codes when text at or above U+0A00 is present (tagged encoding): ONE text alphabet in code-point order --
// code points below U+0A00 through the code map (1..sigma_lo), those above by their rank in the bitmap
// (sigma_lo+1 ..) --, the terminators above it as ever.  s8 / s: the byte stream (sigma_t <= 254) or the u32 codes.
__global__ __launch_bounds__(BLOCK) void remap_hi_kernel(const u32 *__restrict__ sym, const u32 *__restrict__ term_ex,
                                                         const u32 *__restrict__ code_map,
                                                         const u32 *__restrict__ hi_bits, const u32 *__restrict__ hi_rank,
                                                         u32 sigma_lo, u32 sigma_t, u32 n, u32 *__restrict__ s,
                                                         uint8_t *__restrict__ s8)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) {
        const u32 c = sym[i];
        const bool term = c >> 31;
        u32 code;
        if (term) code = s ? sigma_t + 1u + term_ex[i] : 0xFFu;
        else if (c < TEXT_SYMBOLS) code = code_map[c];
        else code = sigma_lo + 1u + hi_rank_of(hi_bits, hi_rank, c < 0x110000u ? c - TEXT_SYMBOLS : 0u);
        if (s) s[i] = code; else s8[i] = (uint8_t)code;
    } else {
        if (s && i < n + 3) s[i] = 0;
        if (s8 && i < n + 16) s8[i] = 0;
    }
}

// byte path: only the byte stream is built (0xFF = terminator); the exact terminator numbers are
// never needed there, so no terminator scan runs
__global__ __launch_bounds__(BLOCK) void remap_bytes_kernel(const u32 *__restrict__ sym,
                                                            const u32 *__restrict__ code_map, u32 n, int vec,
                                                            uint8_t *__restrict__ s8)
{
    // sixteen symbols per thread: four 16-byte loads in flight, one 16-byte store (the grid covers n + 16 bytes)
    const u32 i = (blockIdx.x * BLOCK + threadIdx.x) * 16u;
    if (vec && i + 16u <= n) {
        uint4 c[4];
#pragma unroll
        for (int q = 0; q < 4; q++) c[q] = reinterpret_cast<const uint4 *>(sym + i)[q];
        u32 out[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u32 b0 = c[q].x < TEXT_SYMBOLS ? code_map[c[q].x] & 0xFFu : 0xFFu, b1 = c[q].y < TEXT_SYMBOLS ? code_map[c[q].y] & 0xFFu : 0xFFu;
            const u32 b2 = c[q].z < TEXT_SYMBOLS ? code_map[c[q].z] & 0xFFu : 0xFFu, b3 = c[q].w < TEXT_SYMBOLS ? code_map[c[q].w] & 0xFFu : 0xFFu;
            out[q] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        }
        *reinterpret_cast<uint4 *>(s8 + i) = uint4{out[0], out[1], out[2], out[3]};
    } else {
        for (u32 j = i; j < i + 16u && j < n + 16u; j++) {
            uint8_t v = 0;
            if (j < n) { const u32 c = sym[j]; v = c < TEXT_SYMBOLS ? (uint8_t)code_map[c] : (uint8_t)0xFF; }
            s8[j] = v;
        }
    }
}

// n_strings[d] must equal the terminators of document d.  Terminators sort above every text
// symbol, so the terminator-first suffixes are the tail of the document's suffix array: one
// search per document on the finished array replaces a counting pass over the corpus.  A wavefront
// per document, 64 probes per step: a 64 MiB document takes 5 steps of two dependent loads instead of 26.
template <class SYM>
__global__ __launch_bounds__(BLOCK) void validate_n_strings_kernel(const SYM *__restrict__ s, u32 term_first,
                                                                   const u32 *__restrict__ sa,
                                                                   const u32 *__restrict__ doc_off,
                                                                   const u32 *__restrict__ n_strings, u32 n_docs,
                                                                   u32 *__restrict__ status)
{
    const u32 d = blockIdx.x * WAVES_PER_BLOCK + wave_id(), lane = lane_id();
    if (d >= n_docs) return;
    u32 lo = doc_off[d], hi = doc_off[d + 1];           // the first terminator-first rank lies in [lo, hi]
    const u32 end = hi, last = doc_off[n_docs] - 1u;
    while (lo < hi) {
        const u32 step = (hi - lo + 63u) / 64u;
        const u64 probe = (u64)lo + (u64)lane * step;
        bool term = true;                               // (probes at or behind hi count as terminator-first)
        if (probe < hi) {
            const u32 q = sa[(u32)probe];
            const u32 p = q < last ? q : last;          // (a speculative build that guessed wrong leaves stale entries)
            term = (u32)s[p] >= term_first;
        }
        const u64 bal = __ballot(term);
        const u32 t = bal ? (u32)__ffsll((unsigned long long)bal) - 1u : 64u;
        const u32 new_hi = t < 64u ? (u32)((u64)lo + (u64)t * step < hi ? (u64)lo + (u64)t * step : hi) : hi;
        const u32 new_lo = t > 0u ? lo + (t - 1u) * step + 1u : lo;
        lo = new_lo < new_hi ? new_lo : new_hi;
        hi = new_hi;
    }
    if (lane == 0 && end - lo != n_strings[d]) atomicOr(status, STATUS_N_STRINGS);
}

__global__ __launch_bounds__(BLOCK) void remap_kernel(const u32 *__restrict__ sym,
                                                      const u32 *__restrict__ term_ex,
                                                      const u32 *__restrict__ code_map, u32 sigma_t,
                                                      u32 n, u32 *__restrict__ s, uint8_t *__restrict__ s8)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) {
        const u32 c = sym[i];
        const bool text = c < TEXT_SYMBOLS;
        const u32 code = text ? code_map[c] : sigma_t + 1u + term_ex[i];
        s[i] = code;
        if (s8) s8[i] = text ? (uint8_t)code : (uint8_t)0xFF;
    } else {
        if (i < n + 3) s[i] = 0;
        if (s8 && i < n + 16) s8[i] = 0;
    }
}
