// top.h -- ranked keyphrases on the device: the N best rows of every column of a score table that is already there, or the
// N best columns of every row (include/east_hip.h, "Ranked keyphrases"; `east keyphrases top`).
//
// A *segment* is a column (EAST_HIP_TOP_BY_TEXT: its members are the K rows) or a row (EAST_HIP_TOP_BY_KEYPHRASE: its
// members are the D columns).  A member is eligible when score >= threshold (a NaN never is, -0.0 >= 0.0 is); the eligible
// members are ordered by score descending and, among equal scores (-0.0 == +0.0), by member index ascending.
//
//   K x D doubles --a score becomes a 64-bit key whose unsigned order is the order of the doubles, -0.0 folded onto +0.0,
//     0 = not eligible (top_key)--> tiles of T <= 64 members, a member a lane: its rank inside the tile = the number of keys
//     of the tile in front of it by (key descending, member ascending), counted against the tile's keys in LDS (every lane
//     reads the same word: a broadcast); the best cap = min(n, T) go to slot (segment, tile), each to the place its rank
//     names, the unused places are zeroed--> S x NT sorted candidate lists
//   --a workgroup per segment, a thread per candidate: its final rank = its rank in its own list + for every other list
//     the number of its entries in front of the candidate (a binary search: the lists are sorted; lists of earlier tiles
//     win ties, their members are smaller), given up once it reaches n--> count[S], index[S x n], score[S x n]
//
// By text a column's members lie D * 8 bytes apart.  No lane walks a column: a workgroup takes a strip of 64 consecutive
// columns x one tile of rows, a wavefront reads 64 consecutive columns of a row in one coalesced 512-byte load (as
// graph_bits_kernel does) and writes the keys to LDS transposed, lds[column][row]; a wavefront then ranks 16 of the columns,
// each a contiguous list.  The LDS rows are TOP_LDS_STRIDE = 65 words of 8 bytes long, not 64: on the transposing write
// lane l (a column) goes to word l * 65 + r, and with an odd stride the 16 lanes the LDS serves at a time fall into 16
// different pairs of its 4-byte banks; with 64 they would all hit the same pair.  The reads are either contiguous (lane l
// reads word l of the column) or broadcasts.
//
// Determinism: comparisons of integers only.  (key, member) is unique within a segment, so a member's output slot IS its
// rank: no atomic decides a slot, no atomic exists here at all, and two builds give the same bytes.  The scores that come
// back are the table's own bytes, read again by the merge kernel (the key has lost the sign of a zero).  The tile length
// is a test knob (east_hip_debug_set_top_tile); the result does not depend on it.
//
// The host half is a consumer of the handle (consumer.h); it alone also ranks the matrices of other consumers, three more table
// sources: the similarity's (EAST_HIP_GRAPH_SOURCE_SIMILARITY), the relatedness' (EAST_HIP_GRAPH_SOURCE_RELATED) and the
// text-to-text cosine's (EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS).
#pragma once
#include "consumer.h"

#define TOP_TILE 64u                       // members of a tile at most: one a lane
#define TOP_LDS_STRIDE 65u                 // 8-byte words from one column's keys to the next (see above)
#define TOP_COLS_PER_WAVE (64u / WAVES_PER_BLOCK)
#define TOP_MAX_N 1024

// ordered_key of an eligible score; 0 = not eligible (the only double that would map to 0 is a NaN with every bit set, and
// a NaN is never eligible)
__device__ __forceinline__ u64 top_key(double v, double threshold) { return v >= threshold ? ordered_key(v) : 0ull; }

// list: the 64 keys of a tile in LDS (0 behind its end); the keys in front of (my, lane) -- the same address for every lane
__device__ __forceinline__ u32 top_rank_in_tile(const u64 *list, u64 my, u32 lane)
{
    u32 r = 0;
#pragma unroll 8
    for (u32 j = 0; j < TOP_TILE; j++) {
        const u64 k = list[j];
        r += (k > my || (k == my && j < lane)) ? 1u : 0u;
    }
    return r;
}

// One wavefront, one (segment, tile): lane l holds member `member` with key `my` and rank `rank` among the tile's keys.
// The eligible members rank 0 .. e - 1 without a gap (a key of 0 is in front of nothing), so the places below cnt =
// min(e, cap) are written once each and the lanes cnt .. cap - 1 zero the rest.
__device__ __forceinline__ void top_emit(u64 my, u32 rank, u32 member, u32 cap, size_t slot, u64 *__restrict__ ckey,
                                         u32 *__restrict__ cidx, u32 *__restrict__ ccnt, u32 lane)
{
    const u32 e = (u32)__popcll(__ballot(my != 0ull));
    const u32 cnt = e < cap ? e : cap;
    u64 *k = ckey + slot * cap;
    u32 *x = cidx + slot * cap;
    if (my != 0ull && rank < cap) { k[rank] = my; x[rank] = member; }
    if (lane >= cnt && lane < cap) k[lane] = 0ull;
    if (lane == 0u) ccnt[slot] = cnt;
}

// ---- by text -----------------------------------------------------------------------------------------------------------
// Workgroup (strip, tile): columns [64 strip, 64 strip + 64) x rows [T tile, T tile + T) of the table.  Slot of column d
// and tile t: d * NT + t.
__global__ __launch_bounds__(BLOCK) void top_select_text_kernel(const double *__restrict__ table, u32 K, u32 D, u32 T, u32 NT, u32 cap,
                                                                double threshold, u64 *__restrict__ ckey, u32 *__restrict__ cidx,
                                                                u32 *__restrict__ ccnt)
{
    __shared__ u64 lds[64u * TOP_LDS_STRIDE];
    const u32 tile = blockIdx.x % NT, strip = blockIdx.x / NT;
    const u32 row0 = tile * T, col0 = strip * 64u;
    const u32 tlen = min(T, K - row0);
    const u32 lane = lane_id(), wv = wave_id();
    const u32 col = col0 + lane;
    double v[TOP_TILE / WAVES_PER_BLOCK];
#pragma unroll
    for (u32 i = 0; i < TOP_TILE / WAVES_PER_BLOCK; i++) {        // (all loads requested before the first is used)
        const u32 r = i * WAVES_PER_BLOCK + wv;
        v[i] = r < tlen && col < D ? table[(size_t)(row0 + r) * D + col] : __builtin_nan("");
    }
#pragma unroll
    for (u32 i = 0; i < TOP_TILE / WAVES_PER_BLOCK; i++) lds[lane * TOP_LDS_STRIDE + i * WAVES_PER_BLOCK + wv] = top_key(v[i], threshold);
    __syncthreads();
    for (u32 c = wv * TOP_COLS_PER_WAVE; c < (wv + 1u) * TOP_COLS_PER_WAVE; c++) {
        if (col0 + c >= D) break;                                 // (the same for the whole wavefront)
        const u64 *list = lds + c * TOP_LDS_STRIDE;
        const u64 my = list[lane];
        const u32 rank = top_rank_in_tile(list, my, lane);
        top_emit(my, rank, row0 + lane, cap, (size_t)(col0 + c) * NT + tile, ckey, cidx, ccnt, lane);
    }
}

// ---- by keyphrase ------------------------------------------------------------------------------------------------------
// A wavefront per (row, tile): members [T tile, T tile + T) of row k, one coalesced load.  Slot: k * NT + t.
__global__ __launch_bounds__(BLOCK) void top_select_keyphrase_kernel(const double *__restrict__ table, u32 K, u32 D, u32 T, u32 NT,
                                                                     u32 cap, double threshold, u64 *__restrict__ ckey,
                                                                     u32 *__restrict__ cidx, u32 *__restrict__ ccnt)
{
    __shared__ u64 lds[WAVES_PER_BLOCK][TOP_TILE];
    const u32 lane = lane_id(), wv = wave_id();
    const u64 slot = (u64)blockIdx.x * WAVES_PER_BLOCK + wv;
    const bool live = slot < (u64)K * NT;
    const u32 k = live ? (u32)(slot / NT) : 0u, tile = live ? (u32)(slot % NT) : 0u;
    const u32 member = tile * T + lane;
    const double v = live && lane < T && member < D ? table[(size_t)k * D + member] : __builtin_nan("");
    const u64 my = top_key(v, threshold);
    lds[wv][lane] = my;
    __syncthreads();
    if (!live) return;
    const u32 rank = top_rank_in_tile(lds[wv], my, lane);
    top_emit(my, rank, member, cap, (size_t)slot, ckey, cidx, ccnt, lane);
}

// ---- merge -------------------------------------------------------------------------------------------------------------
// Workgroup s: the NT lists of segment s (cap places each, sorted, zeros behind their ends) -> count[s], index[s * n ..],
// score[s * n ..].  A candidate's final rank is its place in its own list + per other list the entries in front of it:
// those with key >= its own in the lists of earlier tiles (smaller members), key > its own in later ones; a candidate whose
// rank reaches n is dropped where it stands.  score = the table's own value of the member: seg_stride / mem_stride = the
// distance of two segments / two members in the table.
__global__ __launch_bounds__(BLOCK) void top_merge_kernel(const u64 *__restrict__ ckey, const u32 *__restrict__ cidx,
                                                          const u32 *__restrict__ ccnt, u32 NT, u32 cap, u32 n,
                                                          const double *__restrict__ table, size_t seg_stride, size_t mem_stride,
                                                          int32_t *__restrict__ count, int32_t *__restrict__ index,
                                                          double *__restrict__ score)
{
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    const size_t s = blockIdx.x;
    const u64 *kbase = ckey + s * NT * cap;
    const u32 *ibase = cidx + s * NT * cap;
    u32 mine = 0;
    for (u32 t = threadIdx.x; t < NT && mine < n; t += BLOCK) mine += ccnt[s * NT + t];      // (at most cap <= n each: no overflow)
    mine = wave_sum(mine < n ? mine : n);
    if (lane_id() == 0u) lds4[wave_id()] = mine;
    __syncthreads();
    const u32 total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    const u32 cnt = total < n ? total : n;
    if (threadIdx.x == 0u) count[s] = (int32_t)cnt;
    for (u32 r = cnt + threadIdx.x; r < n; r += BLOCK) { index[s * n + r] = -1; score[s * n + r] = 0.0; }
    const u64 places = (u64)NT * cap;
    for (u64 i = threadIdx.x; i < places; i += BLOCK) {
        const u64 kc = kbase[i];
        if (kc == 0ull) continue;
        const u32 tc = (u32)(i / cap);
        u32 rank = (u32)(i % cap);
        for (u32 t = 0; t < NT && rank < n; t++) {
            if (t == tc) continue;
            const u64 *list = kbase + (size_t)t * cap;
            const u64 bound = t < tc ? kc : kc + 1ull;            // in front of the candidate: key >= bound (kc < 2^64 - 1: it is no NaN)
            if (list[0] < bound) continue;
            u32 lo = 1u, hi = cap;                                // the first place whose key is below the bound
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (list[mid] >= bound) lo = mid + 1u; else hi = mid;
            }
            rank += lo;
        }
        if (rank < n) {
            const u32 m = ibase[i];
            index[s * n + rank] = (int32_t)m;
            score[s * n + rank] = table[s * seg_stride + (size_t)m * mem_stride];
        }
    }
}

// ============================================================================================================ host ==
// The ranking's device buffers belong to the handle and to nothing else: not the EASA arena, the cosine buffers or the graph's.
struct TopState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_TOP;
    u32 S = 0, n = 0;                       // segments, places per segment
    i64 total = 0;                          // the sum of the counts
    UploadedTable table;                    // a host table's copy (east_hip_top_build_host)
    DevBuf cand, result;
    int32_t *count = nullptr, *index = nullptr;
    double *score = nullptr;
    TopState() { bufs = {&table.buf, &cand, &result}; }
    void clear() override
    {
        S = n = 0;
        total = 0;
        table.withdraw();
    }
};

static void top_check(int32_t axis, int32_t n_best, double threshold)
{
    if (axis != EAST_HIP_TOP_BY_TEXT && axis != EAST_HIP_TOP_BY_KEYPHRASE) east_throw(EAST_HIP_ERR_INVALID, "ranked keyphrases: unknown axis");
    if (n_best < 1 || n_best > TOP_MAX_N) east_throw(EAST_HIP_ERR_INVALID, "ranked keyphrases: n must be 1 .. 1024");
    if (threshold != threshold) east_throw(EAST_HIP_ERR_INVALID, "ranked keyphrases: the threshold is not a number");
}

static void top_build(east_hip_index *h, TableRef t, int32_t axis, int32_t n_best, double threshold, i64 *out)
{
    top_check(axis, n_best, threshold);
    const double *d_table = t.p;
    const u32 K = t.K, D = t.D;
    if (K < 1 || D < 1 || K >= 0x7FFFFFF0u || D >= 0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "ranked keyphrases: empty score table");
    TopState &g = consumer_begin<TopState>(h);
    g.total = 0;
    const bool by_text = axis == EAST_HIP_TOP_BY_TEXT;
    const u32 S = by_text ? D : K, L = by_text ? K : D, n = (u32)n_best;
    Stats stats;
    Ctx ctx = handle_ctx(h, nullptr, &stats);
    const u32 T = (u32)std::min<int>(std::max(ctx.knobs.top_tile, 1), (int)TOP_TILE);
    const u32 NT = ceil_div_u32(L, T), cap = std::min(n, T);
    const u64 slots = (u64)S * NT;
    const u64 grid = by_text ? (u64)ceil_div_u32(D, 64) * NT : (slots + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (grid >= (u64)0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "ranked keyphrases: more tiles than one launch takes");
    const size_t cand_bytes = (size_t)slots * cap * 12 + (size_t)slots * 4 + 4 * 256;
    const size_t res_bytes = (size_t)S * 4 + (size_t)S * n * 12 + 4 * 256;
    if (!g.cand.try_ensure(cand_bytes, h->stream) || !g.result.try_ensure(res_bytes, h->stream)) {
        char msg[240];
        snprintf(msg, sizeof(msg), "ranked keyphrases: %u segments x %u places need %zu bytes of candidates and %zu bytes of result, "
                 "which the device does not have", S, n, cand_bytes, res_bytes);
        east_throw(EAST_HIP_ERR_OOM, msg);
    }
    Arena a = g.cand.arena(), r = g.result.arena();
    u64 *ckey = a.alloc<u64>((size_t)slots * cap);
    u32 *cidx = a.alloc<u32>((size_t)slots * cap), *ccnt = a.alloc<u32>((size_t)slots);
    g.score = r.alloc<double>((size_t)S * n);
    g.index = r.alloc<int32_t>((size_t)S * n);
    g.count = r.alloc<int32_t>(S);
    g.S = S;
    g.n = n;
    std::vector<int32_t> counts(S);
    ConsumerTimer timer(h, g);
    if (by_text)
        LAUNCH(ctx, top_select_text_kernel, (u32)grid, d_table, K, D, T, NT, cap, threshold, ckey, cidx, ccnt);
    else
        LAUNCH(ctx, top_select_keyphrase_kernel, (u32)grid, d_table, K, D, T, NT, cap, threshold, ckey, cidx, ccnt);
    LAUNCH(ctx, top_merge_kernel, S, (const u64 *)ckey, (const u32 *)cidx, (const u32 *)ccnt, NT, cap, n, d_table,
           by_text ? (size_t)1 : (size_t)D, by_text ? (size_t)D : (size_t)1, g.count, g.index, g.score);
    HIP_CHECK(hipMemcpyAsync(counts.data(), g.count, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
    timer.finish();
    for (int32_t c : counts) g.total += c;
    g.valid = true;
    if (out) { out[0] = (i64)S; out[1] = g.total; }
}

extern "C" {

int east_hip_top_build_resident(east_hip_handle_t h, int32_t source, int32_t axis, int32_t n, double threshold, int64_t *out)
{
    return guarded([&] { top_build(h, consumer_resident<TopState>(h, source, "ranked keyphrases", true), axis, n, threshold, out); });
}

int east_hip_top_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs, int32_t axis, int32_t n,
                            double threshold, int64_t *out)
{
    return guarded([&] {
        const TableRef t = consumer_upload<TopState>(h, table, n_keyphrases, n_docs, "ranked keyphrases: null or empty score table",
                                                     "the ranking's score table", [&] { top_check(axis, n, threshold); });
        top_build(h, t, axis, n, threshold, out);
    });
}

int east_hip_top_fetch(east_hip_handle_t h, int32_t *count, int32_t *index, double *score)
{
    return guarded([&] {
        const TopState &g = consumer_built<TopState>(h, "no keyphrase ranking has been built on this handle");
        const size_t places = (size_t)g.S * g.n;
        if (count) HIP_CHECK(hipMemcpyAsync(count, g.count, (size_t)g.S * 4, hipMemcpyDeviceToHost, h->stream));
        if (index) HIP_CHECK(hipMemcpyAsync(index, g.index, places * 4, hipMemcpyDeviceToHost, h->stream));
        if (score) HIP_CHECK(hipMemcpyAsync(score, g.score, places * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

double east_hip_last_top_ms(east_hip_handle_t h) { return consumer_ms<TopState>(h); }

int east_hip_debug_set_top_tile(int members)
{
    // members of a segment a wavefront ranks at a time: 1 .. TOP_TILE (64, more is taken as 64); 0 or less: the default (64)
    knobs_update([&](Knobs &k) { k.top_tile = members > 0 ? std::min(members, (int)TOP_TILE) : (int)TOP_TILE; });
    return EAST_HIP_OK;
}

}  // extern "C"
