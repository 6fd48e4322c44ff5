// cosine_texts.h -- text-to-text cosine similarity on the device: the cosine of the tf or tf-idf vectors of every two texts
// of the cosine term index (include/east_hip.h, "Text-to-text cosine similarity"; `east texts similar`).
//
// The index holds the postings (unit, document, count) in (unit, document) order, their place in document order and, per
// weighting, the weight x of every posting and the norm of every document (cosine.h).  C = X X^T scaled by the norms, X the
// D x units matrix of the weights: sparse, and never made dense beyond 2 x 64 x 32 entries a workgroup.
//
//   postings --cost_scatter_kernel: one scatter through inv_perm--> per document its units ascending (du) and its weights
//     in the same places (dw)
//   per batch of consecutive segments of the unit range:
//   --cost_tile_kernel: a workgroup per (64 x 64 tile of document pairs, tile_a <= tile_b; segment)--> partial[segment][tile]
//   --cost_fold_kernel: a thread per entry of a tile adds the batch's partial tiles in segment order onto the running G,
//     which lies in the matrix's own upper tiles
//   --cost_finish_kernel: a workgroup per tile: / (norm_a * norm_b), self from the diagonal, NaN on it, the tile and its
//     mirror image as coalesced rows out of LDS
//
// The tile kernel.  Segment s is the units [s SEG, (s + 1) SEG), whatever the collection.  A member is a document of
// strip a (threads 0 .. 63) or of strip b (64 .. 127); its thread finds the member's first posting of the segment by binary
// search and from then on holds the member's cursor and the unit under it.  The segment is walked in chunks of CHUNK = 32
// units aligned to multiples of 32 from unit 0: the next chunk is the one that holds the smallest unit under any cursor (a
// wave-level minimum, then one across the four waves), so a chunk in which no member has a posting is never staged.  The
// chunk is staged dense in LDS -- zero fill, then every member's thread scatters the postings it has in it (units inside a
// document are distinct: no two writes meet) -- in the layout of sim_gram_kernel's by-keyphrase loader, lds[member][entry]
// with the odd stride 33, and multiplied as there: the four wavefronts take the 32 x 32 quadrants as 2 x 2 blocks of
// v_mfma_f64_16x16x4_f64 (similarity.h has the fragment map).  Members behind D and units without a posting are zeros,
// never a branch around the MFMA.
//
// Order of the sums.  Inside a segment an entry of the tile is one accumulator that takes the chunks in ascending order and,
// inside a chunk, the units in ascending order; skipping a chunk leaves out additions of +0.0 to an accumulator that is
// >= +0.0 (the weights are non-negative), which do not change its bytes.  The segments' sums are added in segment order,
// ((P_0 + P_1) + P_2) + ..., and the fold goes on after every batch where the batch before stopped: the sum is the same
// wherever the batches are cut (east_hip_debug_set_text_similarity_batch).  No atomic; nothing depends on timing.
//
// Memory: du, dw (12 bytes a posting), the matrix, and partial tiles of at most COSTEXT_SCRATCH_BYTES -- or of one segment
// where a single segment's tiles take more: half the matrix's own size.
//
// The host half is a MatrixConsumer of the handle (consumer.h: the matrix, its limit, its fetch, what it offers()).
#pragma once
#include "consumer.h"
#include "cosine.h"
#include "similarity.h"

#define COSTEXT_SEG 8192u                          // units of a segment
#define COSTEXT_CHUNK SIM_CHUNK                    // units staged at a time
#define COSTEXT_TILE_WORDS (SIM_TILE * SIM_TILE)   // doubles of a partial tile
#define COSTEXT_MAX_BATCH 65535u                   // segments of a launch at most: the grid's third dimension
#define COSTEXT_SCRATCH_BYTES ((size_t)256 << 20)  // the default batch: as many segments as keep the partial tiles at or below this
#define COSTEXT_MAX_GRID (1u << 22)                // workgroups of the fold at most (it loops)
static_assert(COSTEXT_SEG % COSTEXT_CHUNK == 0, "a chunk must not span two segments");

// ---- document-order operands --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cost_scatter_kernel(const u32 *__restrict__ post_unit, const double *__restrict__ w,
                                                             const u32 *__restrict__ inv_perm, u32 P, u32 *__restrict__ du,
                                                             double *__restrict__ dw)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const u32 i = inv_perm[p];
    if (i >= P) return;                                           // (never: a permutation)
    du[i] = post_unit[p];
    dw[i] = w[p];
}

// the tile pairs (ta <= tb) in row order: pair = the pairs of the rows in front of ta, plus tb - ta
__device__ __host__ __forceinline__ u64 cost_pair_index(u32 ta, u32 tb, u32 NT) { return (u64)ta * (2ull * NT - ta + 1ull) / 2ull + (tb - ta); }

// ---- a tile's sum over a segment ------------------------------------------------------------------------------------------
// Workgroup (blockIdx.y = tile_a, blockIdx.x = tile_b, blockIdx.z = segment seg0 + z of the batch) -> partial[z][pair], all
// 64 x 64 entries (zeros behind D).
__global__ __launch_bounds__(BLOCK) void cost_tile_kernel(const u32 *__restrict__ du, const double *__restrict__ dw,
                                                          const u32 *__restrict__ doc_off, u32 D, u32 n_units, u32 seg0,
                                                          double *__restrict__ partial)
{
    __shared__ double lds[2u * SIM_TILE * SIM_LDS_STRIDE];
    __shared__ u32 wmin[WAVES_PER_BLOCK];
    const u32 ta = blockIdx.y, tb = blockIdx.x, NT = gridDim.x;
    if (ta > tb) return;
    const bool diag = ta == tb;
    const u32 lane = lane_id(), wv = wave_id();
    const u32 lr = lane & 15u, lk = lane >> 4;
    const u32 ra = (wv >> 1) * 32u, cb = (wv & 1u) * 32u;         // this wavefront's quadrant inside the tile
    const u32 a0 = ta * SIM_TILE, b0 = tb * SIM_TILE;
    const u32 lo_u = (seg0 + blockIdx.z) * COSTEXT_SEG;           // (the host launches segments that start below n_units only)
    const u32 hi_u = min(n_units, lo_u + COSTEXT_SEG);
    sim_v4d acc[2][2];
    sim_acc_zero(acc);

    // this thread's member: its cursor, the end of its postings and the unit under the cursor (COS_NONE: none left in the segment)
    u32 cur = 0, end = 0, nu = COS_NONE;
    if (threadIdx.x < (diag ? SIM_TILE : 2u * SIM_TILE)) {
        const u32 doc = threadIdx.x < SIM_TILE ? a0 + threadIdx.x : b0 + (threadIdx.x - SIM_TILE);
        if (doc < D) {
            u32 lo = doc_off[doc];
            end = doc_off[doc + 1u];
            u32 hi = end;
            while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (du[mid] < lo_u) lo = mid + 1u; else hi = mid; }
            cur = lo;
            if (cur < end) nu = du[cur];
            if (nu >= hi_u) nu = COS_NONE;
        }
    }
    double *row = lds + threadIdx.x * SIM_LDS_STRIDE;             // (members only: strip a's rows, then strip b's)
    const double *la = lds, *lb = diag ? lds : lds + SIM_TILE * SIM_LDS_STRIDE;
    for (;;) {
        u32 m = wave_min(nu);
        if (lane == 0u) wmin[wv] = m;
        __syncthreads();                                          // (and: the chunk before has been read)
        m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        if (m == COS_NONE) break;                                 // (the same for every thread of the workgroup)
        const u32 chunk = m & ~(COSTEXT_CHUNK - 1u);
        for (u32 i = threadIdx.x; i < 2u * SIM_TILE * SIM_LDS_STRIDE; i += BLOCK) lds[i] = 0.0;
        __syncthreads();
        while (nu - chunk < COSTEXT_CHUNK) {                      // (nu >= chunk; COS_NONE - chunk is far above)
            row[nu - chunk] = dw[cur];
            cur++;
            nu = cur < end ? du[cur] : COS_NONE;
            if (nu >= hi_u) nu = COS_NONE;
        }
        __syncthreads();
#pragma unroll
        for (u32 s = 0; s < SIM_CHUNK / 4u; s++) {
            const u32 e = 4u * s + lk;
            const double a[2] = {la[(ra + lr) * SIM_LDS_STRIDE + e], la[(ra + 16u + lr) * SIM_LDS_STRIDE + e]};
            const double b[2] = {lb[(cb + lr) * SIM_LDS_STRIDE + e], lb[(cb + 16u + lr) * SIM_LDS_STRIDE + e]};
            sim_mfma_step(acc, a, b);
        }
    }
    // acc[i][j][r] is row ra + 16 i + (lane >> 4) + 4 r, column cb + 16 j + (lane & 15)
    double *out = partial + ((size_t)blockIdx.z * (size_t)cost_pair_index(NT, NT, NT) + (size_t)cost_pair_index(ta, tb, NT)) * COSTEXT_TILE_WORDS;
#pragma unroll
    for (u32 i = 0; i < 2; i++)
#pragma unroll
        for (u32 r = 0; r < 4; r++)
#pragma unroll
            for (u32 j = 0; j < 2; j++) out[(ra + 16u * i + lk + 4u * r) * SIM_TILE + cb + 16u * j + lr] = acc[i][j][r];
}

// Thread (pair, entry): the batch's n_seg partial tiles in segment order onto G, which lies where the matrix will (first:
// the batch starts the sum).  pair_tiles[pair] = ta << 16 | tb.
__global__ __launch_bounds__(BLOCK) void cost_fold_kernel(const double *__restrict__ partial, const u32 *__restrict__ pair_tiles, u64 n_pairs,
                                                          u32 n_seg, int first, u32 D, double *__restrict__ M)
{
    for (u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x; gid < n_pairs * COSTEXT_TILE_WORDS; gid += (u64)gridDim.x * BLOCK) {
        const u64 pair = gid / COSTEXT_TILE_WORDS;
        const u32 e = (u32)(gid % COSTEXT_TILE_WORDS), t = pair_tiles[pair];
        const u32 a = (t >> 16) * SIM_TILE + e / SIM_TILE, b = (t & 0xFFFFu) * SIM_TILE + e % SIM_TILE;
        if (a >= D || b >= D) continue;
        double acc = first ? 0.0 : M[(size_t)a * D + b];
        for (u32 s = 0; s < n_seg; s++) acc += partial[((size_t)s * n_pairs + pair) * COSTEXT_TILE_WORDS + e];
        M[(size_t)a * D + b] = acc;
    }
}

// Workgroup = pair, in place: the tile of G becomes the tile of C and its mirror image (similarity.h's epilogue).
__global__ __launch_bounds__(BLOCK) void cost_finish_kernel(double *__restrict__ M, const u32 *__restrict__ pair_tiles, u32 D,
                                                            const double *__restrict__ norm, double *__restrict__ self)
{
    __shared__ double tile[SIM_TILE * SIM_EPI_STRIDE];
    const u32 t = pair_tiles[blockIdx.x];
    const u32 a0 = (t >> 16) * SIM_TILE, b0 = (t & 0xFFFFu) * SIM_TILE;
    const u32 lane = lane_id(), wv = wave_id();
    for (u32 r = wv; r < SIM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = a0 + r, b = b0 + lane;
        double v = 0.0;
        if (a < D && b < D) {
            v = M[(size_t)a * D + b] / (norm[a] * norm[b]);
            if (a == b) { self[a] = v; v = __builtin_nan(""); }
        }
        tile[r * SIM_EPI_STRIDE + lane] = v;
    }
    __syncthreads();
    sim_tile_store(M, D, a0, b0, a0 == b0, tile, lane, wv);
}

// ============================================================================================================ host ==
// The buffers belong to the handle and to nothing else: not the cosine index's, the EASA arena or another consumer's.
struct CosTextsState : MatrixConsumer {      // per_member: self; count: postings
    static constexpr int SLOT = east_hip_index::SLOT_COSTEXT;
    DevBuf ops, scratch;                    // du, dw, the tile pairs and the squares' scratch; the partial tiles
    CosTextsState() { bufs.insert(bufs.end(), {&ops, &scratch}); }
};

__global__ __launch_bounds__(BLOCK) void cost_postings_kernel(const u32 *__restrict__ doc_off, u32 D, int32_t *__restrict__ postings)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d < D) postings[d] = (int32_t)(doc_off[d + 1u] - doc_off[d]);
}

static void cost_build(east_hip_index *h, int32_t weighting, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (weighting < 0 || weighting > 1) east_throw(EAST_HIP_ERR_INVALID, "text similarity: unknown weighting");
    CosState &c = cos_built(h);
    use_device(h);
    CosTextsState &g = consumer_begin<CosTextsState>(h);
    CosUnits &U = c.use_classes ? c.cls : c.terms;
    const u32 D = c.n_docs, P = U.P, n_units = U.n_units;
    const std::string texts = std::to_string(D) + " texts";
    auto cost_oom = [&](const char *what, double bytes) { consumer_oom("text similarity", what, texts, bytes); };
    if (D < 1) east_throw(EAST_HIP_ERR_INVALID, "text similarity: the index holds no text");
    matrix_reserve(h, g, D, true, "text similarity", texts);
    const u32 NT = ceil_div_u32(D, SIM_TILE);
    const u64 n_pairs = cost_pair_index(NT, NT, NT);
    const u32 n_seg = ceil_div_u32(n_units, COSTEXT_SEG);
    const Knobs kn = knobs_snapshot();
    const size_t tile_bytes = (size_t)n_pairs * COSTEXT_TILE_WORDS * 8;
    u32 batch = kn.cosine_texts_batch > 0 ? (u32)std::min<i64>(kn.cosine_texts_batch, COSTEXT_MAX_BATCH)
                                          : (u32)std::min<size_t>(std::max<size_t>(COSTEXT_SCRATCH_BYTES / tile_bytes, 1), COSTEXT_MAX_BATCH);
    batch = std::max(std::min(batch, n_seg), 1u);
    const size_t ops_bytes = align256(((size_t)P + 1) * 4) + 2 * align256(((size_t)P + 1) * 8) + align256((size_t)n_pairs * 4) + 256;
    if (!g.ops.try_ensure(ops_bytes, h->stream)) cost_oom("the postings in document order", (double)ops_bytes);
    if (!g.scratch.try_ensure((size_t)batch * tile_bytes + 256, h->stream)) cost_oom("a batch's partial tiles", (double)batch * (double)tile_bytes);
    Arena pa = g.ops.arena();
    u32 *du = pa.alloc<u32>((size_t)P + 1), *d_pairs = pa.alloc<u32>((size_t)n_pairs);
    double *dw = pa.alloc<double>((size_t)P + 1);
    std::vector<u32> pairs;
    pairs.reserve((size_t)n_pairs);
    for (u32 ta = 0; ta < NT; ta++)
        for (u32 tb = ta; tb < NT; tb++) pairs.push_back(ta << 16 | tb);
    double *w = nullptr, *norm = nullptr;
    cos_weight_ptrs(U, D, weighting, &w, &norm);
    Stats stats;
    Ctx ctx = handle_ctx(h, &pa, &stats);       // (the squares' scratch comes out of this consumer's buffer, behind du and dw)
    HIP_CHECK(hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, h->stream));
    ConsumerTimer timer(h, g);
    cos_make_weights(ctx, c, U, weighting, w, norm);
    if (P)
        LAUNCH(ctx, cost_scatter_kernel, ceil_div_u32(P, BLOCK), (const u32 *)U.post_unit, (const double *)w, (const u32 *)U.inv_perm, P, du, dw);
    LAUNCH(ctx, cost_postings_kernel, ceil_div_u32(D, BLOCK), (const u32 *)U.doc_off, D, g.count);
    double *partial = g.scratch.as<double>();
    const u32 fold_grid = (u32)std::min<u64>((n_pairs * COSTEXT_TILE_WORDS + BLOCK - 1) / BLOCK, COSTEXT_MAX_GRID);
    i64 launches = 0;
    for (u32 s0 = 0; s0 < n_seg || s0 == 0; s0 += batch) {       // (no unit at all: one fold of nothing, the zeros)
        const u32 nb = std::min(batch, n_seg - s0);
        if (nb) {
            LAUNCH(ctx, cost_tile_kernel, dim3(NT, NT, nb), (const u32 *)du, (const double *)dw, (const u32 *)U.doc_off, D, n_units, s0, partial);
            launches++;
        }
        LAUNCH(ctx, cost_fold_kernel, fold_grid, (const double *)partial, (const u32 *)d_pairs, n_pairs, nb, (int)(s0 == 0), D, g.matrix);
        launches++;
    }
    LAUNCH(ctx, cost_finish_kernel, (u32)n_pairs, g.matrix, (const u32 *)d_pairs, D, (const double *)norm, g.per_member);
    launches++;
    timer.finish();
    U.w_valid[weighting] = true;
    g.valid = true;
    if (out) {
        out[0] = (i64)D; out[1] = (i64)n_units; out[2] = (i64)P; out[3] = (i64)n_pairs;
        out[4] = (i64)n_seg; out[5] = launches; out[6] = (i64)COSTEXT_CHUNK; out[7] = (i64)COSTEXT_SEG;
    }
}

extern "C" {

int east_hip_text_similarity_build(east_hip_handle_t h, int32_t weighting, int64_t *out)
{
    return guarded([&] { cost_build(h, weighting, out); });
}

int east_hip_text_similarity_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *postings)
{
    return guarded([&] {
        matrix_fetch(h, consumer_built<CosTextsState>(h, "no text similarity matrix has been built on this handle"), matrix, self, postings);
    });
}

double east_hip_last_text_similarity_ms(east_hip_handle_t h) { return consumer_ms<CosTextsState>(h); }

int east_hip_debug_set_text_similarity_batch(int64_t segments)
{
    // segments of the unit range per launch of the tile kernel; 0 or less: the default (COSTEXT_SCRATCH_BYTES of partial tiles)
    knobs_update([&](Knobs &k) { k.cosine_texts_batch = segments > 0 ? segments : 0; });
    return EAST_HIP_OK;
}

}  // extern "C"
