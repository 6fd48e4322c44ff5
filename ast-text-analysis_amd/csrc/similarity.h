// similarity.h -- similar texts and similar keyphrases on the device: the cosine of every two columns of a score table that
// is already there, or of every two rows (include/east_hip.h, "Similar texts and keyphrases"; `east keyphrases similar`).
//
// A *member* is a column (EAST_HIP_TOP_BY_TEXT: M = D members, its profile p_d[l] = t[l * D + d], L = K entries) or a row
// (EAST_HIP_TOP_BY_KEYPHRASE: M = K, p_k[l] = t[k * D + l], L = D).  q_a = sum p_a[l]^2, G_ab = sum p_a[l] p_b[l],
// S[a][b] = G_ab / (sqrt(q_a) * sqrt(q_b)); S[a][a] = NaN; S[a][b] = +0.0 where a q is zero.
//
//   K x D doubles --sim_norm_*_kernel: one coalesced pass--> q[M]
//   --sim_gram_kernel: a workgroup per 64 x 64 tile (tile_a <= tile_b) of the Gram matrix, v_mfma_f64_16x16x4_f64; the
//     epilogue divides by the roots of q and writes the tile and its mirror image--> S[M x M]
//   --top.h ranks S like any table (EAST_HIP_GRAPH_SOURCE_SIMILARITY): a NaN is never eligible, so no member lists itself
//
// The MFMA.  D(16 x 16) += A(16 x 4) B(4 x 16) in doubles.  Lane l of the wavefront gives A[l & 15][l >> 4] and
// B[l >> 4][l & 15], one double each, and holds four results: D[(l >> 4) + 4 r][l & 15] in register r = 0 .. 3 (this is NOT
// the row map of the f32 forms, (l >> 4) * 4 + r).  Here A[i][k] = p_(a0 + i)[l0 + k] and B[k][j] = p_(b0 + j)[l0 + k]: both
// operands are "member (lane & 15), entry l0 + (lane >> 4)", so one loader serves both.  The four wavefronts of a workgroup
// take the 32 x 32 quadrants of the tile, each as 2 x 2 MFMA blocks = four accumulators of four doubles; a step over four
// entries of the profiles is four loads and four MFMAs.  Operands behind M or L are zeros, never a branch around the MFMA.
//
// Two loaders.  By text the operand t[(l0 + (lane >> 4)) * D + m0 + (lane & 15)] is sixteen consecutive doubles for each of
// four consecutive rows: it is loaded as it lies.  By keyphrase the same operand would be D * 8 bytes from lane to lane, so
// a chunk of SIM_CHUNK = 32 entries of the 64 + 64 profiles goes through LDS: 32 lanes read 256 consecutive bytes of a row
// (two rows a wavefront: a coalesced 512 bytes) and write them as they lie to lds[member][entry]; the fragment read is
// word (lane & 15) * SIM_LDS_STRIDE + entry.  With the odd stride 33 the sixteen members of an MFMA row go to sixteen
// different pairs of the 4-byte banks (33 i mod 32 = i); with 32 they would all meet in one.  (lane >> 4 moves a lane one
// pair on, so at worst two lanes of a half-wavefront share a pair.)  2 x 64 x 33 x 8 = 33 792 bytes a workgroup.
//
// The epilogue reuses that LDS as a 64 x 64 tile with rows of SIM_EPI_STRIDE = 65 words: every wavefront normalises its
// quadrant into it, then rows go out as coalesced 512-byte stores -- S[a0 + r][b0 ..] read along a row, the mirror image
// S[b0 + c][a0 ..] read down a column (word lane * 65 + c: the odd stride again, as in top.h).  One pass over the M x M
// bytes.  A diagonal tile computes both halves but stores only the values of its upper half, to both places: S[a][b] and
// S[b][a] are the same bytes because they are one value.  Lower-triangle workgroups of the 2-D grid return at once.
//
// Determinism: no atomic, no split of L across workgroups or wavefronts; the order of every sum is fixed by the code.
//
// The tile's geometry is this file's, and so are its pieces that cosine_texts.h runs too: sim_mfma_step, sim_acc_zero and
// sim_tile_store (the tile and its mirror image).  The eight steps over a staged chunk stand in both kernels: as a shared
// function they cost cost_tile_kernel 1.6 % on its largest measured case (profiles/matrix_frame_refactor.json).
//
// The host half is a MatrixConsumer of the handle (consumer.h): the frame has the matrix, its limit, its fetch and what it
// offers() the ranking (top.h) and the clusters as a table; here are the axis, the uploaded table and the launches.
#pragma once
#include "consumer.h"

#define SIM_TILE 64u
#define SIM_CHUNK 32u                      // entries of a profile staged at a time (by keyphrase)
#define SIM_LDS_STRIDE 33u                 // 8-byte words from one member's chunk to the next (see above)
#define SIM_EPI_STRIDE 65u                 // ... from one row of the finished tile to the next
#define SIM_NORM_COLS 16u                  // by text: columns a workgroup of the norm kernel sums (x 16 groups of rows)

typedef double sim_v4d __attribute__((ext_vector_type(4)));

// ---- q ----------------------------------------------------------------------------------------------------------------
// By keyphrase: a wavefront per row, 512 consecutive bytes a load; the 64 partial sums are folded by a butterfly (every
// lane ends with the same bits: a + b == b + a).
__global__ __launch_bounds__(BLOCK) void sim_norm_row_kernel(const double *__restrict__ table, u32 K, u32 D, double *__restrict__ q)
{
    const u32 lane = lane_id();
    const u64 k = (u64)blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (k >= K) return;
    const double *row = table + (size_t)k * D;
    double s = 0.0;
    for (u32 l = lane; l < D; l += WAVE) { const double v = row[l]; s += v * v; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, WAVE);
    if (lane == 0u) q[k] = s;
}

// By text: workgroup b sums columns [16 b, 16 b + 16); thread (g = threadIdx.x >> 4, c = threadIdx.x & 15) adds the rows
// g, g + 16, ... of column c (sixteen lanes read 128 consecutive bytes), the sixteen groups are added in the order of g.
__global__ __launch_bounds__(BLOCK) void sim_norm_col_kernel(const double *__restrict__ table, u32 K, u32 D, double *__restrict__ q)
{
    __shared__ double part[BLOCK];
    const u32 c = threadIdx.x & 15u, g = threadIdx.x >> 4;
    const u32 d = blockIdx.x * SIM_NORM_COLS + c;
    double s = 0.0;
    if (d < D)
        for (u32 k = g; k < K; k += BLOCK / SIM_NORM_COLS) { const double v = table[(size_t)k * D + d]; s += v * v; }
    part[threadIdx.x] = s;
    __syncthreads();
    if (g == 0u && d < D) {
        double sum = part[c];
        for (u32 i = 1; i < BLOCK / SIM_NORM_COLS; i++) sum += part[i * SIM_NORM_COLS + c];
        q[d] = sum;
    }
}

// ---- the Gram tile ----------------------------------------------------------------------------------------------------
// acc[i][j] += A_i B_j for the 2 x 2 MFMA blocks of a quadrant: a[i] / b[j] = this lane's operand of row block i / column block j
__device__ __forceinline__ void sim_mfma_step(sim_v4d (&acc)[2][2], const double (&a)[2], const double (&b)[2])
{
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
}

__device__ __forceinline__ void sim_acc_zero(sim_v4d (&acc)[2][2])
{
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = (sim_v4d){0.0, 0.0, 0.0, 0.0};
}

// The finished tile (rows of SIM_EPI_STRIDE words in LDS) to S[a0 ..][b0 ..], row by row, and its mirror image to
// S[b0 ..][a0 ..], column by column; a diagonal tile stores the values of its upper half to both places.
__device__ __forceinline__ void sim_tile_store(double *__restrict__ S, u32 M, u32 a0, u32 b0, bool diag, const double *tile, u32 lane, u32 wv)
{
    for (u32 r = wv; r < SIM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = a0 + r, b = b0 + lane;
        if (a < M && b < M) S[(size_t)a * M + b] = diag && lane < r ? tile[lane * SIM_EPI_STRIDE + r] : tile[r * SIM_EPI_STRIDE + lane];
    }
    if (diag) return;
    for (u32 c = wv; c < SIM_TILE; c += WAVES_PER_BLOCK) {
        const u32 b = b0 + c, a = a0 + lane;
        if (a < M && b < M) S[(size_t)b * M + a] = tile[lane * SIM_EPI_STRIDE + c];
    }
}

// Workgroup (blockIdx.y = tile_a, blockIdx.x = tile_b), tile_a <= tile_b: S[64 tile_a ..][64 tile_b ..] and its mirror image.
template <bool BY_TEXT>
__global__ __launch_bounds__(BLOCK) void sim_gram_kernel(const double *__restrict__ t, u32 K, u32 D, const double *__restrict__ q,
                                                         double *__restrict__ S)
{
    __shared__ double lds[2u * SIM_TILE * SIM_LDS_STRIDE];       // (>= SIM_TILE * SIM_EPI_STRIDE: the epilogue's tile fits)
    static_assert(2u * SIM_TILE * SIM_LDS_STRIDE >= SIM_TILE * SIM_EPI_STRIDE, "the finished tile must fit the staging buffers");
    const u32 ta = blockIdx.y, tb = blockIdx.x;
    if (ta > tb) return;
    const bool diag = ta == tb;
    const u32 M = BY_TEXT ? D : K, L = BY_TEXT ? K : D;
    const u32 lane = lane_id(), wv = wave_id();
    const u32 lr = lane & 15u, lk = lane >> 4;
    const u32 ra = (wv >> 1) * 32u, cb = (wv & 1u) * 32u;         // this wavefront's quadrant inside the tile
    const u32 a0 = ta * SIM_TILE, b0 = tb * SIM_TILE;
    sim_v4d acc[2][2];
    sim_acc_zero(acc);

    if (BY_TEXT) {
        const u32 ma[2] = {a0 + ra + lr, a0 + ra + 16u + lr}, mb[2] = {b0 + cb + lr, b0 + cb + 16u + lr};
        for (u32 l0 = 0; l0 < L; l0 += 16u) {                     // four steps a turn: sixteen loads in flight
            double a[4][2], b[4][2];
#pragma unroll
            for (u32 s = 0; s < 4; s++) {
                const u32 l = l0 + 4u * s + lk;
#pragma unroll
                for (u32 i = 0; i < 2; i++) {
                    a[s][i] = l < L && ma[i] < M ? t[(size_t)l * D + ma[i]] : 0.0;
                    b[s][i] = l < L && mb[i] < M ? t[(size_t)l * D + mb[i]] : 0.0;
                }
            }
#pragma unroll
            for (u32 s = 0; s < 4; s++) sim_mfma_step(acc, a[s], b[s]);
        }
    } else {
        double *la = lds, *lb = diag ? lds : lds + SIM_TILE * SIM_LDS_STRIDE;
        const u32 srow = threadIdx.x >> 5, sl = threadIdx.x & 31u;      // staging: 8 members x 32 entries a pass
        for (u32 l0 = 0; l0 < L; l0 += SIM_CHUNK) {
            double va[8], vb[8];
            const u32 l = l0 + sl;
#pragma unroll
            for (u32 i = 0; i < 8; i++) {                         // (all loads requested before the first is used)
                const u32 m = a0 + i * 8u + srow;
                va[i] = l < L && m < M ? t[(size_t)m * D + l] : 0.0;
            }
            if (!diag) {
#pragma unroll
                for (u32 i = 0; i < 8; i++) {
                    const u32 m = b0 + i * 8u + srow;
                    vb[i] = l < L && m < M ? t[(size_t)m * D + l] : 0.0;
                }
            }
            __syncthreads();                                      // (the chunk before has been read)
#pragma unroll
            for (u32 i = 0; i < 8; i++) la[(i * 8u + srow) * SIM_LDS_STRIDE + sl] = va[i];
            if (!diag) {
#pragma unroll
                for (u32 i = 0; i < 8; i++) lb[(i * 8u + srow) * SIM_LDS_STRIDE + sl] = vb[i];
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
        __syncthreads();                                          // (the last chunk has been read: the tile takes its place)
    }

    // the quadrant, normalised, into the tile: acc[i][j][r] is row ra + 16 i + (lane >> 4) + 4 r, column cb + 16 j + (lane & 15)
    double rb[2];
#pragma unroll
    for (u32 j = 0; j < 2; j++) {
        const u32 b = b0 + cb + 16u * j + lr;
        rb[j] = b < M ? q[b] : 0.0;
    }
#pragma unroll
    for (u32 i = 0; i < 2; i++)
#pragma unroll
        for (u32 r = 0; r < 4; r++) {
            const u32 row = ra + 16u * i + lk + 4u * r, a = a0 + row;
            const double qa = a < M ? q[a] : 0.0;
            const double sa = sqrt(qa);
#pragma unroll
            for (u32 j = 0; j < 2; j++) {
                const u32 col = cb + 16u * j + lr, b = b0 + col;
                double v = acc[i][j][r] / (sa * sqrt(rb[j]));
                if (qa == 0.0 || rb[j] == 0.0) v = 0.0;
                if (a == b) v = __builtin_nan("");
                lds[row * SIM_EPI_STRIDE + col] = v;
            }
        }
    __syncthreads();
    sim_tile_store(S, M, a0, b0, diag, lds, lane, wv);
}

// ============================================================================================================ host ==
// The similarity's device buffers belong to the handle and to nothing else: not the EASA arena, the cosine buffers, the
// graph's or the ranking's.
struct SimState : MatrixConsumer {           // per_member: q
    static constexpr int SLOT = east_hip_index::SLOT_SIM;
    u32 L = 0;
    UploadedTable table;                    // a host table's copy (east_hip_similarity_build_host)
    SimState() { bufs.push_back(&table.buf); }
    void clear() override
    {
        MatrixConsumer::clear();
        L = 0;
        table.withdraw();
    }
};

static void sim_check(int32_t axis)
{
    if (axis != EAST_HIP_TOP_BY_TEXT && axis != EAST_HIP_TOP_BY_KEYPHRASE) east_throw(EAST_HIP_ERR_INVALID, "similarity: unknown axis");
}

static void sim_build(east_hip_index *h, TableRef t, int32_t axis, i64 *out)
{
    sim_check(axis);
    const double *d_table = t.p;
    const u32 K = t.K, D = t.D;
    if (K < 1 || D < 1 || K >= 0x7FFFFFF0u || D >= 0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "similarity: empty score table");
    SimState &g = consumer_begin<SimState>(h);
    const bool by_text = axis == EAST_HIP_TOP_BY_TEXT;
    const u32 M = by_text ? D : K, L = by_text ? K : D;
    matrix_reserve(h, g, M, false, "similarity", std::to_string(M) + " x " + std::to_string(M) + " members");
    g.L = L;
    Stats stats;
    Ctx ctx = handle_ctx(h, nullptr, &stats);
    double *q = g.per_member;
    const u32 NT = ceil_div_u32(M, SIM_TILE);
    ConsumerTimer timer(h, g);
    if (by_text) {
        LAUNCH(ctx, sim_norm_col_kernel, ceil_div_u32(D, SIM_NORM_COLS), d_table, K, D, q);
        LAUNCH_NAMED(ctx, "sim_gram_text_kernel", sim_gram_kernel<true>, dim3(NT, NT), d_table, K, D, (const double *)q, g.matrix);
    } else {
        LAUNCH(ctx, sim_norm_row_kernel, ceil_div_u32(K, WAVES_PER_BLOCK), d_table, K, D, q);
        LAUNCH_NAMED(ctx, "sim_gram_keyphrase_kernel", sim_gram_kernel<false>, dim3(NT, NT), d_table, K, D, (const double *)q, g.matrix);
    }
    timer.finish();
    g.valid = true;
    if (out) { out[0] = (i64)M; out[1] = (i64)L; }
}

extern "C" {

int east_hip_similarity_build_resident(east_hip_handle_t h, int32_t source, int32_t axis, int64_t *out)
{
    return guarded([&] { sim_build(h, consumer_resident<SimState>(h, source, "similarity"), axis, out); });
}

int east_hip_similarity_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs, int32_t axis, int64_t *out)
{
    return guarded([&] {
        const TableRef t = consumer_upload<SimState>(h, table, n_keyphrases, n_docs, "similarity: null or empty score table",
                                                     "the similarity's score table", [&] { sim_check(axis); });
        sim_build(h, t, axis, out);
    });
}

int east_hip_similarity_fetch(east_hip_handle_t h, double *matrix, double *norm2)
{
    return guarded([&] {
        matrix_fetch(h, consumer_built<SimState>(h, "no similarity matrix has been built on this handle"), matrix, norm2, nullptr);
    });
}

double east_hip_last_similarity_ms(east_hip_handle_t h) { return consumer_ms<SimState>(h); }

}  // extern "C"
