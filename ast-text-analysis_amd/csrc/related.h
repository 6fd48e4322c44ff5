// related.h -- text-to-text relatedness on the device: how much of text A's wording is found in text B, for every two
// texts of the index (include/east_hip.h, "Text-to-text relatedness"; `east texts related`).
//
// The strings of document A -- the runs of text symbols between the terminators of its part of the resident code stream --
// are scored against the tree of every document B by the score walk, exactly as keyphrases are, and the scores of A's
// strings are averaged: F[A][B] = (sum over the scored strings s of A of score(s, B)) / c_A.
//
//   code stream --scan.h over "is a terminator" + rel_ends_kernel--> end[j] of every string j
//   --rel_lengths_kernel: a thread a string--> len[j] = its symbols other than U+0020 (0: not scored); two scans give
//     q[j] = the suffixes of the strings in front of j and rank[j] = the scored strings in front of j.  len[] is read back
//     ONCE (4 bytes a string; the symbols never leave the device): the host packs the walk's workgroups (q_blk) from it,
//     as it does for uploaded keyphrases, cuts the chunks and lists the tiles
//   per chunk of whole tiles:
//   --rel_feed_kernel: a thread a string, q_code straight out of the resident codes (they ARE the dense codes the walk
//     compares with; U+0020 left out as score() leaves it out), q_end, q_off; q_blk copied from the packed list
//   --score_resident (score_host.h), as it stands: fused or not, document stretches, grid limit--> K_c x D table
//   --rel_reduce_kernel: a workgroup per (tile of REL_TILE scored strings, strip of 64 columns)--> partial[tile][D]
//   --rel_fold_kernel: a thread per (document of the chunk, column) adds the document's tile partials in tile order onto
//     what the chunks before left in F
//   --rel_finish_kernel: / c_A, the zero rows, the NaN diagonal, self, the symmetric form (each pair once, both places)
//
// The tile tree.  The scored strings of a document are numbered 0 .. c_A - 1; tile t of the document holds the strings
// [REL_TILE t, REL_TILE t + REL_TILE): tiles are aligned to the document's first scored string and never span two documents.
// Inside a tile wavefront w adds the rows w, w + 4, w + 8, ... in that order, the four sums are added as (p0 + p1) +
// (p2 + p3); the tiles of a document are added from the first to the last, ((t0 + t1) + t2) + ...  The shape depends on
// c_A alone.  A chunk is a run of whole tiles, so a tile's sum does not know of chunks, and the fold goes on where the
// chunk before stopped: F after the last chunk is the same left-to-right sum wherever the cuts fall.  No atomic.
//
// Why the table goes through HBM: the chunk's K_c x D scores are written once by the walk and read once here, 16 bytes a
// score against a walk of dozens of dependent gathers a score.  Parallelism comes from the (tile, strip) pairs -- one
// document of 64 MiB is ~12 000 tiles --, the rows are read as whole 512-byte pieces (a wavefront: 64 consecutive columns).
//
// The host half is a MatrixConsumer of the handle (consumer.h: the matrix, its limit, its fetch, what it offers()); it
// adds whether the matrix is the directed form.
#pragma once
#include "consumer.h"
#include "score_host.h"

#define REL_TILE 256u                              // scored strings of a tile
#define REL_STRIP 64u                              // columns of a strip: a lane each
#define REL_MAX_CHUNK_TILES ((1u << 22) / REL_TILE) // (score_resident: a launch of the walk takes fewer than 2^24 workgroups)
#define REL_MAX_GRID (1u << 22)                     // workgroups of a launch at most: 2^30 threads, below HIP's 2^32 a grid dimension (the sums loop)
#define REL_CHUNK_BYTES ((size_t)256 << 20)        // the default chunk: as many tiles as keep K_c x D x 8 bytes at or below this ("Measured": flat from 64 MiB up)

// ---- the string directory ---------------------------------------------------------------------------------------------
template <class SYM> struct RelTermIn {            // 1 where the stream holds a terminator (text codes are 1 .. sigma_t, build.h)
    const SYM *s;
    u32 term_first;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (u32)s[i] >= term_first ? 1u : 0u; }
};

struct RelScoredIn {                               // 1 where a string is scored
    const u32 *len;
    __device__ __forceinline__ u32 operator()(u32 i) const { return len[i] != 0u ? 1u : 0u; }
};

// before[i] = the terminators in front of position i: the terminator at i ends string before[i]
template <class SYM>
__global__ __launch_bounds__(BLOCK) void rel_ends_kernel(const SYM *__restrict__ s, u32 n, u32 term_first, const u32 *__restrict__ before,
                                                         u32 m, u32 *__restrict__ end)
{
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (u32)s[i] < term_first) return;
    const u32 j = before[i];
    if (j < m) end[j] = (u32)i;
}

// len[j] = the symbols of string j other than U+0020 (space: its dense code, 0 when the texts hold none)
template <class SYM>
__global__ __launch_bounds__(BLOCK) void rel_lengths_kernel(const SYM *__restrict__ s, const u32 *__restrict__ end, u32 m, u32 space,
                                                            u32 *__restrict__ len)
{
    const u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m) return;
    const u32 b = j ? end[j - 1] + 1u : 0u, e = end[j];
    u32 c = 0;
    for (u32 i = b; i < e; i++) c += (u32)s[i] != space ? 1u : 0u;
    len[j] = c;
}

// ---- feeding the walk -------------------------------------------------------------------------------------------------
// The strings [j0, j1) of a chunk: the scored ones are its keyphrases g0 .. g0 + K - 1 (rank), their suffixes Q0 .. Q0 + n_q - 1 (q).
template <class SYM>
__global__ __launch_bounds__(BLOCK) void rel_feed_kernel(const SYM *__restrict__ s, const u32 *__restrict__ end, const u32 *__restrict__ len,
                                                         const u32 *__restrict__ q, const u32 *__restrict__ rank, u32 j0, u32 j1, u32 g0,
                                                         u32 Q0, u32 K, u32 n_q, u32 space, u32 *__restrict__ q_code,
                                                         u32 *__restrict__ q_end, u32 *__restrict__ q_off)
{
    const u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (gid == 0) q_off[K] = n_q;
    if (gid >= (u64)(j1 - j0)) return;
    const u32 j = j0 + (u32)gid;
    const u32 l = len[j];
    if (l == 0u) return;
    const u32 k = rank[j] - g0, base = q[j] - Q0;
    if (k >= K || base + l > n_q) return;                         // (never: the host cut the chunk from the same numbers)
    q_off[k] = base;
    u32 t = base;
    const u32 e = end[j];
    for (u32 i = j ? end[j - 1] + 1u : 0u; i < e; i++) {
        const u32 c = (u32)s[i];
        if (c != space && t < base + l) { q_code[t] = c; q_end[t] = base + l; t++; }
    }
}

// ---- the sums ---------------------------------------------------------------------------------------------------------
// Workgroup (tile, strip): rows [tile_row[t0 + tile] - g0, tile_row[t0 + tile + 1] - g0) of the chunk's table x columns
// [64 strip, 64 strip + 64) -> partial[tile][column].  See "The tile tree" above.
__global__ __launch_bounds__(BLOCK) void rel_reduce_kernel(const double *__restrict__ table, u32 D, const u32 *__restrict__ tile_row, u32 t0,
                                                           u32 g0, u32 strips, double *__restrict__ partial)
{
    __shared__ double part[WAVES_PER_BLOCK][REL_STRIP];
    const u32 tile = blockIdx.x / strips, strip = blockIdx.x % strips;
    const u32 r0 = tile_row[t0 + tile] - g0, r1 = tile_row[t0 + tile + 1u] - g0;
    const u32 lane = lane_id(), wv = wave_id();
    const u32 col = strip * REL_STRIP + lane;
    double acc = 0.0;
    if (col < D) {
        u32 r = r0 + wv;
        for (; r + 3u * WAVES_PER_BLOCK < r1; r += 4u * WAVES_PER_BLOCK) {       // (four loads requested before the first is added)
            double v[4];
#pragma unroll
            for (u32 i = 0; i < 4; i++) v[i] = table[(size_t)(r + i * WAVES_PER_BLOCK) * D + col];
#pragma unroll
            for (u32 i = 0; i < 4; i++) acc += v[i];
        }
        for (; r < r1; r += WAVES_PER_BLOCK) acc += table[(size_t)r * D + col];
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0u && col < D) partial[(size_t)tile * D + col] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// Thread (document d_lo + dd, column): the tiles of the document inside the chunk [t0, t1), in tile order, onto F[d][column]
// (doc_tile: the D + 1 bounds of the documents' tiles).  The document's first tile starts the sum; it is not added to a zero.
__global__ __launch_bounds__(BLOCK) void rel_fold_kernel(const double *__restrict__ partial, u32 D, const u32 *__restrict__ doc_tile, u32 t0,
                                                         u32 t1, u32 d_lo, u32 n_d, double *__restrict__ F)
{
    for (u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x; gid < (u64)n_d * D; gid += (u64)gridDim.x * BLOCK) {
        const u32 d = d_lo + (u32)(gid / D), col = (u32)(gid % D);
        const u32 first = doc_tile[d];
        u32 lo = max(first, t0);
        const u32 hi = min(doc_tile[d + 1u], t1);
        if (lo >= hi) continue;
        double acc;
        if (lo == first) { acc = partial[(size_t)(lo - t0) * D + col]; lo++; }
        else acc = F[(size_t)d * D + col];
        for (; lo < hi; lo++) acc += partial[(size_t)(lo - t0) * D + col];
        F[(size_t)d * D + col] = acc;
    }
}

// Thread (A, B), A <= B, in place: M holds the sums F on entry (rows of documents without a scored string: never written,
// never read) and R on exit.
__global__ __launch_bounds__(BLOCK) void rel_finish_kernel(double *__restrict__ M, u32 D, const int32_t *__restrict__ scored, int symmetric,
                                                           double *__restrict__ self)
{
    for (u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x; gid < (u64)D * D; gid += (u64)gridDim.x * BLOCK) {
        const u32 a = (u32)(gid / D), b = (u32)(gid % D);
        if (a > b) continue;
        const int32_t ca = scored[a], cb = scored[b];
        const double fab = ca ? M[(size_t)a * D + b] / (double)ca : 0.0;
        if (a == b) {
            self[a] = fab;
            M[(size_t)a * D + a] = __builtin_nan("");
            continue;
        }
        const double fba = cb ? M[(size_t)b * D + a] / (double)cb : 0.0;
        if (symmetric) {
            const double v = (fab + fba) * 0.5;
            M[(size_t)a * D + b] = v;
            M[(size_t)b * D + a] = v;
        } else {
            M[(size_t)a * D + b] = fab;
            M[(size_t)b * D + a] = fba;
        }
    }
}

// ============================================================================================================ host ==
// The relatedness' device buffers belong to the handle and to nothing else: not the EASA arena, the score scratch, the
// ranking's buffers or the similarity's.
struct RelState : MatrixConsumer {           // per_member: self; count: scored
    static constexpr int SLOT = east_hip_index::SLOT_REL;
    bool symmetric = false;                 // the matrix is the symmetric form
    DevBuf scan_tmp, dir, partial;          // the terminator counts (released after the directory); the directory and the lists; partial[tile][D]
    RelState() { bufs.insert(bufs.end(), {&scan_tmp, &dir, &partial}); }
    TableRef offers() const override
    {
        TableRef t = MatrixConsumer::offers();
        t.directed = !symmetric;
        return t;
    }
};

static void rel_build(east_hip_index *h, int normalized, int32_t orientation, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (orientation != EAST_HIP_RELATED_DIRECTED && orientation != EAST_HIP_RELATED_SYMMETRIC)
        east_throw(EAST_HIP_ERR_INVALID, "relatedness: unknown orientation");
    if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
    use_device(h);
    RelState &g = consumer_begin<RelState>(h);
    // the handle's resident keyphrases are replaced, its score table withdrawn -- whatever becomes of this call
    h->table_scored = false;
    h->kp.q_code_epoch = 0;
    h->kp.n_kp = h->kp.n_q = 0;
    const u32 D = h->n_docs, n = h->n, m = h->m_total;
    u64 m_sum = 0;
    for (u32 d = 0; d < D; d++) m_sum += h->h_n_strings[d];
    if (m_sum != m || m < 1) east_throw(EAST_HIP_ERR_INTERNAL, "relatedness: the documents' strings do not add up");
    const std::string texts = std::to_string(D) + " texts";
    auto rel_oom = [&](const char *what, double bytes) { consumer_oom("relatedness", what, texts, bytes); };
    const size_t scan_scratch = align256(((size_t)ceil_div_u32((u64)n + 1, SCAN_TILE) + 1) * 8) + 16 * 256;
    matrix_reserve(h, g, D, true, "relatedness", texts);
    if (!g.scan_tmp.try_ensure(align256(((size_t)n + 1) * 4) + scan_scratch, h->stream)) rel_oom("the string directory", ((double)n + 1) * 4.0);
    Stats stats;
    const Knobs kn = knobs_snapshot();
    ConsumerTimer timer(h, g);

    // ---- the directory: end, len, q, rank per string ----
    std::vector<u32> len((size_t)m + 1);
    // (room for the lists below too: tile_row and doc_tile, at most m + D + 2 words, and the packed q_blk lists, at most
    // one bound a scored string and one more a chunk -- chunks are whole tiles, of which there are at most m)
    const size_t dir_bytes = align256((size_t)m * 4) + 3 * align256(((size_t)m + 1) * 4) + align256(((size_t)m + D + 2) * 4) +
                             align256(((size_t)D + 1) * 4) + align256((2 * (size_t)m + 2) * 4) + scan_scratch + 256;
    if (!g.dir.try_ensure(dir_bytes, h->stream)) rel_oom("the string directory", (double)dir_bytes);
    Arena da = g.dir.arena();
    u32 *d_end = da.alloc<u32>(m), *d_len = da.alloc<u32>((size_t)m + 1), *d_q = da.alloc<u32>((size_t)m + 1),
        *d_rank = da.alloc<u32>((size_t)m + 1);
    const u32 term_first = h->use_s8 ? 0xFFu : h->sigma_t + 1u;
    u32 space = 0;                                            // the dense code of U+0020, 0 (no symbol's code) when the texts hold none
    HIP_CHECK(hipMemcpyAsync(&space, h->code_map + 0x20, 4, hipMemcpyDeviceToHost, h->stream));
    {
        Arena ta = g.scan_tmp.arena();
        Ctx ctx = handle_ctx(h, &ta, &stats);
        u32 *before = ta.alloc<u32>((size_t)n + 1);
        HIP_CHECK(hipMemsetAsync(d_end, 0, (size_t)m * 4, h->stream));
        HIP_CHECK(hipMemsetAsync(d_len + m, 0, 4, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));           // (space)
        if (h->use_s8) {
            device_scan<RelTermIn<uint8_t>, false>(ctx, RelTermIn<uint8_t>{h->s8, term_first}, n, before);
            LAUNCH_NAMED(ctx, "rel_ends_kernel", rel_ends_kernel<uint8_t>, ceil_div_u32(n, BLOCK), (const uint8_t *)h->s8, n, term_first, (const u32 *)before, m, d_end);
            LAUNCH_NAMED(ctx, "rel_lengths_kernel", rel_lengths_kernel<uint8_t>, ceil_div_u32(m, BLOCK), (const uint8_t *)h->s8, (const u32 *)d_end, m, space, d_len);
        } else {
            device_scan<RelTermIn<u32>, false>(ctx, RelTermIn<u32>{h->s, term_first}, n, before);
            LAUNCH_NAMED(ctx, "rel_ends_kernel", rel_ends_kernel<u32>, ceil_div_u32(n, BLOCK), (const u32 *)h->s, n, term_first, (const u32 *)before, m, d_end);
            LAUNCH_NAMED(ctx, "rel_lengths_kernel", rel_lengths_kernel<u32>, ceil_div_u32(m, BLOCK), (const u32 *)h->s, (const u32 *)d_end, m, space, d_len);
        }
        HIP_CHECK(hipMemcpyAsync(len.data(), d_len, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    }
    {
        Ctx ctx = handle_ctx(h, &da, &stats);
        device_scan<ArrIn, false>(ctx, ArrIn{d_len}, m + 1, d_q);
        device_scan<RelScoredIn, false>(ctx, RelScoredIn{d_len}, m + 1, d_rank);
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));               // (len)
    g.scan_tmp.release();

    // ---- the host's lists: the scored strings, the tiles, the documents' tiles ----
    std::vector<u32> sel, q_host((size_t)m + 1), tile_row, doc_tile((size_t)D + 1);
    std::vector<int32_t> scored(D);
    u64 q_total = 0;
    {
        u32 j = 0;
        for (u32 d = 0; d < D; d++) {
            doc_tile[d] = (u32)tile_row.size();
            u32 c = 0;
            for (u32 e = j + h->h_n_strings[d]; j < e; j++) {
                q_host[j] = (u32)q_total;
                q_total += len[j];
                if (len[j]) {
                    if (c % REL_TILE == 0u) tile_row.push_back((u32)sel.size());
                    sel.push_back(j);
                    c++;
                }
            }
            scored[d] = (int32_t)c;
        }
        q_host[m] = (u32)q_total;
    }
    const u32 c_total = (u32)sel.size(), NT = (u32)tile_row.size();
    tile_row.push_back(c_total);
    doc_tile[D] = NT;
    if (q_total >= (u64)0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "relatedness: the texts' strings are too long in all");

    // ---- the chunks: whole tiles ----
    u32 chunk_tiles;
    if (kn.related_chunk > 0) chunk_tiles = (u32)std::min<i64>((kn.related_chunk + REL_TILE - 1) / REL_TILE, REL_MAX_CHUNK_TILES);
    else chunk_tiles = (u32)std::min<size_t>(std::max<size_t>(REL_CHUNK_BYTES / ((size_t)D * 8 * REL_TILE), 1), REL_MAX_CHUNK_TILES);
    const u32 strips = ceil_div_u32(D, REL_STRIP);
    chunk_tiles = std::max(std::min(chunk_tiles, REL_MAX_GRID / strips), 1u);     // (a (tile, strip) pair a workgroup; D <= 2^20: 2^14 strips)
    struct Chunk { u32 t0, t1, j0, j1, g0, K, Q0, n_q, blk0, n_blk, d_lo, d_hi; };
    std::vector<Chunk> chunks;
    std::vector<u32> blk_all, blk;
    size_t q_bytes = 0;
    for (u32 t0 = 0, d_lo = 0; t0 < NT; t0 += chunk_tiles) {
        Chunk c;
        c.t0 = t0;
        c.t1 = std::min(NT, t0 + chunk_tiles);
        c.g0 = tile_row[c.t0];
        c.K = tile_row[c.t1] - c.g0;
        c.j0 = sel[c.g0];
        c.j1 = c.t1 == NT ? m : sel[tile_row[c.t1]];
        c.Q0 = q_host[c.j0];
        c.n_q = q_host[c.j1] - c.Q0;
        pack_keyphrase_blocks(c.K, kn.score_fused, [&](u32 k) { return (u64)len[sel[c.g0 + k]]; }, blk);
        c.blk0 = (u32)blk_all.size();
        c.n_blk = blk.empty() ? 0u : (u32)blk.size() - 1;
        blk_all.insert(blk_all.end(), blk.begin(), blk.end());
        while (doc_tile[d_lo + 1] <= c.t0) d_lo++;            // the documents that have tiles in [t0, t1): d_lo .. d_hi
        c.d_lo = c.d_hi = d_lo;
        while (c.d_hi + 1 < D && doc_tile[c.d_hi + 1] < c.t1) c.d_hi++;
        chunks.push_back(c);
        q_bytes = std::max(q_bytes, keyphrase_scratch_bytes(c.K, c.n_q, D, score_doc_chunk(c.n_q, D, kn.score_scratch_bytes)));
    }
    const u32 most_tiles = std::min(chunk_tiles, NT);
    if (!g.partial.try_ensure((size_t)most_tiles * D * 8 + 256, h->stream)) rel_oom("a chunk's partial sums", (double)most_tiles * D * 8.0);
    if (!h->kp.buf.try_ensure(q_bytes, h->stream)) rel_oom("a chunk's score table", (double)q_bytes);
    u32 *d_tile_row = da.alloc<u32>(tile_row.size()), *d_doc_tile = da.alloc<u32>(doc_tile.size()),
        *d_blk = da.alloc<u32>(std::max<size_t>(blk_all.size(), 1));
    HIP_CHECK(hipMemcpyAsync(d_tile_row, tile_row.data(), tile_row.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_doc_tile, doc_tile.data(), doc_tile.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (!blk_all.empty()) HIP_CHECK(hipMemcpyAsync(d_blk, blk_all.data(), blk_all.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(g.count, scored.data(), (size_t)D * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));

    Ctx ctx = handle_ctx(h, nullptr, &stats);
    double *partial = g.partial.as<double>();
    for (const Chunk &c : chunks) {
        set_keyphrases_device(h, c.K, c.n_q, c.n_blk, kn, [&] {
            if (c.n_blk)
                HIP_CHECK(hipMemcpyAsync(h->kp.q_blk, d_blk + c.blk0, ((size_t)c.n_blk + 1) * 4, hipMemcpyDeviceToDevice, h->stream));
            const u32 grid = ceil_div_u32(std::max(c.j1 - c.j0, 1u), BLOCK);
            if (h->use_s8)
                LAUNCH_NAMED(ctx, "rel_feed_kernel", rel_feed_kernel<uint8_t>, grid, (const uint8_t *)h->s8, (const u32 *)d_end, (const u32 *)d_len,
                             (const u32 *)d_q, (const u32 *)d_rank, c.j0, c.j1, c.g0, c.Q0, c.K, c.n_q, space, h->kp.q_code, h->kp.q_end, h->kp.q_off);
            else
                LAUNCH_NAMED(ctx, "rel_feed_kernel", rel_feed_kernel<u32>, grid, (const u32 *)h->s, (const u32 *)d_end, (const u32 *)d_len,
                             (const u32 *)d_q, (const u32 *)d_rank, c.j0, c.j1, c.g0, c.Q0, c.K, c.n_q, space, h->kp.q_code, h->kp.q_end, h->kp.q_off);
            h->kp.q_code_epoch = h->map_epoch;                   // (q_code holds dense codes already: no query_map_kernel)
        });
        score_resident(h, normalized);
        LAUNCH(ctx, rel_reduce_kernel, (c.t1 - c.t0) * strips, (const double *)h->kp.table, D, (const u32 *)d_tile_row, c.t0, c.g0, strips, partial);
        const u32 n_d = c.d_hi - c.d_lo + 1u;
        LAUNCH(ctx, rel_fold_kernel, (u32)std::min<u64>(((u64)n_d * D + BLOCK - 1) / BLOCK, REL_MAX_GRID), (const double *)partial, D, (const u32 *)d_doc_tile, c.t0, c.t1, c.d_lo,
               n_d, g.matrix);
        h->table_scored = false;
        h->kp.q_code_epoch = 0;
        h->kp.n_kp = h->kp.n_q = 0;
    }
    LAUNCH(ctx, rel_finish_kernel, (u32)std::min<u64>(((u64)D * D + BLOCK - 1) / BLOCK, REL_MAX_GRID), g.matrix, D, (const int32_t *)g.count, (int)(orientation == EAST_HIP_RELATED_SYMMETRIC),
           g.per_member);
    timer.finish();
    g.symmetric = orientation == EAST_HIP_RELATED_SYMMETRIC;
    g.valid = true;
    if (out) { out[0] = (i64)D; out[1] = (i64)c_total; out[2] = (i64)chunks.size(); }
}

extern "C" {

int east_hip_related_build(east_hip_handle_t h, int normalized, int32_t orientation, int64_t *out)
{
    return guarded([&] { rel_build(h, normalized, orientation, out); });
}

int east_hip_related_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *scored)
{
    return guarded([&] {
        matrix_fetch(h, consumer_built<RelState>(h, "no relatedness matrix has been built on this handle"), matrix, self, scored);
    });
}

double east_hip_last_related_ms(east_hip_handle_t h) { return consumer_ms<RelState>(h); }

int east_hip_debug_set_related_chunk(int64_t strings)
{
    // scored strings per score launch, rounded up to whole tiles of REL_TILE; 0 or less: the default (REL_CHUNK_BYTES of table)
    knobs_update([&](Knobs &k) { k.related_chunk = strings > 0 ? strings : 0; });
    return EAST_HIP_OK;
}

}  // extern "C"
