// overlap.h -- shared-shingle overlap of the indexed texts: for every two texts of the cosine term index the resemblance
// |A n B| / |A u B| or the containment |A n B| / |A| of their sets of w-word shingles (include/east_hip.h, "Shingle
// overlap"; `east texts overlap`).  Every entry is one division of two exact integers.
//
//   tok_term, tok_doc --levels 1 .. w of phrases.h's naming with min_count 2 (phr_level_step; level w is named only)-->
//     the sorted pairs of level w: a run = a distinct shingle that occurs at least twice in the collection; a member that
//     is its run's head or carries tflag = the first occurrence of the shingle in its text = a POSTING; a run with a text
//     step is SHARED (two texts hold it) and gets a dense unit id from a scan over the heads of the shared runs
//   --count, scan, fill--> the postings of the shared runs, (text, unit), in (unit, text) order
//   --one flag a position, one scan, differences at the texts' bounds--> n_a = |S_a|: a position where w words of one text
//     start counts when it lies outside the level's domain (its shingle occurs once in the collection) or is a posting
//   --one stable radix sort by text--> per text its units ascending (du), doc_off by a lower bound a text
//   --ovl_tile_kernel + ovl_fold_kernel--> I = X X^T, X the D x units 0/1 incidence matrix, as 64 x 64 tiles of 32-bit
//     integers (route 2: cost_tile_kernel + cost_fold_kernel of cosine_texts.h on weights of 1.0, exact below 2^53)
//   --ovl_finish_kernel: a workgroup per tile pair--> the quotients, self, NaN on the diagonal, the tile and its mirror
//
// The first two arrows -- the names, the units, the postings -- are ovl_names_postings, which the shared passages
// (passages.h) run too.
//
// The tile kernel keeps the shape of cost_tile_kernel: a workgroup per (64 x 64 tile of text pairs, tile_a <= tile_b;
// segment of COSTEXT_SEG units), a cursor per member found by binary search, the next chunk the one that holds the smallest
// unit under any cursor, a chunk nobody holds never staged.  The chunk is OVL_CHUNK = 64 units wide and staged as 0/1 BYTES:
// lds[member][unit - chunk], 128 members x 80 bytes (64 and a pad of 16 that spreads the members' 16-byte fragment reads
// over the banks).  v_mfma_i32_16x16x64_i8: lane l gives 16 bytes of A's row l & 15 and 16 bytes of B's column l & 15, both
// k group l >> 4.  A and B fragments are read by ONE rule out of ONE layout -- member (l & 15), bytes 16 (l >> 4) .. + 15
// -- so whatever k the hardware gives byte j of k group g, it is the same k on both sides: in a Gram product a permutation
// of k inside a step cancels.  The results use the standard 16 x 16 map, col = lane & 15, row = (lane >> 4) * 4 + reg --
// NOT the f64 map of the neighbouring kernels.  Integer sums are exact in any order: the fold's order is no contract, and
// the bytes do not depend on the batching (east_hip_debug_set_overlap_batch) or on the route.
//
// Memory: 128 bytes a kept token of work arrays while the levels run; 16 bytes a posting (24 on route 2), 16 KiB a tile
// pair of integer tiles and the partial tiles of a batch (at most OVL_SCRATCH_BYTES, or one segment's).  Buffers of this
// consumer's own: a build does not disturb the extracted phrases.  No atomic in this file.
#pragma once
#include "consumer.h"
#include "cosine.h"
#include "cosine_texts.h"
#include "phrases.h"

#define OVL_CHUNK 64u                              // units staged at a time: the k of one v_mfma_i32_16x16x64_i8
#define OVL_LDS_STRIDE 80u                         // bytes from one member's chunk to the next
#define OVL_TILE_WORDS (SIM_TILE * SIM_TILE)       // 32-bit words of a tile
#define OVL_SCRATCH_BYTES ((size_t)256 << 20)      // the default batch: as many segments as keep the partial tiles at or below this
#define OVL_DEFAULT_ROUTE 1                        // what route 0 means ("Measured")
static_assert(COSTEXT_SEG % OVL_CHUNK == 0, "a chunk must not span two segments");
static_assert(OVL_LDS_STRIDE % 16u == 0 && OVL_LDS_STRIDE >= OVL_CHUNK, "a fragment is 16 aligned bytes of a member's chunk");

typedef int ovl_v4i __attribute__((ext_vector_type(4)));

// ---- postings -------------------------------------------------------------------------------------------------------------
// Over the sorted pairs of level w (phr_level_step: ri, run_start, tflag, tx = the exclusive scan of tflag with its total).
// 1 at the head of a shared run: its exclusive scan numbers the units
struct OvlSharedIn {
    const u32 *ri, *run_start, *tx;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        const u32 r1 = ri[i];
        if (i > 0u && ri[i - 1u] == r1) return 0u;
        return tx[run_start[r1]] != tx[i] ? 1u : 0u;          // (a text step inside [i, the next run's start))
    }
};

// 1 at a posting of a shared run: the head, and every member in front of which the text steps
struct OvlPostIn {
    const u32 *ri, *run_start, *tx, *tflag;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        const u32 r = ri[i] - 1u, a = run_start[r], e = run_start[r + 1u];
        if (tx[e] == tx[a]) return 0u;
        return i == a || tflag[i] ? 1u : 0u;
    }
};

// first[j] = the occurrence at position j is the first of its shingle in its text (positions of the domain only); the
// postings of the shared runs to their slots as (text, unit): ux = the units' scan, px = the postings'
__global__ __launch_bounds__(BLOCK) void ovl_postings_kernel(OvlPostIn post, const u32 *__restrict__ ux, const u32 *__restrict__ px,
                                                             const u32 *__restrict__ svals, const u32 *__restrict__ tok_doc, u32 n,
                                                             u32 *__restrict__ first, u32 *__restrict__ p_doc, u32 *__restrict__ p_unit)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 a = post.run_start[post.ri[i] - 1u], j = svals[i];
    first[j] = i == a || post.tflag[i] ? 1u : 0u;
    if (!post(i)) return;
    const u32 slot = px[i];
    p_doc[slot] = tok_doc[j];
    p_unit[slot] = ux[a];
}

// ---- sizes ----------------------------------------------------------------------------------------------------------------
// One word of flags a position j.  Bit 0: a SHINGLE POSITION, w words of one text start there (tok_doc never decreases: the
// ends' texts decide).  It lies INSIDE the domain of level w when its (w - 1)-gram survived (id_prev; the level's other
// conditions are the shingle position's own) -- w == 1: always; id_prev == nullptr: the level was never reached, no
// position is inside.  Bit 1: a shingle position outside the domain (its shingle occurs once in the collection).  Bit 2: a
// shingle position that adds a shingle to its text's set: outside the domain, or the first occurrence in its text (first:
// ovl_postings_kernel).
__global__ __launch_bounds__(BLOCK) void ovl_position_flags_kernel(const u32 *__restrict__ tok_term, const u32 *__restrict__ tok_doc,
                                                                   const u32 *__restrict__ id_prev, const u32 *__restrict__ first, u32 w,
                                                                   u32 T, u32 *__restrict__ flags)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= T) return;
    const u32 e = j + w - 1u;
    bool shingle = e < T && tok_doc[e] == tok_doc[j];
    for (u32 k = 0; shingle && k < w; k++) shingle = tok_term[j + k] != COS_NONE;
    u32 f = 0u;
    if (shingle) {
        const bool inside = w == 1u || (id_prev && id_prev[j] != COS_NONE);
        f = 1u | (inside ? 0u : 2u) | (!inside || first[j] ? 4u : 0u);
    }
    flags[j] = f;
}

struct OvlBitIn {           // one bit of the flags: an input of the scan
    const u32 *flags;
    u32 bit;
    __device__ __forceinline__ u32 operator()(u32 j) const { return (flags[j] >> bit) & 1u; }
};

// n_a = the flags between the text's first position and the next text's; nx = their exclusive scan with its total
__global__ __launch_bounds__(BLOCK) void ovl_sizes_kernel(const u32 *__restrict__ tok_doc, u32 T, const u32 *__restrict__ nx, u32 D,
                                                          int32_t *__restrict__ shingles)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= D) return;
    shingles[d] = (int32_t)(nx[ascending_lower_bound(tok_doc, T, d + 1u)] - nx[ascending_lower_bound(tok_doc, T, d)]);
}

// doc_off[d] = the first posting, in text order, of a text >= d (d = 0 .. D)
__global__ __launch_bounds__(BLOCK) void ovl_doc_off_kernel(const u32 *__restrict__ sorted_doc, u32 P, u32 D, u32 *__restrict__ doc_off)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d <= D) doc_off[d] = ascending_lower_bound(sorted_doc, P, d);
}

__global__ __launch_bounds__(BLOCK) void ovl_ones_kernel(double *__restrict__ dw, u32 P)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) dw[p] = 1.0;
}

// ---- a tile's intersections over a segment --------------------------------------------------------------------------------
// Workgroup (blockIdx.y = tile_a, blockIdx.x = tile_b, blockIdx.z = segment seg0 + z of the batch) -> partial[z][pair], all
// 64 x 64 entries (zeros behind D).
__global__ __launch_bounds__(BLOCK) void ovl_tile_kernel(const u32 *__restrict__ du, const u32 *__restrict__ doc_off, u32 D, u32 n_units,
                                                         u32 seg0, u32 *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[2u * SIM_TILE * OVL_LDS_STRIDE];
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
    ovl_v4i acc[2][2];
#pragma unroll
    for (u32 i = 0; i < 2; i++)
#pragma unroll
        for (u32 j = 0; j < 2; j++) acc[i][j] = (ovl_v4i){0, 0, 0, 0};

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
    uint8_t *row = lds + (threadIdx.x & (2u * SIM_TILE - 1u)) * OVL_LDS_STRIDE;      // (members only write: strip a's rows, then strip b's)
    const uint8_t *la = lds, *lb = diag ? lds : lds + SIM_TILE * OVL_LDS_STRIDE;
    // the fragments: member (lane & 15) of the 16 x 16 block, bytes 16 (lane >> 4) .. + 15 of its chunk -- A and B alike
    const ovl_v4i *fa[2] = {(const ovl_v4i *)(la + (ra + lr) * OVL_LDS_STRIDE + 16u * lk), (const ovl_v4i *)(la + (ra + 16u + lr) * OVL_LDS_STRIDE + 16u * lk)};
    const ovl_v4i *fb[2] = {(const ovl_v4i *)(lb + (cb + lr) * OVL_LDS_STRIDE + 16u * lk), (const ovl_v4i *)(lb + (cb + 16u + lr) * OVL_LDS_STRIDE + 16u * lk)};
    u32 *words = (u32 *)lds;
    for (;;) {
        u32 m = wave_min(nu);
        if (lane == 0u) wmin[wv] = m;
        __syncthreads();                                          // (and: the chunk before has been read)
        m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        if (m == COS_NONE) break;                                 // (the same for every thread of the workgroup)
        const u32 chunk = m & ~(OVL_CHUNK - 1u);
        for (u32 i = threadIdx.x; i < 2u * SIM_TILE * OVL_LDS_STRIDE / 4u; i += BLOCK) words[i] = 0u;
        __syncthreads();
        while (nu - chunk < OVL_CHUNK) {                          // (nu >= chunk; COS_NONE - chunk is far above)
            row[nu - chunk] = 1;
            cur++;
            nu = cur < end ? du[cur] : COS_NONE;
            if (nu >= hi_u) nu = COS_NONE;
        }
        __syncthreads();
        const ovl_v4i a[2] = {*fa[0], *fa[1]}, b[2] = {*fb[0], *fb[1]};
#pragma unroll
        for (u32 i = 0; i < 2; i++)
#pragma unroll
            for (u32 j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    // acc[i][j][r] is row ra + 16 i + 4 (lane >> 4) + r, column cb + 16 j + (lane & 15)
    u32 *out = partial + ((size_t)blockIdx.z * (size_t)cost_pair_index(NT, NT, NT) + (size_t)cost_pair_index(ta, tb, NT)) * OVL_TILE_WORDS;
#pragma unroll
    for (u32 i = 0; i < 2; i++)
#pragma unroll
        for (u32 r = 0; r < 4; r++)
#pragma unroll
            for (u32 j = 0; j < 2; j++) out[(ra + 16u * i + 4u * lk + r) * SIM_TILE + cb + 16u * j + lr] = (u32)acc[i][j][r];
}

// G[pair][entry] (+)= the batch's n_seg partial tiles (first: the batch starts the sum); words = n_pairs * OVL_TILE_WORDS
__global__ __launch_bounds__(BLOCK) void ovl_fold_kernel(const u32 *__restrict__ partial, u64 words, u32 n_seg, int first, u32 *__restrict__ G)
{
    for (u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x; gid < words; gid += (u64)gridDim.x * BLOCK) {
        u32 acc = first ? 0u : G[gid];
        for (u32 s = 0; s < n_seg; s++) acc += partial[(size_t)s * words + gid];
        G[gid] = acc;
    }
}

// ---- the quotients --------------------------------------------------------------------------------------------------------
// Workgroup = pair.  I comes out of G[pair] (route 1) or, with G == nullptr, out of the matrix's own upper tile, where
// cost_fold_kernel left it as a double (route 2: in place).  symmetric: I / (n_a + n_b - I) to the tile and its mirror
// image through sim_tile_store; directed: I / n_a to the tile, I / n_b to the mirror image.  A zero denominator: +0.0.
__global__ __launch_bounds__(BLOCK) void ovl_finish_kernel(const u32 *__restrict__ G, double *__restrict__ M, const u32 *__restrict__ pair_tiles,
                                                           u32 D, const int32_t *__restrict__ shingles, int symmetric, double *__restrict__ self)
{
    __shared__ double tile[SIM_TILE * SIM_EPI_STRIDE];
    const u32 t = pair_tiles[blockIdx.x];
    const u32 a0 = (t >> 16) * SIM_TILE, b0 = (t & 0xFFFFu) * SIM_TILE;
    const u32 lane = lane_id(), wv = wave_id();
    const bool diag = a0 == b0;
    for (u32 r = wv; r < SIM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = a0 + r, b = b0 + lane;
        double v = 0.0;
        if (a < D && b < D) {
            const u64 I = G ? (u64)G[(size_t)blockIdx.x * OVL_TILE_WORDS + r * SIM_TILE + lane] : (u64)M[(size_t)a * D + b];
            const u64 na = (u64)(u32)shingles[a], nb = (u64)(u32)shingles[b];
            if (symmetric) {
                const u64 den = na + nb - I;
                v = den ? (double)I / (double)den : 0.0;
                if (a == b) v = __builtin_nan("");
            } else {
                v = (double)I;
            }
            if (a == b) self[a] = na ? 1.0 : 0.0;
        }
        tile[r * SIM_EPI_STRIDE + lane] = v;
    }
    __syncthreads();
    if (symmetric) {
        sim_tile_store(M, D, a0, b0, diag, tile, lane, wv);
        return;
    }
    for (u32 r = wv; r < SIM_TILE; r += WAVES_PER_BLOCK) {
        const u32 a = a0 + r, b = b0 + lane;
        if (a < D && b < D) {
            const double na = (double)(u32)shingles[a];
            M[(size_t)a * D + b] = a == b ? __builtin_nan("") : na != 0.0 ? tile[r * SIM_EPI_STRIDE + lane] / na : 0.0;
        }
    }
    if (diag) return;
    for (u32 c = wv; c < SIM_TILE; c += WAVES_PER_BLOCK) {
        const u32 b = b0 + c, a = a0 + lane;
        if (a < D && b < D) {
            const double nb = (double)(u32)shingles[b];
            M[(size_t)b * D + a] = nb != 0.0 ? tile[lane * SIM_EPI_STRIDE + c] / nb : 0.0;
        }
    }
}

// ============================================================================================================ host ==
// ---- names and postings: steps 1 and 2, shared with the passages (passages.h) -------------------------------------------------
struct OvlPostingRoom {     // where ovl_postings_kernel writes: first[T]; the postings' texts and units, P + 1 words each
    u32 *first, *p_doc, *p_unit;
};

struct OvlNames {
    PhrWork W;              // over the sorted pairs of level w (named only): ri, run_start, tflag, tx
    PhrDomainIn din;        // the last level's domain (din.id_prev: the ids of level w - 1)
    u32 dom = 0;            // the positions in it
    int levels = 0, sr = 0; // the levels run; the sort's buffers that hold the sorted pairs
    u32 named = 0;          // level w was reached and named
    u32 U = 0, P = 0, runs = 0;     // the shared runs, their postings, all runs of level w
    u32 *ux = nullptr, *px = nullptr;       // the units' and the postings' scans over the sorted pairs
    OvlPostIn post = {};
};

// Levels 1 .. w - 1 with their survivors and level w named only (phr_level_step, min_count 2), the units' and the postings'
// scans with their read-back, and the postings to the room that room(U, P) makes for them.  Every array comes out of `a`
// (ctx.arena), 18 words and 24 bytes a kept token.
template <class Room> static OvlNames ovl_names_postings(Ctx &ctx, Arena &a, const CosState &c, u32 w, Room room)
{
    const u32 T = c.n_kept, V = c.V;
    const u32 *tok_term = c.tok_term, *tok_doc = c.tok_doc;
    const size_t K1 = (size_t)T + 2;
    OvlNames nm;
    PhrLevel lv[2];
    for (PhrLevel &l : lv) {
        l.id = a.alloc<u32>(K1);
        l.count = a.alloc<u32>(K1);
        l.texts = a.alloc<u32>(K1);
        l.first = a.alloc<u32>(K1);
        l.open = a.alloc<u32>(K1);
    }
    PhrWork &W = nm.W;
    W.dex = a.alloc<u32>(K1);
    W.sb = sort_bufs_alloc<u64>(a, K1);
    W.ri = a.alloc<u32>(K1);
    W.run_start = a.alloc<u32>(K1);
    W.tflag = a.alloc<u32>(K1);
    W.tx = a.alloc<u32>(K1);
    W.sx = a.alloc<u32>(K1);
    W.term_bits = bit_width_u32(V ? V - 1u : 0u);
    nm.ux = a.alloc<u32>(K1);
    nm.px = a.alloc<u32>(K1);

    // ---- 1. the names: levels 1 .. w - 1 with their survivors, level w named only
    int cur = 0;
    u32 dom = 0, n_below = 0;
    PhrDomainIn din{tok_term, tok_doc, nullptr, 1u, T};
    if (T) dom = device_scan_count(ctx, din, T, W.dex);
    for (u32 n = 1; n <= w && dom; n++) {
        const PhrLevel L = lv[cur], B = n > 1u ? lv[cur ^ 1] : PhrLevel{nullptr, nullptr, nullptr, nullptr, nullptr};
        nm.levels = (int)n;
        const PhrStep st = phr_level_step(ctx, din, dom, n_below, 2u, W, L, B, n < w);
        if (n == w) { nm.named = 1u; nm.sr = st.r; break; }
        if (!st.surv) break;                                  // (nothing occurs twice: no longer shingle does, all intersections are 0)
        din = PhrDomainIn{tok_term, tok_doc, L.id, n + 1u, T};
        n_below = st.surv;
        dom = device_scan_count(ctx, din, T, W.dex);
        cur ^= 1;
    }
    nm.din = din;
    nm.dom = dom;

    // ---- 2. the postings of the shared shingles, in (unit, text) order
    nm.post = OvlPostIn{W.ri, W.run_start, W.tx, W.tflag};
    if (nm.named) {
        device_scan_with_total(ctx, OvlSharedIn{W.ri, W.run_start, W.tx}, dom, nm.ux);
        device_scan_with_total(ctx, nm.post, dom, nm.px);
        device_read_words(ctx, {{&nm.U, nm.ux + dom}, {&nm.P, nm.px + dom}, {&nm.runs, W.ri + dom - 1u}});
    }
    const OvlPostingRoom r = room(nm.U, nm.P);
    if (nm.named)
        LAUNCH(ctx, ovl_postings_kernel, ceil_div_u32(dom, BLOCK), nm.post, (const u32 *)nm.ux, (const u32 *)nm.px, (const u32 *)W.sb.vals[nm.sr], tok_doc,
               dom, r.first, r.p_doc, r.p_unit);
    return nm;
}

struct OverlapState : MatrixConsumer {       // per_member: self; count: shingles
    static constexpr int SLOT = east_hip_index::SLOT_OVL;
    bool symmetric = true;                  // the matrix is the symmetric form
    DevBuf work, ops, scratch;              // the levels' arrays; the postings, the tile pairs and the integer tiles; the partial tiles
    hipEvent_t ev_mid = nullptr;            // between the operands and the product (out[12], out[13])
    OverlapState() { bufs.insert(bufs.end(), {&work, &ops, &scratch}); }
    ~OverlapState() override
    {
        if (ev_mid) (void)hipEventDestroy(ev_mid);
    }
    TableRef offers() const override
    {
        TableRef t = MatrixConsumer::offers();
        t.directed = !symmetric;
        return t;
    }
};

static void overlap_build(east_hip_index *h, int32_t words, int32_t orientation, i64 *out)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (words < 1 || words > PHR_MAX_WORDS) east_throw(EAST_HIP_ERR_INVALID, "overlap: words must lie in 1 .. 8");
    if (orientation != EAST_HIP_OVERLAP_DIRECTED && orientation != EAST_HIP_OVERLAP_SYMMETRIC)
        east_throw(EAST_HIP_ERR_INVALID, "overlap: unknown orientation");
    if (!out) east_throw(EAST_HIP_ERR_INVALID, "overlap: out is null");
    CosState *cp = consumer_peek<CosState>(h);
    if (!cp || !cp->valid) east_throw(EAST_HIP_ERR_NOT_BUILT, "overlap: no cosine index has been built on this handle");
    const CosState &c = *cp;
    const u32 T = c.n_kept, D = c.n_docs, w = (u32)words;
    if (D < 1) east_throw(EAST_HIP_ERR_INVALID, "overlap: the index holds no text");
    // (a text's shingle positions are among the collection's T positions)
    if (T >= 0x7FFFFFF0u) east_throw(EAST_HIP_ERR_INVALID, "overlap: a text may have 2^31 or more shingle positions");
    use_device(h);
    OverlapState &g = consumer_begin<OverlapState>(h);          // (every refusal of an argument lies above: an earlier matrix stays until here)
    const std::string texts = std::to_string(D) + " texts";
    auto ovl_oom = [&](const char *what, double bytes) { consumer_oom("overlap", what, texts, bytes); };
    matrix_reserve(h, g, D, true, "overlap", texts);
    const Knobs kn = knobs_snapshot();
    const int route = kn.overlap_route == 0 ? OVL_DEFAULT_ROUTE : kn.overlap_route;
    const u32 *tok_term = c.tok_term, *tok_doc = c.tok_doc;
    const size_t K1 = (size_t)T + 2;
    // (a kept token: two levels of five arrays, the domain's scan, the sort's two pairs of 12 bytes, five arrays over the
    // sorted pairs, the units' and the postings' scans, four arrays over the positions for the sizes -- 112 bytes -- and 16
    // to spare for the sort's and the scans' scratch)
    const size_t work_bytes = K1 * 128 + ((size_t)4 << 20);
    if (!g.work.try_ensure(work_bytes, h->stream)) ovl_oom("the levels' arrays", (double)work_bytes);
    Arena a = g.work.arena();
    Stats stats;
    Ctx ctx = handle_ctx(h, &a, &stats);
    ConsumerTimer timer(h, g);
    u32 *first = a.alloc<u32>(K1), *nx = a.alloc<u32>(K1), *sh_x = a.alloc<u32>(K1), *out_x = a.alloc<u32>(K1);
    std::vector<u32> pairs;                                   // (on its way up until the sizes' read-back)
    u32 NT = 0, n_seg = 0, batch = 1, *doc_off = nullptr, *d_pairs = nullptr, *G = nullptr;
    u64 n_pairs = 0;
    bool integer = true;
    double *dw = nullptr;
    Arena pa;
    SortBufs<u32> pb = {};
    // ---- 1. the names; 2. the postings of the shared shingles, in (unit, text) order: the lambda makes their room
    const OvlNames nm = ovl_names_postings(ctx, a, c, w, [&](u32 U, u32 P) {
        NT = ceil_div_u32(D, SIM_TILE);
        n_pairs = cost_pair_index(NT, NT, NT);
        n_seg = ceil_div_u32(U, COSTEXT_SEG);
        integer = route == 1 || U == 0;                       // (no unit: the zeros, whatever the route)
        const size_t word_bytes = integer ? 4 : 8, tile_bytes = (size_t)n_pairs * OVL_TILE_WORDS * word_bytes;
        batch = kn.overlap_batch > 0 ? (u32)std::min<i64>(kn.overlap_batch, COSTEXT_MAX_BATCH)
                                     : (u32)std::min<size_t>(std::max<size_t>(OVL_SCRATCH_BYTES / tile_bytes, 1), COSTEXT_MAX_BATCH);
        batch = std::max(std::min(batch, n_seg), 1u);
        const size_t P1 = (size_t)P + 2;
        const size_t ops_bytes = 4 * align256(P1 * 4) + (integer ? 0 : align256(P1 * 8)) + align256(((size_t)D + 2) * 4) + align256((size_t)n_pairs * 4) +
                                 (integer ? align256((size_t)n_pairs * OVL_TILE_WORDS * 4) : 0) + P1 / 2 + ((size_t)4 << 20);
        if (!g.ops.try_ensure(ops_bytes, h->stream)) ovl_oom("the postings and the integer tiles", (double)ops_bytes);
        if (U && !g.scratch.try_ensure((size_t)batch * tile_bytes + 256, h->stream)) ovl_oom("a batch's partial tiles", (double)batch * (double)tile_bytes);
        pa = g.ops.arena();
        pb = sort_bufs_alloc<u32>(pa, P1);                      // keys = the text, vals = the unit
        doc_off = pa.alloc<u32>((size_t)D + 2);
        d_pairs = pa.alloc<u32>((size_t)n_pairs);
        dw = integer ? nullptr : pa.alloc<double>(P1);
        G = integer ? pa.alloc<u32>((size_t)n_pairs * OVL_TILE_WORDS) : nullptr;
        pairs.reserve((size_t)n_pairs);
        for (u32 ta = 0; ta < NT; ta++)
            for (u32 tb = ta; tb < NT; tb++) pairs.push_back(ta << 16 | tb);
        HIP_CHECK(hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, h->stream));
        return OvlPostingRoom{first, pb.keys[0], pb.vals[0]};
    });
    const u32 U = nm.U, P = nm.P, runs = nm.runs, named = nm.named;
    const int levels = nm.levels;
    const PhrDomainIn din = nm.din;
    u32 *ux = nm.ux;

    // ---- 3. the sizes
    const u32 *id_w = named && w > 1u ? din.id_prev : nullptr;
    u32 *flags = ux;                                          // (the units' scan has been read: the postings are in their slots)
    if (T) LAUNCH(ctx, ovl_position_flags_kernel, ceil_div_u32(T, BLOCK), tok_term, tok_doc, id_w, (const u32 *)first, w, T, flags);
    device_scan_with_total(ctx, OvlBitIn{flags, 0u}, T, sh_x);
    device_scan_with_total(ctx, OvlBitIn{flags, 1u}, T, out_x);
    device_scan_with_total(ctx, OvlBitIn{flags, 2u}, T, nx);
    LAUNCH(ctx, ovl_sizes_kernel, ceil_div_u32(D, BLOCK), tok_doc, T, (const u32 *)nx, D, g.count);
    u32 n_positions = 0, n_outside = 0;
    device_read_words(ctx, {{&n_positions, sh_x + T}, {&n_outside, out_x + T}});      // (and: the pairs are up, the levels' arrays done with)

    // ---- 4. the operands in text order: the stable sort keeps the units ascending inside a text
    i64 launches = 0;
    ctx.arena = &pa;
    if (!g.ev_mid) HIP_CHECK(hipEventCreate(&g.ev_mid));
    if (U) {
        const int r = radix_sort_pairs<u32>(ctx, pb, P, bit_width_u32(D - 1u));
        const u32 *du = pb.vals[r];
        LAUNCH(ctx, ovl_doc_off_kernel, ceil_div_u32(D + 1u, BLOCK), (const u32 *)pb.keys[r], P, D, doc_off);
        HIP_CHECK(hipEventRecord(g.ev_mid, h->stream));
        // ---- 5. I = X X^T
        if (integer) {
            u32 *partial = g.scratch.as<u32>();
            const u64 tile_words = n_pairs * OVL_TILE_WORDS;
            const u32 fold_grid = (u32)std::min<u64>((tile_words + BLOCK - 1) / BLOCK, COSTEXT_MAX_GRID);
            for (u32 s0 = 0; s0 < n_seg; s0 += batch) {
                const u32 nb = std::min(batch, n_seg - s0);
                LAUNCH(ctx, ovl_tile_kernel, dim3(NT, NT, nb), du, (const u32 *)doc_off, D, U, s0, partial);
                LAUNCH(ctx, ovl_fold_kernel, fold_grid, (const u32 *)partial, tile_words, nb, (int)(s0 == 0), G);
                launches += 2;
            }
        } else {
            double *partial = g.scratch.as<double>();
            LAUNCH(ctx, ovl_ones_kernel, ceil_div_u32(P, BLOCK), dw, P);
            const u32 fold_grid = (u32)std::min<u64>((n_pairs * COSTEXT_TILE_WORDS + BLOCK - 1) / BLOCK, COSTEXT_MAX_GRID);
            for (u32 s0 = 0; s0 < n_seg; s0 += batch) {
                const u32 nb = std::min(batch, n_seg - s0);
                LAUNCH(ctx, cost_tile_kernel, dim3(NT, NT, nb), du, (const double *)dw, (const u32 *)doc_off, D, U, s0, partial);
                LAUNCH(ctx, cost_fold_kernel, fold_grid, (const double *)partial, (const u32 *)d_pairs, n_pairs, nb, (int)(s0 == 0), D, g.matrix);
                launches += 2;
            }
        }
    } else {
        HIP_CHECK(hipEventRecord(g.ev_mid, h->stream));
        HIP_CHECK(hipMemsetAsync(G, 0, (size_t)n_pairs * OVL_TILE_WORDS * 4, h->stream));
    }
    // ---- 6. the quotients
    LAUNCH(ctx, ovl_finish_kernel, (u32)n_pairs, (const u32 *)G, g.matrix, (const u32 *)d_pairs, D, (const int32_t *)g.count,
           (int)(orientation == EAST_HIP_OVERLAP_SYMMETRIC), g.per_member);
    launches++;
    timer.finish();
    float ms_operands = 0.f, ms_product = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms_operands, g.ev0, g.ev_mid));
    HIP_CHECK(hipEventElapsedTime(&ms_product, g.ev_mid, g.ev1));
    g.symmetric = orientation == EAST_HIP_OVERLAP_SYMMETRIC;
    g.valid = true;
    out[0] = (i64)D; out[1] = (i64)T; out[2] = (i64)n_positions; out[3] = (i64)runs + (i64)n_outside;
    out[4] = (i64)U; out[5] = (i64)P; out[6] = (i64)n_seg; out[7] = launches;
    out[8] = (i64)route; out[9] = (i64)levels; out[10] = (i64)n_pairs; out[11] = (i64)w;
    out[12] = (i64)((double)ms_operands * 1e3); out[13] = (i64)((double)ms_product * 1e3);
}

extern "C" {

int east_hip_overlap_build(east_hip_handle_t h, int32_t words, int32_t orientation, int64_t *out)
{
    return guarded([&] { overlap_build(h, words, orientation, out); });
}

int east_hip_overlap_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *shingles)
{
    return guarded([&] {
        matrix_fetch(h, consumer_built<OverlapState>(h, "no overlap matrix has been built on this handle"), matrix, self, shingles);
    });
}

double east_hip_last_overlap_ms(east_hip_handle_t h) { return consumer_ms<OverlapState>(h); }

int east_hip_debug_set_overlap_route(int route)
{
    // 0: the default (OVL_DEFAULT_ROUTE); 1: the integer tile kernel; 2: the f64 tile kernel of cosine_texts.h on weights of 1.0
    if (route < 0 || route > 2) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.overlap_route = route; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_overlap_batch(int64_t segments)
{
    // segments of the unit range per launch of the tile kernel; 0 or less: the default (OVL_SCRATCH_BYTES of partial tiles)
    knobs_update([&](Knobs &k) { k.overlap_batch = segments > 0 ? segments : 0; });
    return EAST_HIP_OK;
}

}  // extern "C"
