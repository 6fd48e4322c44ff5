// debug_api.h -- the debug ABI of include/east_hip.h: the test knobs and the kernel-level test entry points.
#pragma once

struct DebugScope {
    hipStream_t stream = nullptr;
    Arena arena;
    Stats stats;
    Ctx ctx;
    DebugScope(int device, size_t bytes)
    {
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
            east_throw(EAST_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
        if (device < 0 || device >= c) east_throw(EAST_HIP_ERR_NO_DEVICE, "device ordinal out of range");
        use_device_ordinal(device);
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes));
        arena.base = (char *)p;
        arena.cap = bytes;
        ctx.stream = stream;
        ctx.arena = &arena;
        ctx.stats = &stats;
    }
    ~DebugScope()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        if (arena.base) (void)hipFree(arena.base);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <class K> static void debug_sort(int device, K *keys, u32 *vals, i64 n, int bits)
{
    if (n < 0 || n >= (i64)0x7FFFFFF0 || !keys || !vals || bits < 1 || bits > (int)sizeof(K) * 8)
        east_throw(EAST_HIP_ERR_INVALID, "bad radix sort arguments");
    if (n == 0) return;
    DebugScope sc(device, (size_t)n * (sizeof(K) + 4) * 2 + (40u << 20));
    SortBufs<K> sb;
    for (int k = 0; k < 2; k++) { sb.keys[k] = sc.arena.alloc<K>(n); sb.vals[k] = sc.arena.alloc<u32>(n); }
    HIP_CHECK(hipMemcpyAsync(sb.keys[0], keys, (size_t)n * sizeof(K), hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(sb.vals[0], vals, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    const int r = radix_sort_pairs<K>(sc.ctx, sb, (u32)n, bits);
    HIP_CHECK(hipMemcpyAsync(keys, sb.keys[r], (size_t)n * sizeof(K), hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(vals, sb.vals[r], (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
}

template <class K>
static void debug_first_pass_hist(int device, const u32 *symbols, i64 n64, const u32 *code_map, int w, int b, int spare,
                                  u32 term_first, int shift, u32 mask, uint8_t *s8_out, u32 *present_out, u32 *hist_out,
                                  u32 *group_sum_out, u32 *digit_total_out)
{
    if (!symbols || !code_map || !s8_out || !present_out || !hist_out || !group_sum_out || !digit_total_out || n64 < 1 ||
        n64 >= (i64)0x7FFFFFF0 || w < 1 || w > 12 || b < 1 || b > 8 || spare < 0 || spare >= b ||
        w * b + spare > (int)sizeof(K) * 8 || shift < 0 || shift >= (int)sizeof(K) * 8 || mask > 255u || term_first > 255u)
        east_throw(EAST_HIP_ERR_INVALID, "bad first-pass histogram arguments");
    const u32 n = (u32)n64, n_tiles = ceil_div_u32(n, RS_TILE), n_groups = ceil_div_u32(n_tiles, RS_GROUP);
    const size_t hist_words = (size_t)RS_BINS * n_tiles, sum_words = (size_t)RS_BINS * n_groups, total_words = (size_t)RS_TOTAL_SHARDS * RS_BINS;
    DebugScope sc(device, (size_t)n * 4 + 2 * ((size_t)n + 64) + 2 * (hist_words + sum_words + total_words + PRESENT_WORDS + 1) * 4 +
                              TEXT_SYMBOLS * 4 + (1u << 20));
    Arena &ar = sc.arena;
    u32 *d_sym = ar.alloc<u32>(n), *d_map = ar.alloc<u32>(TEXT_SYMBOLS);
    HIP_CHECK(hipMemcpyAsync(d_sym, symbols, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(d_map, code_map, TEXT_SYMBOLS * 4, hipMemcpyHostToDevice, sc.stream));
    for (int v = 0; v < 2; v++) {
        uint8_t *s8 = ar.alloc<uint8_t>((size_t)n + 64);
        u32 *present = ar.alloc<u32>(PRESENT_WORDS + 1), *hist = ar.alloc<u32>(hist_words), *group_sum = ar.alloc<u32>(sum_words);
        u32 *total = ar.alloc<u32>(total_words);
        // (what lies behind the pad differs between the two: no counted key may depend on it)
        HIP_CHECK(hipMemsetAsync(s8, v ? 0xA5 : 0x5A, (size_t)n + 64, sc.stream));
        HIP_CHECK(hipMemsetAsync(present, 0, (PRESENT_WORDS + 1) * 4, sc.stream));
        HIP_CHECK(hipMemsetAsync(hist, 0xEE, hist_words * 4, sc.stream));
        HIP_CHECK(hipMemsetAsync(group_sum, 0xEE, sum_words * 4, sc.stream));
        HIP_CHECK(hipMemsetAsync(total, 0, total_words * 4, sc.stream));
        const TextWindowGen<K> gen{s8, n, w, b, spare, term_first, DocKey()};
        if (v == 0) {
            LAUNCH_NAMED(sc.ctx, "presence_remap_hist_kernel", (presence_remap_hist_kernel<K, TextWindowGen<K>>), n_groups,
                         (const u32 *)d_sym, n, (const u32 *)d_map, present, s8, gen, shift, mask, n_tiles, hist, group_sum, total);
        } else {
            LAUNCH(sc.ctx, presence_kernel, std::min<u32>(ceil_div_u32(n, BLOCK), 2048), (const u32 *)d_sym, n, 1, present);
            LAUNCH(sc.ctx, remap_bytes_kernel, ceil_div_u32((u64)n + 16, BLOCK * 16), (const u32 *)d_sym, (const u32 *)d_map, n, 1, s8);
            hipLaunchKernelGGL((radix_hist_kernel<K, TextWindowGen<K>, false>), dim3(n_groups), dim3(RS_HIST_THREADS), 0, sc.stream, gen, n,
                               shift, mask, n_tiles, hist, group_sum, total, RsSeg());
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(s8_out + (size_t)v * ((size_t)n + 16), s8, (size_t)n + 16, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipMemcpyAsync(present_out + (size_t)v * PRESENT_WORDS, present, PRESENT_WORDS * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipMemcpyAsync(hist_out + v * hist_words, hist, hist_words * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipMemcpyAsync(group_sum_out + v * sum_words, group_sum, sum_words * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipMemcpyAsync(digit_total_out + v * total_words, total, total_words * 4, hipMemcpyDeviceToHost, sc.stream));
    }
    HIP_CHECK(hipStreamSynchronize(sc.stream));
}

// what annotate() and the passes behind it read of a handle, in the scope's arena: the caller's table with the levels of
// its pyramid, the annotation, the document tables (lcp_words of the table go up: n, or the padding as well, or nothing)
static void debug_table_handle(DebugScope &sc, east_hip_index &h, const u32 *lcp, u32 n, const i64 *doc_off, int32_t n_docs,
                               const int32_t *n_strings, u32 lcp_words = 0xFFFFFFFFu)
{
    if (lcp_words == 0xFFFFFFFFu) lcp_words = n;
    Arena &ar = sc.arena;
    std::vector<u32> off32((size_t)n_docs + 1), m32(n_docs);
    for (int32_t d = 0; d <= n_docs; d++) off32[d] = (u32)doc_off[d];
    for (int32_t d = 0; d < n_docs; d++) m32[d] = (u32)n_strings[d];
    h.lcp = ar.alloc<u32>(pyr_padded(n));
    h.ann = ar.alloc<u32>(n);
    h.doc_off = ar.alloc<u32>((size_t)n_docs + 1);
    h.n_strings = ar.alloc<u32>(n_docs);
    h.build_docs = (u32)n_docs;
    h.pyr = pyramid_layout(ar, h.lcp, n);
    // (the table's padding and the annotation start out as something no result is: the pass writes both)
    HIP_CHECK(hipMemsetAsync(h.lcp, 0x5A, (size_t)pyr_padded(n) * 4, sc.stream));
    HIP_CHECK(hipMemsetAsync(h.ann, 0xEE, (size_t)n * 4, sc.stream));
    if (lcp_words) HIP_CHECK(hipMemcpyAsync(h.lcp, lcp, (size_t)lcp_words * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(h.doc_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(h.n_strings, m32.data(), m32.size() * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));     // (the two small tables go up out of this frame)
}

// The annotation pass (build.h: annotate -- ann_stream_kernel, the upper pyramid, ann_wide_kernel) on a caller's table
static void debug_annotate(int device, const u32 *lcp, i64 n64, const i64 *doc_off, int32_t n_docs, const int32_t *n_strings,
                           u32 *ann_out, u32 *geometry_out, u32 *listed_out)
{
    if (!lcp || !doc_off || !n_strings || !ann_out || !geometry_out || !listed_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 ||
        n_docs < 1 || doc_off[0] != 0 || doc_off[n_docs] != n64)
        east_throw(EAST_HIP_ERR_INVALID, "bad annotation arguments");
    for (int32_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] <= doc_off[d]) east_throw(EAST_HIP_ERR_INVALID, "document offsets must increase");
    const u32 n = (u32)n64;
    // table, annotation, the pyramid's upper levels (a sixteenth each), the tiles' lists and counts, the document tables
    DebugScope sc(device, ((size_t)pyr_padded(n) * 2 + (size_t)n / 8 + (size_t)ceil_div_u32(n, ANN_TILE) * (ANN_TILE + 1) + 2 * (size_t)n_docs) * 4 +
                              (1u << 20));
    east_hip_index h;                   // (what annotate() reads of a handle, and no more)
    u32 *listed = sc.arena.alloc<u32>(1);
    HIP_CHECK(hipMemsetAsync(listed, 0, 4, sc.stream));
    debug_table_handle(sc, h, lcp, n, doc_off, n_docs, n_strings);
    sc.ctx.ann_whole_grid = knobs_snapshot().ann_wide_order == 2;       // (east_hip_debug_set_ann_wide_order; no build before: grouped)
    annotate(&h, sc.ctx, listed);
    HIP_CHECK(hipMemcpyAsync(ann_out, h.ann, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(listed_out, listed, 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    geometry_out[0] = ANN_TILE;
    geometry_out[1] = ANN_HALO;
    geometry_out[2] = ANN_NEAR;
}

// The child tables and the lcp-interval lefts (build.h: child_tables, interval_lefts) behind the annotation pass, on a
// caller's table: the raw device values, positions local to the document, 0 = none, NONE_U32 = no left
static void debug_child_tables(int device, const u32 *lcp, i64 n64, const i64 *doc_off, int32_t n_docs, const int32_t *n_strings,
                               u32 *up_out, u32 *down_out, u32 *next_out, u32 *left_out, u32 *geometry_out, u32 *listed_out)
{
    if (!lcp || !doc_off || !n_strings || !up_out || !down_out || !next_out || !left_out || !geometry_out || !listed_out ||
        n64 < 1 || n64 >= (i64)0x7FFFFFF0 || n_docs < 1 || doc_off[0] != 0 || doc_off[n_docs] != n64)
        east_throw(EAST_HIP_ERR_INVALID, "bad child table arguments");
    for (int32_t d = 0; d < n_docs; d++) {
        // (checked in this order: an offset is an index into lcp only once it is known to lie below n)
        if (doc_off[d + 1] <= doc_off[d] || doc_off[d + 1] > n64) east_throw(EAST_HIP_ERR_INVALID, "document offsets must increase");
        if (lcp[doc_off[d]] != 0) east_throw(EAST_HIP_ERR_INVALID, "the table must hold 0 at a document's first rank: it bounds the searches");
    }
    for (i64 k = 0; k < n64; k++)
        if (lcp[k] > 0x7FFFFFEFu) east_throw(EAST_HIP_ERR_INVALID, "a value above 0x7FFFFFEF: an LCP value is below n");
    const u32 n = (u32)n64;
    // as above + the three child tables and the lefts, and the child pass's lists and counts (behind the annotation's)
    DebugScope sc(device, ((size_t)pyr_padded(n) * 6 + (size_t)n / 8 + (size_t)ceil_div_u32(n, ANN_TILE) * (ANN_TILE + 1) +
                           (size_t)ceil_div_u32(n, CH_TILE) * (CH_TILE + 1) + 2 * (size_t)n_docs) * 4 + (1u << 20));
    Arena &ar = sc.arena;
    east_hip_index h;                   // (what annotate(), child_tables() and interval_lefts() read of a handle, and no more)
    h.up = ar.alloc<u32>(n);
    h.down = ar.alloc<u32>(n);
    h.next = ar.alloc<u32>(n);
    u32 *left = ar.alloc<u32>(n);
    for (u32 *t : {h.up, h.down, h.next, left}) HIP_CHECK(hipMemsetAsync(t, 0xEE, (size_t)n * 4, sc.stream));   // (an unwritten rank shows)
    debug_table_handle(sc, h, lcp, n, doc_off, n_docs, n_strings);
    annotate(&h, sc.ctx);
    child_tables(&h, sc.ctx, listed_out);
    for (int32_t d = 0; d < n_docs; d++)
        interval_lefts(&h, sc.ctx, (u32)doc_off[d], (u32)(doc_off[d + 1] - doc_off[d]), left + doc_off[d]);
    HIP_CHECK(hipMemcpyAsync(up_out, h.up, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(down_out, h.down, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(next_out, h.next, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(left_out, left, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    geometry_out[0] = CH_TILE;
    geometry_out[1] = CH_HALO;
    geometry_out[2] = CH_NEAR;
    geometry_out[3] = CH_LOCAL;
}

// The two LCP passes on a caller's text and per-document suffix array: the direct pass (build.h: direct_lcp -- lcp8_kernel
// on the byte stream, width 1, or lcp_kernel on u32 codes, width 4, then lcp_doc_starts_kernel) or, table_in != nullptr,
// the caller's table in its place; then finish_capped_lcp where `capped` is raised, as build_common decides, else
// annotate().  The scope is laid out as build_impl lays a handle out: the text with its pad first, the other arrays behind
// it, so that what the finishing kernels read past a position (8 192 bytes / 1 024 words) lies inside the scope; the
// whole scope starts out as pad_fill.  Every argument is checked here, before anything is launched.
static void debug_lcp(int device, int width, const void *text, i64 n64, u32 term_first, const u32 *sa, const i64 *doc_off,
                      int32_t n_docs, const int32_t *n_strings, int32_t deep_per_slot, const u32 *table_in, int pad_fill,
                      u32 *direct_out, u32 *capped_out, u32 *final_out, u32 *counters_out, u32 *ann_out, u32 *geometry_out)
{
    if ((width != 1 && width != 4) || !text || !sa || !doc_off || !n_strings || !direct_out || !capped_out || !final_out ||
        !counters_out || !ann_out || !geometry_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || n_docs < 1 || deep_per_slot < -1 ||
        pad_fill < 0 || pad_fill > 255 || doc_off[0] != 0)
        east_throw(EAST_HIP_ERR_INVALID, "bad LCP arguments");
    for (int32_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] <= doc_off[d] || doc_off[d + 1] > n64) east_throw(EAST_HIP_ERR_INVALID, "document offsets must increase");
    if (doc_off[n_docs] != n64) east_throw(EAST_HIP_ERR_INVALID, "document offsets end at n");
    const u32 n = (u32)n64;
    const uint8_t *t8 = (const uint8_t *)text;
    const u32 *t32 = (const u32 *)text;
    if (width == 4 && (term_first < 2 || term_first > 0x7FFFFFEFu - n)) east_throw(EAST_HIP_ERR_INVALID, "term_first out of range");
    // symbols in range, the terminators of u32 codes numbered apart (ascending, as the build's scan numbers them)
    u32 last_term = 0;
    for (u32 i = 0; i < n; i++) {
        if (width == 1) {
            if (t8[i] == 0) east_throw(EAST_HIP_ERR_INVALID, "a zero byte: text codes start at 1, the pad is zero");
        } else {
            const u32 c = t32[i];
            if (c == 0 || c >= term_first + n) east_throw(EAST_HIP_ERR_INVALID, "a code outside [1, term_first + n)");
            if (c >= term_first) {
                if (last_term && c <= last_term) east_throw(EAST_HIP_ERR_INVALID, "terminator codes must ascend: each is a symbol of its own");
                last_term = c;
            }
        }
    }
    std::vector<uint8_t> seen(n, 0);
    for (int32_t d = 0; d < n_docs; d++) {
        const u32 lo = (u32)doc_off[d], hi = (u32)doc_off[d + 1];
        const bool ends = width == 1 ? t8[hi - 1] == 0xFFu : t32[hi - 1] >= term_first;
        if (!ends) east_throw(EAST_HIP_ERR_INVALID, "a document does not end in a terminator");
        i64 terms = 0;
        for (u32 i = lo; i < hi; i++) terms += width == 1 ? t8[i] == 0xFFu : t32[i] >= term_first;
        if (n_strings[d] < 1 || terms != n_strings[d]) east_throw(EAST_HIP_ERR_INVALID, "n_strings is not the number of a document's terminators");
        for (u32 r = lo; r < hi; r++) {
            const u32 p = sa[r];
            if (p < lo || p >= hi || seen[p]) east_throw(EAST_HIP_ERR_INVALID, "the suffix array is no permutation of a document's range");
            seen[p] = 1;
        }
    }
    u32 capped_in = 0;
    if (table_in) {
        for (int32_t d = 0; d < n_docs; d++)
            if (table_in[doc_off[d]] & LCP_PARTIAL_BIT) east_throw(EAST_HIP_ERR_INVALID, "an unfinished entry at a document's first rank");
        for (u32 r = 1; r < n; r++) {
            if (!(table_in[r] & LCP_PARTIAL_BIT)) continue;
            capped_in = 1;
            const u32 k = table_in[r] & ~LCP_PARTIAL_BIT, later = std::max(sa[r], sa[r - 1]);
            if (k > n - later) east_throw(EAST_HIP_ERR_INVALID, "an unfinished entry claims more than is left behind its suffixes");
        }
    }
    const u32 padded = pyr_padded(n);
    // text, suffix array, table, annotation, pyramid; rank, count, apos and the two lists of the finishing pass; the
    // annotation pass's lists; and room behind everything for the look-ahead of a comparison at the stream's end
    DebugScope sc(device, (size_t)n * 4 * 14 + 2 * (size_t)n_docs * 4 + (4u << 20));
    Arena &ar = sc.arena;
    HIP_CHECK(hipMemsetAsync(ar.base, pad_fill, ar.cap, sc.stream));
    east_hip_index h;                   // (what direct_lcp() and finish_capped_lcp() read of a handle, and no more)
    h.use_s8 = width == 1;
    if (h.use_s8) {
        h.s8 = ar.alloc<uint8_t>((size_t)n + 64);
        HIP_CHECK(hipMemsetAsync(h.s8 + n, 0, 16, sc.stream));
        HIP_CHECK(hipMemcpyAsync(h.s8, text, n, hipMemcpyHostToDevice, sc.stream));
    } else {
        h.s = ar.alloc<u32>((size_t)n + 3);
        HIP_CHECK(hipMemsetAsync(h.s + n, 0, 12, sc.stream));
        HIP_CHECK(hipMemcpyAsync(h.s, text, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    }
    h.sa = ar.alloc<u32>(n);
    HIP_CHECK(hipMemcpyAsync(h.sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    std::vector<u32> start(padded, NONE_U32);          // (mode B: the padding as the direct pass leaves it)
    if (table_in) memcpy(start.data(), table_in, (size_t)n * 4);
    debug_table_handle(sc, h, start.data(), n, doc_off, n_docs, n_strings, table_in ? padded : 0u);
    u32 *words = ar.alloc<u32>(3 + LCP_BUDGET_SLOTS);   // capped, the two counters, the budget's slots
    u32 *capped = words, *counters = words + 1;
    HIP_CHECK(hipMemsetAsync(words, 0, (3 + LCP_BUDGET_SLOTS) * 4, sc.stream));
    if (table_in) {
        HIP_CHECK(hipMemcpyAsync(capped, &capped_in, 4, hipMemcpyHostToDevice, sc.stream));
        if (n_docs > 1)
            LAUNCH(sc.ctx, lcp_doc_starts_kernel, ceil_div_u32(n_docs, BLOCK), (const u32 *)h.doc_off, (u32)n_docs, h.lcp);
    } else {
        sc.ctx.lcp_budget.slots = deep_per_slot < 0 ? nullptr : words + 3;
        sc.ctx.lcp_budget.per_slot = deep_per_slot < 0 ? 0u : (u32)deep_per_slot;
        direct_lcp(&h, sc.ctx, n, (u32)n_docs, false, capped);
    }
    HIP_CHECK(hipMemcpyAsync(direct_out, h.lcp, (size_t)padded * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(capped_out, capped, 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    if (*capped_out) finish_capped_lcp(&h, sc.ctx, counters);
    else annotate(&h, sc.ctx);
    HIP_CHECK(hipMemcpyAsync(final_out, h.lcp, (size_t)padded * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(counters_out, counters, 8, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(ann_out, h.ann, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    geometry_out[0] = LCP_SOFT_CAP;
    geometry_out[1] = LCP_DIRECT_CAP;
    geometry_out[2] = LCP_BUDGET_SLOTS;
    geometry_out[3] = PHI_WAVE_STEPS * WAVE;
    geometry_out[4] = PHI_LONG_THREADS;
    geometry_out[5] = PYR_FAN;
}

// ---- radix sort, spine and scans in every form the library uses them in --------------------------------------------------
// Every output lies in the arena with DBG_GUARD elements behind it, both filled with 0xEE before the run and both copied
// back: a slot the kernels left out and a write behind the end show on the host.
#define DBG_GUARD EAST_HIP_DEBUG_GUARD
static_assert(DBG_GUARD >= RS_TILE && DBG_GUARD >= SCAN_TILE, "a guard of a tile or more");

static void debug_sort_scan_geometry(u32 *geometry_out)
{
    geometry_out[0] = RS_TILE;
    geometry_out[1] = RS_GROUP;
    geometry_out[2] = RS_TOTAL_SHARDS;
    geometry_out[3] = RS_SPINE_DOC_GROUPS;
    geometry_out[4] = RS_SPINE_PARTS * RS_SPINE_HELD;
    geometry_out[5] = SCAN_TILE;
    geometry_out[6] = SCAN_RAW_TILES;
    geometry_out[7] = DBG_GUARD;
    geometry_out[8] = RS_SPINE_PARTS;
}

// n words (and the guard behind them) of the arena, filled with 0xEE
template <class T> static T *debug_guarded(DebugScope &sc, size_t n)
{
    T *p = sc.arena.alloc<T>(n + DBG_GUARD);
    HIP_CHECK(hipMemsetAsync(p, 0xEE, (n + DBG_GUARD) * sizeof(T), sc.stream));
    return p;
}

static void debug_check_offsets(const i64 *doc_off, int32_t n_docs, i64 n)
{
    if (n_docs < 0 || n_docs > (int32_t)RS_SEG_MAX_DOCS) east_throw(EAST_HIP_ERR_INVALID, "more documents than a segmented sort takes");
    if (!n_docs) return;
    if (!doc_off || doc_off[0] != 0) east_throw(EAST_HIP_ERR_INVALID, "document offsets start at 0");
    for (int32_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] <= doc_off[d] || doc_off[d + 1] > n) east_throw(EAST_HIP_ERR_INVALID, "document offsets must increase");
    if (doc_off[n_docs] != n) east_throw(EAST_HIP_ERR_INVALID, "document offsets end at n");
}

// the offsets on the device, and the segments' tables made by the function the build calls (off32: the host's copy, which
// outlives the uploads)
static RsSeg debug_seg(Ctx &ctx, const i64 *doc_off, int32_t n_docs, u32 n, std::vector<u32> &off32)
{
    if (!n_docs) return RsSeg();
    u32 *d_off = ctx.arena->alloc<u32>((size_t)n_docs + 1);
    if (!ctx.dry) {
        off32.resize((size_t)n_docs + 1);
        for (int32_t d = 0; d <= n_docs; d++) off32[d] = (u32)doc_off[d];
        HIP_CHECK(hipMemcpyAsync(d_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, ctx.stream));
    }
    return rs_seg_make(ctx, d_off, off32.data(), (u32)n_docs, n, ctx.seg_host);
}

// radix_sort_pairs<K> with exactly the caller's arguments; keys / vals: n pairs in, n + DBG_GUARD elements out
template <class K>
static void debug_sort_ex(int device, K *keys, u32 *vals, i64 n64, int bits, int begin_bit, int check_from_bit, const i64 *doc_off,
                          int32_t n_docs, u32 *geometry_out)
{
    if (!keys || !vals || !geometry_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || begin_bit < 0 || bits <= begin_bit ||
        bits > (int)sizeof(K) * 8 || check_from_bit < 0)
        east_throw(EAST_HIP_ERR_INVALID, "bad radix sort arguments");
    debug_check_offsets(doc_off, n_docs, n64);
    const u32 n = (u32)n64;
    const size_t padded = (size_t)n + DBG_GUARD;
    std::vector<u32> off32;
    SortBufs<K> sb;
    int r = 0;
    auto run = [&](Ctx &ctx) {
        for (int k = 0; k < 2; k++) {
            sb.keys[k] = ctx.arena->alloc<K>(padded);
            sb.vals[k] = ctx.arena->alloc<u32>(padded);
            if (ctx.dry) continue;
            HIP_CHECK(hipMemsetAsync(sb.keys[k], 0xEE, padded * sizeof(K), ctx.stream));
            HIP_CHECK(hipMemsetAsync(sb.vals[k], 0xEE, padded * 4, ctx.stream));
        }
        if (!ctx.dry) {
            HIP_CHECK(hipMemcpyAsync(sb.keys[0], keys, (size_t)n * sizeof(K), hipMemcpyHostToDevice, ctx.stream));
            HIP_CHECK(hipMemcpyAsync(sb.vals[0], vals, (size_t)n * 4, hipMemcpyHostToDevice, ctx.stream));
        }
        const RsSeg seg = debug_seg(ctx, doc_off, n_docs, n, off32);
        r = radix_sort_pairs<K>(ctx, sb, n, bits, begin_bit, NoGen(), check_from_bit, seg);
    };
    // (the arena is measured with the same code, then the sort runs in it)
    SizingRun dry;
    run(dry.ctx);
    DebugScope sc(device, dry.arena.high + (8u << 20));
    run(sc.ctx);
    // (a write behind the end of the pair of buffers the result is not in shows in the result's guard as well)
    std::vector<K> gk(DBG_GUARD);
    std::vector<u32> gv(DBG_GUARD);
    HIP_CHECK(hipMemcpyAsync(keys, sb.keys[r], padded * sizeof(K), hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(vals, sb.vals[r], padded * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(gk.data(), sb.keys[r ^ 1] + n, DBG_GUARD * sizeof(K), hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(gv.data(), sb.vals[r ^ 1] + n, DBG_GUARD * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    K untouched;
    memset(&untouched, 0xEE, sizeof(K));
    for (u32 i = 0; i < DBG_GUARD; i++) {
        if (gk[i] != untouched) keys[n + i] = gk[i];
        if (gv[i] != 0xEEEEEEEEu) vals[n + i] = gv[i];
    }
    debug_sort_scan_geometry(geometry_out);
}

// The spine step of one radix pass (radix_sort.h: radix_spine) on the caller's group sums and digit totals.  Segmented:
// the documents' groups follow from doc_off as in a sort, n_groups must be their number; the totals are a row per
// document and shard.  group_prefix_out: n_groups rows + DBG_GUARD words, next_total_out: as many rows as digit_total
// holds + DBG_GUARD words.
static void debug_spine(int device, const u32 *group_sum, i64 n_groups64, const u32 *digit_total, const i64 *doc_off, int32_t n_docs,
                        u32 *group_prefix_out, u32 *next_total_out, u32 *geometry_out)
{
    if (!group_sum || !digit_total || !group_prefix_out || !next_total_out || !geometry_out || n_groups64 < 1 || n_groups64 > ((i64)1 << 20) ||
        n_docs < 0 || n_docs > (int32_t)RS_SEG_MAX_DOCS || (n_docs && !doc_off))
        east_throw(EAST_HIP_ERR_INVALID, "bad spine arguments");
    const i64 n64 = n_docs ? doc_off[n_docs] : 1;       // (one segment: the spine does not ask for the number of pairs)
    if (n64 < 1 || n64 >= (i64)0x7FFFFFF0) east_throw(EAST_HIP_ERR_INVALID, "bad spine arguments");
    debug_check_offsets(doc_off, n_docs, n64);
    const u32 n_groups = (u32)n_groups64, shards = (u32)n_docs < RS_TOTAL_SHARDS ? RS_TOTAL_SHARDS : 1;
    if (n_docs) {
        i64 g = 0;
        for (int32_t d = 0; d < n_docs; d++) g += rs_doc_groups((u32)(doc_off[d + 1] - doc_off[d]));
        if (g != n_groups64) east_throw(EAST_HIP_ERR_INVALID, "n_groups is not the number of the documents' groups");
    }
    const size_t sum_words = (size_t)n_groups * RS_BINS, total_words = (size_t)(n_docs ? (u32)n_docs * shards : RS_TOTAL_SHARDS) * RS_BINS;
    DebugScope sc(device, (2 * (sum_words + total_words + DBG_GUARD) + 3 * ((size_t)n_docs + 64) + n_groups) * 4 + (1u << 20));
    u32 *d_sum = sc.arena.alloc<u32>(sum_words), *d_total = sc.arena.alloc<u32>(total_words);
    u32 *d_prefix = debug_guarded<u32>(sc, sum_words), *d_next = debug_guarded<u32>(sc, total_words);
    HIP_CHECK(hipMemcpyAsync(d_sum, group_sum, sum_words * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(d_total, digit_total, total_words * 4, hipMemcpyHostToDevice, sc.stream));
    std::vector<u32> off32;
    const RsSeg seg = debug_seg(sc.ctx, doc_off, n_docs, (u32)n64, off32);
    radix_spine(sc.ctx, d_sum, n_groups, d_total, d_next, d_prefix, seg);
    HIP_CHECK(hipMemcpyAsync(group_prefix_out, d_prefix, (sum_words + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(next_total_out, d_next, (total_words + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    debug_sort_scan_geometry(geometry_out);
}

// device_scan in the forms of include/east_hip.h (EAST_HIP_SCAN_*); out: n words (n + 1 with the total) + DBG_GUARD
static void debug_scan_ex(int device, int form, const u32 *in, i64 n64, u32 *out, u32 *geometry_out)
{
    if (!in || !out || !geometry_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || form < EAST_HIP_SCAN_EXCLUSIVE || form > EAST_HIP_SCAN_WITH_TOTAL)
        east_throw(EAST_HIP_ERR_INVALID, "bad scan arguments");
    const u32 n = (u32)n64;
    const size_t n_out = (size_t)n + (form == EAST_HIP_SCAN_WITH_TOTAL ? 1 : 0);
    const bool in_place = form == EAST_HIP_SCAN_EXCLUSIVE_IN_PLACE || form == EAST_HIP_SCAN_INCLUSIVE_IN_PLACE;
    DebugScope sc(device, ((size_t)n * 2 + DBG_GUARD + ceil_div_u32(n_out, SCAN_TILE) * 2) * 4 + (8u << 20));
    u32 *d_out = debug_guarded<u32>(sc, n_out), *d_in = in_place ? d_out : sc.arena.alloc<u32>(n);
    HIP_CHECK(hipMemcpyAsync(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    if (form == EAST_HIP_SCAN_WITH_TOTAL) device_scan_with_total(sc.ctx, ArrIn{d_in}, n, d_out);
    else if (form == EAST_HIP_SCAN_INCLUSIVE || form == EAST_HIP_SCAN_INCLUSIVE_IN_PLACE) device_scan<ArrIn, true>(sc.ctx, ArrIn{d_in}, n, d_out);
    else device_scan<ArrIn, false>(sc.ctx, ArrIn{d_in}, n, d_out);
    HIP_CHECK(hipMemcpyAsync(out, d_out, (n_out + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    debug_sort_scan_geometry(geometry_out);
}

// The heads of the runs of sorted 64-bit keys above `shift` (scan.h: RunHeadIn): their inclusive scan, n + DBG_GUARD words,
// and their number as device_scan_count returns it
static void debug_run_heads(int device, const u64 *keys, i64 n64, int shift, u32 *inclusive_out, u32 *count_out)
{
    if (!keys || !inclusive_out || !count_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || shift < 0 || shift > 63)
        east_throw(EAST_HIP_ERR_INVALID, "bad run head arguments");
    const u32 n = (u32)n64;
    DebugScope sc(device, ((size_t)n * 4 + 2 * DBG_GUARD + ceil_div_u32((u64)n + 1, SCAN_TILE) * 2) * 4 + (8u << 20));
    u64 *d_keys = sc.arena.alloc<u64>(n);
    u32 *d_inc = debug_guarded<u32>(sc, n), *d_exc = debug_guarded<u32>(sc, (size_t)n + 1);
    HIP_CHECK(hipMemcpyAsync(d_keys, keys, (size_t)n * 8, hipMemcpyHostToDevice, sc.stream));
    const RunHeadIn<u64> heads{d_keys, shift};
    device_scan<RunHeadIn<u64>, true>(sc.ctx, heads, n, d_inc);
    const u32 count = device_scan_count(sc.ctx, heads, n, d_exc);
    std::vector<u32> behind(DBG_GUARD);
    HIP_CHECK(hipMemcpyAsync(inclusive_out, d_inc, ((size_t)n + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(behind.data(), d_exc + n + 1, DBG_GUARD * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    for (u32 v : behind)
        if (v != 0xEEEEEEEEu) east_throw(EAST_HIP_ERR_INTERNAL, "the counting scan wrote behind its n + 1 words");
    *count_out = count;
}

// device_scan_pair_bounded with the bound in a word of the device; out_a / out_b: n + DBG_GUARD words each
static void debug_scan_pair_bounded(int device, const u32 *a, const u32 *b, i64 n64, u32 n_dev_value, u32 extra, u32 *out_a, u32 *out_b)
{
    if (!a || !b || !out_a || !out_b || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || (u64)n_dev_value + extra > 0xFFFFFFFFull)
        east_throw(EAST_HIP_ERR_INVALID, "bad bounded scan arguments");
    const u32 n = (u32)n64;
    DebugScope sc(device, ((size_t)n * 4 + 2 * DBG_GUARD + ceil_div_u32(n, SCAN_TILE) * 2 + 64) * 4 + (8u << 20));
    u32 *d_a = sc.arena.alloc<u32>(n), *d_b = sc.arena.alloc<u32>(n), *d_n = sc.arena.alloc<u32>(1);
    u32 *d_out_a = debug_guarded<u32>(sc, n), *d_out_b = debug_guarded<u32>(sc, n);
    HIP_CHECK(hipMemcpyAsync(d_a, a, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(d_b, b, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    HIP_CHECK(hipMemcpyAsync(d_n, &n_dev_value, 4, hipMemcpyHostToDevice, sc.stream));
    device_scan_pair_bounded(sc.ctx, d_a, d_b, n, d_n, extra, d_out_a, d_out_b);
    HIP_CHECK(hipMemcpyAsync(out_a, d_out_a, ((size_t)n + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(out_b, d_out_b, ((size_t)n + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
}

// ascending_offsets_kernel as the consumers launch it; off_out: n_values + 1 + DBG_GUARD words
static void debug_ascending_offsets(int device, const u32 *sorted, i64 n64, i64 n_values64, u32 *off_out)
{
    if (!sorted || !off_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 || n_values64 < 0 || n_values64 >= (i64)0x7FFFFFF0)
        east_throw(EAST_HIP_ERR_INVALID, "bad offsets arguments");
    const u32 n = (u32)n64, n_values = (u32)n_values64;
    DebugScope sc(device, ((size_t)n + n_values + 1 + DBG_GUARD) * 4 + (1u << 20));
    u32 *d_sorted = sc.arena.alloc<u32>(n), *d_off = debug_guarded<u32>(sc, (size_t)n_values + 1);
    HIP_CHECK(hipMemcpyAsync(d_sorted, sorted, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
    LAUNCH(sc.ctx, ascending_offsets_kernel, ceil_div_u32((u64)n_values + 1, BLOCK), (const u32 *)d_sorted, n, n_values, d_off);
    HIP_CHECK(hipMemcpyAsync(off_out, d_off, ((size_t)n_values + 1 + DBG_GUARD) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
}

// dc3_suffix_array exactly as build_impl calls it, on a caller's text in one of the three forms a build uses: (0) plain u32
// symbols -- every recursion level --, (1) u32 codes with term_first > 0 -- level 0 of wide-alphabet text --, (2) the byte
// stream -- level 0 in sample mode, the 16-byte records, the merge that also writes the LCP table.  The scope is laid out
// as a handle is: the u32 stream with its three zero words, the byte stream with 16 zero bytes of a 64-byte tail, the two
// outputs behind them, each with its guard; the whole scope starts out as pad_fill.  In form 2 the u32 stream is there and
// holds pad_fill: dc3_suffix_array does not read it, and a read would show as a wrong answer.  Every argument is checked
// here, before anything is launched.
static void debug_suffix_array_ex(int device, int form, const void *text, i64 n64, u32 sigma, u32 term_first, i64 rank_bucket_bytes,
                                  int lean, int want_lcp, int32_t deep_per_slot, int pad_fill, u32 *sa_out, u32 *lcp_out,
                                  u32 *capped_out, i64 *info_out, u32 *geometry_out)
{
    if (form < 0 || form > 2 || !text || !sa_out || !capped_out || !info_out || !geometry_out || n64 < 1 || n64 >= (i64)0x7FFFFFF0 ||
        sigma < 1 || rank_bucket_bytes < -1 || (lean != 0 && lean != 1) || (want_lcp != 0 && want_lcp != 1) || deep_per_slot < -1 ||
        pad_fill < 0 || pad_fill > 255)
        east_throw(EAST_HIP_ERR_INVALID, "bad suffix array arguments");
    if (want_lcp && form != 2) east_throw(EAST_HIP_ERR_INVALID, "the LCP table comes out of the byte form's merge only");
    if (want_lcp && !lcp_out) east_throw(EAST_HIP_ERR_INVALID, "bad suffix array arguments");
    const u32 n = (u32)n64;
    const uint8_t *t8 = (const uint8_t *)text;
    const u32 *t32 = (const u32 *)text;
    if (form == 0 && term_first != 0) east_throw(EAST_HIP_ERR_INVALID, "term_first belongs to forms 1 and 2");
    // (form 1: the level-0 keys hold three symbols of bit_width(term_first) bits in 64: at most 21 bits each)
    if (form == 1 && (term_first < 2 || term_first >= (1u << 21))) east_throw(EAST_HIP_ERR_INVALID, "term_first out of range");
    if (form == 2 && (term_first < 2 || term_first > 255)) east_throw(EAST_HIP_ERR_INVALID, "term_first out of range");
    u32 last_term = 0;
    u64 terms = 0;
    for (u32 i = 0; i < n; i++) {
        if (form == 0) {
            if (t32[i] < 1 || t32[i] > sigma) east_throw(EAST_HIP_ERR_INVALID, "symbol outside [1, sigma]");
        } else if (form == 1) {
            const u32 c = t32[i];
            if (c == 0 || c >= term_first + n) east_throw(EAST_HIP_ERR_INVALID, "a code outside [1, term_first + n)");
            if (c >= term_first) {
                if (last_term && c <= last_term) east_throw(EAST_HIP_ERR_INVALID, "terminator codes must ascend: each is a symbol of its own");
                last_term = c;
                terms++;
            }
        } else {
            if (t8[i] == 0) east_throw(EAST_HIP_ERR_INVALID, "a zero byte: text codes start at 1, the pad is zero");
            if (t8[i] >= term_first && t8[i] != 0xFFu) east_throw(EAST_HIP_ERR_INVALID, "a byte that is neither a text code nor 0xFF");
            terms += t8[i] == 0xFFu;
        }
    }
    if (form != 0) {
        if (!(form == 1 ? t32[n - 1] >= term_first : t8[n - 1] == 0xFFu)) east_throw(EAST_HIP_ERR_INVALID, "the text does not end in a terminator");
        if ((u64)sigma != (u64)term_first - 1 + terms) east_throw(EAST_HIP_ERR_INVALID, "sigma is not term_first - 1 + the number of terminators");
    }
    const size_t guard = DBG_GUARD;
    u32 *s = nullptr, *sa = nullptr, *lcp = nullptr, *words = nullptr;
    uint8_t *s8 = nullptr;
    int levels = 0;
    auto run = [&](Ctx &ctx) {
        Arena &ar = *ctx.arena;
        s = ar.alloc<u32>((size_t)n + 3);
        s8 = ar.alloc<uint8_t>((size_t)n + 64);
        sa = ar.alloc<u32>(n + guard);
        lcp = ar.alloc<u32>(n + guard);
        words = ar.alloc<u32>(1 + LCP_BUDGET_SLOTS);        // capped, the budget's slots
        ctx.lean = lean != 0;
        if (rank_bucket_bytes >= 0) ctx.knobs.rank_bucket_bytes = (size_t)rank_bucket_bytes;
        if (ctx.dry) {                                      // (priced as build_impl's sizing run prices it: no byte stream yet)
            dc3_suffix_array(ctx, nullptr, n, std::max(n, sigma), nullptr, 0, term_first);
            return;
        }
        HIP_CHECK(hipMemsetAsync(ar.base, pad_fill, ar.cap, ctx.stream));
        HIP_CHECK(hipMemsetAsync(sa, 0xEE, (n + guard) * 4, ctx.stream));
        HIP_CHECK(hipMemsetAsync(lcp, 0xEE, (n + guard) * 4, ctx.stream));
        HIP_CHECK(hipMemsetAsync(words, 0, (1 + LCP_BUDGET_SLOTS) * 4, ctx.stream));
        if (form == 2) {
            HIP_CHECK(hipMemsetAsync(s8 + n, 0, 16, ctx.stream));
            HIP_CHECK(hipMemcpyAsync(s8, text, n, hipMemcpyHostToDevice, ctx.stream));
        } else {
            HIP_CHECK(hipMemsetAsync(s + n, 0, 12, ctx.stream));
            HIP_CHECK(hipMemcpyAsync(s, text, (size_t)n * 4, hipMemcpyHostToDevice, ctx.stream));
        }
        ctx.lcp_budget.slots = deep_per_slot < 0 ? nullptr : words + 1;
        ctx.lcp_budget.per_slot = deep_per_slot < 0 ? 0u : (u32)deep_per_slot;
        levels = dc3_suffix_array(ctx, s, n, sigma, sa, 0, term_first, form == 2 ? s8 : nullptr, want_lcp ? lcp : nullptr, words);
    };
    // (the arena is measured with the same code, then the sort runs in it)
    SizingRun dry;
    run(dry.ctx);
    DebugScope sc(device, dry.arena.high + (8u << 20));
    run(sc.ctx);
    HIP_CHECK(hipMemcpyAsync(sa_out, sa, (n + guard) * 4, hipMemcpyDeviceToHost, sc.stream));
    if (lcp_out) HIP_CHECK(hipMemcpyAsync(lcp_out, lcp, (n + guard) * 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipMemcpyAsync(capped_out, words, 4, hipMemcpyDeviceToHost, sc.stream));
    HIP_CHECK(hipStreamSynchronize(sc.stream));
    info_out[0] = levels;
    info_out[1] = sc.stats.levels_resolved;
    info_out[2] = sc.stats.refine_rounds;
    info_out[3] = sc.stats.radix_passes_u32;
    info_out[4] = sc.stats.radix_passes_u64;
    info_out[5] = sc.stats.merge_elems;
    geometry_out[0] = MERGE_TILE;
    geometry_out[1] = RESOLVE_MAX_GROUP;
    geometry_out[2] = RESOLVE_MAX_LEN;
    geometry_out[3] = LCP_SOFT_CAP;
    geometry_out[4] = LCP_DIRECT_CAP;
    geometry_out[5] = LCP_BUDGET_SLOTS;
    geometry_out[6] = DBG_GUARD;
}

extern "C" {

int east_hip_debug_set_rank_bucket_bytes(int64_t bytes)
{
    if (bytes < 0) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.rank_bucket_bytes = (size_t)bytes; k.plan_epoch++; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_window_sort(int enabled)
{
    // 0: DC3 only; 1: the default; 2: lean (no refinement rounds); 3: 64-bit window keys; 4 / 5: as 1 / 3 without the
    // fused finish (every radix pass global, then lvl0_place_kernel)
    knobs_update([&](Knobs &k) {
    k.window_sort = enabled != 0;
    k.force_lean = enabled == 2;
    k.force_wide_keys = enabled == 3 || enabled == 5;
    k.fused_finish = enabled != 4 && enabled != 5 && enabled != 9 && getenv("EAST_HIP_NO_FUSED_FINISH") == nullptr;
    k.force_fused = enabled == 6 || getenv("EAST_HIP_FORCE_FUSED") != nullptr;                        // 6: as 1, the fused finish whatever the plan says (skewed text through it)
    // 7: as 1, first-level keys of variable-length code words wherever a code can be made (ht_code.h); 9: the same
    // without the fused finish; 8: as 1 without such keys
    k.ht_mode = enabled == 7 || enabled == 9 ? 1 : enabled == 8 ? 0 : env_int("EAST_HIP_HT", -1);
    k.plan_epoch++;
    });
    return EAST_HIP_OK;
}

int east_hip_debug_set_segmented_sort(int mode)
{
    // -1: the default (by size: a few large documents); 0: never (the document number is a key digit); 1: wherever it
    // can be done (2 .. RS_SEG_MAX_DOCS documents of any size)
    knobs_update([&](Knobs &k) { k.seg_mode = mode < 0 ? env_int("EAST_HIP_SEG", -1) : (mode != 0); k.plan_epoch++; });
    return EAST_HIP_OK;
}

int east_hip_debug_alphabetic_code(const uint64_t *weights, int32_t n, uint32_t *code, int32_t *len)
{
    // host only: the order-preserving variable-length code of csrc/ht_code.h for n symbols with the given weights
    if (!weights || !code || !len || n < 1) return EAST_HIP_ERR_INVALID;
    std::vector<u64> w(weights, weights + n);
    std::vector<u32> c;
    std::vector<int> l;
    if (!ht_build_code(w, c, l)) return EAST_HIP_ERR_DOMAIN;
    for (int i = 0; i < n; i++) { code[i] = c[i]; len[i] = l[i]; }
    return EAST_HIP_OK;
}

int east_hip_debug_narrow_symbols(const uint32_t *symbols, int64_t n, uint16_t *out, int vector)
{
    // host only: what upload_symbols_narrow's host threads do to a stretch of symbols on its way into the pinned ring
    // (vector != 0: the AVX2 form where the CPU has it; 0: the plain loop)
    if (!symbols || !out || n < 0) return EAST_HIP_ERR_INVALID;
    if (vector) narrow_symbols(symbols, out, (size_t)n);
    else
        for (int64_t i = 0; i < n; i++) out[i] = symbols[i] < TEXT_SYMBOLS ? (uint16_t)symbols[i] : (uint16_t)SYM_TERMINATOR16;
    return vector && g_have_avx2 ? 1 : EAST_HIP_OK;
}

int east_hip_debug_narrow_symbols8(const uint32_t *symbols, int64_t n, uint8_t *out, int vector)
{
    // host only, as above: the narrowing to bytes.  Returns 1 when every symbol fitted (text below 0xFF, terminators from
    // U+0A00 on), 0 when one did not, + 2 when the AVX2 form ran
    if (!symbols || !out || n < 0) return EAST_HIP_ERR_INVALID;
    bool ok = true;
    if (vector) ok = narrow_symbols8(symbols, out, (size_t)n);
    else
        for (int64_t i = 0; i < n; i++) { const u32 c = symbols[i]; ok &= !(c >= 0xFFu && c < TEXT_SYMBOLS); out[i] = c < 0xFFu ? (uint8_t)c : (uint8_t)0xFFu; }
    return (ok ? 1 : 0) + (vector && g_have_avx2 ? 2 : 0);
}

int east_hip_debug_set_lds_rounds(int enabled)
{
    // 0: every round through the global sort; 1: the default (in-LDS rounds that also classify the next domain, small
    // domains finished by one persistent launch); 2: in-LDS rounds with the stand-alone classification pass, launch by
    // launch; 3: as 1, launch by launch (no persistent kernel)
    knobs_update([&](Knobs &k) {
        k.lds_rounds = enabled != 0;
        k.fused_classify = enabled != 2 && getenv("EAST_HIP_NO_FUSED_CLASSIFY") == nullptr;
        k.persist = enabled == 1 && getenv("EAST_HIP_NO_PERSIST") == nullptr;
    });
    return EAST_HIP_OK;
}

int east_hip_debug_set_persist(int force_large, int max_workgroups)
{
    // the persistent rounds (persist_rounds.h): force_large != 0 -- the large form (tiles' state in global memory, several
    // tiles per workgroup) also where the resident form would do; max_workgroups > 0 -- a grid of at most that many
    // workgroups (0: what the device holds).  (0, 0) = the default.
    knobs_update([&](Knobs &k) {
        k.persist_force_large = force_large != 0;
        k.persist_max_wgs = max_workgroups > 0 ? max_workgroups : 0;
    });
    return EAST_HIP_OK;
}

int east_hip_debug_set_score_scratch(int64_t bytes)
{
    knobs_update([&](Knobs &k) { k.score_scratch_bytes = bytes > 0 ? (size_t)bytes : SCORE_SCRATCH_BYTES; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_score_grid(int64_t workgroups)
{
    // workgroups a launch of the score walk may have when the sums run inside it (0 or less: the default, 2^22)
    knobs_update([&](Knobs &k) { k.score_grid_blocks = workgroups > 0 ? (u64)std::min<int64_t>(workgroups, (int64_t)1 << 23) : SCORE_GRID_BLOCKS; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_text_ring(int mode, int64_t slot_bytes)
{
    // mode -1: separate texts go up through the pinned ring when there are four or more of less than 8 MiB on average
    // (and the preparation is streamed); 0: never; 1: whenever the texts lie apart.  slot_bytes: size of a ring slot
    // (0 or less: the default, 8 MiB; at most that)
    knobs_update([&](Knobs &k) {
        k.tp_ring = mode;
        k.tp_ring_slot = slot_bytes > 0 ? (size_t)std::min<int64_t>(slot_bytes, (int64_t)TP_RING_SLOT) : TP_RING_SLOT;
    });
    return EAST_HIP_OK;
}

int east_hip_debug_set_text_stream(int64_t chunk_bytes)
{
    // -1: the default (inputs of 8 MiB or more go up and are prepared in about five chunks); 0: the raw text goes up and
    // is prepared in one piece; > 0: always in chunks of about that many bytes
    knobs_update([&](Knobs &k) { k.tp_stream = chunk_bytes; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_score_path(int mode)
{
    // 1: the default; 0: the walk as rounds 1-3 ran it -- one filled k-gram table of 4-byte entries, per-suffix results in
    // HBM and a reduction kernel; 2: pair tables, separate reduction; 3: filled table, the sums inside the walk.
    // (takes effect with the next build / the next set of keyphrases)
    knobs_update([&](Knobs &k) {
        k.kg_pairs = mode == 1 || mode == 2 || mode == 4 || mode == 5;
        k.kg_pairs_forced = mode == 4;                  // 4: as 1, the pair tables also for collections of fewer than 16 documents
        k.score_fused = mode == 1 || mode == 3 || mode == 4 || mode == 5;
        k.score_endgame = mode == 5 ? 0 : 1;                 // 5: as 1, binary search down to the last suffix (no register endgame)
    });
    return EAST_HIP_OK;
}

int east_hip_debug_set_speculation(int enabled)
{
    // 0: every build waits for the alphabet and the placement counts; 1: the default; 2: as 1, the first radix pass's
    // histogram counted by a launch of its own (no presence_remap_hist_kernel)
    knobs_update([&](Knobs &k) { k.speculate = enabled != 0; k.first_hist = enabled != 2 && getenv("EAST_HIP_NO_FIRST_HIST") == nullptr; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_eager_kgram(int enabled)
{
    // 1 (default): a build with resident keyphrases finishes the k-gram tables it marked behind its flags read-back; 0: the
    // first score call does
    knobs_update([&](Knobs &k) { k.eager_kgram = enabled != 0; });
    return EAST_HIP_OK;
}

int east_hip_debug_set_ann_wide_order(int order)
{
    // ann_wide_kernel's block order: 0 by the count of the build before, 1 grouped, 2 slice-major over the whole grid
    if (order < 0 || order > 2) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.ann_wide_order = order; });
    return EAST_HIP_OK;
}

int east_hip_debug_first_pass_hist(int device, const uint32_t *symbols, int64_t n, const uint32_t *code_map, int key_bytes,
                                   int w, int b, int spare, uint32_t term_first, int shift, uint32_t mask, uint8_t *s8,
                                   uint32_t *present, uint32_t *hist, uint32_t *group_sum, uint32_t *digit_total)
{
    return guarded([&] {
        if (key_bytes == 8) debug_first_pass_hist<u64>(device, symbols, n, code_map, w, b, spare, term_first, shift, mask, s8, present, hist, group_sum, digit_total);
        else if (key_bytes == 4) debug_first_pass_hist<u32>(device, symbols, n, code_map, w, b, spare, term_first, shift, mask, s8, present, hist, group_sum, digit_total);
        else east_throw(EAST_HIP_ERR_INVALID, "key_bytes must be 4 or 8");
    });
}

int east_hip_debug_annotate(int device, const uint32_t *lcp, int64_t n, const int64_t *doc_off, int32_t n_docs,
                            const int32_t *n_strings, uint32_t *ann_out, uint32_t *geometry_out, uint32_t *listed_out)
{
    return guarded([&] { debug_annotate(device, lcp, n, doc_off, n_docs, n_strings, ann_out, geometry_out, listed_out); });
}

int east_hip_debug_child_tables(int device, const uint32_t *lcp, int64_t n, const int64_t *doc_off, int32_t n_docs,
                                const int32_t *n_strings, uint32_t *up_out, uint32_t *down_out, uint32_t *next_out,
                                uint32_t *left_out, uint32_t *geometry_out, uint32_t *listed_out)
{
    return guarded([&] {
        debug_child_tables(device, lcp, n, doc_off, n_docs, n_strings, up_out, down_out, next_out, left_out, geometry_out, listed_out);
    });
}

int east_hip_debug_lcp(int device, int width, const void *text, int64_t n, uint32_t term_first, const uint32_t *sa,
                       const int64_t *doc_off, int32_t n_docs, const int32_t *n_strings, int32_t deep_per_slot,
                       const uint32_t *table_in, int pad_fill, uint32_t *direct_out, uint32_t *capped_out, uint32_t *final_out,
                       uint32_t *counters_out, uint32_t *ann_out, uint32_t *geometry_out)
{
    return guarded([&] {
        debug_lcp(device, width, text, n, term_first, sa, doc_off, n_docs, n_strings, deep_per_slot, table_in, pad_fill, direct_out,
                  capped_out, final_out, counters_out, ann_out, geometry_out);
    });
}

int east_hip_debug_pyramid_level(east_hip_handle_t h, int32_t level, uint32_t *out, int64_t capacity, int64_t *geometry_out)
{
    return guarded([&] {
        if (!h || !geometry_out) east_throw(EAST_HIP_ERR_INVALID, "null handle or output");
        if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
        geometry_out[0] = h->pyr.levels;
        geometry_out[1] = geometry_out[2] = 0;
        if (level < 0 || level >= h->pyr.levels) return;     // (the caller learns the number of levels)
        const u32 len = h->pyr.len[level], padded = pyr_padded(len);
        geometry_out[1] = len;
        geometry_out[2] = padded;
        if (!out) return;
        if (capacity < (i64)padded) east_throw(EAST_HIP_ERR_INVALID, "the output is smaller than the padded level");
        use_device(h);
        HIP_CHECK(hipMemcpyAsync(out, h->pyr.ptr[level], (size_t)padded * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int east_hip_debug_radix_sort_u64(int device, uint64_t *keys, uint32_t *vals, int64_t n, int bits)
{
    return guarded([&] { debug_sort<u64>(device, keys, vals, n, bits); });
}

int east_hip_debug_radix_sort_u32(int device, uint32_t *keys, uint32_t *vals, int64_t n, int bits)
{
    return guarded([&] { debug_sort<u32>(device, keys, vals, n, bits); });
}

int east_hip_debug_exclusive_scan(int device, const uint32_t *in, uint32_t *out, int64_t n)
{
    return guarded([&] {
        if (n < 0 || n >= (i64)0x7FFFFFF0 || !in || !out) east_throw(EAST_HIP_ERR_INVALID, "bad scan arguments");
        if (n == 0) return;
        DebugScope sc(device, (size_t)n * 8 + (size_t)ceil_div_u32(n, SCAN_TILE) * 16 + (8u << 20));
        u32 *d_in = sc.arena.alloc<u32>(n), *d_out = sc.arena.alloc<u32>(n);
        HIP_CHECK(hipMemcpyAsync(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
        device_scan<ArrIn, false>(sc.ctx, ArrIn{d_in}, (u32)n, d_out);
        HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipStreamSynchronize(sc.stream));
    });
}

int east_hip_debug_radix_sort_ex(int device, int key_bytes, void *keys, uint32_t *vals, int64_t n, int bits, int begin_bit,
                                 int check_from_bit, const int64_t *doc_off, int32_t n_docs, uint32_t *geometry_out)
{
    return guarded([&] {
        if (key_bytes == 8) debug_sort_ex<u64>(device, (u64 *)keys, vals, n, bits, begin_bit, check_from_bit, doc_off, n_docs, geometry_out);
        else if (key_bytes == 4) debug_sort_ex<u32>(device, (u32 *)keys, vals, n, bits, begin_bit, check_from_bit, doc_off, n_docs, geometry_out);
        else east_throw(EAST_HIP_ERR_INVALID, "key_bytes must be 4 or 8");
    });
}

int east_hip_debug_radix_spine(int device, const uint32_t *group_sum, int64_t n_groups, const uint32_t *digit_total,
                               const int64_t *doc_off, int32_t n_docs, uint32_t *group_prefix_out, uint32_t *next_total_out,
                               uint32_t *geometry_out)
{
    return guarded([&] { debug_spine(device, group_sum, n_groups, digit_total, doc_off, n_docs, group_prefix_out, next_total_out, geometry_out); });
}

int east_hip_debug_scan_ex(int device, int form, const uint32_t *in, int64_t n, uint32_t *out, uint32_t *geometry_out)
{
    return guarded([&] { debug_scan_ex(device, form, in, n, out, geometry_out); });
}

int east_hip_debug_run_heads(int device, const uint64_t *keys64, int64_t n, int shift, uint32_t *inclusive_out, uint32_t *count_out)
{
    return guarded([&] { debug_run_heads(device, (const u64 *)keys64, n, shift, inclusive_out, count_out); });
}

int east_hip_debug_scan_pair_bounded(int device, const uint32_t *a, const uint32_t *b, int64_t n, uint32_t n_dev_value,
                                     uint32_t extra, uint32_t *out_a, uint32_t *out_b)
{
    return guarded([&] { debug_scan_pair_bounded(device, a, b, n, n_dev_value, extra, out_a, out_b); });
}

int east_hip_debug_ascending_offsets(int device, const uint32_t *sorted, int64_t n, int64_t n_values, uint32_t *off_out)
{
    return guarded([&] { debug_ascending_offsets(device, sorted, n, n_values, off_out); });
}

int east_hip_debug_suffix_array(int device, const uint32_t *symbols, int64_t n, uint32_t sigma, int32_t *sa_out,
                                int32_t *levels_out)
{
    return guarded([&] {
        if (n < 1 || n >= (i64)0x7FFFFFF0 || !symbols || !sa_out || sigma < 1)
            east_throw(EAST_HIP_ERR_INVALID, "bad suffix array arguments");
        for (i64 i = 0; i < n; i++)
            if (symbols[i] < 1 || symbols[i] > sigma) east_throw(EAST_HIP_ERR_INVALID, "symbol outside [1, sigma]");
        // measure the arena with the same code path, then run it
        SizingRun dry;
        (void)dry.arena.alloc<u32>((size_t)n + 3);
        (void)dry.arena.alloc<u32>(n);
        dc3_suffix_array(dry.ctx, nullptr, (u32)n, (u32)std::max<i64>(n, sigma), nullptr);
        DebugScope sc(device, dry.arena.high + (8u << 20));
        u32 *s = sc.arena.alloc<u32>((size_t)n + 3), *sa = sc.arena.alloc<u32>(n);
        HIP_CHECK(hipMemsetAsync(s + n, 0, 12, sc.stream));
        HIP_CHECK(hipMemcpyAsync(s, symbols, (size_t)n * 4, hipMemcpyHostToDevice, sc.stream));
        const int levels = dc3_suffix_array(sc.ctx, s, (u32)n, sigma, sa);
        HIP_CHECK(hipMemcpyAsync(sa_out, sa, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_CHECK(hipStreamSynchronize(sc.stream));
        if (levels_out) *levels_out = levels;
    });
}

int east_hip_debug_suffix_array_ex(int device, int form, const void *text, int64_t n, uint32_t sigma, uint32_t term_first,
                                   int64_t rank_bucket_bytes, int lean, int want_lcp, int32_t deep_per_slot, int pad_fill,
                                   uint32_t *sa_out, uint32_t *lcp_out, uint32_t *capped_out, int64_t *info_out,
                                   uint32_t *geometry_out)
{
    return guarded([&] {
        debug_suffix_array_ex(device, form, text, n, sigma, term_first, rank_bucket_bytes, lean, want_lcp, deep_per_slot, pad_fill,
                              sa_out, lcp_out, capped_out, info_out, geometry_out);
    });
}

}  // extern "C"
