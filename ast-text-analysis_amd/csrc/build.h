// build.h -- the build of the enhanced annotated suffix array: build_impl queues it (or, dry, sizes its arena),
// build_common is the driver behind every build entry point.
#pragma once
#include "dc3.h"
#include "score.h"
#include "tables.h"
#include "upload.h"
#include <chrono>

static bool kgram_reserve(east_hip_index *h, u64 bins, u32 n_docs);      // (score_host.h: the build marks the score walk's k-gram tables)
static bool kgram_finish_marked(east_hip_index *h, Ctx &ctx, u32 n_docs);   // (... and queues the launches that finish them)

// min pyramid over the LCP table and the annotation table: the streaming pass decides all but the widest
// intervals and writes pyramid levels 1 and 2 on the way, the upper levels follow, then the listed wide ones
// (listed_total != nullptr, a test's: a zeroed device word that takes the number of ranks ann_wide_kernel decided)
static void annotate(east_hip_index *h, Ctx &ctx, u32 *listed_total = nullptr)
{
    const Pyramid &pyr = h->pyr;
    const u32 n = pyr.len[0];
    Arena &ar = *ctx.arena;
    const size_t mark = ar.mark();
    const u32 n_tiles = ceil_div_u32(n, ANN_TILE);
    u32 *wide_list = ar.alloc<u32>((size_t)n_tiles * ANN_TILE);       // every tile has its own stretch
    u32 *wide_count = ar.alloc<u32>(n_tiles);
    const bool has_lvl1 = pyr.levels > 1;                // (a table of at most 16 entries has no level 1,
    const bool has_lvl2 = pyr.levels > 2;                // one of at most 256 no level 2)
    LAUNCH(ctx, ann_stream_kernel, n_tiles, pyr.ptr[0], (const u32 *)h->doc_off, (const u32 *)h->n_strings,
           h->build_docs, n, h->ann, has_lvl1 ? (u32 *)pyr.ptr[1] : (u32 *)nullptr, has_lvl1 ? pyr.len[1] : 0u,
           has_lvl1 ? pyr_padded(pyr.len[1]) : 0u, wide_list, wide_count, h->lcp,
           has_lvl2 ? (u32 *)pyr.ptr[2] : (u32 *)nullptr, has_lvl2 ? pyr.len[2] : 0u, has_lvl2 ? pyr_padded(pyr.len[2]) : 0u);
    // the levels above those two: one launch each while they are large, the top of the pyramid in a single one
    int l = 3;
    for (; l < pyr.levels && pyr.len[l] > PYR_TOP; l++)
        LAUNCH(ctx, pyramid_level_kernel, ceil_div_u32(pyr_padded(pyr.len[l]), BLOCK), pyr.ptr[l - 1], pyr.len[l],
               pyr_padded(pyr.len[l]), (u32 *)pyr.ptr[l]);
    if (l < pyr.levels) LAUNCH(ctx, pyramid_top_kernel, 1, pyr, l);
    // (the block order: ctx.ann_whole_grid -- build_common's choice from the last build's count, a test's from the knob)
    LAUNCH(ctx, ann_wide_kernel, ceil_div_u32(n_tiles, ANN_WIDE_RUN) * ANN_WIDE_SLICES, pyr, n, n_tiles, (const u32 *)wide_list,
           (const u32 *)wide_count, h->ann, listed_total ? listed_total : ctx.ann_listed, (int)ctx.ann_whole_grid);
    ar.release(mark);
}

// childtab_up / down / next_l_index of the whole shard: the streaming pass, then the ranks it listed through the pyramid
// (the lists live in the arena's temporary region).
// (listed_total != nullptr, a test's: a host word that takes the number of ranks child_wide_kernel decided -- the call
// then waits for the stream)
static void child_tables(east_hip_index *h, Ctx &ctx, u32 *listed_total = nullptr)
{
    const Pyramid &pyr = h->pyr;
    const u32 n = pyr.len[0];
    Arena &ar = *ctx.arena;
    const size_t mark = ar.mark();
    const u32 n_tiles = ceil_div_u32(n, CH_TILE);
    u32 *wide_list = ar.alloc<u32>((size_t)n_tiles * CH_TILE);        // every tile has its own stretch
    u32 *wide_count = ar.alloc<u32>(n_tiles);
    LAUNCH(ctx, child_stream_kernel, n_tiles, pyr, (const u32 *)h->doc_off, h->build_docs, n, h->up, h->down, h->next,
           wide_list, wide_count);
    LAUNCH(ctx, child_wide_kernel, ceil_div_u32(n_tiles, BLOCK / CH_WIDE_SLOTS), pyr, (const u32 *)h->doc_off,
           h->build_docs, n, n_tiles, (const u32 *)wide_list, (const u32 *)wide_count, h->up, h->down, h->next);
    if (listed_total) {
        std::vector<u32> counts(n_tiles);
        HIP_CHECK(hipMemcpyAsync(counts.data(), wide_count, (size_t)n_tiles * 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
        u64 sum = 0;
        for (u32 c : counts) sum += c;
        *listed_total = (u32)sum;
    }
    ar.release(mark);
}

// the lcp-interval lefts of the document of nd ranks from rank seg on, into left[nd] (device memory)
static void interval_lefts(east_hip_index *h, Ctx &ctx, u32 seg, u32 nd, u32 *left)
{
    LAUNCH(ctx, interval_left_kernel, ceil_div_u32(nd, BLOCK), h->pyr, (const u32 *)h->ann, seg, nd, left);
}

// symbol counts of the byte stream (the weights of the variable-length code, ht_code.h): 16 bytes per thread and step,
// per-lane-class counters in LDS
__global__ __launch_bounds__(BLOCK) void byte_hist_kernel(const uint8_t *__restrict__ s8, u32 n, u32 *__restrict__ counts)
{
    __shared__ u32 bins[4][256];
    for (int c = 0; c < 4; c++) bins[c][threadIdx.x] = 0;
    __syncthreads();
    u32 *mine = bins[threadIdx.x & 3u];
    for (u64 i = ((u64)blockIdx.x * BLOCK + threadIdx.x) * 16u; i < n; i += (u64)gridDim.x * BLOCK * 16u) {
        const uint4 x = *reinterpret_cast<const uint4 *>(s8 + i);          // (the stream is padded to 16 bytes behind n)
        const u32 wds[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (i + q < n) atomicAdd(&mine[(wds[q >> 2] >> ((q & 3) * 8)) & 0xFFu], 1u);
    }
    __syncthreads();
    const u32 t = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
    if (t) atomicAdd(&counts[threadIdx.x], t);
}

// The variable-length code of this build's text (ht_code.h), for the window sort to use if it pays: made from the symbol
// counts on a build that waits for the device anyway, taken over from the build before on a speculative one (same
// alphabet -- any alphabetic code orders correctly, a stale one is merely less compact).
static void prepare_ht_code(east_hip_index *h, Ctx &ctx, u32 n, u32 sigma_t, u32 m_total)
{
    ctx.ht_max_len = 0;
    if (ctx.dry || !h->use_s8 || !ctx.knobs.window_sort || ctx.knobs.ht_mode == 0) return;
    if (ctx.spec) {
        if (!h->ht.valid || h->ht.sigma != sigma_t) {
            // (no code from the build before.  Forced -- the tests -- the build starts over with its read-backs in place and makes one)
            if (ctx.knobs.ht_mode == 1 && sigma_t + 1 >= 8 && n >= 64) throw SpecAbort();
            return;
        }
    } else {
        h->ht.valid = false;
        // (an alphabet of at most 5 bits -- letters only -- has nothing to gain: at best a fraction of a symbol per key)
        if (sigma_t + 1 < 8 || (ctx.knobs.ht_mode != 1 && (bit_width_u32(sigma_t + 1) < 6 || n < 65536)) || n < 64) return;
        Arena &ar = *ctx.arena;
        const size_t mark = ar.mark();
        u32 *d_counts = ar.alloc<u32>(256);
        HIP_CHECK(hipMemsetAsync(d_counts, 0, 256 * sizeof(u32), ctx.stream));
        LAUNCH(ctx, byte_hist_kernel, std::min<u32>(ceil_div_u32(n, BLOCK * 16), 2048), (const uint8_t *)h->s8, n, d_counts);
        u32 h_counts[256];
        HIP_CHECK(hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(sync_stream(ctx.stream));
        ar.release(mark);
        std::vector<u64> counts(256);
        for (int c = 0; c < 256; c++) counts[c] = h_counts[c];
        std::vector<u32> enc;
        std::vector<uint16_t> dec;
        double mean_len = 0.0;
        if (!ht_make_tables(counts, sigma_t, m_total, enc, dec, &mean_len)) return;
        if (!h->ht.tab.try_ensure(256 * 4 + HT_DEC_SIZE * 2)) return;
        // (pageable host buffers: the copies are staged before the calls return)
        HIP_CHECK(hipMemcpyAsync(h->ht.tab.p, enc.data(), 256 * 4, hipMemcpyHostToDevice, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(h->ht.tab.p + 256 * 4, dec.data(), HT_DEC_SIZE * 2, hipMemcpyHostToDevice, ctx.stream));
        HIP_CHECK(sync_stream(ctx.stream));
        int longest = 0;
        for (u32 c = 0; c < 256; c++) longest = std::max(longest, (int)(enc[c] & 0xFFu));
        h->ht.valid = true;
        h->ht.sigma = sigma_t;
        h->ht.max_len = longest;
        h->ht.mean_len = mean_len;
        if (g_trace) fprintf(stderr, "[east_hip] variable-length code: %u symbols, %.2f bits per symbol on average, longest code word %d\n",
                             sigma_t + 1, mean_len, longest);
    }
    ctx.ht_enc = h->ht.tab.as<const u32>();
    ctx.ht_dec = (const uint16_t *)(h->ht.tab.p + 256 * 4);
    ctx.ht_max_len = h->ht.max_len;
    ctx.ht_mean_len = h->ht.mean_len;
}

// The direct pass over the LCP table where it did not come with the suffix array (fused_lcp): neighbouring suffixes
// compared on the byte stream or on the u32 codes, cut entries marked and `capped` raised (tables.h), then 0 at every
// document's first rank.  (build_impl and the kernel-level test entry east_hip_debug_lcp both call this.)
static void direct_lcp(east_hip_index *h, Ctx &ctx, u32 n, u32 n_docs, bool fused_lcp, u32 *capped)
{
    Arena &ar = *ctx.arena;
    const size_t mark = ar.mark();
    u32 *rank = ctx.dry ? ar.alloc<u32>(n) : nullptr;       // only allocated for real when needed
    if (fused_lcp) {
        // (the table's padding up to a multiple of 16 is written by ann_stream_kernel)
    } else if (h->use_s8) {
        LAUNCH(ctx, lcp8_kernel, ceil_div_u32(pyr_padded(n), BLOCK), (const uint8_t *)h->s8, (const u32 *)h->sa,
               n, h->lcp, capped, ctx.lcp_budget);
    } else {
        LAUNCH(ctx, lcp_kernel, ceil_div_u32(pyr_padded(n), BLOCK), (const u32 *)h->s, (const u32 *)h->sa,
               n, h->lcp, capped, ctx.lcp_budget);
    }
    if (n_docs > 1)
        LAUNCH(ctx, lcp_doc_starts_kernel, ceil_div_u32(n_docs, BLOCK), (const u32 *)h->doc_off, n_docs, h->lcp);
    (void)rank;
    ar.release(mark);
}

// The build proper.  With ctx.dry it only measures the arena high-water mark
// (worst case: widest keys, recursion to the bottom).
static void build_impl(east_hip_index *h, Ctx &ctx, const u32 *d_sym, u32 n, u32 n_docs,
                       const i64 *doc_offsets, const int32_t *n_strings, u32 spec_sigma = 0, bool tagged = false)
{
    Arena &ar = *ctx.arena;
    ar.release(0);
    // ---- persistent arrays --------------------------------------------------
    h->s = ar.alloc<u32>((size_t)n + 3);
    h->s8 = ar.alloc<uint8_t>((size_t)n + 64);           // (16 zero bytes behind the stream; comparisons look up to 32 bytes ahead)
    h->sa = ar.alloc<u32>(n);
    h->lcp = ar.alloc<u32>(pyr_padded(n));
    h->ann = ar.alloc<u32>(n);
    h->up = ar.alloc<u32>(n);
    h->down = ar.alloc<u32>(n);
    h->next = ar.alloc<u32>(n);
    h->doc_off = ar.alloc<u32>(2 * (size_t)n_docs + 1);  // (one block, n_strings behind the offsets: they go up in one copy)
    h->n_strings = h->doc_off + n_docs + 1;
    // + the flag words (FLAG_*) + the presence bitmap and its status word + the budget of deep LCP comparisons + the digit
    // totals of the first-level sort (a row set for the pass counted ahead, two for the sort): everything one fill zeroes
    constexpr size_t ZEROED_WORDS = FLAG_WORDS + PRESENT_WORDS + 1 + LCP_BUDGET_SLOTS, TOTAL_WORDS = (size_t)RS_TOTAL_SHARDS * RS_BINS;
    h->code_map = ar.alloc<u32>(TEXT_SYMBOLS + ZEROED_WORDS + 3 * TOTAL_WORDS);
    h->hi_bits = tagged ? ar.alloc<u32>(HI_WORDS) : nullptr;
    h->hi_rank = tagged ? ar.alloc<u32>(HI_WORDS) : nullptr;
    h->pyr = pyramid_layout(ar, h->lcp, n);
    h->build_docs = n_docs;

    // ---- host-side small tables ---------------------------------------------
    // the offsets, then n_strings: the device block's layout, written straight into the handle's pinned block (behind the
    // words the flags come back into; build_common has made room): no staging copy on the host.  It is queued here, in
    // front of the fill -- behind the first streaming kernel it is a dispatch of its own between two kernels, which gains
    // nothing on the 64 MiB document and costs builds of a few hundred microseconds 1 % (measured)
    u32 *const off32 = ctx.dry ? nullptr : h->pin + FLAG_WORDS;
    const size_t off32_words = 2 * (size_t)n_docs + 1;
    u32 longest_doc = ctx.dry ? n : 0;                    // (sizing run: as if one document held everything)
    if (!ctx.dry) {
        for (u32 d = 0; d <= n_docs; d++) off32[d] = (u32)doc_offsets[d];
        for (u32 d = 0; d < n_docs; d++) longest_doc = std::max(longest_doc, off32[d + 1] - off32[d]);
        for (u32 d = 0; d < n_docs; d++) off32[(size_t)n_docs + 1 + d] = (u32)n_strings[d];
        HIP_CHECK(hipMemcpyAsync(h->doc_off, off32, off32_words * 4, hipMemcpyHostToDevice, ctx.stream));
    }

    const u32 gn = ceil_div_u32(n, BLOCK);
    u32 sigma_t = TEXT_SYMBOLS - 1, m_total = n;          // dry-run worst case
    u32 sigma_hi = tagged ? HI_SYMBOLS : 0;
    u32 *flags = h->code_map + TEXT_SYMBOLS;              // flag words behind the code map
    u32 *capped = flags + FLAG_CAPPED, *status = flags + FLAG_STATUS;
    u32 *present = flags + FLAG_WORDS;                    // PRESENT_WORDS + 1 (a spare word): zeroed in the same fill
    if (!ctx.dry) HIP_CHECK(hipMemsetAsync(flags, 0, (ZEROED_WORDS + 3 * TOTAL_WORDS) * sizeof(u32), ctx.stream));
    ctx.zeroed_totals = ctx.dry ? nullptr : flags + ZEROED_WORDS + TOTAL_WORDS;
    // Speculative build of one document whose first level the build before sorted on fixed-width text keys: the remap
    // pass counts that sort's first histogram on the way (presence_remap_hist_kernel).  Its tables outlive the alphabet
    // block below; the sort takes them if it turns out to run that very pass (radix_sort_pairs), else counts itself.
    RsFirstHist first_hist;
    ctx.first_hist = nullptr;
    const FirstPassPlan fp = ctx.spec && ctx.knobs.first_hist && n_docs == 1 && !tagged ? ctx.plan.first : FirstPassPlan();
    if (ctx.dry || fp.valid) {
        first_hist.n = n;
        first_hist.n_tiles = ceil_div_u32(n, RS_TILE);
        first_hist.n_groups = ceil_div_u32(first_hist.n_tiles, RS_GROUP);
        first_hist.hist = ar.alloc<u32>((size_t)RS_BINS * first_hist.n_tiles);
        first_hist.group_sum = ar.alloc<u32>((size_t)RS_BINS * first_hist.n_groups);
        first_hist.digit_total = flags + ZEROED_WORDS;
    }
    // (deep LCP comparisons -- beyond LCP_SOFT_CAP symbols -- this build may make: n / 256, see common.h)
    ctx.lcp_budget.slots = ctx.dry ? nullptr : present + PRESENT_WORDS + 1;
    ctx.lcp_budget.per_slot = std::max<u32>(n / 256u / LCP_BUDGET_SLOTS, 4u);
    ctx.spec_out = flags + FLAG_KEEP;
    ctx.zeroed_word = ctx.dry ? nullptr : flags + FLAG_PLACE_FAIL;
    ctx.spec_fail = flags + FLAG_PLACE_FAIL;
    ctx.kg_bad = ctx.dry ? nullptr : flags + FLAG_KG_BAD;
    ctx.ann_listed = ctx.dry ? nullptr : flags + FLAG_ANN_LISTED;
    {
        // ---- alphabet, dense remap ---------------------------------------------
        const size_t mark = ar.mark();
        u32 *term_ex = ar.alloc<u32>((size_t)n + 1);      // wide-alphabet path only
        const int vec = ((uintptr_t)d_sym & 15u) == 0;
        const bool fused = ctx.spec && vec && h->guess.p;     // (the bytes come out of the same pass, through the last build's map)
        ctx.map_checked = fused && !ctx.dry;                  // (only then does the code map's kernel compare the two bitmaps)
        if (fused && fp.valid && !ctx.dry) {
            first_hist.s8 = h->s8;
            first_hist.key_bytes = fp.key_bytes; first_hist.w = fp.w; first_hist.b = fp.b; first_hist.spare = fp.spare;
            first_hist.term_first = fp.term_first; first_hist.shift = fp.shift; first_hist.mask = fp.mask;
            if (fp.key_bytes == 8)
                LAUNCH_NAMED(ctx, "presence_remap_hist_kernel", (presence_remap_hist_kernel<u64, TextWindowGen<u64>>), first_hist.n_groups,
                             d_sym, n, h->guess.as<const u32>(), present, h->s8,
                             TextWindowGen<u64>{h->s8, n, fp.w, fp.b, fp.spare, fp.term_first, DocKey()}, fp.shift, fp.mask,
                             first_hist.n_tiles, first_hist.hist, first_hist.group_sum, first_hist.digit_total);
            else
                LAUNCH_NAMED(ctx, "presence_remap_hist_kernel", (presence_remap_hist_kernel<u32, TextWindowGen<u32>>), first_hist.n_groups,
                             d_sym, n, h->guess.as<const u32>(), present, h->s8,
                             TextWindowGen<u32>{h->s8, n, fp.w, fp.b, fp.spare, fp.term_first, DocKey()}, fp.shift, fp.mask,
                             first_hist.n_tiles, first_hist.hist, first_hist.group_sum, first_hist.digit_total);
            ctx.first_hist = &first_hist;
        } else if (fused) LAUNCH(ctx, presence_remap_kernel, std::min<u32>(gn, 2048), d_sym, n, h->guess.as<const u32>(), present, h->s8);
        else LAUNCH(ctx, presence_kernel, std::min<u32>(gn, 2048), d_sym, n, vec, present);
        if (tagged) {
            if (!ctx.dry) HIP_CHECK(hipMemsetAsync(h->hi_bits, 0, HI_WORDS * 4, ctx.stream));
            LAUNCH_BLOCK(ctx, presence_hi_kernel, std::min<u32>(ceil_div_u32(n, PRESENCE_HI_THREADS), 256), PRESENCE_HI_THREADS,
                         d_sym, n, h->hi_bits, status);
            LAUNCH(ctx, hi_rank_kernel, 1, (const u32 *)h->hi_bits, h->hi_rank, flags);
        }
        // (+ every document's last symbol: one launch for the check and the code map)
        LAUNCH(ctx, validate_codemap_kernel, ceil_div_u32(n_docs, BLOCK), d_sym, (const u32 *)h->doc_off, n_docs, (u32)tagged,
               (const u32 *)present, ctx.spec ? spec_sigma : 0xFFFFFFFFu, h->code_map, flags, h->guess.as<u32>(), (int)fused);
        ctx.sample_n = 0;
        ctx.rep_n = ctx.rep_dup = 0;
        bool sample_plans = false;                          // the sample is large enough to plan the window and the fused finish from
        if (!ctx.dry && !ctx.spec && !tagged && n >= 1024u) {
            // the planning sample: the middle of the longest document (read back together with the alphabet)
            u32 dl = 0;
            for (u32 d = 1; d < n_docs; d++)
                if (off32[d + 1] - off32[d] > off32[dl + 1] - off32[dl]) dl = d;
            const u32 len = off32[dl + 1] - off32[dl], cnt = std::min<u32>(SAMPLE_N, len);
            // (many short documents: a sample of a few dozen suffixes decides nothing -- no sample, the uniform estimates.
            // A small input's sample -- 512 suffixes or more -- only answers "is this text repetitive?": the reference's
            // worst-case collection at n = 300, 30 K symbols, took 3.7 ms through the endgame's direct ordering of its
            // groups of 100 and takes 0.6 through the persistent rounds, window_sort.h)
            sample_plans = n >= 4 * SAMPLE_N && cnt >= SAMPLE_N / 4;
            if (cnt >= 512u)
                LAUNCH_BLOCK(ctx, sample_prefix_kernel, SAMPLE_MAX_L, SAMPLE_THREADS, d_sym, n, off32[dl] + (len - cnt) / 2, cnt,
                             flags + FLAG_SAMPLE);
        }
        if (!ctx.dry) {
            if (ctx.spec) {
                sigma_t = spec_sigma;                        // (checked on the device; found out at the end of the build)
            } else {
                u32 *const hf = h->pin;                       // (the pinned words the flags come back into at the end as well)
                HIP_CHECK(hipMemcpyAsync(hf, flags, FLAG_WORDS * sizeof(u32), hipMemcpyDeviceToHost, ctx.stream));
                HIP_CHECK(sync_stream(ctx.stream));
                if (hf[FLAG_STATUS] & STATUS_NO_TERMINATOR)
                    east_throw(EAST_HIP_ERR_DOMAIN, tagged ? "a document does not end in a (tagged) string terminator"
                                                           : "a document does not end in a string terminator (>= U+0A00)");
                if (hf[FLAG_STATUS] & STATUS_BAD_SYMBOL)
                    east_throw(EAST_HIP_ERR_DOMAIN, "a symbol is neither a tagged terminator nor a code point < U+110000");
                sigma_t = hf[FLAG_SIGMA];
                sigma_hi = tagged ? hf[FLAG_SIGMA_HI] : 0;
                ctx.sample_n = hf[FLAG_SAMPLE + 2 * SAMPLE_MAX_L];
                for (int l = 1; l <= SAMPLE_MAX_L; l++) {
                    ctx.sample_dup2[l] = hf[FLAG_SAMPLE + 2 * (l - 1)];
                    ctx.sample_dup4[l] = hf[FLAG_SAMPLE + 2 * (l - 1) + 1];
                }
                ctx.rep_n = ctx.sample_n;
                ctx.rep_dup = ctx.sample_dup4[SAMPLE_MAX_L];
                if (!sample_plans) ctx.sample_n = 0;          // (too small to plan from)
                if (g_trace && ctx.sample_n) {
                    fprintf(stderr, "[east_hip] sample of %u suffixes, shared prefixes (>= 2 / >= 4 of the sample) by length:", ctx.sample_n);
                    for (int l = 1; l <= SAMPLE_MAX_L; l++) fprintf(stderr, " %d: %u/%u", l, ctx.sample_dup2[l], ctx.sample_dup4[l]);
                    fprintf(stderr, "\n");
                }
            }
            m_total = 0;
            for (u32 d = 0; d < n_docs; d++) m_total += (u32)n_strings[d];     // checked after the build
            h->use_s8 = sigma_t + sigma_hi <= 254;
        }
        sigma_t += sigma_hi;                                  // one text alphabet, the high code points above the low ones
        if (sigma_hi && h->use_s8 && !ctx.dry) {
            LAUNCH(ctx, remap_hi_kernel, ceil_div_u32((u64)n + 16, BLOCK), d_sym, (const u32 *)nullptr,
                   (const u32 *)h->code_map, (const u32 *)h->hi_bits, (const u32 *)h->hi_rank, sigma_t - sigma_hi, sigma_t, n,
                   (u32 *)nullptr, h->s8);
        } else if (fused) {
            // (done)
        } else if (h->use_s8 && !ctx.dry) {
            LAUNCH(ctx, remap_bytes_kernel, ceil_div_u32((u64)n + 16, BLOCK * 16), d_sym, (const u32 *)h->code_map, n,
                   vec, h->s8);
        } else {
            // wide alphabets: dense u32 codes, terminators numbered globally by a scan
            device_scan<TermIn, false>(ctx, TermIn{d_sym, n, (u32)tagged}, n + 1, term_ex);
            if (sigma_hi)
                LAUNCH(ctx, remap_hi_kernel, ceil_div_u32((u64)n + 16, BLOCK), d_sym, (const u32 *)term_ex,
                       (const u32 *)h->code_map, (const u32 *)h->hi_bits, (const u32 *)h->hi_rank, sigma_t - sigma_hi, sigma_t, n,
                       h->s, (uint8_t *)nullptr);
            else
                LAUNCH(ctx, remap_kernel, ceil_div_u32((u64)n + 16, BLOCK), d_sym, (const u32 *)term_ex,
                       (const u32 *)h->code_map, sigma_t, n, h->s, (uint8_t *)nullptr);
        }
        ar.release(mark);
    }
    const u32 sigma = sigma_t + m_total;
    const u32 term_first = sigma_t + 1u;
    h->sigma_hi = ctx.dry ? 0u : sigma_hi;
    h->sigma_t = sigma_t;
    h->m_total = m_total;
    h->bits0 = bit_width_u32(sigma);

    // ---- suffix array of the whole shard, then partition by document -------------
    // Text first goes through the window sort over all suffixes -- with several documents the keys carry
    // the document number on top, so that every document's tables come out side by side --; DC3 is the
    // bounded-work fallback (several documents: one suffix sort of the whole shard, then a stable
    // partition by document).
    bool window_sorted = false;
    const int doc_bits = n_docs > 1 ? bit_width_u32(n_docs - 1) : 0;
    h->kg.marked = false;
    prepare_ht_code(h, ctx, n, sigma_t, m_total);
    if ((h->use_s8 || ctx.dry) && ctx.knobs.window_sort) {       // (the sizing run prices it with 64-bit keys)
        DocKey docs;
        if (n_docs > 1) { docs.doc_off = h->doc_off; docs.n_docs = n_docs; docs.bits = doc_bits; docs.h_doc_off = off32; }
        // the score walk's k-gram tables are marked off the sorted keys on the way (KgMark): as many levels
        // as a table of at most twice a document's size (and 1 GiB in all) has room for
        KgMark km;
        if (!ctx.dry && n_docs <= 65535 && !getenv("EAST_HIP_NO_KG_MARKS")) {     // (the variable: experiments -- the score side then builds its tables itself)
            km.A = sigma_t + 2;
            u64 bins = 1;
            while (km.k < KGRAM_KEYS_MAX_K && bins * km.A <= KGRAM_KEYS_MAX_BINS && bins * km.A <= 2 * ((u64)n / n_docs) + 4096 &&
                   (bins * km.A + 1) * n_docs * 8 <= ((u64)1 << 31)) {
                bins *= km.A;
                km.k++;
            }
            if (km.k > 0 && kgram_reserve(h, bins, n_docs)) {
                km.kg = h->kg.buf.as<u32>();
                km.doc_off = h->doc_off;
                km.n_docs = n_docs;
                // (the pair layout: the level above the last in a table of its own, behind the 8-byte entries)
                // (... where the score table has many columns: with a handful of long documents the 8-byte marks cost the
                // build more than the few thousand walks of a score call get back; forced by the test knob)
                if (ctx.knobs.kg_pairs && (n_docs >= 16 || ctx.knobs.kg_pairs_forced)) km.kg3 = km.kg + 2 * (size_t)(bins + 1) * n_docs;
                h->kg.kg3 = km.kg3;
                h->kg.up = km.kg3 ? km.kg3 + (size_t)(bins / km.A + 1) * n_docs : nullptr;
            } else {
                km.k = 0;
            }
        }
        window_sorted = window_suffix_sort(ctx, h->s8, n, sigma_t + 1, h->sa, h->lcp, capped, docs, longest_doc,
                                           km.k > 0 ? &km : nullptr);
        if (window_sorted && km.k > 0) {                 // (km.k is 0 if the sort did not mark: small inputs)
            h->kg.marked = true;
            h->kg.pairs = km.pairs != 0;
            h->kg.k = km.k;
            h->kg.A = km.A;
            h->kg.bins = km.bins;
        }
    }
    ctx.stats->window_sorted = window_sorted;
    if (ctx.spec && !window_sorted) throw SpecAbort();   // (DC3 is not written to survive a wrong guess of the alphabet)
    // on the byte stream the LCP table comes with the suffix array: from the window keys, or (one
    // document) out of the level-0 merge of DC3
    const bool fused_lcp = h->use_s8 && (window_sorted || n_docs == 1);
    if (window_sorted) {
        ctx.stats->levels = 0;
    } else if (n_docs == 1) {
        ctx.stats->levels = dc3_suffix_array(ctx, h->s, n, sigma, h->sa, 0, term_first, h->use_s8 ? h->s8 : nullptr,
                                             fused_lcp ? h->lcp : nullptr, capped);
    } else {
        // the suffix array of the whole shard lands in vals[0]; the partition is a stable radix sort of
        // (document, suffix) pairs whose last pass writes into h->sa (pass i reads buffers [i % 2], writes the others)
        const size_t mark_sa = ar.mark();
        SortBufs<u32> sb;
        const int last = radix_pass_count(doc_bits) & 1;
        for (int k = 0; k < 2; k++) { sb.keys[k] = ar.alloc<u32>((size_t)n + 4); sb.vals[k] = k == last ? h->sa : ar.alloc<u32>((size_t)n + 4); }
        u32 *sa_whole = sb.vals[0];
        ctx.stats->levels = dc3_suffix_array(ctx, h->s, n, sigma, sa_whole, 0, term_first, h->use_s8 ? h->s8 : nullptr);
        if (n_docs <= DOC_LDS_MAX) {
            LAUNCH(ctx, doc_keys_lds_kernel, ceil_div_u32(n, BLOCK * 4), (const u32 *)sa_whole, (const u32 *)h->doc_off, n_docs,
                   n, sb.keys[0]);
        } else {
            const int shift = std::max(0, bit_width_u32(n) - 20);
            const u32 n_coarse = (u32)(((u64)n >> shift) + 1);
            u32 *coarse = ar.alloc<u32>(n_coarse);
            LAUNCH(ctx, doc_coarse_kernel, ceil_div_u32(n_coarse, BLOCK), (const u32 *)h->doc_off, n_docs, n, shift,
                   n_coarse, coarse);
            LAUNCH(ctx, doc_keys_kernel, ceil_div_u32(n, BLOCK * 4), (const u32 *)sa_whole, (const u32 *)h->doc_off,
                   (const u32 *)coarse, shift, n, sb.keys[0]);
        }
        const int r = radix_sort_pairs<u32>(ctx, sb, n, doc_bits);
        if (sb.vals[r] != h->sa) east_throw(EAST_HIP_ERR_INTERNAL, "document partition ended in the wrong buffer");
        ar.release(mark_sa);
    }

    // n_strings against the terminators actually present (read back at the end of the build)
    if (h->use_s8)
        LAUNCH_NAMED(ctx, "validate_n_strings_kernel", (validate_n_strings_kernel<uint8_t>), ceil_div_u32(n_docs, WAVES_PER_BLOCK),
                     (const uint8_t *)h->s8, 0xFFu, (const u32 *)h->sa, (const u32 *)h->doc_off,
                     (const u32 *)h->n_strings, n_docs, status);
    else
        LAUNCH_NAMED(ctx, "validate_n_strings_kernel", (validate_n_strings_kernel<u32>), ceil_div_u32(n_docs, WAVES_PER_BLOCK),
                     (const u32 *)h->s, sigma_t + 1u, (const u32 *)h->sa, (const u32 *)h->doc_off,
                     (const u32 *)h->n_strings, n_docs, status);

    // ---- LCP, min pyramid, annotation + child tables ------------------------------
    direct_lcp(h, ctx, n, n_docs, fused_lcp, capped);
    // (comparisons that hit the cap -- a repetitive input -- are found out about at the end of the build,
    // together with the status word: build_common then finishes those ranks and redoes the two steps below)
    annotate(h, ctx);
    h->kg.built = false;
    h->child_built = false;      // childtab_up / down / next_l_index: built on first east_hip_get_tables request
}

// A repetitive input: the ranks whose direct comparison was capped are finished with the Kasai carry
// over the text (blocked, O(n + marked work)), then pyramid and annotation are built again.
// (counts_out != nullptr, a test's: two device words that take the numbers of positions listed and handed to the long kernel)
static void finish_capped_lcp(east_hip_index *h, Ctx &ctx, u32 *counts_out = nullptr)
{
    Arena &ar = *ctx.arena;
    const u32 n = h->pyr.len[0];
    const size_t mark = ar.mark();
    const u32 gn = ceil_div_u32(n, BLOCK);
    u32 *rank = ar.alloc<u32>(n), *count = ar.alloc<u32>(n), *apos = ar.alloc<u32>(n);
    u32 *list = ar.alloc<u32>(n), *long_list = ar.alloc<u32>(n), *counters = ar.alloc<u32>(2);
    uint8_t *anchor = ar.alloc<uint8_t>((size_t)n + 16);
    const void *sym = h->use_s8 ? (const void *)h->s8 : (const void *)h->s;
    HIP_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(u32), ctx.stream));
    LAUNCH(ctx, inverse_sa_kernel, gn, (const u32 *)h->sa, n, rank);
    // (tables.h, "finishing pass for unfinished LCP entries": classify, compare the irreducible positions, fill the rest)
    if (h->use_s8) {
        LAUNCH(ctx, (lcp_phi_classify_kernel<true>), gn, sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)h->lcp, n, anchor, list, counters);
        LAUNCH(ctx, (lcp_phi_compare_kernel<true>), std::min<u32>(ceil_div_u32(n, WAVES_PER_BLOCK), 8192u), sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)list,
               (const u32 *)counters, n, h->lcp, long_list, counters + 1);
        LAUNCH_BLOCK(ctx, (lcp_phi_long_kernel<true>), 512, PHI_LONG_THREADS, sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)long_list,
                     (const u32 *)(counters + 1), n, h->lcp);
    } else {
        LAUNCH(ctx, (lcp_phi_classify_kernel<false>), gn, sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)h->lcp, n, anchor, list, counters);
        LAUNCH(ctx, (lcp_phi_compare_kernel<false>), std::min<u32>(ceil_div_u32(n, WAVES_PER_BLOCK), 8192u), sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)list,
               (const u32 *)counters, n, h->lcp, long_list, counters + 1);
        LAUNCH_BLOCK(ctx, (lcp_phi_long_kernel<false>), 512, PHI_LONG_THREADS, sym, (const u32 *)h->sa, (const u32 *)rank, (const u32 *)long_list,
                     (const u32 *)(counters + 1), n, h->lcp);
    }
    if (counts_out) HIP_CHECK(hipMemcpyAsync(counts_out, counters, 2 * sizeof(u32), hipMemcpyDeviceToDevice, ctx.stream));
    device_scan<U8In, true>(ctx, U8In{anchor}, n, count);
    LAUNCH(ctx, lcp_phi_anchors_kernel, gn, (const uint8_t *)anchor, (const u32 *)count, n, apos);
    LAUNCH(ctx, lcp_phi_fill_kernel, gn, (const uint8_t *)anchor, (const u32 *)count, (const u32 *)apos, (const u32 *)rank, n, h->lcp);
    ar.release(mark);
    // (the second annotation of the build: the grouped order unless the knob says otherwise -- this table lists every rank
    // or close to it.  Its count comes on top of the first one's in the same word: build_common reads the word again and
    // takes the difference -- no fill of one word on a path that small repetitive builds take)
    ctx.ann_whole_grid = ctx.knobs.ann_wide_order == 2;
    annotate(h, ctx);
}

static size_t plan_arena_bytes(u32 n, u32 n_docs, bool lean = false, bool tagged = false, const Knobs *knobs = nullptr)
{
    // (a tagged stream is priced both ways: as the byte stream it becomes when its alphabet is small -- the window
    // sort with its rounds, which the sizing run of the widest alphabet never enters -- and as dense u32 codes)
    size_t high = 0;
    for (int t = 0; t <= (tagged ? 1 : 0); t++) {
        east_hip_index tmp;
        SizingRun dry;
        if (knobs) dry.ctx.knobs = *knobs;
        dry.ctx.lean = lean;
        build_impl(&tmp, dry.ctx, nullptr, n, n_docs, nullptr, nullptr, 0, t == 1);
        high = std::max(high, dry.arena.high + (tagged ? 2 * (size_t)HI_WORDS * 4 + 1024 : 0));
    }
    return high + (1u << 20);
}

static void ensure_arena(east_hip_index *h, size_t bytes)
{
    if (h->arena.cap >= bytes) return;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->arena.base) HIP_CHECK(hipFree(h->arena.base));
    h->arena.base = nullptr;
    h->arena.cap = 0;
    h->built = false;
    h->table_scored = false;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        char b[160];
        snprintf(b, sizeof(b), "hipMalloc of the %.2f GiB build arena failed: %s", bytes / 1073741824.0,
                 hipGetErrorString(e));
        east_throw(EAST_HIP_ERR_OOM, b);
    }
    h->arena.base = (char *)p;
    h->arena.cap = bytes;
}

// The plan of the next (speculative) build on the handle: what this build's window sort did, where it did well by it
static SortPlan next_plan(const Stats &stats, const SortPlan &did)
{
    if (!stats.window_sorted) return SortPlan();
    SortPlan plan = did;
    // (hardly anything tied behind the wide window -- another kind of text on the same handle: back to the estimate)
    if (did.wide && stats.first_n > 0 && stats.first_kept * 50 < stats.first_n) plan.wide = -1;
    // (the same for the fused finish: it handed more than a few per cent of the suffixes to the rounds, or the separate
    // placement pass left next to nothing -- another kind of text than the plan was made for: the next build decides anew)
    if (stats.first_n > 0 && ((did.fused && stats.first_kept * 20 > stats.first_n) ||
                              (!did.fused && stats.first_kept * 50 < stats.first_n)))
        plan.fused = -1;
    // (the first radix pass as this build ran it, for the next remap pass to count ahead: only while the plan it came from stands)
    if (plan.wide < 0 || plan.fused < 0) plan.first = FirstPassPlan();
    return plan;
}

static void check_build_args(i64 n_total, const i64 *doc_offsets, const int32_t *n_strings, int32_t n_docs)
{
    if (n_docs < 1 || !doc_offsets || !n_strings) east_throw(EAST_HIP_ERR_INVALID, "n_docs < 1 or null offsets");
    if (n_total < 1 || n_total >= (i64)0x7FFFFFF0) east_throw(EAST_HIP_ERR_INVALID, "n_total must be in [1, 2^31-16)");
    if (doc_offsets[0] != 0 || doc_offsets[n_docs] != n_total)
        east_throw(EAST_HIP_ERR_INVALID, "doc_offsets must start at 0 and end at n_total");
    for (int32_t d = 0; d < n_docs; d++) {
        if (doc_offsets[d + 1] <= doc_offsets[d]) east_throw(EAST_HIP_ERR_INVALID, "empty document (the reference raises EmptyStringsCollectionException)");
        if (n_strings[d] < 1 || n_strings[d] > doc_offsets[d + 1] - doc_offsets[d])
            east_throw(EAST_HIP_ERR_INVALID, "n_strings[d] must be in [1, n_d]");
    }
}

static void build_common(east_hip_index *h, const u32 *sym, bool sym_on_host, i64 n_total, const i64 *doc_offsets,
                         const int32_t *n_strings, int32_t n_docs, bool tagged)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (!sym) east_throw(EAST_HIP_ERR_INVALID, "null symbols");
    check_build_args(n_total, doc_offsets, n_strings, n_docs);
    use_device(h);
    h->built = false;
    h->table_scored = false;
    const u64 map_epoch_before = h->map_epoch++;         // (handle.h; put back below by a build that confirms the code map)
    const Knobs kn = knobs_snapshot();                   // (the test knobs of this call, from its sizing run to its last launch)
    const u32 n = (u32)n_total;
    // (host symbols of the reference encoding go up as 16-bit words where that pays: upload_symbols_narrow)
    ring_adopt(h, false);
    const bool narrow_shape = sym_on_host && !tagged && n >= SYM_NARROW_MIN && getenv("EAST_HIP_NO_SYMBOL_NARROW") == nullptr;
    if (narrow_shape && !h->ring) {
        // The first host-resident build of this size pins the ring in line (3-5 ms, once per handle) and goes up narrowed
        // already: until round 6 it took the plain copy, left the pinning to a background thread, and the call behind it
        // -- arriving while that thread was still at work -- took the plain copy again (6.9, 6.7, then 3.5 ms a call).
        ring_adopt(h, true);                                // (a background pin under way: its ring)
        (void)ring_pin_now(h);                              // (no ring: the plain copy)
    }
    const bool narrow = narrow_shape && h->ring != nullptr;
    const size_t narrow_bytes = narrow_shape ? (((size_t)n + 8) * 2 + 255) & ~(size_t)255 : 0;    // (also while the ring is still being pinned: the arena is sized once)
    const size_t staging_bytes = (sym_on_host ? ((size_t)n * 4 + 255) & ~(size_t)255 : 0) + narrow_bytes;
    if (h->sized.n != n || h->sized.docs != (u32)n_docs || h->sized.epoch != kn.plan_epoch || h->sized.tagged != tagged) {     // (the sizing run costs host time: remembered per shape)
        h->sized.bytes = plan_arena_bytes(n, (u32)n_docs, false, tagged, &kn);
        h->sized.tagged = tagged;
        h->sized.n = n;
        h->sized.docs = (u32)n_docs;
        h->sized.epoch = kn.plan_epoch;
    }
    size_t need = h->sized.bytes + staging_bytes;
    bool lean = kn.force_lean;
    if (!lean && need > h->arena.cap) {
        // the tie-refinement rounds are the largest consumer: when they do not fit next to what else
        // lives on the device, build without them (heavy ties then take the DC3 recursion)
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        lean = need > (size_t)(0.92 * (double)(free_b + h->arena.cap));
    }
    if (lean) need = plan_arena_bytes(n, (u32)n_docs, true, tagged, &kn) + staging_bytes;
    u32 *staging = nullptr;
    {
        const size_t cap_before = h->arena.cap;
        const auto t_a = std::chrono::steady_clock::now();
        ensure_arena(h, need);
        if (g_trace && h->arena.cap != cap_before)
            fprintf(stderr, "[east_hip] build: arena grown to %.2f GiB in %.2f ms\n", h->arena.cap / 1073741824.0,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_a).count());
    }
    if (sym_on_host) {   // raw symbols are staged at the top of the arena
        staging = (u32 *)(h->arena.base + (h->arena.cap - (((size_t)n * 4 + 255) & ~(size_t)255)));
        int went = 0;
        if (narrow) {
            // bytes first where the text may fit them (the first 64 Ki symbols say: word text does, Cyrillic does not); a
            // symbol that does not fit further on starts the upload over with 16-bit words, for this call and the handle's later ones
            static const bool no_bytes = getenv("EAST_HIP_NO_SYMBOL_BYTES") != nullptr;
            bool bytes = !no_bytes && !h->bytes_refused;
            for (u32 i = 0; bytes && i < std::min<u32>(n, 65536u); i++) bytes = sym[i] < 0xFFu || sym[i] >= TEXT_SYMBOLS;
            if (bytes && upload_symbols_narrow<uint8_t>(h, sym, n, staging, (uint8_t *)((char *)staging - narrow_bytes))) went = 2;
            else {
                if (bytes) h->bytes_refused = true;
                (void)upload_symbols_narrow<uint16_t>(h, sym, n, staging, (uint16_t *)((char *)staging - narrow_bytes));
                went = 1;
            }
        } else HIP_CHECK(hipMemcpyAsync(staging, sym, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        h->narrow_upload = went;
        sym = staging;
    } else h->narrow_upload = 0;
    h->stats = Stats();
    h->arena.high = 0;
    Ctx ctx = handle_ctx(h, &h->arena, &h->stats);
    ctx.knobs = kn;
    ctx.lean = lean;
    // The build is queued WITHOUT waiting for the device wherever the previous build on this handle says what
    // to expect (alphabet size, no large tie groups): one read-back at the end finds out whether it was
    // right.  If not -- or on a handle's first build -- the build runs with its read-backs in place.
    // The flags come back into the handle's pinned block (pageable memory would be staged: a copy and a blit with the
    // device idle), and the build waits for an event right behind that copy, not for the stream: where keyphrases are
    // resident, the k-gram tables the build marked are finished behind the event, while the host reads the flags and
    // returns (kgram_finish_marked, score_host.h: 11 us of launches off the score call's critical path; the same 11 us
    // stand in front of whatever comes next where no score call follows).  They read the index alone -- the caller may
    // reuse its symbol buffer as soon as the call returns -- and count as done only once the flags say the build stood.
    ensure_pin(h, FLAG_WORDS + 2 * (size_t)n_docs + 1);
    u32 *const flags = h->pin;
    std::fill_n(flags, FLAG_WORDS, 0u);
    // (other n_docs: the keyphrases go, below.  Under the library's profiler every call's report lists the launches that
    // call needed: the tables stay with the score call, and the build waits for the whole stream before it collects)
    const bool eager = kn.eager_kgram && !h->prof.enabled && h->kp.n_kp > 0 && h->n_docs == (u32)n_docs;
    bool kg_queued = false;
    auto run = [&](bool spec, bool spec_rounds) -> bool {
        ctx.spec = spec;
        ctx.spec_rounds = spec && spec_rounds;
        ctx.plan = spec ? h->plan : SortPlan();          // (a build that waits for the alphabet plans from its own sample)
        ctx.did.first = FirstPassPlan();
        // ann_wide_kernel's block order: whole-grid where the build before listed no more ranks than slice 0 of the
        // average run takes in its first stretch (BLOCK entries per ANN_WIDE_RUN tiles), else -- and without a count -- grouped
        ctx.ann_whole_grid = kn.ann_wide_order == 2 ||
                             (kn.ann_wide_order == 0 && h->ann_hint.valid &&
                              (u64)h->ann_hint.listed * ANN_WIDE_RUN <= (u64)h->ann_hint.n_tiles * ANN_WHOLE_GRID_MAX);
        h->ann_order_used = ctx.ann_whole_grid ? 2 : 1;
        kg_queued = false;
        try {
            build_impl(h, ctx, sym, n, (u32)n_docs, doc_offsets, n_strings, h->hint.sigma, tagged);
        } catch (const SpecAbort &) {
            HIP_CHECK(hipStreamSynchronize(h->stream));
            return false;
        } catch (const EastError &) {
            if (!spec) throw;                            // (whatever a wrong guess ran into: the build is repeated without guesses)
            (void)hipStreamSynchronize(h->stream);
            return false;
        }
        HIP_CHECK(hipEventRecord(h->ev1, h->stream));
        HIP_CHECK(hipMemcpyAsync(flags, h->code_map + TEXT_SYMBOLS, FLAG_WORDS * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipEventRecord(h->ev_flags, h->stream));
        // (h->kg.marked is this attempt's: build_impl resets it before anything is marked, so a repeat never queues the
        // marks of the attempt before; `eager` itself holds for both attempts -- keyphrases and n_docs do not change in between)
        if (eager) kg_queued = kgram_finish_marked(h, ctx, (u32)n_docs);
        // (the library's profiler reads its events behind the build: the whole stream then)
        HIP_CHECK(h->prof.enabled ? sync_stream(h->stream) : sync_event(h->ev_flags));
        return true;
    };
    HIP_CHECK(hipEventRecord(h->ev0, h->stream));
    // (the alphabet is guessed whenever the last build took the window sort; that no tie group is large only if it found none)
    const bool speculate = kn.speculate && kn.window_sort && h->hint.valid && h->hint.window && h->hint.sigma <= 254 && !tagged;
    const bool spec_rounds = speculate && h->hint.no_rounds;
    const bool went_through = run(speculate, spec_rounds);
    const bool repeat = speculate && (!went_through || (flags[FLAG_STATUS] & STATUS_SIGMA_GUESS) ||
                                      (spec_rounds && (flags[FLAG_KEEP] || flags[FLAG_FAIL] || flags[FLAG_PLACE_FAIL])));
    if (repeat) {
        if (g_trace) fprintf(stderr, "[east_hip] speculative build guessed wrong: building again\n");
        h->stats = Stats();
        run(false, false);
    }
    // (the presence bitmap of the build before, hence its code map -- where the two bitmaps were compared: a speculative
    // build from a symbol pointer that is not 16-byte aligned only has its alphabet SIZE checked)
    const bool map_confirmed = speculate && !repeat && ctx.map_checked;
    const u32 status = flags[FLAG_STATUS];
    if (status & STATUS_NO_TERMINATOR)
        east_throw(EAST_HIP_ERR_DOMAIN, "a document does not end in a string terminator (>= U+0A00)");
    if (flags[FLAG_CAPPED] && !(status & STATUS_N_STRINGS)) {
        const u32 listed_first = flags[FLAG_ANN_LISTED];     // (the second annotation adds its count to the same word)
        finish_capped_lcp(h, ctx);
        HIP_CHECK(hipEventRecord(h->ev1, h->stream));
        HIP_CHECK(hipMemcpyAsync(flags + FLAG_ANN_LISTED, h->code_map + TEXT_SYMBOLS + FLAG_ANN_LISTED, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        flags[FLAG_ANN_LISTED] -= listed_first;
    }
    if (status & STATUS_N_STRINGS)
        east_throw(EAST_HIP_ERR_DOMAIN, tagged ? "n_strings does not match the tagged terminators found in a document"
                                               : "n_strings does not match the terminators found in a document "
                                                 "(text symbols must be < U+0A00 unless the terminators are tagged)");
    if (flags[FLAG_KG_BAD]) h->kg.marked = false;    // (the score side then builds its k-gram tables itself)
    // (the tables queued behind the flags count only now that the build stands: a wrong guess's were overwritten by the
    // repeat's marks, incomplete marks are built over by the score side)
    h->kg.built = kg_queued && h->kg.marked;
    h->kg_queued = kg_queued ? (h->kg.marked ? 1 : 2) : 0;
    h->ann_hint.valid = true;
    h->ann_hint.listed = flags[FLAG_ANN_LISTED];
    h->ann_hint.n_tiles = ceil_div_u32(n, ANN_TILE);
    h->hint.valid = !tagged || h->sigma_hi == 0;
    h->hint.sigma = h->sigma_t;
    h->hint.window = h->stats.window_sorted != 0;
    h->plan = next_plan(h->stats, ctx.did);
    h->hint.no_rounds = h->stats.window_sorted && h->stats.refine_rounds == 0 && !h->stats.long_repeats;
    h->prof.collect();
    HIP_CHECK(hipEventElapsedTime(&h->last_build_ms, h->ev0, h->ev1));
    h->n = n;
    if (h->n_docs != (u32)n_docs) h->kp.n_kp = 0;       // resident keyphrase scratch is sized per n_docs
    h->n_docs = (u32)n_docs;
    h->h_doc_off.assign(doc_offsets, doc_offsets + n_docs + 1);
    h->h_n_strings.assign(n_strings, n_strings + n_docs);
    if (map_confirmed) h->map_epoch = map_epoch_before;
    h->built = true;
    ring_pin_later(h);
}
