// level0.h -- the host drivers of the first level of every suffix sort (the kernels they launch: window_sort.h,
// lds_group_sort.h, persist_rounds.h, radix_sort.h, scan.h):
//
//   clear_add / clear_run        several stretches of device memory preset in one launch
//   persist_capacity             what the device holds of the persistent rounds' workgroups, and their lock
//   dc3_level0_bytes             level 0 on the byte stream (all suffixes: n0 == 0; DC3's sample: n0 > 0)
//   lvl0_window                  the width of the first window
//   window_suffix_sort           construction A of dc3.h's header: the plan of the first level, and the second attempt
//                                with the full sort where the fused finish gives up
#pragma once
#include "window_sort.h"

// (a stretch the kernel cannot take -- not 16-byte aligned, no whole words, 16 GiB or more -- gets a fill of its own)
static void clear_add(Ctx &ctx, ClearRegions &r, void *p, size_t bytes, int byte_value)
{
    if (ctx.dry || !bytes) return;
    if (((uintptr_t)p & 15u) || (bytes & 3u) || (bytes >> 2) > 0xFFFFFFFFull - CLEAR_BLOCK_WORDS || r.count == CLEAR_MAX_REGIONS) {
        HIP_CHECK(hipMemsetAsync(p, byte_value, bytes, ctx.stream));
        return;
    }
    if (!r.count) r.first_block[0] = 0;
    r.p[r.count] = (u32 *)p;
    r.words[r.count] = (u32)(bytes >> 2);
    r.value[r.count] = 0x01010101u * (u32)(byte_value & 0xFF);
    r.first_block[r.count + 1] = r.first_block[r.count] + ceil_div_u32(bytes >> 2, CLEAR_BLOCK_WORDS);
    r.count++;
}
static void clear_run(Ctx &ctx, const ClearRegions &r)
{
    if (ctx.dry || !r.count) return;
    LAUNCH(ctx, clear_regions_kernel, r.first_block[r.count], r);
}

// The persistent rounds (persist_rounds.h): how many of its workgroups the device holds at once -- the launch never asks
// for more -- and the lock that keeps two such launches of one process from sharing the chip half resident each.
#define PERSIST_SMALL_INPUT ((u32)4 << 20)      // inputs whose names cost next to nothing to initialise (0.1 ms)
static std::mutex g_persist_mutex;
struct PersistCap { u32 one_per_cu = 0, large = 0; };      // workgroups resident at once: the resident form / the large form (0: not available)
static PersistCap persist_capacity()
{
    static std::mutex mu;
    static PersistCap cap[64];
    static bool asked[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return PersistCap();
    std::lock_guard<std::mutex> lock(mu);
    if (!asked[dev]) {
        asked[dev] = true;
        int per1 = 0, per3 = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per1, refine_persist_kernel<4>, LG_THREADS, 0) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per3, refine_persist2_kernel, LG_THREADS, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); per1 = per3 = 0; }
        // (one workgroup of 1 024 threads per CU: see the launch below)
        if (cus > 0 && per1 >= 1) cap[dev].one_per_cu = (u32)cus;
        if (cus > 0 && per3 >= 1) cap[dev].large = (u32)cus;
    }
    return cap[dev];
}

// Level 0 on the byte stream: the window keys are sorted, then one classify pass places everything
// that is untied or tied in a small group (ordered directly on the text); large groups go through
// refinement rounds (step 2c).  Returns true when sa12 is final (no name string is ever written);
// otherwise the refined names are scanned and scattered into s12 for the recursion (sample mode),
// or the caller falls back to DC3 (all-suffix mode, s12 == nullptr).
#define FIN_LOW_BITS 8                   // key bits the fused finish orders in LDS (one global radix pass less)
#define FIN_MAX_EXPECTED 32.0            // ... when a bucket of the top part is expected to hold at most this many suffixes
// ht != nullptr (all-suffix mode, 32-bit keys): the first-level keys are the first bits of the suffixes coded with
// variable-length code words (ht_code.h); w = the least number of whole symbols a key holds -- the depth the rounds start
// from, every position carrying what its group shares beyond it (xdep).
struct HtKeys {
    const u32 *enc = nullptr;           // device: byte -> code << 8 | length
    const uint16_t *dec = nullptr;      // device: 12 stream bits -> symbol << 8 | terminator << 7 | length
    int max_len = 0;                    // the longest code word
    int sb = 0;                         // stream bits of a key (<= HT_MAX_STREAM), under the document number
};

// ---- the driver's state, by owner ---------------------------------------------------------------
// Plain structs: they own nothing (every pointer lies in the arena or is the caller's), and each is filled by the one step
// named with it.

// The key plan of one attempt (Level0::plan_keys)
struct KeyPlan {
    int spare = 0;                      // key bits below the w full symbols: they take the top bits of symbol w + 1
    int total_bits = 0, low_bits = 0;   // the bits of a key / those of them the fused finish orders in LDS (0: no fused finish)
    int depth0 = 0;                     // the symbols wholly inside the top part: what the members of a bucket are known to share
    int w = 0;                          // the window; variable-length keys: the depth the rounds start from (what every key, or its top part, holds at least)
    int ht_sb = 0;                      // variable-length keys: the stream bits of a key
    bool fused = false, fin_small_halo = false;     // the fused finish / buckets of at most ten suffixes expected: the kernel with the halo of 32
};

// The whole sorted input as the first domain (Level0::sort_keys: sb .. sorted_vals, alloc_first: keep .. repetitive_text,
// setup_marks: km, fa)
template <class K> struct FirstDomain {
    SortBufs<K> sb;                     // the sort's buffers,
    int r = 0;                          // ... of which keys[r] / vals[r] hold the result
    KeyNeqWindowIn<K> starts;           // the naming predicate on the sorted keys
    const u32 *sorted_vals = nullptr;
    u64 *keep = nullptr;                // n02 + 1 bits: LIVES IN sb.keys[r ^ 1], idle since the sort (one spare element each: scratch after the sort)
    u32 *idx = nullptr;                 // n02 + 1 entries: LIVES IN sb.vals[r ^ 1], likewise
    u64 *gstart_bits = nullptr;         // fused finish: the first rank of every group left to the rounds
    u32 *names_g = nullptr;             // sample mode: the naming predicate as refined so far
    u32 *fail = nullptr;                // "a repeat too long to order directly"
    bool fail_is_zero = false;          // ... taken over from ctx.zeroed_word (zeroed with the build's flag words: one fill less)
    u32 gp = 0, *block_keep = nullptr;  // workgroups of the placement pass, what each of them kept
    u32 nb = 0, *block_sums = nullptr;
    u32 *bad = nullptr;                 // groups with a repeat too long to compare directly (rare)
    uint8_t *xdep0 = nullptr;           // variable-length keys: extra depth per rank
    KgMark km;                          // k-gram bucket starts ride along with the first placement pass
    FinishArgs<K> fa;
    SegRanks sr;
    // A speculative build that expects no rounds only asks "was anything kept, did the placement give up?" at its very end:
    // where `fail` already is the flag word build_common reads for the second, the workgroups that keep a suffix set the
    // first themselves and no launch has to sum their counts (otherwise: spec_counts_kernel)
    bool spec_direct = false;
    // (a small input is better off with the direct ordering of much larger groups than with a round of ~50 launches)
    bool small_input = false;
    // (repetitive text -- the sample says, or the build before did -- is not ordered directly however small it is: its tie
    // groups agree for hundreds of symbols, and every member would compare itself with every other to the end; the
    // persistent rounds take it, persist_rounds.h)
    bool repetitive_text = false;
};

// The verdict that travels between the steps: the domain's size, what the last pass left in large groups, whether it gave up
struct Verdict {
    u32 m = 0, m_next = 0, h_fail = 0;  // (sizing run: as if everything were tied)
    bool long_repeats = false;          // small groups were handed to the rounds
};

// The rounds' buffers (Level0::alloc_rounds)
struct RoundBufs {
    u32 *ebuf[3], *sbuf[2], *fbuf[2];   // the rotating buffers of a domain: elements, slots, group-start flags
    u32 *gstart = nullptr, *group = nullptr;
    // the round sort's buffers; idle until a sort runs, they also hold: keys[0] / vals[0] = name1 / ctl of the persistent launch
    // (the second copy of the names, the control words), vals[1] = sub_gstart of the rest's compaction (idle until the sort's first pass)
    SortBufs<u64> rb;
    u32 *name_of = nullptr;             // all-suffix mode: names for prefix doubling
    uint8_t *xbuf[2] = {nullptr, nullptr};      // variable-length first-level keys: what the group of a domain position shares beyond `depth` (see HtKeys)
    // the in-LDS round (lds_group_sort.h): what each workgroup took, and the compaction of the rest (sub_idx also holds its
    // elements, sub_elem).  The large form of the persistent launch keeps the second copy of the group bounds, the tiles'
    // ranges and "changed" flags in full_idx, cover and rest_cnt: buffers of the launch-by-launch rounds that are idle there.
    uint2 *cover = nullptr;
    u32 *sub_idx = nullptr, *full_idx = nullptr, *rest_cnt = nullptr, *rest_pre = nullptr;
    PersistCap persist_caps;
};

// The current domain (Level0::open_domain; Level0::advance moves on to the next)
struct Domain {
    const u32 *elem = nullptr, *slot = nullptr, *flag = nullptr;
    int e_dom = -1, s_dom = 0, f_dom = 0;   // which of the rotating buffers hold the domain
    u32 depth = 0;                      // what the members of a group are known to share
    bool doubling = false;
    int stalled = 0;                    // rounds in a row that placed (almost) nothing
    u32 persist_cap = 0;
    bool have_idx = false;              // idx = exclusive scan of keep over the domain
    bool have_x = false;                // xbuf[x_dom] describes the current domain
    int x_dom = 0;
    // the placement pass's verdict is kept: the LCP entries of everything it placed are final
    // (the ranks whose entries the rounds do NOT write -- those that go through prefix-doubling rounds, whose keys are
    // names -- are marked when the rounds switch over, and only they are computed at the end: the slots of the domain of
    // the round that switched over)
    u32 *lcp_redo = nullptr;
    u32 redo_n = 0;
    bool redo_pending = false, redo_hinted = false;
    bool lcp_from_rounds = true;        // the rounds write the LCP entries of what they place (symbol windows)
    int e_c() const { return (e_dom + 4) % 3; }         // the two buffers the domain is not in: the compacted domain,
    int e_out() const { return (e_dom + 5) % 3; }       // ... and the next one
};

// One round's own: decided at its start or between its steps
struct Round {
    int round = 0;
    bool slow = false, try_persist = false, endgame = false, fuse_cls = false;
    int gbits = 0;
    u32 gt = 0, round_left = 0;         // workgroups over the compacted domain / what the in-LDS round left to the global sort
    const uint8_t *xdep = nullptr;
};

// The call (dc3_level0_bytes' arguments), the state above, and the steps in the order they run
template <class K> struct Level0 {
    Ctx &ctx;
    Arena &ar;
    const uint8_t *const s8;
    const u32 n0, n02;
    const int bt;
    const u32 term_first;
    u32 *const sa12, *const s12, *const lcp_out, *const lcp_capped;
    DocKey docs;
    KgMark *const kg_mark;
    const HtKeys *const ht;
    KeyPlan kp; FirstDomain<K> fd; Verdict v; RoundBufs bufs; Domain dom;

    // ---- the first domain ----
    void plan_keys(int w, bool allow_fused, u32 longest)
    {
        const int ht_sb = ht ? ht->sb : 0;
        // whole passes are paid for anyway: fill the last digit with the top bits of the next symbol
        // (the document number, if any, sits above window and spare bits)
        const int spare = ht ? 0 : lvl0_spare_bits(w * bt + docs.bits, (int)sizeof(K) * 8, bt, w);
        // The fused finish (lvl0_finish_kernel): the global passes stop above the low FIN_LOW_BITS key bits.  depth0 = the
        // symbols that lie wholly inside the top part -- what the members of a bucket are known to share.
        const int total_bits = ht ? ht_sb + docs.bits : w * bt + spare + docs.bits;
        int depth0 = 0;
        for (int j = 0; j < w; j++)
            if (spare + j * bt >= FIN_LOW_BITS) depth0++;
        if (ht) depth0 = (ht_sb - FIN_LOW_BITS) / ht->max_len;          // the whole symbols any top part holds at least
        bool fused = allow_fused && ctx.knobs.fused_finish && n0 == 0 && total_bits >= 2 * FIN_LOW_BITS && depth0 >= 1;
        bool fin_small_halo = false;
        if (fused && !ctx.dry) {
            if (ctx.knobs.force_fused) {
                // (test knob: buckets of any size -- the large ones go to the rounds)
            } else if (ctx.plan.fused >= 0) {
                fused = ctx.plan.fused != 0;                 // (speculative build: as the build before)
                fin_small_halo = ctx.plan.fused == 2 && !ht;
            } else if (ht) {
                // (variable-length keys come with a wide window: few suffixes per bucket of the top part)
            } else {
                // expected members of a bucket, were the text uniform
                double top_codes = pow((double)term_first, depth0);
                const int part = (spare + (w - depth0) * bt) - FIN_LOW_BITS;   // bits of the next symbol inside the top part
                if (part > 0) top_codes *= std::max(1.0, (double)term_first / (double)(1u << (bt - part)));
                const double expected = (double)(longest ? longest : n02) / top_codes;
                fused = expected <= FIN_MAX_EXPECTED;
                fin_small_halo = expected <= 10.0;
                // skewed text behind a narrow window: many buckets would be handed to the rounds whole (measured on the
                // Zipf stand-in: 8.9 against 8.2 ms); the sample tells -- more than 1 in 20 of its suffixes sharing the
                // symbols of the top part with three others of the sample is natural language, random text has none
                if (fused && ctx.sample_n && sizeof(K) == 4)
                    fused = (u64)ctx.sample_dup4[std::min(depth0 + 1, 8)] * 20u <= ctx.sample_n;
            }
        }
        const int low_bits = fused ? FIN_LOW_BITS : 0;
        if (g_trace && n0 == 0 && !ctx.dry)
            fprintf(stderr, "[east_hip] level-0 keys: %d-bit, w = %d x %d bits + %d spare%s, %d key bits, global passes from bit %d, fused finish %d%s, "
                            "top part holds %d symbols, segmented by document %d\n", (int)sizeof(K) * 8, w, bt, spare, ht ? " (variable-length)" : "",
                    total_bits, low_bits, (int)fused, fin_small_halo ? " (halo 32)" : "", depth0, (int)(docs.seg.n_docs != 0));
        if (ht) w = fused ? depth0 : ht_sb / ht->max_len;
        if (n0 == 0) ctx.did.fused = fused ? (fin_small_halo ? 2 : 1) : 0;
        if (ctx.stats && n0 == 0) ctx.stats->fused_finish = fused;
        kp = KeyPlan{spare, total_bits, low_bits, depth0, w, ht_sb, fused, fin_small_halo};
    }

    void sort_keys()
    {
        SortBufs<K> &sb = fd.sb;
        // (8 spare entries: the placement pass reads whole 16-byte groups; >= 64 so that the idle half can hold its scratch)
        const size_t n_alloc = (size_t)(n02 > 56 ? n02 : 56) + 8;
        for (int k = 0; k < 2; k++) { sb.keys[k] = ar.alloc<K>(n_alloc); sb.vals[k] = ar.alloc<u32>(n_alloc); }
        if (docs.bits) {
            const u32 n_dt = (n02 >> DOC_TILE_SHIFT) + 1;
            u32 *tile_doc = ar.alloc<u32>(n_dt);
            LAUNCH(ctx, doc_tiles_kernel, ceil_div_u32(n_dt, BLOCK), docs.doc_off, docs.n_docs, n_dt, tile_doc);
            docs.tile_doc = tile_doc;
        }
        const int w = kp.w, spare = kp.spare, total_bits = kp.total_bits, low_bits = kp.low_bits;
        fd.r = n0 ? radix_sort_pairs<K, WindowSrc<K>>(ctx, sb, n02, total_bits, 0,
                                                      WindowSrc<K>{s8, n0, w, bt, spare, term_first, docs})
               : ht ? radix_sort_pairs<K, HtWindowGen<K>>(ctx, sb, n02, total_bits, low_bits,
                                                          HtWindowGen<K>{s8, n02, kp.ht_sb, ht->enc, docs},
                                                          docs.bits ? total_bits - docs.bits : total_bits + RS_DB, docs.seg)
                    : radix_sort_pairs<K, TextWindowGen<K>>(ctx, sb, n02, total_bits, low_bits,
                                                            TextWindowGen<K>{s8, n02, w, bt, spare, term_first, docs},
                                                            // (suffixes in text order: only the document number is sorted)
                                                            docs.bits ? total_bits - docs.bits : total_bits + RS_DB, docs.seg,
                                                            ctx.first_hist);
        if (n0 == 0 && !ctx.dry) {
            // what the next speculative build's remap pass may count ahead (build.h): the first pass of fixed-width text keys
            FirstPassPlan &fp = ctx.did.first;
            fp.valid = !ht && !docs.bits && !docs.seg.n_docs && total_bits > low_bits;
            fp.key_bytes = (int)sizeof(K); fp.w = w; fp.b = bt; fp.spare = spare; fp.term_first = term_first;
            fp.shift = low_bits; fp.mask = (1u << std::min(RS_DB, total_bits - low_bits)) - 1u;
        }
        fd.starts = KeyNeqWindowIn<K>::make(sb.keys[fd.r], ht ? 0 : w, bt, spare, term_first);
        if (ht) { fd.starts.ht_sb = kp.ht_sb; fd.starts.ht_wmin = w; fd.starts.ht_dec = ht->dec; }
        fd.sorted_vals = sb.vals[fd.r];
    }

    void alloc_first()
    {
        fd.keep = (u64 *)fd.sb.keys[fd.r ^ 1];
        fd.gstart_bits = ar.alloc<u64>(((size_t)n02 >> 6) + 2);
        fd.idx = fd.sb.vals[fd.r ^ 1];
        fd.names_g = s12 ? ar.alloc<u32>(n02) : nullptr;
        fd.fail = ar.alloc<u32>(1);
        fd.fail_is_zero = ctx.zeroed_word != nullptr;
        if (fd.fail_is_zero) { fd.fail = ctx.zeroed_word; ctx.zeroed_word = nullptr; }
        fd.gp = ceil_div_u32((u64)n02 + 1, BLOCK * PLACE_IPT);
        fd.block_keep = ar.alloc<u32>(fd.gp);
        fd.nb = ceil_div_u32(fd.gp, SCAN_TILE);
        fd.block_sums = ar.alloc<u32>(fd.nb);
        fd.bad = ar.alloc<u32>(((size_t)n02 >> 5) + 2);
        fd.xdep0 = ht || ctx.dry ? ar.alloc<uint8_t>((size_t)n02 + 16) : nullptr;
        if (!ctx.dry && !fd.fail_is_zero) HIP_CHECK(hipMemsetAsync(fd.fail, 0, sizeof(u32), ctx.stream));
        fd.repetitive_text = n0 == 0 && !ctx.dry && ctx.knobs.lds_rounds && ctx.knobs.persist && n02 >= 4u * PR_CTL_WORDS &&
                             (ctx.rep_n ? ctx.rep_dup * 2u > ctx.rep_n : ctx.plan.persist == 1);
        fd.small_input = n02 <= REFINE_SMALL_INPUT && !fd.repetitive_text;
        fd.sr = SegRanks{docs.seg.n_docs ? docs.seg.doc_off : nullptr, docs.seg.n_docs};
        fd.spec_direct = ctx.spec_rounds && n0 == 0 && !ctx.dry && ctx.spec_out && fd.fail_is_zero && fd.fail == ctx.spec_fail;
        v.m = v.m_next = n02;
    }

    // the k-gram marks (kg_mark: in = the largest k the table has room for, out = the k marked), the fused finish's
    // arguments, and what the first placement wants preset: one launch for all of it
    void setup_marks()
    {
        KgMark &km = fd.km;
        ClearRegions clears;
        const int w = kp.w, spare = kp.spare;
        if (kg_mark) kg_mark->k = kg_mark->kg && n0 == 0 && !ctx.dry && !fd.small_input && !ht ? kg_mark->k : 0;   // (variable-length keys: the score side builds its tables itself)
        if (kg_mark && kg_mark->k > 0) {
            km = *kg_mark;
            km.k = std::min(km.k, w);
            km.bins = 1;
            for (int i = 0; i < km.k; i++) km.bins *= km.A;
            km.pairs = km.kg3 && km.k >= 2;
            km.by_rank = docs.seg.n_docs != 0;
            clear_add(ctx, clears, km.kg, (size_t)(km.bins + 1) * km.n_docs * (km.pairs ? 8 : 4), 0xFF);
            if (km.pairs) clear_add(ctx, clears, km.kg3, (size_t)(km.bins / km.A + 1) * km.n_docs * sizeof(u32), 0xFF);
            *kg_mark = km;
        }
        if (kp.fused) {
            FinishArgs<K> &fa = fd.fa;
            fa.keys = fd.sb.keys[fd.r]; fa.vals = fd.sorted_vals; fa.m = n02; fa.s8 = s8;
            fa.w = w; fa.b = bt; fa.spare = spare; fa.low_bits = kp.low_bits;
            fa.inv_b = (65536u + (u32)bt - 1u) / (u32)bt;
            fa.rep_t = fd.starts.rep_t; fa.ones = fd.starts.ones; fa.highs = fd.starts.highs;
            fa.top_mask = 0;
            for (int j = 0; j < w; j++)
                if (spare + j * bt >= kp.low_bits) fa.top_mask |= (K)(((K)1 << bt) - 1) << (spare + j * bt);
            fa.kg_top = spare + (w - km.k) * bt < kp.low_bits;
            fa.order_g = sa12; fa.lcp_g = lcp_out; fa.keep = fd.keep; fa.gstart = fd.gstart_bits;
            fa.block_keep = fd.block_keep; fa.fail = fd.fail; fa.kg_bad = ctx.kg_bad ? ctx.kg_bad : fd.fail;
            fa.km = fd.small_input ? KgMark() : km;
            if (ht) { fa.ht_sb = kp.ht_sb; fa.ht_wmin = w; fa.ht_dec = ht->dec; fa.xdep0 = fd.xdep0; }
            if (fd.sr.n_docs) { fa.km.by_rank = 1; fa.km.doc_off = fd.sr.doc_off; fa.km.n_docs = fd.sr.n_docs; }
            // (keep lies in the keys the sort's last pass read: cleared behind it, with the rest)
            clear_add(ctx, clears, fd.keep, (((size_t)n02 >> 6) + 2) * sizeof(u64), 0);
            clear_add(ctx, clears, fd.gstart_bits, (((size_t)n02 >> 6) + 2) * sizeof(u64), 0);
        }
        clear_run(ctx, clears);
    }

    // The placement pass over the sorted input (mode: LongRepeats -- 0 = the first attempt, 1 = mark, 2 = commit), and what
    // it left in large groups
    void place(int mode)
    {
        u32 *spec_keep = fd.spec_direct && mode == 0 ? ctx.spec_out : nullptr;
        const bool small = fd.small_input;
        if (kp.fused) {
            if (mode != 0) throw FusedAbort();
            fd.fa.spec_keep = spec_keep;
            auto finish = [&](auto kernel) { LAUNCH_NAMED(ctx, "lvl0_finish_kernel", kernel, fd.gp, fd.fa); };
            const bool sg = fd.sr.n_docs != 0;
            if (ht && small && sg) finish(lvl0_finish_kernel<K, true, 64, true, true>);
            else if (ht && small) finish(lvl0_finish_kernel<K, true, 64, true>);
            else if (ht && sg) finish(lvl0_finish_kernel<K, false, 64, true, true>);
            else if (ht) finish(lvl0_finish_kernel<K, false, 64, true>);
            else if (small && sg) finish(lvl0_finish_kernel<K, true, 64, false, true>);
            else if (small) finish(lvl0_finish_kernel<K, true, 64>);
            else if (kp.fin_small_halo && sg) finish(lvl0_finish_kernel<K, false, 32, false, true>);
            else if (kp.fin_small_halo) finish(lvl0_finish_kernel<K, false, 32>);
            else if (sg) finish(lvl0_finish_kernel<K, false, 64, false, true>);
            else finish(lvl0_finish_kernel<K, false, 64>);
        } else {
            // (the k-gram marks ride with the first attempt over fixed-width keys of an input that is not small)
            auto pass = [&](auto kernel) {
                LAUNCH_NAMED(ctx, "lvl0_place_kernel", kernel, fd.gp, fd.starts, fd.sorted_vals, n02, s8, n0, kp.w, bt, kp.spare,
                             sa12, fd.names_g, lcp_out, fd.keep, fd.block_keep, fd.fail, LongRepeats{fd.bad, mode},
                             !ht && !small && mode == 0 ? fd.km : KgMark(), ht ? fd.xdep0 : (uint8_t *)nullptr, fd.sr, spec_keep);
            };
            if (ht && small) pass(lvl0_place_kernel<K, true, false, true>);
            else if (ht && mode == 0) pass(lvl0_place_kernel<K, false, true, true>);
            else if (ht) pass(lvl0_place_kernel<K, false, false, true>);
            else if (small) pass(lvl0_place_kernel<K, true, false>);
            else if (mode == 0) pass(lvl0_place_kernel<K, false, true>);
            else pass(lvl0_place_kernel<K, false, false>);
        }
        if (mode == 1 || ctx.dry) return;
        if (ctx.spec_rounds && mode == 0 && n0 == 0) {
            // speculative build: the host goes on as if nothing were left in large groups; the counts are
            // put next to the build's other flags and read at the end (build_common repeats the build if
            // they are not zero)
            if (!fd.spec_direct)
                LAUNCH(ctx, spec_counts_kernel, ceil_div_u32(fd.gp, SPEC_COUNT_TILE), (const u32 *)fd.block_keep, fd.gp,
                       (const u32 *)fd.fail, ctx.spec_out);
            v.m_next = 0;
            v.h_fail = 0;
            return;
        }
        LAUNCH(ctx, (scan_reduce_kernel<ArrIn>), fd.nb, ArrIn{fd.block_keep}, fd.gp, fd.block_sums);
        std::vector<u32> h_sums(fd.nb);
        HIP_CHECK(hipMemcpyAsync(h_sums.data(), fd.block_sums, (size_t)fd.nb * 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(&v.h_fail, fd.fail, 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(sync_stream(ctx.stream));
        v.m_next = 0;
        for (u32 x : h_sums) v.m_next += x;
        if (ctx.stats && n0 == 0 && mode == 0) { ctx.stats->first_kept = v.m_next; ctx.stats->first_n = n02; }
        if (g_trace)
            fprintf(stderr, "[east_hip] level-0 (%s, %u elements, w = %d): %u in large groups%s\n", n0 ? "sample" : "all suffixes",
                    n02, kp.w, v.m_next, v.h_fail ? ", a repeat too long to order directly" : "");
    }

    // Mark and commit, what the first domain and the rounds share: the flag and the marks of a domain of m cleared, and --
    // behind the marking pass and the one that places the rest -- nothing may be left undecided
    void mark_fills(u32 m)
    {
        HIP_CHECK(hipMemsetAsync(fd.fail, 0, sizeof(u32), ctx.stream));
        HIP_CHECK(hipMemsetAsync(fd.bad, 0, (((size_t)m >> 5) + 2) * sizeof(u32), ctx.stream));
        v.long_repeats = true;
    }
    void mark_decided() const
    {
        if (v.h_fail) east_throw(EAST_HIP_ERR_INTERNAL, "level 0: undecided comparison after the marking pass");
    }

    // duplicated passages inside small groups of the first domain: put the domain back, mark those groups, place the others
    void mark_commit_first()
    {
        if (kp.fused) throw FusedAbort();                // (duplicated passages: the mark + commit passes want the sorted pairs)
        if (ctx.stats) ctx.stats->long_repeats++;
        LAUNCH(ctx, (dc3_refine_restore_kernel<KeyNeqWindowIn<K>>), ceil_div_u32((u64)n02 + 1, BLOCK), fd.sorted_vals, fd.starts,
               (const u32 *)nullptr, n02, sa12, fd.names_g);
        mark_fills(n02);
        place(1);
        place(2);
        mark_decided();
    }

    // ---- the refinement rounds on the members of large groups ----
    void alloc_rounds()
    {
        const u32 cap = n02 + 1;                        // natural-language text: most suffixes can be in large groups
        for (auto &e : bufs.ebuf) e = ar.alloc<u32>(cap);
        for (auto &e : bufs.sbuf) e = ar.alloc<u32>(cap);
        for (auto &e : bufs.fbuf) e = ar.alloc<u32>(cap);
        bufs.gstart = ar.alloc<u32>(cap); bufs.group = ar.alloc<u32>(cap);
        for (int k = 0; k < 2; k++) { bufs.rb.keys[k] = ar.alloc<u64>(cap); bufs.rb.vals[k] = ar.alloc<u32>(cap); }
        bufs.name_of = n0 == 0 ? ar.alloc<u32>(n02) : nullptr;
        if (ht || ctx.dry) for (auto &x : bufs.xbuf) x = ar.alloc<uint8_t>((size_t)cap + 16);
        bufs.cover = ar.alloc<uint2>((size_t)cap / LG_CHUNK + 2);
        bufs.sub_idx = ar.alloc<u32>((size_t)cap + 1); bufs.full_idx = ar.alloc<u32>(cap);
        bufs.rest_cnt = ar.alloc<u32>((size_t)cap / LG_CHUNK + 3); bufs.rest_pre = ar.alloc<u32>((size_t)cap / LG_CHUNK + 3);
        if (ctx.dry) {                                  // sizing run: the transient buffers of one round (on top of all of the above)
            device_scan<BitIn, false>(ctx, BitIn{fd.keep}, n02 + 1, fd.idx);
            (void)radix_sort_pairs<u64>(ctx, bufs.rb, cap, 8);
        }
        PersistCap &caps = bufs.persist_caps;
        caps = ctx.knobs.lds_rounds && ctx.knobs.persist && !ctx.dry ? persist_capacity() : PersistCap();
        if (ctx.knobs.persist_max_wgs > 0) {             // (tests / experiments: a smaller grid -- several tiles per workgroup on small inputs)
            const u32 cap_wgs = (u32)ctx.knobs.persist_max_wgs;
            caps.one_per_cu = std::min(caps.one_per_cu, cap_wgs);
            caps.large = std::min(caps.large, cap_wgs);
        }
    }

    void open_domain(u32 *lcp_redo)
    {
        dom = Domain();
        dom.persist_cap = bufs.persist_caps.one_per_cu;
        dom.depth = kp.fused ? (u32)kp.depth0 : (u32)kp.w;
        dom.elem = kp.fused ? (const u32 *)sa12 : fd.sorted_vals;
        dom.lcp_redo = lcp_redo;
    }

    // A domain that fits the chip at one tile per resident workgroup can be finished by ONE launch (persist_rounds.h):
    // prefix doubling with the tiles kept in LDS, a grid barrier per round.  It is taken where the rounds below would
    // go over to prefix doubling -- a domain that shrinks slowly: long repeats -- and for the FIRST domain of text
    // the planning sample calls repetitive (most of 8 192 consecutive suffixes share 8 symbols with three others of
    // the sample: the reference's worst case, 100 identical strings; a speculative build: as the build before).
    // Natural language is better off launch by launch: its domains shrink eightfold per round and the endgame orders
    // what is left directly (measured on 0.25 .. 4 MiB of prose: 0.29-0.89 ms against 0.31-0.98 through doubling).
    // The launch gives up -- having changed nothing the rounds below rely on -- when a tie group is longer than a tile
    // takes; a later, smaller domain may fit.
    // (the launch needs the name of every placed suffix first -- a scatter over all n02 ranks, 2.1 ms for the 94 M
    // symbols of the Zipf stand-in: only where the domain is a good part of the input, or the input small)
    void decide_persist(Round &r) const
    {
        const u32 m = v.m, m_next = v.m_next;
        r.slow = r.round > 0 && m_next > m / 2;          // slow shrinking = long repeats
        // (a domain of more tiles than the device holds workgroups: the same rounds with the tiles' state in global
        // memory, several tiles per workgroup -- refine_persist2_kernel)
        r.try_persist = dom.persist_cap > 0 && bufs.name_of && !dom.doubling && n02 >= 4u * PR_CTL_WORDS &&
                        (m_next <= dom.persist_cap * LG_CHUNK || (bufs.persist_caps.large > 0 && ctx.knobs.persist_large)) &&
                        (n02 <= PERSIST_SMALL_INPUT || n02 / 8u <= m_next) &&
                        // (... or whose first window -- wide enough to tell random suffixes apart -- left nineteen of
                        // twenty suffixes tied: copies further apart than the sample is long)
                        (r.round == 0 ? fd.repetitive_text || m_next >= n02 - n02 / 20u : r.slow);
    }

    // the names of a domain's members: where their (possibly split) group now starts
    void rename_members(u32 grid, const u32 *flag, const u32 *slot, const u32 *elem, const u64 *keep)
    {
        device_scan<ArrIn, true>(ctx, ArrIn{flag}, v.m, bufs.group);
        LAUNCH(ctx, dc3_group_starts_kernel, grid, flag, (const u32 *)bufs.group, slot, v.m, bufs.gstart);
        LAUNCH(ctx, dc3_names_update_kernel, grid, elem, (const u32 *)bufs.group, (const u32 *)bufs.gstart, v.m, keep, bufs.name_of);
    }

    // slow shrinking = long repeats: from here on the depth doubles every round
    void switch_to_doubling()
    {
        dom.doubling = true;
        dom.lcp_from_rounds = false;                    // (names instead of symbols: the seams' entries are computed at the end)
        dom.redo_pending = dom.lcp_redo != nullptr;     // (the compaction below lists the slots of the members still open)
        LAUNCH(ctx, dc3_names_init_kernel, ceil_div_u32(n02, BLOCK), (const u32 *)sa12, n02, bufs.name_of);
        rename_members(ceil_div_u32((u64)v.m + 1, BLOCK), dom.flag, dom.slot, dom.elem, (const u64 *)fd.keep);
        if (g_trace) fprintf(stderr, "[east_hip]   switching to prefix doubling at depth %u\n", dom.depth);
    }

    // compact the members of large groups (the domain shrinks to them: v.m = v.m_next)
    void compact(Round &r)
    {
        const u32 m = v.m;
        const u32 *elem = dom.elem, *slot = dom.slot;
        if (!dom.have_idx) device_scan<PopIn, false>(ctx, PopIn{fd.keep, (m >> 6) + 1u}, (m >> 6) + 2u, fd.idx);
        u32 *slot_c = bufs.sbuf[dom.s_dom ^ 1], *elem_c = bufs.ebuf[dom.e_c()];
        const u32 gc = ceil_div_u32((u64)m + 1, BLOCK * COMPACT_IPT);
        // (xdep: computed from the keys by the first compaction, copied along by the later ones; prefix doubling rounds
        // go by the common depth alone)
        const uint8_t *x_in = dom.have_x ? (const uint8_t *)bufs.xbuf[dom.x_dom] : !slot && ht ? (const uint8_t *)fd.xdep0 : (const uint8_t *)nullptr;
        uint8_t *x_out = ht && !dom.doubling ? bufs.xbuf[dom.x_dom ^ 1] : (uint8_t *)nullptr;
        auto run = [&](auto kernel, auto group_starts, u32 *lcp, int w, int b, int spare) {
            LAUNCH_NAMED(ctx, "dc3_refine_compact_kernel", kernel, gc, elem, group_starts, slot, BitIn{fd.keep}, BitRank{fd.keep, fd.idx}, m,
                         slot_c, elem_c, bufs.gstart, lcp, w, b, spare, x_in, x_out);
        };
        if (!slot && kp.fused) run(dc3_refine_compact_kernel<BitStarts>, BitStarts{fd.gstart_bits}, nullptr, 0, 0, 0);
        else if (!slot) run(dc3_refine_compact_kernel<KeyNeqWindowIn<K>>, fd.starts, lcp_out, kp.w, bt, kp.spare);
        else run(dc3_refine_compact_kernel<FlagArrIn>, FlagArrIn{dom.flag}, nullptr, 0, 0, 0);
        if (x_out) { dom.x_dom ^= 1; dom.have_x = true; } else dom.have_x = false;
        if (dom.redo_pending) {
            HIP_CHECK(hipMemcpyAsync(dom.lcp_redo, slot_c, (size_t)v.m_next * 4, hipMemcpyDeviceToDevice, ctx.stream));
            dom.redo_n = v.m_next;
            dom.redo_pending = false;
        }
        r.xdep = dom.have_x ? (const uint8_t *)bufs.xbuf[dom.x_dom] : (const uint8_t *)nullptr;
        v.m = v.m_next;
    }

#ifdef PR_STAMPS
    void persist_stamps(const u32 *ctl, const u32 *h_ctl) const
    {
        std::vector<unsigned long long> st(8 * PR_MAX_ROUNDS);
        HIP_CHECK(hipMemcpy(st.data(), ctl + PR_CTL_STAMPS, st.size() * 8, hipMemcpyDeviceToHost));
        for (u32 r = 0; r < h_ctl[PR_CTL_ROUNDS]; r++) {
            auto d = [&](int x, int y) { return (double)(long long)(st[r * 8 + x] - st[r * 8 + y]) * 0.01; };
            fprintf(stderr, "[east_hip]     round %u (block 0): gather+test %.2f us, sort %.2f, bounds %.2f, held loads %.2f, names+stores %.2f, count %.2f, barrier %.2f\n",
                    r, d(1, 0), d(2, 1), d(5, 2), d(6, 5), d(7, 6), d(3, 7), d(4, 3));
        }
        const u32 nwg = ceil_div_u32(v.m, LG_CHUNK);
        std::vector<unsigned long long> ab(2 * (size_t)nwg);
        HIP_CHECK(hipMemcpy(ab.data(), ctl + PR_CTL_WORDS, ab.size() * 8, hipMemcpyDeviceToHost));
        if (h_ctl[PR_CTL_ROUNDS] > 3) {
            unsigned long long t0 = ~0ull;
            for (u32 b = 0; b < nwg; b++) t0 = std::min(t0, ab[2 * b]);
            fprintf(stderr, "[east_hip]     round 3, arrival / departure of every 16th block (us after the first arrival):");
            for (u32 b = 0; b < nwg; b += 16) fprintf(stderr, " %u:%.1f/%.1f", b, (ab[2 * b] - t0) * 0.01, (ab[2 * b + 1] - t0) * 0.01);
            double mx = 0; u32 who = 0;
            for (u32 b = 0; b < nwg; b++) if ((ab[2 * b] - t0) * 0.01 > mx) { mx = (ab[2 * b] - t0) * 0.01; who = b; }
            fprintf(stderr, "\n[east_hip]     last arrival: block %u at %.1f us\n", who, mx);
        }
    }
#endif

    // The persistent launch over the compacted domain.  Returns true when it finished the level (false: it gave up on a
    // group longer than a tile, the rounds go on launch by launch).
    bool persistent_launch(const Round &r)
    {
        const u32 m = v.m, depth = dom.depth;
        u32 *elem_c = bufs.ebuf[dom.e_c()], *slot_c = bufs.sbuf[dom.s_dom ^ 1];
        u32 *name1 = (u32 *)bufs.rb.keys[0], *ctl = bufs.rb.vals[0];     // (see RoundBufs::rb)
        HIP_CHECK(hipMemsetAsync(ctl, 0, PR_CTL_WORDS * sizeof(u32), ctx.stream));
        LAUNCH(ctx, persist_names_init_kernel, ceil_div_u32(n02, BLOCK), (const u32 *)sa12,
               !dom.slot && !kp.fused ? fd.sorted_vals : (const u32 *)nullptr, (const u64 *)fd.keep, n02, bufs.name_of, name1);
        const int name_bits = bit_width_u32(n02 > 1 ? n02 - 1 : 1);
        u32 *lcp_p = dom.lcp_redo ? lcp_out : (u32 *)nullptr;
        const PrArgs pa{elem_c, bufs.gstart, slot_c, m, depth, name_bits, bufs.name_of, name1, sa12, lcp_p, ctl};
        const u32 tiles = ceil_div_u32(m, LG_CHUNK);
        // (the large form: see RoundBufs::cover)
        const Pr2Args pa2{elem_c, slot_c, bufs.gstart, bufs.full_idx, m, depth, name_bits, bufs.name_of, sa12, lcp_p,
                          ctl, bufs.cover, bufs.rest_cnt, tiles};
        const PersistCap &caps = bufs.persist_caps;
        u32 h_ctl[4] = {0, 0, 0, 0};
        {
            std::lock_guard<std::mutex> lock(g_persist_mutex);
            const bool force_large = ctx.knobs.persist_force_large && caps.large > 0;      // (tests: the large form on small domains)
            if (tiles <= caps.one_per_cu && !force_large) LAUNCH_BLOCK(ctx, refine_persist_kernel<4>, tiles, LG_THREADS, pa);
            // (between one and two tiles per CU the resident form at two workgroups per CU -- 64 registers, spills, and
            // with the barrier's fences 1.07 ms for the 488 tiles of the worst case at n = 10^4 -- loses to the large
            // form at one workgroup per CU, 0.8 ms: it is not used)
            else LAUNCH_BLOCK(ctx, refine_persist2_kernel, std::min(tiles, caps.large), LG_THREADS, pa2);
            HIP_CHECK(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, ctx.stream));
            HIP_CHECK(sync_stream(ctx.stream));
        }
        if (h_ctl[PR_CTL_ABORT])
            east_throw(EAST_HIP_ERR_INTERNAL, h_ctl[PR_CTL_ABORT] == 2 ? "persistent rounds: groups still open after the last round"
                                                                        : "persistent rounds: a grid barrier timed out");
        if (g_trace)
            fprintf(stderr, "[east_hip]   round %d: persistent launch over a domain of %u at depth %u: %s\n", r.round, m, depth,
                    h_ctl[PR_CTL_BAIL] ? "a group too long for a tile, the rounds go on launch by launch" : "done");
        if (h_ctl[PR_CTL_BAIL] && r.slow) dom.persist_cap = 0;     // (long groups that do not split: prefix doubling launch by launch)
#ifdef PR_STAMPS
        if (g_trace && !h_ctl[PR_CTL_BAIL]) persist_stamps(ctl, h_ctl);
#endif
        if (h_ctl[PR_CTL_BAIL]) return false;
        if (ctx.stats) {
            ctx.stats->refine_rounds += h_ctl[PR_CTL_ROUNDS];
            ctx.stats->persist_rounds += h_ctl[PR_CTL_ROUNDS];
            ctx.stats->lds_sorted += (i64)m * h_ctl[PR_CTL_ROUNDS];
        }
        // the LCP entries of the domain's ranks: compared on the text once the suffix array stands (lcp_of_doubling)
        if (dom.lcp_redo) {
            HIP_CHECK(hipMemcpyAsync(dom.lcp_redo, slot_c, (size_t)m * 4, hipMemcpyDeviceToDevice, ctx.stream));
            dom.redo_n = m;
            dom.lcp_from_rounds = false;
            dom.redo_hinted = true;
        }
        if (r.round == 0 && n0 == 0) ctx.did.persist = 1;
        v.m_next = 0;
        return true;
    }

    // what a round's sort goes by, once the domain is compacted
    void plan_round(Round &r) const
    {
        // (every group here has more than REFINE_SMALL_GROUP members -- at least 2 once groups with long repeats
        // were handed over: a bound on their number saves a read-back)
        r.gbits = bit_width_u32(v.m / (v.long_repeats ? 2u : REFINE_SMALL_GROUP + 1u) + 1);
        r.gt = ceil_div_u32((u64)v.m + 1, BLOCK);
        // (once groups with long repeats are known to exist the direct ordering of large groups only burns time: every
        // member of such a group compares REFINE_ENDGAME_LEN symbols with every other before it gives up)
        r.endgame = v.m <= REFINE_ENDGAME_DOMAIN && !v.long_repeats && !fd.repetitive_text;
        // (the classification of the next domain rides along with the in-LDS round, see LgClassify: symbol windows, the
        // usual limits, no groups with long repeats known)
        r.fuse_cls = ctx.knobs.lds_rounds && ctx.knobs.fused_classify && !dom.doubling && !r.endgame && !v.long_repeats;
        r.round_left = v.m;
    }

    // One round's sort: the members of every group ordered by their round key -- the next window of symbols, or
    // (prefix doubling) the name of the suffix `depth` symbols further on.  Groups that fit a workgroup's LDS are
    // sorted there, keys, sort and write-back in one launch (lds_group_sort.h): returns what that left.
    u32 sort_round_lds(const Round &r, bool names, int w2, const KeyNeqWindowIn<u64> &f)
    {
        const u32 m = v.m;
        u32 m_left = m;
        if (r.fuse_cls) HIP_CHECK(hipMemsetAsync(fd.keep, 0, (((size_t)m >> 6) + 2) * sizeof(u64), ctx.stream));
        LAUNCH_BLOCK(ctx, refine_lds_sort_kernel, ceil_div_u32(m, LG_CHUNK), LG_THREADS, s8, (const u32 *)bufs.ebuf[dom.e_c()],
                     (const u32 *)bufs.gstart, (const u32 *)bufs.sbuf[dom.s_dom ^ 1], m, n0, dom.depth, w2, bt, term_first, (u64)f.rep_t,
                     (u64)f.ones, (u64)f.highs, sa12, fd.names_g, bufs.ebuf[dom.e_out()], bufs.fbuf[dom.f_dom ^ 1],
                     names ? (u32 *)nullptr : lcp_out, bufs.cover, names ? (const u32 *)bufs.name_of : (const u32 *)nullptr,
                     r.fuse_cls ? LgClassify{fd.keep, fd.fail, (u32)REFINE_SMALL_GROUP, (u32)RESOLVE_MAX_LEN, names ? nullptr : r.xdep}
                                : LgClassify{nullptr, nullptr, 0u, 0u, names ? nullptr : r.xdep});
        // what is left: counted per chunk from cover[] (no pass over the elements)
        const u32 n_chunks = ceil_div_u32(m, LG_CHUNK);
        LAUNCH(ctx, lg_rest_count_kernel, ceil_div_u32(n_chunks + 1, BLOCK), (const uint2 *)bufs.cover, m, n_chunks, bufs.rest_cnt);
        device_scan<ArrIn, false>(ctx, ArrIn{bufs.rest_cnt}, n_chunks + 1, bufs.rest_pre);
        HIP_CHECK(hipMemcpyAsync(&m_left, bufs.rest_pre + n_chunks, 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(sync_stream(ctx.stream));
        if (ctx.stats) ctx.stats->lds_sorted += m - m_left;
        if (g_trace) fprintf(stderr, "[east_hip]   round %d: %u of %u sorted in LDS\n", r.round, m - m_left, m);
        return m_left;
    }

    // ... the rest is compacted and takes the global radix sort by (group, key)
    void sort_round(Round &r, bool names, int w2, const KeyNeqWindowIn<u64> &f)
    {
        const u32 m = v.m, depth = dom.depth;
        const u32 *elem_c = bufs.ebuf[dom.e_c()], *slot_c = bufs.sbuf[dom.s_dom ^ 1];
        SortBufs<u64> &rb = bufs.rb;
        const int kbits = names ? w2 : w2 * bt;     // (names: w2 = the bits of a name)
        const u32 m_left = ctx.knobs.lds_rounds ? sort_round_lds(r, names, w2, f) : m;
        r.round_left = m_left;
        if (m_left == 0) return;
        const u32 *elems_s = elem_c;                // what goes through the global sort: the domain, or its rest
        const u32 *full = nullptr;
        int gb = r.gbits;
        if (m_left == m) {
            device_scan<ArrIn, true>(ctx, ArrIn{bufs.gstart}, m, bufs.group);      // group[] = inclusive scan of gstart: the groups' numbers
            // (the in-LDS round ran and took nothing: every group is longer than a tile takes -- the same bound on
            // their number as below: a run of one letter is ONE group of 16 M, whose number was sorted on 24 bits)
            if (ctx.knobs.lds_rounds) gb = std::min(r.gbits, bit_width_u32(m_left / (LG_MAX_GROUP + 1u) + 1u));
        } else {
            // the rest, compacted (elements, group starts, where they came from), its groups numbered -- every
            // one of them has more than LG_MAX_GROUP members, which bounds their number
            u32 *sub_elem = bufs.sub_idx, *sub_gstart = rb.vals[1];             // (see RoundBufs)
            LAUNCH(ctx, lg_rest_compact_kernel, r.gt, LgUncovered{bufs.cover, m}, (const u32 *)bufs.rest_pre, elem_c,
                   (const u32 *)bufs.gstart, m, sub_elem, sub_gstart, bufs.full_idx);
            device_scan<ArrIn, true>(ctx, ArrIn{sub_gstart}, m_left, bufs.group);
            elems_s = sub_elem;
            full = bufs.full_idx;
            gb = std::min(r.gbits, bit_width_u32(m_left / (LG_MAX_GROUP + 1u) + 1u));
        }
        const u32 gl = ceil_div_u32(m_left, BLOCK);
        if (names)
            LAUNCH(ctx, dc3_double_keys_kernel, gl, (const u32 *)bufs.name_of, elems_s, (const u32 *)bufs.group, m_left, depth, w2,
                   rb.keys[0], rb.vals[0]);
        else
            LAUNCH(ctx, dc3_refine_keys_kernel, gl, s8, elems_s, (const u32 *)bufs.group, m_left, n0, depth, w2, bt, term_first,
                   rb.keys[0], rb.vals[0], r.xdep, full);
        const int rr = radix_sort_pairs<u64>(ctx, rb, m_left, gb + kbits);
        LAUNCH(ctx, dc3_refine_writeback_kernel, gl, (const u64 *)rb.keys[rr], (const u32 *)rb.vals[rr], slot_c, elem_c, m_left,
               f.rep_t, f.ones, f.highs, sa12, fd.names_g, bufs.ebuf[dom.e_out()], bufs.fbuf[dom.f_dom ^ 1],
               names ? (u32 *)nullptr : lcp_out, depth, names ? 0 : w2, bt, full, names ? (const uint8_t *)nullptr : r.xdep);
    }

    // The round's sort by the next window, or by names where the rounds double; false: no room for a window (the rounds end)
    bool sort_domain(Round &r)
    {
        if (dom.doubling) {
            sort_round(r, true, bit_width_u32(n02 > 1 ? n02 - 1 : 1), KeyNeqWindowIn<u64>{nullptr, 0, 0, 0});
            rename_members(r.gt, bufs.fbuf[dom.f_dom ^ 1], bufs.sbuf[dom.s_dom ^ 1], bufs.ebuf[dom.e_out()], (const u64 *)nullptr);
            dom.depth *= 2;
            return true;
        }
        // (13 bits: room for the group numbers inside a workgroup's tile of the in-LDS round)
        int w2 = std::min(12, (64 - std::max(r.gbits, 13)) / bt);
        if (getenv("EAST_HIP_ROUND_W2")) w2 = std::max(1, std::min(w2, atoi(getenv("EAST_HIP_ROUND_W2"))));   // (experiments)
        if (w2 < 1) return false;
        sort_round(r, false, w2, KeyNeqWindowIn<u64>::make(nullptr, w2, bt, 0, term_first));
        dom.depth += (u32)w2;
        return true;
    }

    // the sorted domain becomes the current one
    void advance()
    {
        dom.e_dom = dom.e_out(); dom.s_dom ^= 1; dom.f_dom ^= 1;
        dom.elem = bufs.ebuf[dom.e_dom]; dom.slot = bufs.sbuf[dom.s_dom]; dom.flag = bufs.fbuf[dom.f_dom];
        if (ctx.stats) ctx.stats->refine_rounds++;
    }

    // the new, smaller domain: place what is untied or in small groups now, count the rest
    // a small domain is finished by direct ordering of much larger groups (a round costs ~60 launches
    // however few suffixes are left); the comparisons are kept short so that the work stays bounded
    void classify(const Round &r, int mode, bool rest_only = false)
    {
        const u32 m = v.m, depth = dom.depth;
        const bool doubling = dom.doubling;
        if (!rest_only || r.round_left > 0)       // (rest_only: the in-LDS round has classified its own tiles)
            LAUNCH(ctx, dc3_refine_classify_kernel, r.gt, dom.elem, FlagArrIn{dom.flag}, dom.slot, m, s8, n0, depth, sa12, fd.names_g, fd.keep,
                   // (doubling rounds with long repeats known, once the depth is beyond what a direct comparison may
                   // look at: the members of a small group would compare REFINE_DOUBLING_LEN symbols, give up, and do it
                   // again next round -- 19 of the 53 ms of a 16 M-symbol Fibonacci string; the next round's name look-up
                   // decides them: only what is alone in its group is placed)
                   fd.fail, doubling && mode != 0 && depth >= REFINE_DOUBLING_LEN ? 1u : r.endgame ? (u32)REFINE_ENDGAME_GROUP : (u32)REFINE_SMALL_GROUP,
                   // (doubling rounds with long repeats known -- mark + commit, an undecided group simply stays for the
                   // next round, which doubles the depth by one name look-up per member: comparing 2 048 symbols of text
                   // for it first was 60 of the 96 ms of a 16 M-symbol Fibonacci string)
                   // (... and the first attempt of a doubling round is short as well: in a Fibonacci string the members of
                   // small groups DO differ within 2 048 symbols, and found that out 256 dependent loads at a time, every
                   // round -- 0.73 ms a launch)
                   r.endgame ? (u32)REFINE_ENDGAME_LEN : doubling ? (u32)REFINE_DOUBLING_LEN : (u32)RESOLVE_MAX_LEN,
                   doubling ? bufs.name_of : (u32 *)nullptr,
                   LongRepeats{fd.bad, mode}, lcp_out, rest_only ? (const uint2 *)bufs.cover : (const uint2 *)nullptr,
                   doubling ? (const uint8_t *)nullptr : r.xdep);
        if (mode == 1) return;
        device_scan<PopIn, false>(ctx, PopIn{fd.keep, (m >> 6) + 1u}, (m >> 6) + 2u, fd.idx);
        dom.have_idx = true;
        HIP_CHECK(hipMemcpyAsync(&v.m_next, fd.idx + ((m >> 6) + 1u), 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(&v.h_fail, fd.fail, 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(sync_stream(ctx.stream));
        if (g_trace)
            fprintf(stderr, "[east_hip]   round %d: domain %u, %u still in large groups, depth %u%s\n", r.round, m, v.m_next,
                    depth, v.h_fail ? ", a repeat too long to order directly" : "");
    }

    // as in the first domain: restore, mark, place the rest
    void mark_commit_round(const Round &r)
    {
        const bool gave_up = v.h_fail != 0;
        if (gave_up) LAUNCH(ctx, (dc3_refine_restore_kernel<FlagArrIn>), r.gt, dom.elem, FlagArrIn{dom.flag}, dom.slot, v.m, sa12, fd.names_g);
        mark_fills(v.m);
        // (the abandoned pass named some suffixes by a place they do not get)
        if (dom.doubling && gave_up) rename_members(r.gt, dom.flag, dom.slot, dom.elem, (const u64 *)nullptr);
        classify(r, 1);
        classify(r, 2);
        mark_decided();
    }

    // Returns true when the rounds placed everything.
    bool rounds()
    {
        for (int round = 0; !ctx.dry; round++) {
            if (v.m_next == 0) return true;
            // Strings of a few words dissolve within their own length, a round takes 6-12 symbols off.  A domain
            // that stops shrinking is a long repeat: all-suffix mode goes over to prefix doubling (switch_to_doubling), the
            // sample mode of DC3 stops here (every round would cost the same again) and recurses on the names.
            dom.stalled = (round > 0 && v.m_next > v.m - v.m / 32) ? dom.stalled + 1 : 0;
            if (round == REFINE_MAX_ROUNDS || (dom.stalled == 2 && !dom.doubling && !bufs.name_of)) break;
            Round r;
            r.round = round;
            decide_persist(r);
            if (bufs.name_of && !dom.doubling && r.slow && !r.try_persist) switch_to_doubling();
            compact(r);
            if (r.try_persist && persistent_launch(r)) return true;
            plan_round(r);
            if (!sort_domain(r)) break;
            advance();
            if (!v.long_repeats) classify(r, 0, r.fuse_cls);    // (once such groups are known to exist: mark + place right away)
            if (v.h_fail || v.long_repeats) mark_commit_round(r);
        }
        return false;
    }

    // ---- the end ----
    // (prefix doubling: the LCP entries of everything those rounds placed)
    void lcp_of_doubling()
    {
        if (lcp_out && !dom.lcp_from_rounds && dom.redo_n)
            LAUNCH(ctx, lvl0_lcp_text_list_kernel, ceil_div_u32(dom.redo_n, BLOCK), s8, (const u32 *)sa12, (const u32 *)dom.lcp_redo,
                   dom.redo_n, lcp_out, lcp_capped, ctx.lcp_budget, dom.redo_hinted);
    }

    // recursion ahead: names by an inclusive scan of the refined predicate, scattered into the name string
    void names_for_recursion(u32 &n_names)
    {
        u32 *names = ar.alloc<u32>(n02);
        device_scan<FlagArrIn, true>(ctx, FlagArrIn{fd.names_g}, n02, names);
        if (ctx.dry) {
            n_names = n02 > 4 ? n02 - 1 : n02;            // worst case: recurse
        } else {
            HIP_CHECK(hipMemcpyAsync(&n_names, names + (n02 - 1), 4, hipMemcpyDeviceToHost, ctx.stream));
            HIP_CHECK(sync_stream(ctx.stream));
            if (n_names == 0 || n_names > n02) east_throw(EAST_HIP_ERR_INTERNAL, "dc3: impossible name count");
        }
        LAUNCH(ctx, dc3_scatter_names_kernel, ceil_div_u32((u64)n02 + 3, BLOCK), (const u32 *)sa12, (const u32 *)names, n02, s12);
    }
};

template <class K>
static bool dc3_level0_bytes(Ctx &ctx, const uint8_t *s8, u32 n0, u32 n02, int w, int bt, u32 term_first, u32 *sa12,
                             u32 *s12, u32 &n_names, u32 *lcp_out = nullptr, u32 *lcp_capped = nullptr,
                             DocKey docs = DocKey(), KgMark *kg_mark = nullptr, bool allow_fused = false, u32 longest = 0,
                             const HtKeys *ht = nullptr)
{
    Level0<K> l{ctx, *ctx.arena, s8, n0, n02, bt, term_first, sa12, s12, lcp_out, lcp_capped, docs, kg_mark, ht};
    l.plan_keys(w, allow_fused, longest);
    l.sort_keys();
    l.alloc_first();
    l.setup_marks();
    l.place(0);
    if (l.v.h_fail) l.mark_commit_first();
    if (!ctx.dry && l.v.m_next == 0) {                  // everything is in place (and the LCP table written)
        if (ctx.stats) ctx.stats->levels_resolved++;
        return true;
    }
    u32 *lcp_redo = lcp_out ? ctx.arena->alloc<u32>((size_t)n02 + 1) : nullptr;
    bool done = false;
    // (ctx.lean: the device is short of memory for the rounds' buffers -- straight on to the recursion / DC3)
    if (!ctx.lean) {
        const size_t mark_rounds = ctx.arena->mark();
        l.alloc_rounds();
        l.open_domain(lcp_redo);
        done = l.rounds();
        ctx.arena->release(mark_rounds);
    }
    if (done) {
        if (ctx.stats) ctx.stats->levels_resolved++;
        l.lcp_of_doubling();
        return true;
    }
    if (!s12) return false;                            // all-suffix mode: the caller falls back to DC3
    l.names_for_recursion(n_names);
    return false;
}

// Width of the level-0 name window.  Widest window: names almost unique (sigma^w >= 64 n) within
// 64-bit keys; but if the window that still fits 32-bit keys leaves only a few per cent of ties
// (sigma^w >= 4 n), the cheaper sort wins and the tie resolution absorbs the difference.
// (doc_bits key bits are taken by the document number; n is then the length of the longest document)
static int lvl0_window(u32 n, int bt, u32 term_first, int doc_bits = 0)
{
    int w = 3;
    const int w_max = (64 - doc_bits) / bt < 12 ? (64 - doc_bits) / bt : 12;
    double reach = (double)term_first * term_first * term_first;
    while (w < w_max && reach < 64.0 * (double)n) { reach *= term_first; w++; }
    const int w32 = (32 - doc_bits) / bt;
    if (w32 >= 3 && w32 < w) {
        // the spare bits of the last digit hold the top bits of one more symbol: that many more buckets
        const int spare32 = lvl0_spare_bits(w32 * bt + doc_bits, 32, bt, w32);
        const double buckets = spare32 > 0 ? (double)((term_first >> (bt - spare32)) + 1u) : 1.0;
        if (pow((double)term_first, w32) * buckets >= 4.0 * (double)n) w = w32;
    }
    return w;
}

// The fast path for text: ALL n suffixes keyed by their first w symbols, one stable sort, the tied
// ones ordered directly / refined by further windows / by prefix doubling -- no sample, no ranks, no
// merge.  Returns false only in the rare cases it gives up (REFINE_MAX_ROUNDS, or no room for a
// window next to the document number); the caller then runs DC3, whose work is bounded whatever the input.
// Several documents (docs.bits > 0, longest = symbols of the longest one): the keys carry the document
// number on top, sa_out / lcp_out receive every document's tables side by side (lcp_out: the first
// entry of each document still has to be reset, lcp_doc_starts_kernel).
static bool window_suffix_sort(Ctx &ctx, const uint8_t *s8, u32 n, u32 term_first, u32 *sa_out, u32 *lcp_out,
                               u32 *lcp_capped, DocKey docs = DocKey(), u32 longest = 0, KgMark *kg_mark = nullptr)
{
    Arena &ar = *ctx.arena;
    const size_t mark = ar.mark();
    const int bt = bit_width_u32(term_first);
    const int kg_k_in = kg_mark ? kg_mark->k : 0;
    // Segmented sort (radix_sort.h: RsSeg): a handful to a few thousand LARGE documents keep their ranges in every pass and
    // the key holds text only -- 256 documents of 1 MiB: 6 symbols + 2 bits of the 7th in a 32-bit key instead of 4 + 4
    // bits; the buckets of the fused finish shrink from 28 suffixes to one, next to nothing stays tied.  Worth it while the
    // documents' own tiles and groups (the last group of a document is partly empty) stay within twice the flat count:
    // decided from n and the number of documents alone, so that the sizing run prices the same plan.
    const bool multi = docs.bits > 0;
    {
        const u32 flat_groups = ceil_div_u32(ceil_div_u32(n, RS_TILE), RS_GROUP);
        const bool can = multi && docs.n_docs <= RS_SEG_MAX_DOCS && (ctx.dry || docs.h_doc_off);
        // (documents of a histogram group -- 32 768 suffixes -- or more on average: measured on 256 MiB of word text, build
        // with / without: 256 x 1 MiB 7.3 / 7.8 ms, 1 024 x 256 KiB 6.9 / 7.3, 4 096 x 64 KiB 7.3 / 7.8, 8 192 x 32 KiB 7.9 / 8.4,
        // 16 384 x 16 KiB 7.9 / 7.7 -- short tiles and mostly empty groups)
        const u32 per_groups = getenv("EAST_HIP_SEG_DIV") ? (u32)std::max(1, atoi(getenv("EAST_HIP_SEG_DIV"))) : 1u;   // (experiments)
        // (... and five or more of them: the document number of two to four documents costs the key a bit or two, less than
        // the segments' short tiles cost the passes -- 2 x 32 MiB: 1.71 ms with, 1.68 without)
        if (can && ctx.knobs.seg_mode != 0 && (ctx.knobs.seg_mode == 1 || (docs.n_docs >= 5 && docs.n_docs <= flat_groups / per_groups + 1))) {
            // (the host's copies of the tables live as long as the build: the uploads are asynchronous)
            docs.seg = rs_seg_make(ctx, docs.doc_off, docs.h_doc_off, docs.n_docs, n, ctx.seg_host);
            docs.bits = 0;                              // (no document number in the keys)
        }
    }
    const size_t mark_lvl = ar.mark();                  // (what a repeated level 0 gives back: not the tables above)
    ctx.did_seg = docs.seg.n_docs != 0;
    if (ctx.stats) ctx.stats->seg_sort = ctx.did_seg;
    if (docs.bits + 3 * bt > 64) return false;          // (no room for a window next to the document number)
    int w = lvl0_window(multi ? longest : n, bt, term_first, docs.bits);
    // (natural-language text over a large alphabet -- upper-case prose with digits and accents: 7 bits a symbol, 3 symbols
    // in a 32-bit key -- resolves far less per symbol than the estimate above assumes; where most suffixes stay tied
    // behind it, the widest window that fits 64 bits costs less than the rounds it saves: real prose 7.45 -> 6.55 ms)
    // Which of the two it is comes from the text itself ("The plan of a first build"): when more than half
    // of the sample's suffixes share the symbols of the narrow window with another suffix of the SAMPLE -- 8192
    // consecutive suffixes --, most of the corpus is tied behind it.  (A speculative build does as the build before.)
    const int w_wide = std::min(12, (64 - docs.bits) / bt);
    bool wide = false;
    if (ctx.plan.wide >= 0) wide = ctx.plan.wide != 0;
    else if (ctx.sample_n && w < w_wide && w * bt + docs.bits <= 32)
        wide = (u64)ctx.sample_dup2[std::min(w, 8)] * 2u > ctx.sample_n;
    if (getenv("EAST_HIP_WIDE")) wide = atoi(getenv("EAST_HIP_WIDE")) != 0;      // (experiments)
    // Variable-length code words in a 32-bit key (ht_code.h): taken where they put at least one symbol more into the key
    // than the fixed width does -- text over a large alphabet in which a few symbols make up most of it (prose: 7 bits a
    // symbol fixed, under 5 coded).  They go before the wide window: the narrow sort is half the passes on two thirds of
    // the bytes, and with 5-6 symbols in the key the rounds have no more to do than behind the 8 symbols of the wide one.
    // They are worth their decoding where the text pays far more bits per symbol than it needs AND the wide window is
    // the plan anyway: the same 64-bit pairs, sorted on fewer bits (48 stream bits: a pass less), holding half as many
    // symbols again.  (Behind a narrow 32-bit key they were measured and lose to the wide fixed-width window: 6.75 against
    // 6.1 ms on 64 x 1 MiB of prose -- twice the suffixes in the rounds.  Forced -- mode 1 -- they take the key width the
    // fixed-width plan would have taken: the tests go through both.)
    bool use_ht = false, ht_wide = false;
    if (ctx.ht_max_len > 0 && !ctx.dry && ctx.knobs.ht_mode != 0) {
        if (ctx.knobs.ht_mode == 1) { use_ht = true; ht_wide = wide || ctx.knobs.force_wide_keys || w * bt + docs.bits > 32; }
        else if (ctx.plan.ht >= 0) { use_ht = ctx.plan.ht != 0; ht_wide = ctx.plan.ht == 2; }
        else if (docs.seg.n_docs) {
            // (segmented sort: all 32 bits of a narrow key are text -- six and a half symbols of prose, sorted in four passes
            // of 8-byte pairs; measured on 64 x 1 MiB of prose: 5.29 ms, against 5.35 with 48 stream bits in 64-bit keys,
            // 5.74 with the wide fixed-width window and 6.0 with the narrow one)
            use_ht = ctx.ht_mean_len <= (double)bt - 1.5;
            ht_wide = false;
            if (use_ht) wide = false;
        } else { use_ht = ht_wide = wide && ctx.ht_mean_len <= (double)bt - 1.5; }
        if (use_ht && !ht_wide && (32 - docs.bits < 20 || ctx.knobs.force_wide_keys)) ht_wide = true;
        if (use_ht && ht_wide && 64 - docs.bits < 20) use_ht = false;
    }
    int ht_sb = !use_ht ? 0 : ht_wide ? std::min(HT_MAX_STREAM, 64 - docs.bits) : std::min(HT_MAX_STREAM, 32 - docs.bits);
    // (a wide key is cut to whole radix digits: 42 stream bits next to 6 document bits sort in five global passes where
    // 48 take six -- measured on 64 x 1 MiB of prose: 5.77 against 5.82 ms, the 8.6 symbols of the shorter key are enough)
    if (use_ht && ht_wide) ht_sb -= (ht_sb + docs.bits) % RS_DB;
    // (experiments: EAST_HIP_HT_SB=<bits> overrides the stream bits of a wide key -- 42 next to 6 document bits is a pass less than 48)
    if (use_ht && ht_wide && getenv("EAST_HIP_HT_SB")) ht_sb = std::max(20, std::min(ht_sb, atoi(getenv("EAST_HIP_HT_SB"))));
    ctx.did.ht = use_ht ? (ht_wide ? 2 : 1) : 0;
    if (ctx.stats) ctx.stats->ht_keys = ctx.did.ht;
    if (wide) w = std::max(w, w_wide);
    ctx.did.wide = wide;
    // (experiments, DESIGN.md 5.2: EAST_HIP_WINDOW=<symbols> overrides the width of the first window)
    if (getenv("EAST_HIP_WINDOW")) w = std::max(3, std::min(atoi(getenv("EAST_HIP_WINDOW")), std::min(12, (64 - docs.bits) / bt)));
    u32 n_names = 0;
    const HtKeys hk{ctx.ht_enc, ctx.ht_dec, ctx.ht_max_len, ht_sb};
    auto level0 = [&](bool allow_fused) {
        auto run = [&](auto driver, int w_keys, const HtKeys *ht) {
            return driver(ctx, s8, 0, n, w_keys, bt, term_first, sa_out, nullptr, n_names, lcp_out, lcp_capped, docs, kg_mark,
                          allow_fused, multi ? longest : n, ht);
        };
        if (use_ht) return ht_wide ? run(dc3_level0_bytes<u64>, 0, &hk) : run(dc3_level0_bytes<u32>, 0, &hk);
        return w * bt + docs.bits <= 32 && !ctx.knobs.force_wide_keys ? run(dc3_level0_bytes<u32>, w, nullptr)
                                                                      : run(dc3_level0_bytes<u64>, w, nullptr);
    };
    bool ok;
    const Stats stats_in = ctx.stats ? *ctx.stats : Stats();
    try {
        ok = level0(true);
    } catch (const FusedAbort &) {
        if (g_trace) fprintf(stderr, "[east_hip] fused finish gave up (a repeat too long to order directly): full sort\n");
        ar.release(mark_lvl);
        if (kg_mark) kg_mark->k = kg_k_in;
        // nothing of the abandoned attempt is left behind: its pass counts (the bench's byte model reads them), and the
        // "k-gram marks incomplete" flag it may have raised -- the full sort's placement pass marks every bucket start
        if (ctx.stats) *ctx.stats = stats_in;
        if (ctx.kg_bad && !ctx.dry) HIP_CHECK(hipMemsetAsync(ctx.kg_bad, 0, sizeof(u32), ctx.stream));
        ok = level0(false);
    }
    ar.release(mark);
    return ok;
}
