// east_hip.hip -- the public C ABI (include/east_hip.h) of the gfx950 enhanced-annotated-suffix-array build and the
// score table: argument checks and one call each into the host drivers included below.
//
// Device data layout (all in one arena, one HIP stream per handle):
//   s        u32[n+3]  dense symbol codes of the concatenated corpus: text code
//                      points ranked 1..sigma_t in code-point order, the g-th
//                      terminator of the corpus = sigma_t+1+g, three 0 pads
//   sa       u32[n]    suffix array, partitioned by document (document d owns
//                      ranks [doc_off[d], doc_off[d+1])), values = global positions
//   lcp/ann  u32[n]    per-document LCP and annotation tables, same layout
//   up/down/next u32[n] child tables, values local to the document
//   s8       u8[n+16]  the same stream, one byte per symbol (0xFF = terminator), when sigma_t <= 254
//   pyramid            16-ary min pyramid over lcp (tables.h)
//
// One suffix sort covers the whole shard: terminators are numbered globally
// (order inside a document preserved, every terminator above every text
// symbol), so stable-partitioning the global suffix array by document yields
// each document's own reference suftab bit for bit.
//
// The host side by concern, in dependency order (each header includes the kernels it drives):
#include "common.h"         // errors, Arena, DevBuf, Knobs, Ctx, the launch macros
#include "alphabet.h"       // the kernels in front of the suffix sort
#include "handle.h"         // struct east_hip_index
#include "consumer.h"       // what the handle's consumers share: state and lifetime, table sources, uploads, count-scan-fill
#include "upload.h"         // the pinned ring, host symbols narrowed on their way up
#include "build.h"          // build_impl, the arena planner, build_common
#include "textfront.h"      // raw texts: streamed or one-piece preparation, then the build
#include "score_host.h"     // keyphrases, k-gram tables, the score walk
#include <string.h>

static thread_local std::string g_last_error;

// ------------------------------------------------------------------ C ABI --
template <class F> static int guarded(F f)
{
    int rc = EAST_HIP_OK;
    try {
        f();
    } catch (const EastError &e) {
        g_last_error = e.msg;
        rc = e.code;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        rc = EAST_HIP_ERR_INTERNAL;
    }
    restore_device();
    return rc;
}

extern "C" {

const char *east_hip_version(void) { return "east-hip 0.1 (gfx950)"; }
const char *east_hip_last_error(void) { return g_last_error.c_str(); }

int east_hip_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) {
        g_last_error = "no HIP device available (this library has no CPU fallback)";
        return EAST_HIP_ERR_NO_DEVICE;
    }
    return c;
}

int east_hip_create(int device, int64_t reserve_symbols, east_hip_handle_t *out)
{
    if (out) *out = nullptr;
    return guarded([&] {
        if (!out) east_throw(EAST_HIP_ERR_INVALID, "null out pointer");
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
            east_throw(EAST_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
        if (device < 0 || device >= c) east_throw(EAST_HIP_ERR_NO_DEVICE, "device ordinal out of range");
        if (reserve_symbols < 0 || reserve_symbols >= (i64)0x7FFFFFF0)
            east_throw(EAST_HIP_ERR_INVALID, "reserve_symbols out of range");
        east_hip_index *h = new east_hip_index();
        h->device = device;
        try {
            use_device_ordinal(device);
            HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
            HIP_CHECK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));      // (the streamed text preparation's uploads)
            HIP_CHECK(hipEventCreate(&h->ev0));
            HIP_CHECK(hipEventCreate(&h->ev1));
            h->guess.ensure((TEXT_SYMBOLS + PRESENT_WORDS) * sizeof(u32), "the alphabet of the last build");
            if (reserve_symbols > 0) {
                // (a handle made for builds large enough to go up narrowed -- upload_symbols_narrow -- reserves the narrow
                // staging too: its first east_hip_build does not find the arena a few MB short and grow it.  The upload ring is
                // NOT pinned here: with it in place a fresh handle's first device-resident build measured 3 % slower -- 1.93
                // against 1.86 ms wall for the 64 MiB document, with the ring pinned in the background 3.2 --; the first
                // host-resident build of that size pins it, build_common)
                const bool narrow_size = (u64)reserve_symbols >= SYM_NARROW_MIN && getenv("EAST_HIP_NO_SYMBOL_NARROW") == nullptr;
                const size_t narrow_bytes = narrow_size ? (((size_t)reserve_symbols + 8) * 2 + 255) & ~(size_t)255 : 0;
                ensure_arena(h, plan_arena_bytes((u32)reserve_symbols, 1) + (((size_t)reserve_symbols * 4 + 255) & ~(size_t)255) + narrow_bytes);
            }
        } catch (...) {
            east_hip_destroy(h);
            throw;
        }
        *out = h;
    });
}

void east_hip_destroy(east_hip_handle_t h)
{
    if (!h) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (Consumer *c : h->consumers) delete c;
    if (h->arena.base) (void)hipFree(h->arena.base);
    for (DevBuf *b : h->bufs) b->release();
    for (auto e : h->copy_events) (void)hipEventDestroy(e);
    ring_adopt(h, true);
    for (auto e : h->ring_events) (void)hipEventDestroy(e);
    if (h->ring) (void)hipHostFree(h->ring);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_flags) (void)hipEventDestroy(h->ev_flags);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (cur >= 0 && cur != h->device) (void)hipSetDevice(cur);
    delete h;
}

int east_hip_build(east_hip_handle_t h, const uint32_t *symbols, int64_t n_total, const int64_t *doc_offsets,
                   const int32_t *n_strings, int32_t n_docs)
{
    return guarded([&] { build_common(h, symbols, true, n_total, doc_offsets, n_strings, n_docs, h && h->tagged_input); });
}

int east_hip_build_device(east_hip_handle_t h, const uint32_t *d_symbols, int64_t n_total,
                          const int64_t *doc_offsets, const int32_t *n_strings, int32_t n_docs)
{
    return guarded([&] { build_common(h, d_symbols, false, n_total, doc_offsets, n_strings, n_docs, h && h->tagged_input); });
}

int east_hip_set_symbol_encoding(east_hip_handle_t h, int32_t encoding)
{
    return guarded([&] {
        if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
        if (encoding != EAST_HIP_SYMBOLS_REFERENCE && encoding != EAST_HIP_SYMBOLS_TAGGED)
            east_throw(EAST_HIP_ERR_INVALID, "unknown symbol encoding");
        h->tagged_input = encoding == EAST_HIP_SYMBOLS_TAGGED;
    });
}

int east_hip_prepared_encoding(east_hip_handle_t h)
{
    return h && h->prep_tagged ? EAST_HIP_SYMBOLS_TAGGED : EAST_HIP_SYMBOLS_REFERENCE;
}

int east_hip_build_texts(east_hip_handle_t h, const uint8_t *bytes, int64_t n_bytes, const int64_t *text_offsets,
                         int32_t n_docs, const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                         const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                         int32_t n_hi_upper)
{
    return guarded([&] {
        build_from_texts(h, host_texts_joined(bytes, n_bytes, text_offsets, n_docs), UnicodeTablesHost{cp_class, cp_upper, word_hi, digit_hi, hi_upper_from, hi_upper_to, n_hi_upper});
    });
}

int east_hip_build_texts_v(east_hip_handle_t h, const uint8_t *const *texts, const int64_t *lengths, int32_t n_docs,
                           const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                           const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                           int32_t n_hi_upper)
{
    return guarded([&] {
        build_from_texts(h, host_texts_separate(texts, lengths, n_docs), UnicodeTablesHost{cp_class, cp_upper, word_hi, digit_hi, hi_upper_from, hi_upper_to, n_hi_upper});
    });
}

int east_hip_get_prepared(east_hip_handle_t h, int64_t *n_total, int64_t *doc_offsets, int32_t *n_strings,
                          uint32_t *symbols)
{
    return guarded([&] {
        if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
        if (!h->prep_sym.p || h->prep_doc_off.empty()) east_throw(EAST_HIP_ERR_NOT_BUILT, "no texts have been prepared on this handle");
        use_device(h);
        if (n_total) *n_total = h->prep_n;
        if (doc_offsets) memcpy(doc_offsets, h->prep_doc_off.data(), h->prep_doc_off.size() * sizeof(i64));
        if (n_strings) memcpy(n_strings, h->prep_n_strings.data(), h->prep_n_strings.size() * sizeof(int32_t));
        if (symbols) {
            HIP_CHECK(hipMemcpyAsync(symbols, h->prep_sym.p, (size_t)h->prep_n * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    });
}

double east_hip_last_prep_ms(east_hip_handle_t h) { return h ? (double)h->last_prep_ms : -1.0; }

int east_hip_get_tables(east_hip_handle_t h, int32_t doc, int32_t *suftab, int32_t *lcptab, int32_t *anntab,
                        int32_t *childtab_up, int32_t *childtab_down, int32_t *childtab_next_l_index)
{
    return guarded([&] {
        if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
        if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
        if (doc < 0 || (u32)doc >= h->n_docs) east_throw(EAST_HIP_ERR_INVALID, "document index out of range");
        use_device(h);
        if ((childtab_up || childtab_down || childtab_next_l_index) && !h->child_built) {
            Ctx ctx = handle_ctx(h, &h->arena);
            child_tables(h, ctx);
            h->child_built = true;
        }
        const size_t b = (size_t)h->h_doc_off[doc], nd = (size_t)(h->h_doc_off[doc + 1] - h->h_doc_off[doc]);
        struct { int32_t *dst; const u32 *src; } jobs[6] = {
            {suftab, h->sa}, {lcptab, h->lcp}, {anntab, h->ann},
            {childtab_up, h->up}, {childtab_down, h->down}, {childtab_next_l_index, h->next}};
        for (auto &j : jobs)
            if (j.dst) HIP_CHECK(hipMemcpyAsync(j.dst, j.src + b, nd * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (suftab)
            for (size_t i = 0; i < nd; i++) suftab[i] -= (int32_t)b;      // global -> document-local positions
    });
}

int east_hip_set_keyphrases(east_hip_handle_t h, const uint32_t *q_symbols, const int64_t *q_offsets,
                            int32_t n_keyphrases)
{
    return guarded([&] { set_keyphrases(h, q_symbols, q_offsets, n_keyphrases); });
}

int east_hip_score_resident(east_hip_handle_t h, int normalized, double *d_out)
{
    return guarded([&] {
        // A small table goes to the caller's block from the score kernels themselves (every score written twice: a copy's
        // launch costs more than its bytes).  A large one is copied behind the walk: its 8-byte stores are the strided side
        // of the kernel, and doubling them cost 29 us at 10 000 x 256 where the copy takes 13.
        const bool direct = d_out && h && (u64)h->kp.n_kp * h->n_docs <= SCORE_DIRECT_OUT_MAX;
        score_resident(h, normalized, nullptr, nullptr, direct ? d_out : nullptr);
        if (d_out && !direct)
            HIP_CHECK(hipMemcpyAsync(d_out, h->kp.table, (size_t)h->kp.n_kp * h->n_docs * 8, hipMemcpyDeviceToDevice,
                                     h->stream));
        // (polled, as the build's read-backs are: a sleeping waiter comes back tens of microseconds after a walk this short)
        HIP_CHECK(sync_stream(h->stream));
        HIP_CHECK(hipEventElapsedTime(&h->last_score_ms, h->ev0, h->ev1));
    });
}

int east_hip_score_probes(east_hip_handle_t h, int normalized, int64_t *probes)
{
    return guarded([&] {
        if (!h || !probes) east_throw(EAST_HIP_ERR_INVALID, "null handle or output");
        if (!h->kp.n_kp) east_throw(EAST_HIP_ERR_INVALID, "no keyphrases set");
        use_device(h);
        unsigned long long *d_count = h->kp.buf.as<unsigned long long>();
        HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), h->stream));
        score_resident(h, normalized, d_count);
        unsigned long long c = 0;
        HIP_CHECK(hipMemcpyAsync(&c, d_count, sizeof(c), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *probes = (int64_t)c;
    });
}

int east_hip_score_resident_async(east_hip_handle_t h, int normalized)
{
    return guarded([&] { score_resident(h, normalized); });
}

int east_hip_score_table(east_hip_handle_t h, const uint32_t *q_symbols, const int64_t *q_offsets,
                         int32_t n_keyphrases, int normalized, double *out, double *suffix_out)
{
    return guarded([&] {
        if (!out) east_throw(EAST_HIP_ERR_INVALID, "null output table");
        set_keyphrases(h, q_symbols, q_offsets, n_keyphrases);
        score_resident(h, normalized, nullptr, suffix_out);
        HIP_CHECK(hipMemcpyAsync(out, h->kp.table, (size_t)h->kp.n_kp * h->n_docs * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipEventElapsedTime(&h->last_score_ms, h->ev0, h->ev1));
    });
}

int east_hip_score_table_grouped(east_hip_handle_t h, const uint32_t *q_symbols, const int64_t *q_offsets,
                                 int32_t n_queries, const int64_t *group_offsets, int32_t n_groups, int normalized,
                                 double *out)
{
    return guarded([&] {
        if (!out || !group_offsets || n_groups < 1) east_throw(EAST_HIP_ERR_INVALID, "null output table or no groups");
        if (group_offsets[0] != 0 || group_offsets[n_groups] != n_queries)
            east_throw(EAST_HIP_ERR_INVALID, "group_offsets must start at 0 and end at n_queries");
        for (int32_t g = 0; g < n_groups; g++)
            if (group_offsets[g + 1] <= group_offsets[g]) east_throw(EAST_HIP_ERR_INVALID, "empty group");
        set_keyphrases(h, q_symbols, q_offsets, n_queries);
        std::vector<u32> goff((size_t)n_groups + 1);
        for (int32_t g = 0; g <= n_groups; g++) goff[g] = (u32)group_offsets[g];
        HIP_CHECK(hipMemcpyAsync(h->kp.group_off, goff.data(), goff.size() * 4, hipMemcpyHostToDevice, h->stream));
        score_resident(h, normalized);
        Ctx ctx = handle_ctx(h);
        LAUNCH(ctx, score_group_max_kernel, ceil_div_u32((u64)n_groups * h->n_docs, BLOCK), (const double *)h->kp.table,
               (const u32 *)h->kp.group_off, (u32)n_groups, h->n_docs, h->kp.table_g);
        HIP_CHECK(hipEventRecord(h->ev1, h->stream));
        HIP_CHECK(hipMemcpyAsync(out, h->kp.table_g, (size_t)n_groups * h->n_docs * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));       // (also covers goff)
        HIP_CHECK(hipEventElapsedTime(&h->last_score_ms, h->ev0, h->ev1));
    });
}

int east_hip_get_lcp_intervals(east_hip_handle_t h, int32_t doc, int32_t *left)
{
    return guarded([&] {
        if (!h || !left) east_throw(EAST_HIP_ERR_INVALID, "null handle or output");
        if (!h->built) east_throw(EAST_HIP_ERR_NOT_BUILT, "no index has been built on this handle");
        if (doc < 0 || (u32)doc >= h->n_docs) east_throw(EAST_HIP_ERR_INVALID, "document index out of range");
        use_device(h);
        Ctx ctx = handle_ctx(h);
        const u32 seg = (u32)h->h_doc_off[doc], nd = (u32)(h->h_doc_off[doc + 1] - h->h_doc_off[doc]);
        // (scratch from the arena's temporary region, idle between builds: the child tables stay as they are)
        const size_t mark = h->arena.mark();
        u32 *scratch = h->arena.alloc<u32>(nd);
        interval_lefts(h, ctx, seg, nd, scratch);
        HIP_CHECK(hipMemcpyAsync(left, scratch, (size_t)nd * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->arena.release(mark);
    });
}

int east_hip_reset(east_hip_handle_t h)
{
    return guarded([&] {
        if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
        use_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        // the index and the prepared texts are gone, the handle takes the reference encoding and does not profile
        h->built = h->child_built = h->table_scored = false;
        h->n = h->n_docs = h->sigma_hi = 0;
        h->prep_n = 0;
        h->prep_doc_off.clear();
        h->prep_n_strings.clear();
        h->prep_tagged = h->tagged_input = false;
        h->prof.enabled = false;
        h->prof.only.clear();
        h->stats = Stats();
        // Every group forgets what it holds and keeps its allocation (handle.h).  The plan goes, the hints stay: the next
        // owner's first build speculates on this one's alphabet as a second build on one handle would (hip_backend.py's
        // handle pool counts on it), but decides its sort anew.  What else stays costs time to make and says nothing about
        // an index -- the sizing cache, the upload ring with bytes_refused, the Unicode tables, the alphabet guess --, only
        // ever advances (map_epoch) or reports the last call (last_*_ms, narrow_upload)
        h->plan = SortPlan();
        h->ann_hint = east_hip_index::AnnHint();
        h->ann_order_used = 0;
        h->kg_queued = 0;
        h->kp.forget();
        h->kg.forget();
        h->ht.forget();
        // a recycled handle keeps its stream and a small arena, not gigabytes of side allocations
        const size_t keep = (size_t)64 << 20;
        for (DevBuf *b : h->bufs)
            if (b->cap > keep) b->release();
        for (Consumer *c : h->consumers)
            if (c) c->reset();
    });
}

int east_hip_synchronize(east_hip_handle_t h)
{
    return guarded([&] {
        if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
        use_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

void *east_hip_stream(east_hip_handle_t h) { return h ? (void *)h->stream : nullptr; }

int east_hip_build_info(east_hip_handle_t h, int64_t *out, int32_t cap)
{
    if (!h || !out) return EAST_HIP_ERR_INVALID;
    const int64_t v[31] = {h->n, h->n_docs, h->m_total, h->sigma_t, h->bits0, h->stats.levels,
                           (int64_t)h->arena.cap, (int64_t)h->arena.high, h->stats.radix_passes,
                           h->stats.radix_elems, h->stats.radix_elem_bytes, h->stats.radix_passes_u32,
                           h->stats.radix_elems_u32, h->stats.radix_passes_u64, h->stats.radix_elems_u64,
                           h->stats.levels_resolved, h->stats.merge_elems, h->stats.refine_rounds,
                           h->stats.window_sorted, h->stats.lds_sorted, h->stats.fused_finish, h->stats.first_kept,
                           h->stats.first_n, h->stats.ht_keys, h->stats.seg_sort, h->narrow_upload,
                           h->stats.persist_rounds, h->stats.first_hist_fused, h->ann_order_used, h->kg_queued,
                           h->ann_hint.valid ? (int64_t)h->ann_hint.listed : -1};
    for (int i = 0; i < 31 && i < cap; i++) out[i] = v[i];
    return 31;
}

int east_hip_profile_enable(east_hip_handle_t h, int on)
{
    if (!h) return EAST_HIP_ERR_INVALID;
    return guarded([&] {
        use_device(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->prof.reset();
        h->prof.enabled = on != 0;
    });
}

int east_hip_profile_only(east_hip_handle_t h, const char *kernel)
{
    if (!h) return EAST_HIP_ERR_INVALID;
    h->prof.only = kernel ? kernel : "";
    return EAST_HIP_OK;
}

int64_t east_hip_profile_report(east_hip_handle_t h, char *buf, int64_t cap)
{
    if (!h || !buf || cap < 1) return EAST_HIP_ERR_INVALID;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->prof.collect();
    if (cur >= 0 && cur != h->device) (void)hipSetDevice(cur);
    std::string out;
    for (auto &s : h->prof.sums) {
        char line[256];
        snprintf(line, sizeof(line), "%s\t%lld\t%.6f\n", s.name.c_str(), (long long)s.count, s.ms);
        out += line;
    }
    const int64_t nb = (int64_t)out.size() < cap - 1 ? (int64_t)out.size() : cap - 1;
    memcpy(buf, out.data(), (size_t)nb);
    buf[nb] = 0;
    return (int64_t)out.size();
}

int64_t east_hip_plan_arena_bytes(int64_t n_total, int32_t n_docs)
{
    if (n_total < 1 || n_total >= (i64)0x7FFFFFF0 || n_docs < 1) return EAST_HIP_ERR_INVALID;
    int64_t r = EAST_HIP_ERR_INTERNAL;
    guarded([&] { r = (int64_t)plan_arena_bytes((u32)n_total, (u32)n_docs); });
    return r;
}

int64_t east_hip_plan_arena_bytes_lean(int64_t n_total, int32_t n_docs)
{
    if (n_total < 1 || n_total >= (i64)0x7FFFFFF0 || n_docs < 1) return EAST_HIP_ERR_INVALID;
    int64_t r = EAST_HIP_ERR_INTERNAL;
    guarded([&] { r = (int64_t)plan_arena_bytes((u32)n_total, (u32)n_docs, true); });
    return r;
}

double east_hip_last_build_ms(east_hip_handle_t h) { return h ? (double)h->last_build_ms : -1.0; }
double east_hip_last_score_ms(east_hip_handle_t h) { return h ? (double)h->last_score_ms : -1.0; }

}  // extern "C"

#include "debug_api.h"
// ---- several devices in one process ------------------------------------------------------------------
#include "multi.h"
#include "format.h"
// ---- the consumers (consumer.h), each with its kernels, its state and its entry points -------------------
#include "cosine.h"         // the cosine relevance measure
#include "bm25.h"           // the BM25 relevance measure on the cosine index
#include "graph.h"          // the keyphrase graph
#include "synonyms.h"       // synonym extraction from dependency triples
#include "similarity.h"     // similar texts and keyphrases
#include "top.h"            // ranked keyphrases
#include "related.h"        // text-to-text relatedness
#include "cosine_texts.h"   // text-to-text cosine similarity
#include "clusters.h"       // single-linkage clusters of a square matrix
#include "linkage.h"        // complete and average linkage on a working copy of it
#include "phrases.h"        // repeated phrases of the indexed texts as keyphrase candidates
#include "terms.h"          // characteristic terms of texts and of groups of texts
#include "overlap.h"        // shared-shingle overlap of the texts: resemblance and containment
#include "passages.h"       // the shared passages of pairs of texts: which positions share which wording
