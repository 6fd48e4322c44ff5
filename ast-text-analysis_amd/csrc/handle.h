// handle.h -- what an east_hip_handle_t points to, and the helpers every host driver needs.
#pragma once
#include "common.h"
#include "tables.h"
#include <atomic>
#include <thread>

struct Consumer;            // consumer.h

struct east_hip_index {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Arena arena;
    Stats stats;
    Profiler prof;
    bool built = false, child_built = false;
    u32 n = 0, n_docs = 0, sigma_t = 0, m_total = 0;
    u32 sigma_hi = 0;            // text code points >= U+0A00 present (tagged encoding only): the top sigma_hi codes of the text alphabet
    u32 *hi_bits = nullptr, *hi_rank = nullptr;      // presence bitmap over [U+0A00, U+110000) and its rank directory
    DevBuf guess;                // code map + presence bitmap of the last build (own allocation): what a speculative build starts from
    bool tagged_input = false;   // east_hip_set_symbol_encoding: the symbol entry points take the tagged encoding
    bool prep_tagged = false;    // the prepared symbols (east_hip_build_texts) are in the tagged encoding
    int bits0 = 0;
    std::vector<i64> h_doc_off;
    std::vector<u32> h_n_strings;
    // persistent device arrays (inside the arena)
    uint8_t *s8 = nullptr;
    bool use_s8 = false;
    u32 *s = nullptr, *sa = nullptr, *lcp = nullptr, *ann = nullptr, *up = nullptr, *down = nullptr,
        *next = nullptr, *doc_off = nullptr, *n_strings = nullptr, *code_map = nullptr;
    Pyramid pyr;
    // what the last successful build found, the guesses of the next (speculative) one.  The hints say whether and how far
    // to speculate; east_hip_reset KEEPS them -- a recycled handle's first build speculates on its previous owner's text
    // as a second build on one handle would (the device checks the guess, a wrong one costs a second build)
    struct Hints {
        bool valid = false;
        u32 sigma = 0;                     // the size of the text alphabet
        bool window = false;               // the window sort took it
        bool no_rounds = false;            // ... and left no suffix in a large tie group
    } hint;
    // ... and what that build's window sort did, first radix pass included: a speculative build does the same (build.h:
    // next_plan).  east_hip_reset forgets it: a plan is worth following only on the kind of text it was made on
    SortPlan plan;
    u32 build_docs = 0;          // documents of the build in progress (h->n_docs is set when it has succeeded)
    // ... and how many ranks its ann_wide_kernel decided, of how many tiles: the next build's block order for that kernel
    // (build.h: ann_order -- a short list takes the whole-grid order).  Either order is correct for any table; a stale
    // hint costs time only.  east_hip_reset forgets it
    struct AnnHint {
        bool valid = false;
        u32 listed = 0, n_tiles = 0;
    } ann_hint;
    int ann_order_used = 0;      // the last build's order: 1 grouped, 2 whole-grid (east_hip_build_info [28])
    int kg_queued = 0;           // the last build queued the marked k-gram tables behind its flags read-back: 1, and 2 where the
                                 // flags then said the marks were incomplete (FLAG_KG_BAD: the work is discarded) ([29])
    // The build's small transfers go through one pinned block the handle owns (pageable memory is staged by the runtime: a
    // copy and a blit on the critical path): FLAG_WORDS words the flags come back into, behind them the doc_off /
    // n_strings upload in the device block's layout.  It grows with n_docs and is freed with the handle
    u32 *pin = nullptr;
    size_t pin_words = 0;
    hipEvent_t ev_flags = nullptr;       // recorded right behind the flags copy: what the build waits for
    // the order-preserving variable-length code of the last build that made one (ht_code.h): device tables (own
    // allocation: 256 x u32 enc, 4096 x u16 dec), valid for text with `sigma` text symbols
    struct HtCode {
        DevBuf tab;
        bool valid = false;
        u32 sigma = 0;
        int max_len = 0;
        double mean_len = 0.0;
        void forget() { const DevBuf keep = tab; *this = HtCode(); tab = keep; }
    } ht;
    // the last sizing run (build.h: plan_arena_bytes): its shape and test-knob epoch, its result.  Kept by east_hip_reset
    struct Sized {
        u32 n = 0, docs = 0, epoch = 0;
        bool tagged = false;
        size_t bytes = 0;
    } sized;
    // the resident keyphrases + score scratch (own allocation, grown on demand; laid out by set_keyphrases_device)
    struct Keyphrases {
        DevBuf buf;
        u32 n_kp = 0, n_q = 0, score_chunk = 0;     // score_chunk: documents per stretch the scratch was sized for
        u32 *q_raw = nullptr, *q_code = nullptr, *q_end = nullptr, *q_off = nullptr, *group_off = nullptr;
        u64 q_code_epoch = 0;        // the map_epoch (below) q_code was made under (0: not made -- new keyphrases)
        u32 *q_blk = nullptr;        // whole keyphrases per workgroup of the score walk: [q_blk[i], q_blk[i + 1]), n_blk of them
        u32 n_blk = 0;               // (0: a keyphrase is longer than a workgroup -- the walk writes per-suffix results, a second kernel sums)
        double *suffix = nullptr, *table = nullptr, *table_g = nullptr;
        void forget() { const DevBuf keep = buf; *this = Keyphrases(); buf = keep; }
    } kp;
    // q_code is a function of the resident keyphrases and the code map: map_epoch advances with every build that may have
    // changed the map (all but a speculative build whose alphabet guess was confirmed: same presence bitmap, same map).
    // It only ever advances: no reset puts it back
    u64 map_epoch = 1;
    // k-gram bucket tables for the score walk (own allocation, rebuilt after every build)
    struct Kgram {
        DevBuf buf;
        int k = 0;
        u32 A = 0, bins = 0;
        bool built = false;
        bool marked = false;         // the bucket starts were written by the build (off the window keys): only the fill is due
        bool pairs = false;          // ... in the pair layout (score.h: KgTables); kg3 = the table of the levels above the last,
        u32 *kg3 = nullptr, *up = nullptr;           // up = the small tables of the levels above kg3's own
        u32 up_stride = 0;
        void forget() { const DevBuf keep = buf; *this = Kgram(); buf = keep; }
    } kg;
    float last_build_ms = -1.f, last_score_ms = -1.f, last_prep_ms = -1.f;
    // the caller's Unicode tables of the device text preparation (own allocation, re-uploaded when their hash changes)
    DevBuf tp_tables;
    u64 tp_tables_hash = 0;
    std::vector<uint8_t> tp_host_tables;
    // the streamed text preparation: a copy stream of its own and one event per chunk
    hipStream_t copy_stream = nullptr;     // (created with the handle: creating a stream costs milliseconds)
    std::vector<hipEvent_t> copy_events;
    // ... and a ring of pinned host memory through which MANY separate texts go up (tp_upload_through_ring): allocated on
    // first use, kept with the handle
    char *ring = nullptr;
    std::vector<hipEvent_t> ring_events;
    std::thread ring_alloc;                 // pins the ring in the background after a first call that went without it
    std::atomic<char *> ring_pending{nullptr};
    std::atomic<bool> ring_done{false};     // the background thread is through (with or without a ring): it can be joined without waiting
    int narrow_upload = 0;                  // the last build's host symbols went up as 16-bit words (1) / as bytes (2) (east_hip_build_info [25])
    bool bytes_refused = false;             // a text symbol of 0xFF .. 0x9FF was met on the way up as bytes: this handle's later uploads take 16 bits at once
    bool ring_wanted = false;               // (the call under way would have taken the ring: pin it once the call is over --
                                            // while it runs, the pinning and the call's own copies fight over the runtime's locks)
    // symbols prepared on the device by east_hip_build_texts (own allocation)
    DevBuf prep_sym;
    i64 prep_n = 0;
    std::vector<i64> prep_doc_off;
    std::vector<int32_t> prep_n_strings;
    // the AST score table of the resident keyphrases (h->table) holds the scores of the index as it stands: set by the score
    // walk, withdrawn by every build and every new set of keyphrases (consumer.h: resolve_table hands it out where it lies)
    bool table_scored = false;
    // the consumers (consumer.h): the cosine measure's term index (cosine.h), the keyphrase graph (graph.h), the synonyms'
    // feature rows and pair list (synonyms.h), the ranking (top.h), the similarity matrix (similarity.h), the text-to-text
    // relatedness (related.h), the text-to-text cosine (cosine_texts.h), the clusters (clusters.h), the extracted phrases
    // (phrases.h) and the characteristic terms (terms.h).  Each owns its device allocations and is made by its first call; east_hip_reset and east_hip_destroy go over the array
    // (the tenth, SLOT_TERMS, is numbered behind SLOT_PHR but written behind the count: tests/test_phrases_host.py reads the
    // first line of the enum as it stood when the phrases were the last consumer; the eleventh, SLOT_OVL -- the shingle
    // overlap, overlap.h -- follows it there, and the twelfth, SLOT_PAS -- the shared passages, passages.h -- follows that)
    enum { SLOT_COS, SLOT_GRAPH, SLOT_SYN, SLOT_TOP, SLOT_SIM, SLOT_REL, SLOT_COSTEXT, SLOT_CLU, SLOT_PHR, N_CONSUMERS = SLOT_PHR + 4,
           SLOT_TERMS = SLOT_PHR + 1, SLOT_OVL = SLOT_PHR + 2, SLOT_PAS = SLOT_PHR + 3 };
    Consumer *consumers[N_CONSUMERS] = {};
    // the handle's own device allocations besides the arena: east_hip_destroy frees them, east_hip_reset the large ones
    // (a DevBuf has no destructor: the groups' forget() carries theirs over)
    DevBuf *bufs[6] = {&guess, &ht.tab, &kp.buf, &kg.buf, &tp_tables, &prep_sym};
};

struct SpecAbort {};             // a speculative build cannot go on: build_common starts over with the read-backs in place

// Every entry point runs on the handle's device and puts the calling thread's current device back on the way
// out (a caller that also drives torch or other HIP code on another GPU must not find its device changed).
static thread_local int g_saved_device = -1;
static void use_device_ordinal(int device)
{
    int cur = -1;
    if (g_saved_device < 0 && hipGetDevice(&cur) == hipSuccess && cur != device) g_saved_device = cur;
    HIP_CHECK(hipSetDevice(device));
}
static void use_device(east_hip_index *h) { use_device_ordinal(h->device); }
static void restore_device()
{
    if (g_saved_device >= 0) { (void)hipSetDevice(g_saved_device); g_saved_device = -1; }
}

// the handle's pinned block with room for `words` words (what it held is lost when it grows)
static void ensure_pin(east_hip_index *h, size_t words)
{
    if (!h->ev_flags) HIP_CHECK(hipEventCreateWithFlags(&h->ev_flags, hipEventDisableTiming));
    if (words <= h->pin_words) return;
    HIP_CHECK(hipStreamSynchronize(h->stream));      // (a copy out of the old block may still be queued)
    if (h->pin) (void)hipHostFree(h->pin);
    h->pin = nullptr;
    h->pin_words = 0;
    void *p = nullptr;
    const size_t grown = std::max(words + words / 2, (size_t)1024);
    HIP_CHECK(hipHostMalloc(&p, grown * sizeof(u32), hipHostMallocDefault));
    h->pin = (u32 *)p;
    h->pin_words = grown;
}

// a launch context on the handle's stream, timed by its profiler (arena, stats: what the caller's launches need of them)
static Ctx handle_ctx(east_hip_index *h, Arena *arena = nullptr, Stats *stats = nullptr)
{
    Ctx ctx;
    ctx.stream = h->stream;
    ctx.arena = arena;
    ctx.stats = stats;
    ctx.prof = &h->prof;
    return ctx;
}
