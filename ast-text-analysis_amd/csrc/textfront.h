// textfront.h -- the host side of textprep.h: raw UTF-8 texts go up, are prepared on the device and built from.
#pragma once
#include "build.h"
#include "textprep.h"
#include <string.h>

#define TP_WORD_HI_WORDS ((0x110000u - TP_TEXT_LIMIT + 31u) / 32u)

// ---- the input: D raw texts, joined or apart --------------------------------------------------------------------------
// Joined: `bytes` holds the texts, each followed by one 0xFF byte.  Apart: text d = texts[d], never joined on the host;
// text_offsets then says where the texts would lie if they were joined with their separators.
struct HostTexts {
    const uint8_t *bytes = nullptr;
    const uint8_t *const *texts = nullptr;
    const i64 *text_offsets = nullptr;      // D + 1
    int32_t D = 0;
    i64 n_bytes = 0;                        // of the joined stream, separators included
    std::vector<i64> own_offsets;           // what text_offsets points to when the input came as lengths
    std::vector<u32> off32;                 // the offsets as the device takes them (host_texts_check)
    HostTexts() = default;
    HostTexts(HostTexts &&) = default;      // (no copies: text_offsets may point into own_offsets)
};

static HostTexts host_texts_joined(const uint8_t *bytes, i64 n_bytes, const i64 *text_offsets, int32_t n_docs)
{
    HostTexts in;
    in.bytes = bytes; in.text_offsets = text_offsets; in.D = n_docs; in.n_bytes = n_bytes;
    return in;
}

static HostTexts host_texts_separate(const uint8_t *const *texts, const i64 *lengths, int32_t n_docs)
{
    if (!texts || !lengths || n_docs < 1) east_throw(EAST_HIP_ERR_INVALID, "null argument or no documents");
    HostTexts in;
    in.own_offsets.assign((size_t)n_docs + 1, 0);
    for (int32_t d = 0; d < n_docs; d++) {
        if (lengths[d] < 0) east_throw(EAST_HIP_ERR_INVALID, "negative text length");
        in.own_offsets[d + 1] = in.own_offsets[d] + lengths[d] + 1;                 // + the separator
    }
    in.texts = texts; in.text_offsets = in.own_offsets.data(); in.D = n_docs; in.n_bytes = in.own_offsets[n_docs];
    return in;
}

// The caller's Unicode tables (hip_backend.py: unicode_tables()).
struct UnicodeTablesHost {
    const uint8_t *cp_class;
    const u32 *cp_upper, *word_hi, *digit_hi, *hi_upper_from, *hi_upper_to;
    int32_t n_hi_upper;
    bool ok() const { return cp_class && cp_upper && word_hi && digit_hi && n_hi_upper >= 0 && (n_hi_upper == 0 || (hi_upper_from && hi_upper_to)); }
};

// The one check of a text input (after it the sizes fit 32 bits: off32).  Missing tables and missing texts are one error.
static void host_texts_check(HostTexts &in, const UnicodeTablesHost &tables)
{
    if ((!in.bytes && !in.texts) || !in.text_offsets || !tables.ok() || in.D < 1) east_throw(EAST_HIP_ERR_INVALID, "null argument or no documents");
    if (in.n_bytes < in.D || in.n_bytes >= (i64)0x7FFFFFF0) east_throw(EAST_HIP_ERR_INVALID, "total bytes out of range");
    const i64 *off = in.text_offsets;
    if (off[0] != 0 || off[in.D] != in.n_bytes) east_throw(EAST_HIP_ERR_INVALID, "text_offsets must start at 0 and end at the total");
    in.off32.assign((size_t)in.D + 1, 0);
    for (int32_t d = 0; d < in.D; d++) {
        if (off[d + 1] <= off[d]) east_throw(EAST_HIP_ERR_INVALID, "text_offsets must increase");
        if (in.texts ? (off[d + 1] - off[d] > 1 && !in.texts[d]) : in.bytes[off[d + 1] - 1] != 0xFFu)
            east_throw(EAST_HIP_ERR_INVALID, in.texts ? "null text" : "every text must be followed by one 0xFF separator byte");
        in.off32[d + 1] = (u32)off[d + 1];
    }
}

// ---- the streamed preparation (textprep.h, "the streamed preparation") --------------------------------------------
// -1: streamed for inputs of TP_STREAM_MIN bytes or more, in about TP_STREAM_CHUNKS chunks; 0: never; > 0: always, in chunks
// of about that many bytes (east_hip_debug_set_text_stream: the tests push the fixtures through chunks of a few dozen bytes)
#define TP_STREAM_MIN ((u32)8 << 20)
#define TP_STREAM_CHUNKS 4

struct TpChunk {
    u32 b0 = 0, b1 = 0;             // bytes [b0, b1) of the concatenated stream (separators included)
    u32 doc_first = 0, n_docs = 0;  // the documents it touches
    bool cont_in = false, cont_out = false;
    std::vector<u32> text_off;      // n_docs + 1: where they start, relative to b0 (the last entry = b1 - b0)
};

// byte p of the concatenated stream (document d holds it)
static inline u32 tp_byte_at(const HostTexts &in, u32 d, u32 p)
{
    if (p + 1 == in.off32[d + 1]) return 0xFFu;                       // the separator
    return in.texts ? in.texts[d][p - in.off32[d]] : in.bytes[p];
}

// Cuts of the stream where neither a token nor a UTF-8 unit can span them: behind a separator, or behind an ASCII byte
// that is no word character (looked for in the 4 KiB in front of where the chunk would end; a document without one there
// -- one endless token, binary junk -- stays whole).
static std::vector<TpChunk> tp_plan_chunks(const HostTexts &in, u32 chunk_bytes, const uint8_t *cls256)
{
    const u32 *text_offsets = in.off32.data();
    const u32 n_bytes = (u32)in.n_bytes;
    // (the first chunk is a quarter of the others: the preparation -- the slower side -- starts that much earlier)
    const u32 first_div = getenv("EAST_HIP_TP_FIRST_DIV") ? (u32)std::max(1, atoi(getenv("EAST_HIP_TP_FIRST_DIV"))) : 4u;   // (experiments)
    std::vector<TpChunk> chunks;
    u32 pos = 0, d = 0;                                  // d: the document that holds byte pos
    while (pos < n_bytes) {
        u32 cut = n_bytes;
        const u32 want = pos == 0 && chunk_bytes >= 4096u ? chunk_bytes / first_div : chunk_bytes;
        if ((u64)pos + want < n_bytes) {
            const u32 target = pos + want;
            u32 dt = d;
            while ((u32)text_offsets[dt + 1] < target) dt++;         // the document that holds byte target - 1
            cut = (u32)text_offsets[dt + 1];                         // (its end, unless a cut inside it is found)
            const u32 lowest = std::max(pos + 1, target > 4096u ? target - 4096u : 0u);
            for (u32 q = target; q-- > lowest;) {
                if (q < (u32)text_offsets[dt]) { cut = (u32)text_offsets[dt]; break; }     // (the document starts in the window: cut in front of it)
                const u32 c = tp_byte_at(in, dt, q);
                if (c == 0xFFu || (c < 0x80u && !(cls256[c] & TP_CLASS_WORD))) { cut = q + 1; break; }
            }
        }
        TpChunk ch;
        ch.b0 = pos; ch.b1 = cut;
        while ((u32)text_offsets[d + 1] <= pos) d++;
        ch.doc_first = d;
        ch.cont_in = pos > (u32)text_offsets[d];
        u32 dl = d;
        ch.text_off.push_back(0);
        while ((u32)text_offsets[dl + 1] < cut) { ch.text_off.push_back((u32)text_offsets[dl + 1] - pos); dl++; }
        ch.text_off.push_back(cut - pos);
        ch.n_docs = dl - d + 1;
        ch.cont_out = cut < (u32)text_offsets[dl + 1];
        chunks.push_back(std::move(ch));
        pos = cut;
    }
    return chunks;
}

static thread_local std::chrono::steady_clock::time_point g_tp_call_start;     // (EAST_HIP_TRACE: when build_from_texts was entered)

// ---- many separate texts: through a ring of pinned memory -------------------------------------------------------------
// A copy out of pageable memory is pinned in place by the runtime, copied, unpinned: ~45 us of set-up per call, which a
// 64 MiB text hides and 64 texts of 1 MiB do not (2.75 ms against 1.5 ms; 256 x 1 MiB: 11 ms).  Separate texts of less
// than TP_RING_MAX_TEXT bytes on average therefore go through TP_RING_SLOTS slots of pinned memory: a few host threads
// copy the stream -- text bytes and the 0xFF separators -- into a slot, each its share, while the slots before it are on
// their way to the device (one DMA per slot and chunk, no set-up); the uploader thread alone talks to the runtime.
#define TP_RING_MAX_TEXT ((u64)8 << 20)
#define TP_RING_FIRST_TEXTS 128u              // a handle's first call pins the ring in line only for this many texts or more

// bytes [a, b) of the concatenated stream (the texts of `in`, which lie apart, with their 0xFF separators) -> dst
static void tp_fill_stream(char *dst, u64 a, u64 b, const HostTexts &in)
{
    const i64 *text_offsets = in.text_offsets;
    u32 d = (u32)(std::upper_bound(text_offsets, text_offsets + in.D + 1, (i64)a) - text_offsets) - 1u;
    while (a < b) {
        const u64 t0 = (u64)text_offsets[d], sep = (u64)text_offsets[d + 1] - 1u;      // text d = [t0, sep), then its separator
        if (a < sep) {
            const u64 e = std::min(b, sep);
            memcpy(dst, in.texts[d] + (a - t0), (size_t)(e - a));
            dst += e - a;
            a = e;
        }
        if (a == sep && a < b) { *dst++ = (char)0xFF; a++; }
        if (a > sep) d++;
    }
}

// The caller's Unicode tables (290 KB) stay on the device between calls (own allocation): they are uploaded again only
// when their content changes -- a 64-bit hash over all of them, taken while the text is on its way.  With them go the two
// 256-entry tables of the byte-wise fast path (class and upper-cased code point of a byte that is a code point of its own).
struct TpDevTables {
    TpTables t;
    const uint8_t *cls256;     // the 256-entry tables of the byte-wise fast path
    const u32 *up256;
};
static TpDevTables tp_upload_tables(east_hip_index *h, const UnicodeTablesHost &u)
{
    const auto [cp_class, cp_upper, word_hi, digit_hi, hi_upper_from, hi_upper_to, n_hi_upper] = u;
    const size_t tb_class = 0, tb_upper = tb_class + TP_TEXT_LIMIT, tb_word = tb_upper + (size_t)TP_TEXT_LIMIT * 4,
                 tb_digit = tb_word + (size_t)TP_WORD_HI_WORDS * 4, tb_from = tb_digit + (size_t)TP_WORD_HI_WORDS * 4,
                 tb_to = tb_from + ((size_t)n_hi_upper + 1) * 4, tb_cls256 = tb_to + ((size_t)n_hi_upper + 1) * 4,
                 tb_up256 = tb_cls256 + 256, tb_total = tb_up256 + 1024;
    {
        u64 hash = 0x9E3779B97F4A7C15ull ^ (u64)n_hi_upper;
        auto mix = [&](const void *p, size_t bytes) {
            const u64 *q = (const u64 *)p;
            for (size_t i = 0; i < bytes / 8; i++) hash = (hash ^ q[i]) * 0x100000001B3ull + (hash >> 29);
        };
        mix(cp_class, TP_TEXT_LIMIT); mix(cp_upper, (size_t)TP_TEXT_LIMIT * 4); mix(word_hi, (size_t)TP_WORD_HI_WORDS * 4);
        mix(digit_hi, (size_t)TP_WORD_HI_WORDS * 4);
        for (int32_t q = 0; q < n_hi_upper; q++) hash = (hash ^ (((u64)hi_upper_from[q] << 32) | hi_upper_to[q])) * 0x100000001B3ull + (hash >> 29);
        if (h->tp_tables.cap < tb_total || h->tp_tables_hash != hash) {
            h->tp_tables.ensure(tb_total, "the Unicode tables", h->stream);
            h->tp_host_tables.resize(256 + 1024);
            uint8_t *cls256 = h->tp_host_tables.data();
            u32 *up256 = reinterpret_cast<u32 *>(h->tp_host_tables.data() + 256);
            for (u32 x = 0; x < 256; x++) {              // (as tp_decode_kernel: upper first, then the class of the result)
                u32 cp = x < 0x80u ? cp_upper[x] : TP_REPLACEMENT;
                if (cp >= TP_TEXT_LIMIT) {
                    for (int32_t q = 0; q < n_hi_upper; q++)
                        if (hi_upper_from[q] == cp) { cp = hi_upper_to[q]; break; }
                }
                u32 cls;
                if (cp < TP_TEXT_LIMIT) cls = cp_class[cp];
                else { const u32 k = cp - TP_TEXT_LIMIT; cls = ((word_hi[k >> 5] >> (k & 31u)) & 1u) | (((digit_hi[k >> 5] >> (k & 31u)) & 1u) << 1); }
                cls256[x] = (uint8_t)cls;
                up256[x] = cp;
            }
            char *t = h->tp_tables.p;
            HIP_CHECK(hipMemcpyAsync(t + tb_class, cp_class, TP_TEXT_LIMIT, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(t + tb_upper, cp_upper, (size_t)TP_TEXT_LIMIT * 4, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(t + tb_word, word_hi, (size_t)TP_WORD_HI_WORDS * 4, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(t + tb_digit, digit_hi, (size_t)TP_WORD_HI_WORDS * 4, hipMemcpyHostToDevice, h->stream));
            if (n_hi_upper) {
                HIP_CHECK(hipMemcpyAsync(t + tb_from, hi_upper_from, (size_t)n_hi_upper * 4, hipMemcpyHostToDevice, h->stream));
                HIP_CHECK(hipMemcpyAsync(t + tb_to, hi_upper_to, (size_t)n_hi_upper * 4, hipMemcpyHostToDevice, h->stream));
            }
            HIP_CHECK(hipMemcpyAsync(t + tb_cls256, cls256, 256, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(t + tb_up256, up256, 1024, hipMemcpyHostToDevice, h->stream));
            h->tp_tables_hash = hash;                   // (the read-back below waits for the stream: the host buffers are the caller's / the handle's)
        }
    }
    const uint8_t *d_class = (const uint8_t *)(h->tp_tables.p + tb_class), *d_cls256 = (const uint8_t *)(h->tp_tables.p + tb_cls256);
    const u32 *d_upper = (const u32 *)(h->tp_tables.p + tb_upper), *d_word_hi = (const u32 *)(h->tp_tables.p + tb_word),
              *d_digit_hi = (const u32 *)(h->tp_tables.p + tb_digit), *d_hi_from = (const u32 *)(h->tp_tables.p + tb_from),
              *d_hi_to = (const u32 *)(h->tp_tables.p + tb_to), *d_up256 = (const u32 *)(h->tp_tables.p + tb_up256);
    return TpDevTables{TpTables{d_class, d_upper, d_word_hi, d_digit_hi, d_hi_from, d_hi_to, (u32)n_hi_upper}, d_cls256, d_up256};
}

// ---- the streamed preparation, one chunk ------------------------------------------------------------------------------
// device state shared by the chunks
struct TpStreamState {
    TpCarry *carry;                 // [2]: what chunk c reads of its first document, chunk c + 1 writes
    u32 *d_high, *doc_sym_off_all, *m_all, *prep_sym;
};

// per-chunk scratch (sized for the largest chunk, used by one chunk after the other)
struct TpChunkScratch {
    u32 *d_text_off, *byte_prefix, *tok_prefix, *cpu, *doc_cp_off, *tstart, *tend, *tok_nd, *keep, *klen, *keep_ex, *klen_ex, *first_tok, *n_loc,
        *off_loc, *kept_tot, *chars_tot;
    uint8_t *cw;
    uint4 *tok_rec;
    void alloc(Arena &ar, u32 nb_max, u32 dl_max, u32 ub_tok)
    {
        d_text_off = ar.alloc<u32>((size_t)dl_max + 1);
        byte_prefix = ar.alloc<u32>((size_t)nb_max / TP_RANK_BLOCK + 2), tok_prefix = ar.alloc<u32>((size_t)nb_max / TP_RANK_BLOCK + 2);
        cpu = ar.alloc<u32>(nb_max);
        cw = ar.alloc<uint8_t>((size_t)nb_max + 32);
        doc_cp_off = ar.alloc<u32>((size_t)dl_max + 1);
        tstart = ar.alloc<u32>(ub_tok), tend = ar.alloc<u32>(ub_tok);
        // (tok_nd, keep and klen side by side: one fill per chunk)
        tok_nd = ar.alloc<u32>(3 * ((size_t)ub_tok + 1)), keep = tok_nd + ((size_t)ub_tok + 1), klen = keep + ((size_t)ub_tok + 1);
        keep_ex = ar.alloc<u32>((size_t)ub_tok + 1), klen_ex = ar.alloc<u32>((size_t)ub_tok + 1);
        tok_rec = ar.alloc<uint4>(ub_tok);
        first_tok = ar.alloc<u32>((size_t)dl_max + 1), n_loc = ar.alloc<u32>((size_t)dl_max + 1);
        off_loc = ar.alloc<u32>((size_t)dl_max + 1), kept_tot = ar.alloc<u32>(dl_max), chars_tot = ar.alloc<u32>(dl_max);
    }
};

// Chunk c, whose bytes are on the device and hold n_cp code points: bytes -> code points -> tokens -> the symbols of its
// documents, behind what the chunks before it emitted.
static void tp_prepare_chunk(Ctx &ctx, const TpChunkScratch &s, const TpChunk &ch, u32 c, u32 n_cp, const uint8_t *d_bytes,
                             const TpDevTables &tb, const TpStreamState &st)
{
    const u32 nb = ch.b1 - ch.b0, Dl = ch.n_docs;
    const uint8_t *b = d_bytes + ch.b0;
    HIP_CHECK(hipMemcpyAsync(s.d_text_off, ch.text_off.data(), ((size_t)Dl + 1) * 4, hipMemcpyHostToDevice, ctx.stream));
    // bytes -> code points (a chunk in which every byte is a code point of its own needs no index)
    const bool bytewise = n_cp == nb;
    const u32 *ranks = bytewise ? nullptr : s.byte_prefix;
    if (bytewise) {
        LAUNCH(ctx, tp_classify_bytes_kernel, ceil_div_u32(nb, BLOCK * 16), b, nb, tb.cls256, s.cw);
    } else {
        const u32 n_bblk = ceil_div_u32(nb, TP_RANK_BLOCK);
        LAUNCH(ctx, (tp_block_counts_kernel<TpStartIn>), ceil_div_u32((u64)n_bblk + 1, 8), TpStartIn{b, nb}, nb, n_bblk, s.byte_prefix);
        device_scan<ArrIn, false>(ctx, ArrIn{s.byte_prefix}, n_bblk + 1, s.byte_prefix);
        LAUNCH(ctx, tp_decode_kernel, ceil_div_u32(nb, BLOCK), b, nb, ranks, tb.t, s.cpu, s.cw);
    }
    LAUNCH(ctx, tp_doc_cp_offsets_kernel, ceil_div_u32(Dl + 1, WAVES_PER_BLOCK), b, nb, ranks, s.d_text_off, Dl, s.doc_cp_off);
    // code points -> tokens (their number stays on the device: the last entry of the blocks' prefix sums)
    const u32 n_tblk = ceil_div_u32(n_cp, TP_RANK_BLOCK);
    LAUNCH(ctx, (tp_block_counts_kernel<TpTokStartIn>), ceil_div_u32((u64)n_tblk + 1, 8), TpTokStartIn{s.cw, n_cp}, n_cp, n_tblk, s.tok_prefix);
    device_scan<ArrIn, false>(ctx, ArrIn{s.tok_prefix}, n_tblk + 1, s.tok_prefix);
    const u32 *n_tok_dev = s.tok_prefix + n_tblk;
    const u32 ub = n_cp / 2 + 2;
    // (everything over the tokens is bounded by their number on the device -- a third to a quarter of the upper bound ub:
    // the zeroing, and ONE scan for kept tokens and kept symbols together, scan.h: device_scan_pair_bounded)
    LAUNCH(ctx, tp_zero_tokens_kernel, ceil_div_u32((u64)ub + 1, BLOCK * 4), s.tok_nd, s.keep, s.klen, ub, n_tok_dev);
    LAUNCH(ctx, tp_token_bounds_kernel, ceil_div_u32(n_cp, BLOCK * TP_VEC), s.cw, s.tok_prefix, n_cp, s.tstart, s.tend, s.tok_nd);
    LAUNCH(ctx, tp_token_keep_kernel, ceil_div_u32(ub, BLOCK), s.tstart, s.tend, s.tok_nd, ub, s.keep, s.klen, n_tok_dev);
    device_scan_pair_bounded(ctx, s.keep, s.klen, ub + 1, n_tok_dev, 1u, s.keep_ex, s.klen_ex);
    // tokens -> the documents' strings and symbols, with what earlier chunks emitted of the first document
    const TpCarry *cin = st.carry + (c & 1u);
    TpCarry *cout = st.carry + ((c + 1u) & 1u);
    LAUNCH(ctx, tp_stream_docs_kernel, ceil_div_u32(Dl + 1, WAVES_PER_BLOCK), s.doc_cp_off, s.cw, n_cp, s.tok_prefix, s.keep_ex, s.klen_ex, Dl, ch.cont_in, ch.cont_out,
           cin, s.first_tok, s.n_loc, s.kept_tot, s.chars_tot);
    device_scan<ArrIn, false>(ctx, ArrIn{s.n_loc}, Dl + 1, s.off_loc);
    LAUNCH(ctx, tp_stream_token_out_kernel, ceil_div_u32(ub, BLOCK), s.tstart, s.tend, s.keep_ex, s.klen_ex, s.doc_cp_off, s.first_tok, s.off_loc,
           s.kept_tot, Dl, ch.cont_in, ch.cont_out, cin, n_tok_dev, s.tok_rec);
    LAUNCH(ctx, tp_emit_kernel, ceil_div_u32(n_cp, BLOCK), bytewise ? nullptr : s.cpu, b, tb.up256, s.cw, s.tok_prefix, s.tok_rec, n_cp, st.prep_sym,
           st.d_high);
    LAUNCH(ctx, tp_stream_close_docs_kernel, ceil_div_u32(Dl, BLOCK), s.off_loc, s.n_loc, s.kept_tot, s.chars_tot, Dl, ch.doc_first, ch.cont_in, ch.cont_out, cin, cout,
           st.doc_sym_off_all, st.m_all, st.prep_sym);
}

// Prepares the collection chunk by chunk; the symbols end up in h->prep_sym, the per-document offsets and string counts in
// h_off / h_m.  Returns false when the monolithic preparation has to take over: kept text at or above U+0A00 (the tagged
// encoding rewrites terminators the chunks no longer remember).  d_bytes: n_bytes + 32 bytes of the arena, nothing uploaded yet.
static bool prepare_texts_streamed(east_hip_index *h, Ctx &ctx, const HostTexts &in, u32 chunk_bytes, uint8_t *d_bytes,
                                   const TpDevTables &tb, std::vector<u32> &h_off, std::vector<u32> &h_m)
{
    Arena &ar = *ctx.arena;
    const uint8_t *bytes = in.bytes, *const *texts = in.texts;
    const i64 *text_offsets = in.text_offsets;
    const u32 D = (u32)in.D, n_bytes = (u32)in.n_bytes;
    const std::vector<TpChunk> chunks = tp_plan_chunks(in, chunk_bytes, h->tp_host_tables.data());
    const u32 C = (u32)chunks.size();
    u32 nb_max = 0, dl_max = 0;
    for (const TpChunk &c : chunks) { nb_max = std::max(nb_max, c.b1 - c.b0); dl_max = std::max(dl_max, c.n_docs); }
    if (!h->copy_stream) HIP_CHECK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    while (h->copy_events.size() < C) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->copy_events.push_back(e);
    }
    // the symbols: every kept code point one, every string of three tokens (of three code points or more) a terminator,
    // an empty document two
    const size_t sym_cap = (size_t)n_bytes + (size_t)n_bytes / 9 + 2 * (size_t)D + 64;
    h->prep_sym.ensure(sym_cap * 4, "the prepared symbols", h->stream);
    // ---- device state shared by the chunks ----
    const TpStreamState st{ar.alloc<TpCarry>(2), ar.alloc<u32>(1), ar.alloc<u32>((size_t)D + 1), ar.alloc<u32>(D), h->prep_sym.as<u32>()};
    HIP_CHECK(hipMemsetAsync(st.carry, 0, 2 * sizeof(TpCarry), h->stream));
    HIP_CHECK(hipMemsetAsync(st.d_high, 0, 4, h->stream));
    TpChunkScratch scratch;
    scratch.alloc(ar, nb_max, dl_max, nb_max / 2 + 2);   // (tokens: one needs a character and something behind it)
    // (the counts of the chunks: on the copy stream, each into a stretch of its own -- the host reads chunk c's while
    // chunk c + 1's may already be written)
    std::vector<u32> cnt_off(C + 1, 0);
    for (u32 c = 0; c < C; c++) cnt_off[c + 1] = cnt_off[c] + ceil_div_u32((u64)(chunks[c].b1 - chunks[c].b0) + 1, SCAN_TILE);
    u32 *cp_sums_aux = ar.alloc<u32>(cnt_off[C]);
    std::vector<std::vector<u32>> h_counts(C);
    for (u32 c = 0; c < C; c++) h_counts[c].resize(cnt_off[c + 1] - cnt_off[c]);

    // ---- the uploads: a thread of their own (a copy out of pageable memory returns when it is staged) ----
    // (ONE uploader: two threads with a copy stream each, the chunks' halves side by side, were measured and are slower --
    // 2.9 against 1.95 ms for 64 MiB: the staging copies of the runtime do not run side by side.  More, smaller chunks
    // towards the end -- a shorter tail behind the last upload -- lose to their launches and read-backs: 2.3 ms with six.)
    std::atomic<int> uploaded{0}, upload_failed{0}, upload_abort{0};
    // The copy stream writes d_bytes (the bottom of the arena) and the chunks' counts: it must not start before what is
    // still queued on the handle's stream -- a score call of the index before, say, reading its tables in the arena --
    // has finished ("one HIP stream per handle": calls are ordered).  ev0 was recorded on h->stream when this call began.
    HIP_CHECK(hipStreamWaitEvent(h->copy_stream, h->ev0, 0));
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    const double t_before = std::chrono::duration<double, std::milli>(t_begin - g_tp_call_start).count();
    std::atomic<double> t_first_fill{0.0}, t_first_dma{0.0};
    std::vector<double> t_up(C, 0.0), t_cnt(C, 0.0), t_queued(C, 0.0);     // (EAST_HIP_TRACE: when a chunk was staged / counted / queued)
    const int device = h->device;
    hipStream_t copy_stream = h->copy_stream;
    const std::vector<hipEvent_t> &events = h->copy_events;
    // (the ring: see tp_fill_stream above)
    // Pinning the ring costs 3-5 ms (hipHostMalloc of 24 MiB), a copy out of pageable memory ~45 us: a handle's FIRST call
    // takes the ring only where that pays at once (TP_RING_FIRST_TEXTS texts or more) -- otherwise it goes the old way and
    // leaves the pinning to a background thread, for the calls after it (`east keyphrases table` over a few dozen files
    // is one call: 64 texts of 1 MiB, first call 11.4-13 ms with the ring pinned in line, second call 5.9).
    ring_adopt(h, ctx.knobs.tp_ring > 0);
    const bool ring_shape = texts && ctx.knobs.tp_ring != 0 && (ctx.knobs.tp_ring > 0 || (D >= 4 && (u64)n_bytes / D < TP_RING_MAX_TEXT));
    const bool use_ring = ring_shape && (h->ring || ctx.knobs.tp_ring > 0 || D >= TP_RING_FIRST_TEXTS);
    if (ring_shape && !use_ring && !h->ring_alloc.joinable() && !h->ring_pending.load()) h->ring_wanted = true;   // (pinned when this call is over: ring_pin_later)
    const size_t ring_slot = ctx.knobs.tp_ring_slot;
    const u32 n_slots = use_ring ? ceil_div_u32(n_bytes, ring_slot) : 0u;
    // (fill threads: three -- measured on the 256-thread host of the MI355X box, 64 texts of 1 MiB: 4 threads 2.25 ms of
    // preparation, 8: 2.3-2.6, 16: 2.6, 32: 2.95 -- starting the threads costs more than their copies save; a 16 MiB
    // chunk is staged in 0.45 ms either way, 37 GB/s)
    static const int ring_threads_env = getenv("EAST_HIP_RING_THREADS") ? atoi(getenv("EAST_HIP_RING_THREADS")) : 0;     // (experiments)
    const int n_fill = !use_ring ? 0 : ring_threads_env > 0 ? std::min(ring_threads_env, 64)
                                     : (int)std::min<u32>(3u, std::max<u32>(2u, std::thread::hardware_concurrency() / 2u));
    if (use_ring && !h->ring) ring_adopt(h, true);       // (a background pin under way: its ring, not a second one)
    if (use_ring) {
        const bool had_ring = h->ring != nullptr;
        if (!ring_pin_now(h)) east_throw(EAST_HIP_ERR_OOM, "hipHostMalloc of the upload ring failed");
        if (g_trace && !had_ring)
            fprintf(stderr, "[east_hip] text preparation: pinned ring of %zu MiB allocated, %.2f ms into the call\n", (TP_RING_SLOT * TP_RING_SLOTS) >> 20,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_tp_call_start).count());
    }
    std::vector<std::atomic<int>> slot_parts(n_slots);         // fill threads done with their share of a slot
    for (auto &a : slot_parts) a.store(0, std::memory_order_relaxed);
    std::atomic<u32> slots_free{TP_RING_SLOTS};                 // stream slots [0, slots_free) may be filled (their ring slot's last DMA is done)
    char *ring = h->ring;
    std::vector<std::thread> fillers;
    for (int j = 0; j < n_fill; j++)
        fillers.emplace_back([&, j]() {
            for (u32 sl = 0; sl < n_slots; sl++) {
                while (slots_free.load(std::memory_order_acquire) <= sl) {
                    if (upload_abort.load(std::memory_order_acquire)) return;
                    std::this_thread::yield();
                }
                const u64 a = (u64)sl * ring_slot, len = std::min<u64>(ring_slot, (u64)n_bytes - a);
                const u64 lo = a + len * (u64)j / (u64)n_fill, hi = a + len * (u64)(j + 1) / (u64)n_fill;
                if (hi > lo) tp_fill_stream(ring + (size_t)(sl % TP_RING_SLOTS) * ring_slot + (lo - a), lo, hi, in);
                if (slot_parts[sl].fetch_add(1, std::memory_order_release) + 1 == n_fill && sl == 0) t_first_fill.store(since());
            }
        });
    const std::vector<hipEvent_t> &ring_events = h->ring_events;
    std::thread uploader([&, device, copy_stream]() {
        bool ok = hipSetDevice(device) == hipSuccess;
        if (ok && texts && !use_ring) ok = hipMemsetAsync(d_bytes, 0xFF, n_bytes, copy_stream) == hipSuccess;       // the separators
        if (ok) ok = hipMemsetAsync(d_bytes + n_bytes, 0, 32, copy_stream) == hipSuccess;
        u32 sl_next = 0;                                          // (ring) the next stream slot to send, and how far it has been sent
        u64 sent = 0;
        for (u32 c = 0; c < C && ok && !upload_abort.load(std::memory_order_acquire); c++) {
            const TpChunk &ch = chunks[c];
            if (use_ring) {
                // the chunk's bytes: the pieces of the slots it overlaps, one DMA each; a slot is handed back to the fill
                // threads when the DMA of its last piece is done (waited for one slot behind, so that the next is queued)
                while (ok && sent < ch.b1) {
                    while (slot_parts[sl_next].load(std::memory_order_acquire) < n_fill) {
                        if (upload_abort.load(std::memory_order_acquire)) { ok = false; break; }
                        std::this_thread::yield();
                    }
                    if (!ok) break;
                    const u64 s_end = std::min<u64>((u64)(sl_next + 1) * ring_slot, n_bytes), e = std::min<u64>(s_end, ch.b1);
                    ok = hipMemcpyAsync(d_bytes + sent, ring + (size_t)(sl_next % TP_RING_SLOTS) * ring_slot + (sent - (u64)sl_next * ring_slot),
                                        (size_t)(e - sent), hipMemcpyHostToDevice, copy_stream) == hipSuccess;
                    if (sent == 0) t_first_dma.store(since());
                    sent = e;
                    if (ok && sent == s_end) {
                        ok = hipEventRecord(ring_events[sl_next % TP_RING_SLOTS], copy_stream) == hipSuccess;
                        if (ok && sl_next >= 1) {
                            ok = hipEventSynchronize(ring_events[(sl_next - 1) % TP_RING_SLOTS]) == hipSuccess;
                            slots_free.store(sl_next - 1 + 1 + TP_RING_SLOTS, std::memory_order_release);
                        }
                        sl_next++;
                    }
                }
            } else if (texts) {
                for (u32 i = 0; i < ch.n_docs && ok; i++) {
                    const u32 d = ch.doc_first + i;
                    const u32 lo = std::max(ch.b0, (u32)text_offsets[d]), hi = std::min(ch.b1, (u32)text_offsets[d + 1] - 1u);    // (without the separator)
                    if (hi > lo)
                        ok = hipMemcpyAsync(d_bytes + lo, texts[d] + (lo - (u32)text_offsets[d]), hi - lo, hipMemcpyHostToDevice,
                                            copy_stream) == hipSuccess;
                }
            } else {
                ok = hipMemcpyAsync(d_bytes + ch.b0, bytes + ch.b0, ch.b1 - ch.b0, hipMemcpyHostToDevice, copy_stream) == hipSuccess;
            }
            if (ok) {
                // the chunk's code point count (per tile of the scan; the host adds them up), behind its bytes
                const u32 nb = ch.b1 - ch.b0, nb_cp = ceil_div_u32((u64)nb + 1, SCAN_TILE);
                hipLaunchKernelGGL((scan_reduce_kernel<TpStartIn>), dim3(nb_cp), dim3(BLOCK), 0, copy_stream,
                                   TpStartIn{d_bytes + ch.b0, nb}, nb + 1, cp_sums_aux + cnt_off[c]);
                ok = hipGetLastError() == hipSuccess &&
                     hipMemcpyAsync(h_counts[c].data(), cp_sums_aux + cnt_off[c], (size_t)nb_cp * 4, hipMemcpyDeviceToHost,
                                    copy_stream) == hipSuccess;
            }
            if (ok) ok = hipEventRecord(events[c], copy_stream) == hipSuccess;
            t_up[c] = since();
            if (ok) uploaded.store((int)c + 1, std::memory_order_release);
        }
        if (!ok) { (void)hipGetLastError(); upload_failed.store(1, std::memory_order_release); }
    });
    // (unwinding -- a HIP error or a thrown status on the compute side: the uploader stops queueing, and nothing it has
    // queued may still be writing the arena or the host-side counts when they are released)
    struct Joiner {
        std::thread &t;
        std::vector<std::thread> &fill;
        std::atomic<int> &abort;
        hipStream_t copy;
        ~Joiner()
        {
            if (t.joinable()) {                          // (the regular path has joined already)
                abort.store(1, std::memory_order_release);
                t.join();
                (void)hipStreamSynchronize(copy);
            }
            for (auto &f : fill)
                if (f.joinable()) f.join();
        }
    } joiner{uploader, fillers, upload_abort, copy_stream};

    for (u32 c = 0; c < C; c++) {
        const TpChunk &ch = chunks[c];
        // the chunk's bytes: recorded by the uploader, waited for by the compute stream
        while (uploaded.load(std::memory_order_acquire) <= (int)c) {
            if (upload_failed.load(std::memory_order_acquire)) east_throw(EAST_HIP_ERR_HIP, "upload of the raw text failed");
            std::this_thread::yield();
        }
        HIP_CHECK(hipStreamWaitEvent(h->stream, events[c], 0));
        HIP_CHECK(hipEventSynchronize(events[c]));         // (the host reads the chunk's counts)
        t_cnt[c] = since();
        // the chunk's code point count: the uploader queued it on the copy stream right behind the bytes (and recorded the event
        // behind it), so that the host has the answer -- and queues the chunk's kernels -- while the chunk before is still prepared
        u32 n_cp = 0;
        for (u32 x : h_counts[c]) n_cp += x;
        tp_prepare_chunk(ctx, scratch, ch, c, n_cp, d_bytes, tb, st);
        t_queued[c] = since();
    }
    uploader.join();
    for (auto &f : fillers) f.join();
    // the total, the per-document offsets and string counts, "kept text at or above U+0A00"
    h_off.resize((size_t)D + 1);
    h_m.resize(D);
    u32 high = 0;
    TpCarry last;
    HIP_CHECK(hipEventRecord(h->ev1, h->stream));
    HIP_CHECK(hipMemcpyAsync(h_off.data(), st.doc_sym_off_all, (size_t)D * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(h_m.data(), st.m_all, (size_t)D * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(&last, st.carry + (C & 1u), sizeof(last), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(&high, st.d_high, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (g_trace) {
        fprintf(stderr, "[east_hip] streamed preparation, %u chunks (ms since its start: staged / counted / queued):", C);
        for (u32 c = 0; c < C; c++) fprintf(stderr, " [%u MiB %.2f %.2f %.2f]", (chunks[c].b1 - chunks[c].b0) >> 20, t_up[c], t_cnt[c], t_queued[c]);
        fprintf(stderr, " done %.2f", since());
        if (use_ring) fprintf(stderr, "; %.2f ms of the call in front of it, first ring slot filled at %.2f, its DMA queued at %.2f", t_before,
                              t_first_fill.load(), t_first_dma.load());
        fprintf(stderr, "\n");
    }
    h_off[D] = last.sym_base;
    return high == 0;
}

// ---- the inputs that are prepared in one piece: the upload and the tokenizer ------------------------------------------
// The whole stream to d_bytes (n_bytes + 32: the byte-class pass loads whole 16-byte groups) and the offsets to d_text_off,
// on h->stream; a null destination is left out.
static void upload_texts_whole(east_hip_index *h, const HostTexts &in, uint8_t *d_bytes, u32 *d_text_off)
{
    const u32 D = (u32)in.D, n_bytes = (u32)in.n_bytes;
    if (d_bytes && in.texts) {                            // (the texts one by one, unjoined)
        HIP_CHECK(hipMemsetAsync(d_bytes, 0xFF, n_bytes, h->stream));              // the separators
        for (u32 d = 0; d < D; d++) {
            const size_t len = (size_t)(in.off32[d + 1] - in.off32[d] - 1);
            if (len) HIP_CHECK(hipMemcpyAsync(d_bytes + in.off32[d], in.texts[d], len, hipMemcpyHostToDevice, h->stream));
        }
    } else if (d_bytes) {
        HIP_CHECK(hipMemcpyAsync(d_bytes, in.bytes, n_bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (d_bytes) HIP_CHECK(hipMemsetAsync(d_bytes + n_bytes, 0, 32, h->stream));
    if (d_text_off) HIP_CHECK(hipMemcpyAsync(d_text_off, in.off32.data(), in.off32.size() * 4, hipMemcpyHostToDevice, h->stream));
}

// bytes -> code points -> tokens of a stream that lies on the device in one piece, out of ctx.arena
struct TpTokens {
    u32 n_cp = 0, n_tok = 0;
    bool bytewise = false;          // every byte a code point of its own: no cpu, the classes come from the byte table
    u32 *cpu = nullptr, *doc_cp_off; // the code points, upper-cased; per document its first one
    uint8_t *cw;                    // the code points' classes
    u32 *byte_prefix, *tok_prefix;  // textprep.h, "ranks without a per-element index"
    u32 *tstart, *tend, *tok_nd;    // n_tok + 1 each: a token's code points [tstart, tend), whether one of them is no digit
};
// bytewise_ok: the caller reads no code points of text in which every byte is one (it maps the kept bytes when it emits
// them); otherwise cpu is always decoded, with one entry to spare.  Two read-backs: n_cp and n_tok.
static TpTokens tp_tokenize(Ctx &ctx, u32 D, u32 n_bytes, const uint8_t *d_bytes, const u32 *d_text_off, const TpDevTables &tb,
                            bool bytewise_ok)
{
    Arena &ar = *ctx.arena;
    TpTokens t;
    // (unit starts in front of every block of 256 bytes, the last entry: their total.  First only this count: text in which
    // every byte is a code point of its own -- ASCII, Latin-1 junk -- needs no index at all, and it has to come back anyway)
    const u32 n_bblk = ceil_div_u32(n_bytes, TP_RANK_BLOCK);
    t.byte_prefix = ar.alloc<u32>((size_t)n_bblk + 1);
    LAUNCH(ctx, (tp_block_counts_kernel<TpStartIn>), ceil_div_u32((u64)n_bblk + 1, 8), TpStartIn{d_bytes, n_bytes}, n_bytes, n_bblk, t.byte_prefix);
    device_scan<ArrIn, false>(ctx, ArrIn{t.byte_prefix}, n_bblk + 1, t.byte_prefix);
    HIP_CHECK(hipMemcpyAsync(&t.n_cp, t.byte_prefix + n_bblk, 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_CHECK(hipStreamSynchronize(ctx.stream));          // also covers the caller's uploads
    const u32 n_cp = t.n_cp;
    t.bytewise = bytewise_ok && n_cp == n_bytes;
    if (!t.bytewise) t.cpu = ar.alloc<u32>((size_t)n_cp + (bytewise_ok ? 0u : 1u));
    t.cw = ar.alloc<uint8_t>((size_t)n_cp + 32);
    t.doc_cp_off = ar.alloc<u32>((size_t)D + 1);
    const u32 *ranks = t.bytewise ? nullptr : t.byte_prefix;
    if (t.bytewise) LAUNCH(ctx, tp_classify_bytes_kernel, ceil_div_u32(n_bytes, BLOCK * 16), d_bytes, n_bytes, tb.cls256, t.cw);
    else LAUNCH(ctx, tp_decode_kernel, ceil_div_u32(n_bytes, BLOCK), d_bytes, n_bytes, ranks, tb.t, t.cpu, t.cw);
    LAUNCH(ctx, tp_doc_cp_offsets_kernel, ceil_div_u32((u64)D + 1, WAVES_PER_BLOCK), d_bytes, n_bytes, ranks, d_text_off, D, t.doc_cp_off);
    // code points -> tokens (token starts in front of every block of 256 code points; the last entry: their number)
    const u32 n_tblk = ceil_div_u32(n_cp, TP_RANK_BLOCK);
    t.tok_prefix = ar.alloc<u32>((size_t)n_tblk + 1);
    LAUNCH(ctx, (tp_block_counts_kernel<TpTokStartIn>), ceil_div_u32((u64)n_tblk + 1, 8), TpTokStartIn{t.cw, n_cp}, n_cp, n_tblk, t.tok_prefix);
    device_scan<ArrIn, false>(ctx, ArrIn{t.tok_prefix}, n_tblk + 1, t.tok_prefix);
    HIP_CHECK(hipMemcpyAsync(&t.n_tok, t.tok_prefix + n_tblk, 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    const size_t n1 = (size_t)t.n_tok + 1;
    t.tstart = ar.alloc<u32>(n1), t.tend = ar.alloc<u32>(n1), t.tok_nd = ar.alloc<u32>(n1);
    HIP_CHECK(hipMemsetAsync(t.tok_nd, 0, n1 * 4, ctx.stream));
    if (t.n_tok) LAUNCH(ctx, tp_token_bounds_kernel, ceil_div_u32(n_cp, BLOCK * TP_VEC), t.cw, t.tok_prefix, n_cp, t.tstart, t.tend, t.tok_nd);
    return t;
}

// The preparation in one piece (small inputs, and kept text at or above U+0A00): d_bytes holds the whole stream.  The symbols
// end up in h->prep_sym, the per-document offsets and string counts in h_off / h_m; returns whether the symbols are in the
// tagged encoding.
static bool prepare_texts_whole(east_hip_index *h, Ctx &ctx, u32 D, u32 n_bytes, const uint8_t *d_bytes, const u32 *d_text_off,
                                u32 *d_high, const TpDevTables &tb, std::vector<u32> &h_off, std::vector<u32> &h_m)
{
    Arena &ar = *ctx.arena;
    const TpTokens t = tp_tokenize(ctx, D, n_bytes, d_bytes, d_text_off, tb, true);
    const u32 n_cp = t.n_cp, n_tok = t.n_tok;
    const u32 *cpu = t.cpu, *doc_cp_off = t.doc_cp_off, *tok_prefix = t.tok_prefix, *tstart = t.tstart, *tend = t.tend, *tok_nd = t.tok_nd;
    const uint8_t *cw = t.cw;
    u32 high = 0;
    u32 *keep = ar.alloc<u32>((size_t)n_tok + 1), *klen = ar.alloc<u32>((size_t)n_tok + 1);
    u32 *keep_ex = ar.alloc<u32>((size_t)n_tok + 1), *klen_ex = ar.alloc<u32>((size_t)n_tok + 1);
    HIP_CHECK(hipMemsetAsync(keep + n_tok, 0, 4, h->stream));
    HIP_CHECK(hipMemsetAsync(klen + n_tok, 0, 4, h->stream));
    if (n_tok) LAUNCH(ctx, tp_token_keep_kernel, ceil_div_u32(n_tok, BLOCK), tstart, tend, tok_nd, n_tok, keep, klen);
    device_scan<ArrIn, false>(ctx, ArrIn{keep}, n_tok + 1, keep_ex);
    device_scan<ArrIn, false>(ctx, ArrIn{klen}, n_tok + 1, klen_ex);

    // tokens -> per-document strings and symbols
    u32 *first_tok = ar.alloc<u32>((size_t)D + 1), *m_d = ar.alloc<u32>(D), *n_d = ar.alloc<u32>((size_t)D + 1);
    u32 *doc_sym_off = ar.alloc<u32>((size_t)D + 1);
    HIP_CHECK(hipMemsetAsync(n_d + D, 0, 4, h->stream));
    LAUNCH(ctx, tp_doc_counts_kernel, ceil_div_u32(D + 1, WAVES_PER_BLOCK), doc_cp_off, cw, n_cp, tok_prefix, keep_ex, klen_ex, D, first_tok, m_d, n_d);
    device_scan<ArrIn, false>(ctx, ArrIn{n_d}, D + 1, doc_sym_off);
    h_off.resize((size_t)D + 1);
    h_m.resize(D);
    HIP_CHECK(hipMemcpyAsync(h_off.data(), doc_sym_off, h_off.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(h_m.data(), m_d, h_m.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    const u32 n_sym = h_off[D];
    h->prep_sym.ensure((size_t)n_sym * 4, "the prepared symbols");     // (the stream has just drained)
    u32 *prep_sym = h->prep_sym.as<u32>();
    if (n_tok) {
        u32 *tok_out = keep, *tok_term = klen;           // (keep / klen are dead once their scans exist)
        uint4 *tok_rec = ar.alloc<uint4>(n_tok);
        LAUNCH(ctx, tp_token_out_kernel, ceil_div_u32(n_tok, BLOCK), tstart, keep_ex, klen_ex, doc_cp_off, first_tok, doc_sym_off, D, n_tok, tend, tok_out,
               tok_term, tok_rec);
        LAUNCH(ctx, tp_emit_kernel, ceil_div_u32(n_cp, BLOCK), cpu, d_bytes, tb.up256, cw, tok_prefix, tok_rec, n_cp, prep_sym, d_high);
    }
    LAUNCH(ctx, tp_empty_docs_kernel, ceil_div_u32(D, BLOCK), first_tok, keep_ex, doc_sym_off, D, prep_sym);
    HIP_CHECK(hipEventRecord(h->ev1, h->stream));
    HIP_CHECK(hipMemcpyAsync(&high, d_high, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    HIP_CHECK(hipEventElapsedTime(&h->last_prep_ms, h->ev0, h->ev1));
    const bool tagged = high != 0;
    if (tagged) {
        // kept word characters at or above U+0A00: the symbols go on in the tagged encoding
        if (n_tok) LAUNCH(ctx, tp_tag_terminators_kernel, ceil_div_u32(n_tok, BLOCK), tstart, tend, keep, klen, n_tok, prep_sym);
        LAUNCH(ctx, tp_tag_empty_docs_kernel, ceil_div_u32(D, BLOCK), first_tok, keep_ex, doc_sym_off, D, prep_sym);
    }
    return tagged;
}

// what a preparation found becomes the handle's: east_hip_get_prepared hands it out, build_common builds from it
static void prep_publish(east_hip_index *h, const std::vector<u32> &offsets, const std::vector<u32> &counts, u32 n_sym, bool tagged)
{
    h->prep_tagged = tagged;
    h->prep_n = n_sym;
    h->prep_doc_off.resize(offsets.size());
    h->prep_n_strings.resize(counts.size());
    for (size_t d = 0; d < offsets.size(); d++) h->prep_doc_off[d] = offsets[d];
    for (size_t d = 0; d < counts.size(); d++) h->prep_n_strings[d] = (int32_t)counts[d];
}

// Prepares the texts of `in` on the device -- streamed, or in one piece -- and builds the index from the symbols.
static void build_from_texts(east_hip_index *h, HostTexts in, const UnicodeTablesHost &tables)
{
    g_tp_call_start = std::chrono::steady_clock::now();
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    host_texts_check(in, tables);
    // ---- size the arena, upload the tables (and, in one piece, the text) ----
    use_device(h);
    h->built = false;
    h->table_scored = false;
    const u32 n_bytes = (u32)in.n_bytes, D = (u32)in.D;
    const size_t arena_before = h->arena.cap;
    size_t arena_need = (size_t)n_bytes * 46 + (size_t)D * 96 + (8u << 20);
    if (arena_before < arena_need) {
        // (the arena has to grow anyway -- a handle's first call: sized for the build behind the preparation at once, on the
        // most symbols these bytes can turn into, instead of a second hipMalloc + hipFree of gigabytes in the same call)
        const u64 n_upper = std::min<u64>((u64)n_bytes + (u64)n_bytes / 9 + 2 * (u64)D + 64, 0x7FFFFFE0ull);
        size_t free_b = 0, total_b = 0;
        const size_t both = plan_arena_bytes((u32)n_upper, D);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && both < (size_t)(0.5 * (double)(free_b + arena_before))) arena_need = std::max(arena_need, both);
        else (void)hipGetLastError();
    }
    ensure_arena(h, arena_need);
    if (g_trace && h->arena.cap != arena_before)
        fprintf(stderr, "[east_hip] text preparation: arena of %.2f GiB allocated, %.2f ms into the call\n", h->arena.cap / 1073741824.0,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_tp_call_start).count());
    Arena &ar = h->arena;
    ar.release(0);
    ar.high = 0;
    Ctx ctx = handle_ctx(h, &ar, &h->stats);
    HIP_CHECK(hipEventRecord(h->ev0, h->stream));

    uint8_t *d_bytes = ar.alloc<uint8_t>((size_t)n_bytes + 32);    // (padding: the byte-class pass loads whole 16-byte groups)
    u32 *d_text_off = ar.alloc<u32>((size_t)D + 1);
    u32 *d_high = ar.alloc<u32>(1);
    // (large inputs: the text goes up chunk by chunk and is prepared as it arrives, see prepare_texts_streamed)
    const u32 stream_chunk = ctx.knobs.tp_stream > 0 ? (u32)std::min<i64>(ctx.knobs.tp_stream, 0x40000000)
                             : ctx.knobs.tp_stream < 0 && n_bytes >= TP_STREAM_MIN ? std::max<u32>(n_bytes / TP_STREAM_CHUNKS + 1, 1u << 20) : 0u;
    upload_texts_whole(h, in, stream_chunk ? nullptr : d_bytes, d_text_off);
    const TpDevTables tb = tp_upload_tables(h, tables);
    HIP_CHECK(hipMemsetAsync(d_high, 0, 4, h->stream));

    // ---- the preparation: streamed, or in one piece ----
    std::vector<u32> h_off, h_m;
    bool streamed = false, tagged = false;
    if (stream_chunk) {
        const size_t mark = ar.mark();
        streamed = prepare_texts_streamed(h, ctx, in, stream_chunk, d_bytes, tb, h_off, h_m);
        ar.release(mark);
        if (streamed) HIP_CHECK(hipEventElapsedTime(&h->last_prep_ms, h->ev0, h->ev1));
        else upload_texts_whole(h, in, d_bytes, nullptr);   // (kept text at or above U+0A00: the preparation in one piece, tagged encoding)
    }
    if (!streamed) tagged = prepare_texts_whole(h, ctx, D, n_bytes, d_bytes, d_text_off, d_high, tb, h_off, h_m);

    // ---- publish and build ----
    prep_publish(h, h_off, h_m, h_off[D], tagged);
    build_common(h, h->prep_sym.as<u32>(), false, h->prep_n, h->prep_doc_off.data(), h->prep_n_strings.data(), in.D, tagged);
    if (streamed) ring_pin_later(h);
}
