// cosine.h -- the cosine relevance measure on the device: a term index of the whole collection.
//
// Replaces the reference's CosineRelevanceMeasure (east/relevance.py:56-168) and the token filter it uses
// (east/utils.py:31-46).  The reference re-tokenizes the keyphrase for every (keyphrase, text) pair and takes a dense
// dot product over the whole vocabulary -- K x D x V work.  Here the collection is indexed once:
//
//   bytes --decode, classes, 1:1 upper (textprep.h)--> code points --token bounds--> tokens of >= 3 code points
//   --polynomial hash mod 2^61 - 1, a segmented sum over pieces of COS_PIECE code points--> (hash, token) pairs
//   --stable radix sort--> runs of equal hashes = candidate terms; the head of a run is its first occurrence
//   --verification per piece of code points (every member equals its head), else a new seed-->
//   --stopword look-up, term ids by first occurrence--> postings (term, document, count) ordered by (term, document)
//
// and a keyphrase is scored by walking the posting lists of its distinct terms: the work is the length of the posting
// lists the queries touch, plus writing the K x D table.
//
// Determinism: every step is integer work or a floating-point sum in an order fixed by the data (no float atomics).
// Term ids do not depend on the hash seed, so a rebuild after a collision gives the same bits.
//
// Included at the end of east_hip.hip: the host half needs the handle and the C-ABI helpers defined there.
#pragma once
#include "common.h"
#include "radix_sort.h"
#include "scan.h"
#include "textprep.h"

#define COS_MIN_LEN 3u                     // tokenize_and_filter: min_word_length (utils.py:41-46)
#define COS_PIECE 2048u                    // code points per piece of the hash and of the verification
#define COS_MERSENNE ((1ull << 61) - 1ull)
#define COS_HASH_BITS 61
#define COS_MAX_ATTEMPTS 4                 // seeds tried before a build gives up (EAST_HIP_ERR_INTERNAL)
#define COS_NONE 0xFFFFFFFFu

// ---- arithmetic modulo the Mersenne prime 2^61 - 1 ---------------------------------------------------------------
__device__ __forceinline__ u64 cos_mod_reduce(u64 r)       // r < 2^62
{
    r = (r & COS_MERSENNE) + (r >> 61);
    return r >= COS_MERSENNE ? r - COS_MERSENNE : r;
}

__device__ __forceinline__ u64 cos_mulmod(u64 a, u64 b)    // a, b < 2^61: the product has at most 122 bits
{
    const u64 lo = a * b, hi = __umul64hi(a, b);
    return cos_mod_reduce((lo & COS_MERSENNE) + ((lo >> 61) | (hi << 3)));
}

__device__ __forceinline__ u64 cos_addmod(u64 a, u64 b)
{
    const u64 r = a + b;
    return r >= COS_MERSENNE ? r - COS_MERSENNE : r;
}

__device__ __forceinline__ u64 cos_powmod(u64 b, u32 e)
{
    u64 r = 1;
    for (; e; e >>= 1) {
        if (e & 1u) r = cos_mulmod(r, b);
        b = cos_mulmod(b, b);
    }
    return r;
}

static inline u64 cos_host_mulmod(u64 a, u64 b)
{
    const unsigned __int128 p = (unsigned __int128)a * b;
    u64 r = (u64)(p & COS_MERSENNE) + (u64)(p >> 61);
    r = (r & COS_MERSENNE) + (r >> 61);
    return r >= COS_MERSENNE ? r - COS_MERSENNE : r;
}

static inline u64 cos_host_powmod(u64 b, u32 e)
{
    u64 r = 1;
    for (; e; e >>= 1) {
        if (e & 1u) r = cos_host_mulmod(r, b);
        b = cos_host_mulmod(b, b);
    }
    return r;
}

// the base of attempt `seed`: a splitmix64 draw in [2^32, 2^61 - 1), above every code point
static inline u64 cos_base_of_seed(u64 seed)
{
    u64 z = seed * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (1ull << 32) + z % (COS_MERSENNE - (1ull << 32));
}

// ---- tokens --------------------------------------------------------------------------------------------------------
// The predicates the build scans are inputs of the scan (scan.h) where they read what lies in a row; those that gather are
// arrays (pflag, tn, ns).  Token k has at least COS_MIN_LEN code points (no isdigit filter and no U+0A00 limit here)
struct CosKeepIn {
    const u32 *tstart, *tend;
    __device__ __forceinline__ u32 operator()(u32 k) const { return tend[k] - tstart[k] + 1u >= COS_MIN_LEN ? 1u : 0u; }
};

// the kept tokens, compacted: first code point, length, document, and the number of pieces
__global__ __launch_bounds__(BLOCK) void cos_compact_kernel(const u32 *__restrict__ tstart, const u32 *__restrict__ tend,
                                                            const u32 *__restrict__ keep_ex, u32 n_tok,
                                                            const u32 *__restrict__ doc_cp_off, u32 n_docs,
                                                            u32 *__restrict__ kstart, u32 *__restrict__ klen,
                                                            u32 *__restrict__ kdoc, u32 *__restrict__ npc)
{
    const u32 k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n_tok || keep_ex[k + 1u] == keep_ex[k]) return;
    const u32 j = keep_ex[k], len = tend[k] - tstart[k] + 1u;
    kstart[j] = tstart[k];
    klen[j] = len;
    kdoc[j] = tp_doc_of_cp(doc_cp_off, n_docs, tstart[k]);
    npc[j] = (len + COS_PIECE - 1u) / COS_PIECE;
}

// piece q of the collection belongs to kept token piece_tok[q] (a token of L code points has ceil(L / COS_PIECE))
__global__ __launch_bounds__(BLOCK) void cos_piece_map_kernel(const u32 *__restrict__ pc_base, u32 n_kept, u32 *__restrict__ piece_tok)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_kept) return;
    for (u32 q = pc_base[j]; q < pc_base[j + 1u]; q++) piece_tok[q] = j;
}

// Horner over one piece [a, e) of a token: h = sum of cp[i] * B^(e - 1 - i)
__global__ __launch_bounds__(BLOCK) void cos_piece_hash_kernel(const u32 *__restrict__ cp, const u32 *__restrict__ kstart,
                                                               const u32 *__restrict__ klen, const u32 *__restrict__ pc_base,
                                                               const u32 *__restrict__ piece_tok, u32 n_pieces, u64 B,
                                                               u64 *__restrict__ piece_h)
{
    const u32 q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_pieces) return;
    const u32 j = piece_tok[q];
    const u32 a = (q - pc_base[j]) * COS_PIECE, e = min(a + COS_PIECE, klen[j]);
    const u32 *s = cp + kstart[j];
    u64 h = 0;
    for (u32 i = a; i < e; i++) h = cos_addmod(cos_mulmod(h, B), s[i]);
    piece_h[q] = h;
}

// the pieces of a token combined in order, H = H * B^(length of the piece) + h: the value Horner over all its code points
// gives (cos_lookup_kernel).  keys = hash & mask, vals = token number.
__global__ __launch_bounds__(BLOCK) void cos_token_hash_kernel(const u64 *__restrict__ piece_h, const u32 *__restrict__ pc_base,
                                                               const u32 *__restrict__ klen, u32 n_kept, u64 B, u64 B_piece,
                                                               u64 mask, u64 *__restrict__ keys, u32 *__restrict__ vals)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_kept) return;
    const u32 q0 = pc_base[j], q1 = pc_base[j + 1u];
    u64 H = piece_h[q0];
    if (q1 - q0 > 1u) {
        for (u32 q = q0 + 1u; q + 1u < q1; q++) H = cos_addmod(cos_mulmod(H, B_piece), piece_h[q]);
        const u32 last = klen[j] - (q1 - q0 - 1u) * COS_PIECE;
        H = cos_addmod(cos_mulmod(H, cos_powmod(B, last)), piece_h[q1 - 1u]);
    }
    keys[j] = H & mask;
    vals[j] = j;
}

// ---- runs of equal hashes ------------------------------------------------------------------------------------------
// ri = inclusive scan of the run heads (RunHeadIn over the sorted keys): the run of sorted position i is ri[i] - 1, and i
// is a head where ri steps.  Per run: its first sorted position (and n behind the last run), its key, and where its head
// token -- the first occurrence: the sort is stable and the tokens went in ascending -- lies in the code points
__global__ __launch_bounds__(BLOCK) void cos_run_heads_kernel(const u32 *__restrict__ ri, const u64 *__restrict__ skeys,
                                                              const u32 *__restrict__ svals, const u32 *__restrict__ kstart,
                                                              const u32 *__restrict__ klen, u32 n, u32 *__restrict__ run_start,
                                                              u64 *__restrict__ run_key, u32 *__restrict__ run_hstart,
                                                              u32 *__restrict__ run_hlen)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r1 = ri[i];
    if (i + 1u == n) run_start[r1] = n;
    if (i > 0 && ri[i - 1u] == r1) return;
    const u32 r = r1 - 1u, t = svals[i];
    run_start[r] = i;
    run_key[r] = skeys[i];
    run_hstart[r] = kstart[t];
    run_hlen[r] = klen[t];
}

// per kept token: its run and the head token of its run
__global__ __launch_bounds__(BLOCK) void cos_token_runs_kernel(const u32 *__restrict__ svals, const u32 *__restrict__ ri,
                                                               const u32 *__restrict__ run_start, u32 n,
                                                               u32 *__restrict__ run_of_tok, u32 *__restrict__ head_of)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r = ri[i] - 1u;
    run_of_tok[svals[i]] = r;
    head_of[svals[i]] = svals[run_start[r]];
}

// every member of a run equals its head in length and code point by code point (a piece per thread, so that a long token
// is checked by many threads); any difference raises *bad
__global__ __launch_bounds__(BLOCK) void cos_verify_kernel(const u32 *__restrict__ cp, const u32 *__restrict__ kstart,
                                                           const u32 *__restrict__ klen, const u32 *__restrict__ pc_base,
                                                           const u32 *__restrict__ piece_tok, const u32 *__restrict__ head_of,
                                                           u32 n_pieces, u32 *__restrict__ bad)
{
    const u32 q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_pieces) return;
    const u32 j = piece_tok[q], hd = head_of[j];
    if (hd == j) return;
    if (klen[hd] != klen[j]) { *bad = 1u; return; }
    const u32 a = (q - pc_base[j]) * COS_PIECE, e = min(a + COS_PIECE, klen[j]);
    const u32 *s = cp + kstart[j], *t = cp + kstart[hd];
    for (u32 i = a; i < e; i++)
        if (s[i] != t[i]) { *bad = 1u; return; }
}

// ---- word look-up (the stopwords at build time, query words later) --------------------------------------------------
// Per word: its hash (Horner: the same value as the pieces combined), a binary search among the run keys and an exact
// comparison with the run's text.  run_term == nullptr: out = the run, its text at s_off / s_len [run]; otherwise out =
// the run's term (-1 for a stop run), its text at s_off / s_len [term].  -1 where the word is not there.
__global__ __launch_bounds__(BLOCK) void cos_lookup_kernel(const u32 *__restrict__ words, const u32 *__restrict__ w_off, u32 n_words,
                                                           u64 B, u64 mask, const u64 *__restrict__ run_key, u32 n_runs,
                                                           const u32 *__restrict__ run_term, const u32 *__restrict__ s_off,
                                                           const u32 *__restrict__ s_len, const u32 *__restrict__ s_cp,
                                                           int32_t *__restrict__ out)
{
    const u32 w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= n_words) return;
    const u32 a = w_off[w], len = w_off[w + 1u] - a;
    u64 h = 0;
    for (u32 i = 0; i < len; i++) h = cos_addmod(cos_mulmod(h, B), words[a + i]);
    h &= mask;
    u32 lo = 0, hi = n_runs;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (run_key[mid] < h) lo = mid + 1u; else hi = mid; }
    int32_t res = -1;
    if (len && lo < n_runs && run_key[lo] == h) {
        const u32 id = run_term ? run_term[lo] : lo;
        if (id != COS_NONE && s_len[id] == len) {
            const u32 *t = s_cp + s_off[id];
            bool same = true;
            for (u32 i = 0; i < len && same; i++) same = t[i] == words[a + i];
            if (same) res = (int32_t)id;
        }
    }
    out[w] = res;
}

__global__ __launch_bounds__(BLOCK) void cos_mark_stops_kernel(const int32_t *__restrict__ found, u32 n_words, u32 *__restrict__ is_stop)
{
    const u32 w = blockIdx.x * BLOCK + threadIdx.x;
    if (w < n_words && found[w] >= 0) is_stop[found[w]] = 1u;
}

// ---- term ids by first occurrence ----------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cos_term_heads_kernel(const u32 *__restrict__ run_start, const u32 *__restrict__ svals,
                                                               const u32 *__restrict__ is_stop, u32 n_runs, u32 *__restrict__ head_flag)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r < n_runs && !is_stop[r]) head_flag[svals[run_start[r]]] = 1u;
}

// th_ex = exclusive scan of head_flag over the kept tokens: the term of a run is th_ex at its head token
__global__ __launch_bounds__(BLOCK) void cos_run_terms_kernel(const u32 *__restrict__ run_start, const u32 *__restrict__ svals,
                                                              const u32 *__restrict__ is_stop, const u32 *__restrict__ th_ex,
                                                              u32 n_runs, u32 *__restrict__ run_term, u32 *__restrict__ term_run)
{
    const u32 r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_runs) return;
    if (is_stop[r]) { run_term[r] = COS_NONE; return; }
    const u32 t = th_ex[svals[run_start[r]]];
    run_term[r] = t;
    term_run[t] = r;
}

// ---- postings -------------------------------------------------------------------------------------------------------
// Inside a run the tokens are in collection order, so its segments of one document are its postings.  pflag[i] = sorted
// position i starts a posting (stop runs have none).  (Gathers: an array, since the scan evaluates its input twice)
__global__ __launch_bounds__(BLOCK) void cos_posting_flags_kernel(const u32 *__restrict__ svals, const u32 *__restrict__ ri,
                                                                  const u32 *__restrict__ run_start, const u32 *__restrict__ run_term,
                                                                  const u32 *__restrict__ kdoc, u32 n, u32 *__restrict__ pflag)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r = ri[i] - 1u;
    pflag[i] = run_term[r] != COS_NONE && (i == run_start[r] || kdoc[svals[i - 1u]] != kdoc[svals[i]]) ? 1u : 0u;
}

// postings per term, in term order; px = exclusive scan of pflag.  (Gathers: an array, since the scan evaluates its input twice)
__global__ __launch_bounds__(BLOCK) void cos_term_counts_kernel(const u32 *__restrict__ term_run, const u32 *__restrict__ run_start,
                                                                const u32 *__restrict__ px, u32 V, u32 *__restrict__ tn)
{
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= V) return;
    const u32 r = term_run[t];
    tn[t] = px[run_start[r + 1u]] - px[run_start[r]];
}

// every posting to its slot in (term, document) order: document, term, first sorted position, last sorted position + 1
__global__ __launch_bounds__(BLOCK) void cos_postings_kernel(const u32 *__restrict__ svals, const u32 *__restrict__ ri,
                                                             const u32 *__restrict__ run_start, const u32 *__restrict__ run_term,
                                                             const u32 *__restrict__ kdoc, const u32 *__restrict__ pflag,
                                                             const u32 *__restrict__ px, const u32 *__restrict__ unit_off, u32 n,
                                                             u32 *__restrict__ post_doc, u32 *__restrict__ post_unit,
                                                             u32 *__restrict__ post_beg, u32 *__restrict__ post_end)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 r = ri[i] - 1u, t = run_term[r];
    if (t == COS_NONE) return;
    const u32 d = kdoc[svals[i]];
    const u32 slot = unit_off[t] + (px[i] + pflag[i] - 1u) - px[run_start[r]];
    if (pflag[i]) {
        post_doc[slot] = d;
        post_unit[slot] = t;
        post_beg[slot] = i;
    }
    if (i + 1u == run_start[r + 1u] || kdoc[svals[i + 1u]] != d) post_end[slot] = i + 1u;
}

__global__ __launch_bounds__(BLOCK) void cos_counts_kernel(const u32 *__restrict__ post_beg, const u32 *__restrict__ post_end, u32 P,
                                                           u32 *__restrict__ post_cnt)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) post_cnt[p] = post_end[p] - post_beg[p];
}

// ---- per document: the kept tokens that are not stopwords (n_d) -----------------------------------------------------
// ns[j] = kept token j is no stopword (a gather: an array, as tn)
__global__ __launch_bounds__(BLOCK) void cos_nonstop_kernel(const u32 *__restrict__ run_of_tok, const u32 *__restrict__ run_term,
                                                            u32 n_kept, u32 *__restrict__ ns)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < n_kept) ns[j] = run_term[run_of_tok[j]] != COS_NONE ? 1u : 0u;
}

// the kept tokens of document d are those from the first of a document >= d to the first of one >= d + 1 (kdoc ascends);
// nsx = exclusive scan of ns
__global__ __launch_bounds__(BLOCK) void cos_doc_lengths_kernel(const u32 *__restrict__ kdoc, u32 n_kept, const u32 *__restrict__ nsx,
                                                                u32 n_docs, u32 *__restrict__ n_d)
{
    const u32 d = blockIdx.x * BLOCK + threadIdx.x;
    if (d >= n_docs) return;
    n_d[d] = nsx[ascending_lower_bound(kdoc, n_kept, d + 1u)] - nsx[ascending_lower_bound(kdoc, n_kept, d)];
}

// ---- the token sequence (phrases.h) ---------------------------------------------------------------------------------
// what stays of the kept tokens themselves: the term of kept token j (COS_NONE: a stopword) and its document
__global__ __launch_bounds__(BLOCK) void cos_tok_terms_kernel(const u32 *__restrict__ run_of_tok, const u32 *__restrict__ run_term,
                                                              const u32 *__restrict__ kdoc, u32 n_kept, u32 *__restrict__ tok_term,
                                                              u32 *__restrict__ tok_doc)
{
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_kept) return;
    tok_term[j] = run_term[run_of_tok[j]];
    tok_doc[j] = kdoc[j];
}

// ---- the terms' text (east_hip_cosine_get_terms, query look-ups) ----------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cos_term_len_kernel(const u32 *__restrict__ term_run, const u32 *__restrict__ run_hlen, u32 V,
                                                             u32 *__restrict__ tlen)
{
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < V) tlen[t] = run_hlen[term_run[t]];
}

// a wavefront per term
__global__ __launch_bounds__(BLOCK) void cos_term_text_kernel(const u32 *__restrict__ cp, const u32 *__restrict__ term_run,
                                                              const u32 *__restrict__ run_hstart, const u32 *__restrict__ tlen,
                                                              const u32 *__restrict__ toff, u32 V, u32 *__restrict__ tcp)
{
    const u32 t = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (t >= V) return;
    const u32 *s = cp + run_hstart[term_run[t]];
    for (u32 i = lane_id(); i < tlen[t]; i += WAVE) tcp[toff[t] + i] = s[i];
}

// ---- classes (the stems vector space): the postings re-keyed by class and merged --------------------------------------
__global__ __launch_bounds__(BLOCK) void cos_class_keys_kernel(const u32 *__restrict__ post_unit, const u32 *__restrict__ post_doc,
                                                               const u32 *__restrict__ term_class, u32 P, u64 *__restrict__ keys,
                                                               u32 *__restrict__ vals)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    keys[p] = ((u64)term_class[post_unit[p]] << 32) | post_doc[p];
    vals[p] = p;
}

// one merged posting per segment of equal (class, document), fx = exclusive scan of the segment starts (RunHeadIn over the
// sorted keys); the counts are integers, added in term order
__global__ __launch_bounds__(BLOCK) void cos_class_merge_kernel(const u64 *__restrict__ skeys, const u32 *__restrict__ svals,
                                                                const u32 *__restrict__ post_cnt, const u32 *__restrict__ fx, u32 n,
                                                                u32 *__restrict__ c_doc, u32 *__restrict__ c_unit,
                                                                u32 *__restrict__ c_cnt)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (i > 0 && skeys[i] == skeys[i - 1u])) return;
    u32 c = 0;
    for (u32 e = i; e < n && skeys[e] == skeys[i]; e++) c += post_cnt[svals[e]];
    const u32 slot = fx[i];
    c_doc[slot] = (u32)skeys[i];
    c_unit[slot] = (u32)(skeys[i] >> 32);
    c_cnt[slot] = c;
}

// ---- document order of the postings, weights and norms ---------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cos_doc_keys_kernel(const u32 *__restrict__ post_doc, u32 P, u32 *__restrict__ keys,
                                                             u32 *__restrict__ vals)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    keys[p] = post_doc[p];
    vals[p] = p;
}

__global__ __launch_bounds__(BLOCK) void cos_invert_perm_kernel(const u32 *__restrict__ perm, u32 P, u32 *__restrict__ inv)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < P) inv[perm[i]] = i;
}

// w = tf * idf, tf = count / max(n_d, 1), idf = 1 + ln(D / df) under tf-idf and no factor under tf (relevance.py:105-141);
// the squares go to the posting's place in document order
__global__ __launch_bounds__(BLOCK) void cos_weights_kernel(const u32 *__restrict__ post_doc, const u32 *__restrict__ post_unit,
                                                            const u32 *__restrict__ post_cnt, const u32 *__restrict__ unit_off,
                                                            const u32 *__restrict__ n_d, const u32 *__restrict__ inv_perm, u32 P,
                                                            u32 n_docs, int tfidf, double *__restrict__ w, double *__restrict__ sq)
{
    const u32 p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const u32 nd = n_d[post_doc[p]];
    const double tf = (double)post_cnt[p] / (double)(nd > 1u ? nd : 1u);
    double x = tf;
    if (tfidf) {
        const u32 u = post_unit[p];
        x = tf * (1.0 + log((double)n_docs / (double)(unit_off[u + 1u] - unit_off[u])));
    }
    w[p] = x;
    sq[inv_perm[p]] = x * x;
}

// A wavefront per document: its squared weights in ascending unit order, cut into 64 consecutive slices; every lane adds
// its slice in order, then the 64 partial sums are added in lane order -- an order fixed by the document alone.
// norm = the square root, or 1.0 for a document without terms (relevance.py:144-147)
__global__ __launch_bounds__(BLOCK) void cos_norms_kernel(const double *__restrict__ sq, const u32 *__restrict__ doc_off, u32 n_docs,
                                                          double *__restrict__ norm)
{
    const u32 d = blockIdx.x * WAVES_PER_BLOCK + wave_id();
    if (d >= n_docs) return;
    const u32 a = doc_off[d], n = doc_off[d + 1u] - a;
    const u32 chunk = (n + WAVE - 1u) / WAVE;
    const u32 b = min(n, lane_id() * chunk), e = min(n, b + chunk);
    double s = 0.0;
    for (u32 i = b; i < e; i++) s += sq[a + i];
    double total = 0.0;
    for (int l = 0; l < WAVE; l++) total += __shfl(s, l, WAVE);
    if (lane_id() == 0) norm[d] = n ? sqrt(total) : 1.0;
}

// ---- score ----------------------------------------------------------------------------------------------------------
// per query token: its entry of the query vector where it is the first occurrence of a vocabulary unit in its query --
// count / query length, the length counting every kept token, in the vocabulary or not -- and 0 elsewhere
__global__ __launch_bounds__(BLOCK) void cos_query_weights_kernel(const int32_t *__restrict__ q_ids, const u32 *__restrict__ q_off, u32 K,
                                                                  u32 total, u32 n_units, double *__restrict__ qw)
{
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    u32 lo = 0, hi = K;                                   // the query of token i: q_off[lo] <= i < q_off[lo + 1]
    while (hi - lo > 1u) { const u32 mid = (lo + hi) >> 1; if (q_off[mid] <= i) lo = mid; else hi = mid; }
    const int32_t id = q_ids[i];
    double v = 0.0;
    if (id >= 0 && (u32)id < n_units) {
        const u32 a = q_off[lo], e = q_off[lo + 1u];
        bool first = true;
        u32 c = 0;
        for (u32 x = a; x < e; x++) {
            if (q_ids[x] == id) { c++; if (x < i) first = false; }
        }
        if (first) v = (double)c / (double)(e - a);
    }
    qw[i] = v;
}

// A workgroup per query: the row is zeroed, the posting lists of the query's distinct units are added one after the other
// in the order of their first occurrence in the query (a document appears once in a list: no two threads of a step touch
// the same score), then every score is divided by (document norm * query norm), relevance.py:144-147.
__global__ __launch_bounds__(BLOCK) void cos_score_kernel(const int32_t *__restrict__ q_ids, const u32 *__restrict__ q_off,
                                                          const double *__restrict__ qw, u32 K, const u32 *__restrict__ unit_off,
                                                          const u32 *__restrict__ post_doc, const double *__restrict__ w,
                                                          const double *__restrict__ norm, u32 n_docs, double *__restrict__ out)
{
    __shared__ double qnorm;
    for (u32 k = blockIdx.x; k < K; k += gridDim.x) {
        double *row = out + (size_t)k * n_docs;
        for (u32 d = threadIdx.x; d < n_docs; d += BLOCK) row[d] = 0.0;
        const u32 a = q_off[k], e = q_off[k + 1u];
        if (threadIdx.x == 0) {
            double s = 0.0;
            bool any = false;
            for (u32 i = a; i < e; i++) {
                if (qw[i] != 0.0) { s += qw[i] * qw[i]; any = true; }
            }
            qnorm = any ? sqrt(s) : 1.0;
        }
        __syncthreads();
        for (u32 i = a; i < e; i++) {
            const double q = qw[i];
            if (q == 0.0) continue;                       // (the same for every thread of the workgroup)
            const u32 u = (u32)q_ids[i];
            for (u32 p = unit_off[u] + threadIdx.x; p < unit_off[u + 1u]; p += BLOCK) row[post_doc[p]] += w[p] * q;
            __syncthreads();
        }
        const double qn = qnorm;
        for (u32 d = threadIdx.x; d < n_docs; d += BLOCK) row[d] = row[d] / (norm[d] * qn);
        __syncthreads();
    }
}

// ============================================================================================================ host ==
// The cosine state's device buffers are the handle's own (DevBuf): a cosine build never touches the EASA index's arena.
// a vector space the scores are taken in: the terms, or classes of terms (the stems)
struct CosUnits {
    u32 n_units = 0, P = 0;
    u32 *unit_off = nullptr, *post_doc = nullptr, *post_unit = nullptr, *post_cnt = nullptr;
    u32 *inv_perm = nullptr, *doc_off = nullptr;        // a posting's place in document order; per document its range there
    DevBuf weights;                                       // per weighting (0 tf, 1 tf-idf): P weights and D norms, made on first use
    bool w_valid[2] = {false, false};
    DevBuf bm_weights;                                    // the BM25 weights (bm25.h): P doubles, made for (bm_k1, bm_b)
    double bm_k1 = 0.0, bm_b = 0.0;
    bool bm_valid = false;
};

struct CosState : Consumer {
    static constexpr int SLOT = east_hip_index::SLOT_COS;
    bool use_classes = false;                             // (valid: the index is built)
    u32 n_docs = 0, n_kept = 0, n_runs = 0, V = 0, attempts = 0;
    u64 B = 0, mask = 0;                                  // hash base and mask of the attempt that passed the verification
    DevBuf text;             // scratch: bytes, code points, tokens (after the build: the scratch of the weights)
    DevBuf work;             // scratch: the term sort and what goes with it (after the build: classes, look-ups)
    DevBuf index;            // what stays: runs, the terms' places, per-document lengths, the terms' postings
    DevBuf term_text;        // the terms' code points
    DevBuf classes;          // the classes' postings
    DevBuf score;            // the last score call's queries and table
    u64 *run_key = nullptr;
    u32 *run_term = nullptr, *term_off = nullptr, *term_len = nullptr, *tcp = nullptr, *n_d = nullptr;
    u32 *tok_term = nullptr, *tok_doc = nullptr;          // per kept token, in text order: its term (COS_NONE: a stopword), its document
    CosUnits terms, cls;
    float build_ms = -1.f, score_ms = -1.f;               // the timer's ms of the last build and of the last score call
    double *table = nullptr;                              // the last score call's K x D table, where it lies in `score` (offers(): the graph, the ranking and the similarity read it there)
    u32 table_K = 0;
    bool table_valid = false;
    u32 bm_N = 0, bm_made = 0;                            // bm25.h: the sum of n_d; how often BM25 weights were computed on this index
    double bm_avgdl = 0.0;                                // ... (double)bm_N / (double)n_docs
    bool bm_total_valid = false;
    CosState()
    {
        bufs = {&text, &work, &index, &term_text, &classes, &score, &terms.weights, &cls.weights, &terms.bm_weights, &cls.bm_weights};
        keep_bytes = (size_t)64 << 20;                      // (a recycled handle keeps small buffers only, as east_hip_reset does)
    }
    void clear() override
    {
        use_classes = table_valid = false;
        terms.w_valid[0] = terms.w_valid[1] = cls.w_valid[0] = cls.w_valid[1] = false;
        terms.bm_valid = cls.bm_valid = bm_total_valid = false;
        bm_made = 0;
        build_ms = score_ms = -1.f;
    }
    TableRef offers() const override
    {
        TableRef t;
        if (valid && table_valid) { t.p = table; t.K = table_K; t.D = n_docs; }
        return t;
    }
};

// the text-to-text cosine matrix (cosine_texts.h) is a function of the index and of its vector space: every build and every
// change of the classes withdraws it
static void cos_withdraw_texts_matrix(east_hip_index *h)
{
    if (Consumer *t = h->consumers[east_hip_index::SLOT_COSTEXT]) t->withdraw();
}

// the extracted phrases (phrases.h) are a function of the index's token sequence: every build withdraws them
static void cos_withdraw_phrases(east_hip_index *h)
{
    if (Consumer *p = h->consumers[east_hip_index::SLOT_PHR]) p->withdraw();
}

// the characteristic terms (terms.h) are a function of the index and of its vector space, as the texts' matrix is
static void cos_withdraw_terms(east_hip_index *h)
{
    if (Consumer *t = h->consumers[east_hip_index::SLOT_TERMS]) t->withdraw();
}

// the shingle overlap (overlap.h) is a function of the token sequence alone: a new index withdraws it, a new vector space does not
static void cos_withdraw_overlap(east_hip_index *h)
{
    if (Consumer *o = h->consumers[east_hip_index::SLOT_OVL]) o->withdraw();
}

// the shared passages (passages.h) are a function of the token sequence alone, as the overlap is
static void cos_withdraw_passages(east_hip_index *h)
{
    if (Consumer *p = h->consumers[east_hip_index::SLOT_PAS]) p->withdraw();
}

static CosState &cos_built(east_hip_index *h) { return consumer_built<CosState>(h, "no cosine index has been built on this handle"); }

// A ragged host array: n + 1 offsets into a payload of offsets[n] words, narrowed to 32 bits for the device.  bad: the
// message where they do not start at 0, the payload has 2^31 - 16 words or more, or it is null and not empty; decreasing:
// where an offset is below the one in front.
static std::vector<u32> ragged_offsets_u32(const i64 *offsets, int32_t n, const void *payload, const char *bad, const char *decreasing)
{
    std::vector<u32> off32((size_t)n + 1, 0);
    if (!n) return off32;
    if (offsets[0] != 0 || offsets[n] >= (i64)0x7FFFFFF0 || (offsets[n] > 0 && !payload)) east_throw(EAST_HIP_ERR_INVALID, bad);
    for (int32_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) east_throw(EAST_HIP_ERR_INVALID, decreasing);
        off32[i + 1] = (u32)offsets[i + 1];
    }
    return off32;
}

// The postings in document order: a stable sort by document keeps the ascending unit order inside every document
// (the order its squared weights are added in).
static void cos_doc_order(Ctx &ctx, CosUnits &U, u32 D)
{
    const u32 P = U.P;
    if (!P) {
        HIP_CHECK(hipMemsetAsync(U.doc_off, 0, ((size_t)D + 1) * 4, ctx.stream));
        return;
    }
    const size_t mark = ctx.arena->mark();
    SortBufs<u32> sb = sort_bufs_alloc<u32>(*ctx.arena, P);
    LAUNCH(ctx, cos_doc_keys_kernel, ceil_div_u32(P, BLOCK), (const u32 *)U.post_doc, P, sb.keys[0], sb.vals[0]);
    const int r = radix_sort_pairs<u32>(ctx, sb, P, std::max(1, bit_width_u32(D - 1)));
    LAUNCH(ctx, cos_invert_perm_kernel, ceil_div_u32(P, BLOCK), (const u32 *)sb.vals[r], P, U.inv_perm);
    // (the postings of document d in document order are [doc_off[d], doc_off[d + 1]))
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)D + 1, BLOCK), (const u32 *)sb.keys[r], P, D, U.doc_off);
    ctx.arena->release(mark);
}

static void cos_build(east_hip_index *h, HostTexts in, const UnicodeTablesHost &tables, const u32 *stop_cps, const i64 *stop_offsets, int32_t n_stop)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    host_texts_check(in, tables);
    if (n_stop < 0 || (n_stop > 0 && !stop_offsets)) east_throw(EAST_HIP_ERR_INVALID, "bad stopword arguments");
    const std::vector<u32> stop_off32 = ragged_offsets_u32(stop_offsets, n_stop, stop_cps, "bad stopword offsets", "stopword offsets must not decrease");
    const u32 n_stop_cps = stop_off32[n_stop];
    use_device(h);
    CosState &c = consumer_begin<CosState>(h);
    c.clear();
    cos_withdraw_texts_matrix(h);
    cos_withdraw_phrases(h);
    cos_withdraw_terms(h);
    cos_withdraw_overlap(h);
    cos_withdraw_passages(h);
    const u32 N = (u32)in.n_bytes, D = (u32)in.D;
    Stats stats;

    // ---- bytes -> code points -> tokens (at most one token per two code points, plus one)
    const size_t n_tok_max = (size_t)N / 2 + 2;
    // (a token: its two bounds, tok_nd and keep_ex)
    c.text.ensure((size_t)N * 6 + n_tok_max * 16 + (size_t)N / 32 + (size_t)D * 16 + ((size_t)1 << 20), "the cosine index");
    Arena a1 = c.text.arena();
    Ctx ctx = handle_ctx(h, &a1, &stats);
    ConsumerTimer timer(h, c);
    uint8_t *d_bytes = a1.alloc<uint8_t>((size_t)N + 32);
    u32 *d_text_off = a1.alloc<u32>((size_t)D + 1);
    upload_texts_whole(h, in, d_bytes, d_text_off);
    const TpDevTables tb = tp_upload_tables(h, tables);
    // (the cosine kernels read the code points: always decoded)
    const TpTokens tk = tp_tokenize(ctx, D, N, d_bytes, d_text_off, tb, false);
    const u32 n_cp = tk.n_cp, n_tok = tk.n_tok;
    const u32 *cpu = tk.cpu, *doc_cp_off = tk.doc_cp_off, *tstart = tk.tstart, *tend = tk.tend;
    u32 *keep_ex = a1.alloc<u32>((size_t)n_tok + 1);
    const u32 n_kept = device_scan_count(ctx, CosKeepIn{tstart, tend}, n_tok, keep_ex);

    // ---- what stays (runs, terms and postings are at most as many as the kept tokens)
    const size_t K1 = (size_t)n_kept + 2;
    // (... and the token sequence: 8 bytes a kept token)
    c.index.ensure(K1 * 56 + (size_t)D * 12 + ((size_t)1 << 16), "the cosine index");
    Arena ai = c.index.arena();
    c.run_key = ai.alloc<u64>(K1);
    c.run_term = ai.alloc<u32>(K1);
    c.term_off = ai.alloc<u32>(K1);
    c.term_len = ai.alloc<u32>(K1);
    c.n_d = ai.alloc<u32>((size_t)D + 1);
    CosUnits &T = c.terms;
    T.unit_off = ai.alloc<u32>(K1);
    T.post_doc = ai.alloc<u32>(K1);
    T.post_unit = ai.alloc<u32>(K1);
    T.post_cnt = ai.alloc<u32>(K1);
    T.inv_perm = ai.alloc<u32>(K1);
    T.doc_off = ai.alloc<u32>((size_t)D + 1);
    c.tok_term = ai.alloc<u32>(K1);
    c.tok_doc = ai.alloc<u32>(K1);

    // ---- the kept tokens and their pieces
    const size_t n_pc_max = (size_t)n_kept + n_cp / COS_PIECE + 2;
    // (a kept token: 128 bytes -- the twenty-two arrays of a word each below, the term sort's two pairs of 12 bytes and
    // cos_doc_order's two of 8 -- and 28 to spare for the sorts' scratch)
    c.work.ensure(K1 * 156 + n_pc_max * 12 + ((size_t)n_stop_cps + 3 * (size_t)n_stop) * 4 + ((size_t)4 << 20), "the cosine index");
    Arena a2 = c.work.arena();
    ctx.arena = &a2;
    u32 *kstart = a2.alloc<u32>(K1), *klen = a2.alloc<u32>(K1), *kdoc = a2.alloc<u32>(K1), *npc = a2.alloc<u32>(K1),
        *pc_base = a2.alloc<u32>(K1);
    if (n_tok)
        LAUNCH(ctx, cos_compact_kernel, ceil_div_u32(n_tok, BLOCK), (const u32 *)tstart, (const u32 *)tend, (const u32 *)keep_ex, n_tok,
               (const u32 *)doc_cp_off, D, kstart, klen, kdoc, npc);
    const u32 n_pieces = device_scan_count(ctx, ArrIn{npc}, n_kept, pc_base);
    u32 *piece_tok = a2.alloc<u32>((size_t)n_pieces + 1);
    u64 *piece_h = a2.alloc<u64>((size_t)n_pieces + 1);
    if (n_kept) LAUNCH(ctx, cos_piece_map_kernel, ceil_div_u32(n_kept, BLOCK), (const u32 *)pc_base, n_kept, piece_tok);
    SortBufs<u64> sb = sort_bufs_alloc<u64>(a2, K1);
    u32 *ri = a2.alloc<u32>(K1), *run_start = a2.alloc<u32>(K1), *run_hstart = a2.alloc<u32>(K1), *run_hlen = a2.alloc<u32>(K1),
        *run_of_tok = a2.alloc<u32>(K1), *head_of = a2.alloc<u32>(K1), *bad = a2.alloc<u32>(1);

    // ---- term hashes: sort, runs, verification; the next seed while two different words share a hash
    int r = 0;
    u32 n_runs = 0;
    c.attempts = 0;
    c.B = cos_base_of_seed(0);
    c.mask = COS_MERSENNE;
    while (n_kept) {
        const int attempt = (int)++c.attempts;
        if (attempt > COS_MAX_ATTEMPTS) east_throw(EAST_HIP_ERR_INTERNAL, "cosine index: the term hashes of every seed tried collide");
        const int bits = attempt == 1 && ctx.knobs.term_hash_bits > 0 ? ctx.knobs.term_hash_bits : COS_HASH_BITS;
        const u64 B = cos_base_of_seed((u64)attempt - 1u), mask = bits >= COS_HASH_BITS ? COS_MERSENNE : ((u64)1 << bits) - 1u;
        LAUNCH(ctx, cos_piece_hash_kernel, ceil_div_u32(n_pieces, BLOCK), (const u32 *)cpu, (const u32 *)kstart, (const u32 *)klen,
               (const u32 *)pc_base, (const u32 *)piece_tok, n_pieces, B, piece_h);
        LAUNCH(ctx, cos_token_hash_kernel, ceil_div_u32(n_kept, BLOCK), (const u64 *)piece_h, (const u32 *)pc_base, (const u32 *)klen,
               n_kept, B, cos_host_powmod(B, COS_PIECE), mask, sb.keys[0], sb.vals[0]);
        r = radix_sort_pairs<u64>(ctx, sb, n_kept, bits);
        device_scan<RunHeadIn<u64>, true>(ctx, RunHeadIn<u64>{sb.keys[r], 0}, n_kept, ri);
        LAUNCH(ctx, cos_run_heads_kernel, ceil_div_u32(n_kept, BLOCK), (const u32 *)ri, (const u64 *)sb.keys[r],
               (const u32 *)sb.vals[r], (const u32 *)kstart, (const u32 *)klen, n_kept, run_start, c.run_key, run_hstart, run_hlen);
        LAUNCH(ctx, cos_token_runs_kernel, ceil_div_u32(n_kept, BLOCK), (const u32 *)sb.vals[r], (const u32 *)ri,
               (const u32 *)run_start, n_kept, run_of_tok, head_of);
        HIP_CHECK(hipMemsetAsync(bad, 0, 4, h->stream));
        LAUNCH(ctx, cos_verify_kernel, ceil_div_u32(n_pieces, BLOCK), (const u32 *)cpu, (const u32 *)kstart, (const u32 *)klen,
               (const u32 *)pc_base, (const u32 *)piece_tok, (const u32 *)head_of, n_pieces, bad);
        u32 rb[2] = {0, 0};
        device_read_words(ctx, {{&rb[0], bad}, {&rb[1], ri + n_kept - 1}});
        if (!rb[0]) {
            n_runs = rb[1];
            c.B = B;
            c.mask = mask;
            break;
        }
    }
    const u32 *svals = sb.vals[r];

    // ---- stopwords: their runs lose their postings
    u32 *is_stop = a2.alloc<u32>(K1);
    HIP_CHECK(hipMemsetAsync(is_stop, 0, K1 * 4, h->stream));
    if (n_stop && n_runs) {
        u32 *d_sw = a2.alloc<u32>((size_t)n_stop_cps + 1), *d_sw_off = a2.alloc<u32>((size_t)n_stop + 1);
        int32_t *found = a2.alloc<int32_t>((size_t)n_stop);
        if (n_stop_cps) HIP_CHECK(hipMemcpyAsync(d_sw, stop_cps, (size_t)n_stop_cps * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(d_sw_off, stop_off32.data(), stop_off32.size() * 4, hipMemcpyHostToDevice, h->stream));
        LAUNCH(ctx, cos_lookup_kernel, ceil_div_u32((u32)n_stop, BLOCK), (const u32 *)d_sw, (const u32 *)d_sw_off, (u32)n_stop, c.B,
               c.mask, (const u64 *)c.run_key, n_runs, (const u32 *)nullptr, (const u32 *)run_hstart, (const u32 *)run_hlen,
               (const u32 *)cpu, found);
        LAUNCH(ctx, cos_mark_stops_kernel, ceil_div_u32((u32)n_stop, BLOCK), (const int32_t *)found, (u32)n_stop, is_stop);
    }

    // ---- term ids by first occurrence
    u32 *head_flag = a2.alloc<u32>(K1), *th_ex = a2.alloc<u32>(K1), *term_run = a2.alloc<u32>(K1);
    HIP_CHECK(hipMemsetAsync(head_flag, 0, K1 * 4, h->stream));
    if (n_runs)
        LAUNCH(ctx, cos_term_heads_kernel, ceil_div_u32(n_runs, BLOCK), (const u32 *)run_start, svals, (const u32 *)is_stop, n_runs,
               head_flag);
    // (head_flag is an array: the runs scatter to it)
    const u32 V = device_scan_count(ctx, ArrIn{head_flag}, n_kept, th_ex);
    if (n_runs)
        LAUNCH(ctx, cos_run_terms_kernel, ceil_div_u32(n_runs, BLOCK), (const u32 *)run_start, svals, (const u32 *)is_stop,
               (const u32 *)th_ex, n_runs, c.run_term, term_run);
    if (n_kept)
        LAUNCH(ctx, cos_tok_terms_kernel, ceil_div_u32(n_kept, BLOCK), (const u32 *)run_of_tok, (const u32 *)c.run_term,
               (const u32 *)kdoc, n_kept, c.tok_term, c.tok_doc);

    // ---- postings (term, document, count) in (term, document) order
    u32 *pflag = a2.alloc<u32>(K1), *px = a2.alloc<u32>(K1), *post_beg = a2.alloc<u32>(K1), *post_end = a2.alloc<u32>(K1);
    if (n_kept)
        LAUNCH(ctx, cos_posting_flags_kernel, ceil_div_u32(n_kept, BLOCK), svals, (const u32 *)ri, (const u32 *)run_start,
               (const u32 *)c.run_term, (const u32 *)kdoc, n_kept, pflag);
    device_scan_with_total(ctx, ArrIn{pflag}, n_kept, px);
    u32 *tn = a2.alloc<u32>(K1);
    if (V) LAUNCH(ctx, cos_term_counts_kernel, ceil_div_u32(V, BLOCK), (const u32 *)term_run, (const u32 *)run_start, (const u32 *)px, V, tn);
    const u32 P = device_scan_count(ctx, ArrIn{tn}, V, T.unit_off);
    if (n_kept)
        LAUNCH(ctx, cos_postings_kernel, ceil_div_u32(n_kept, BLOCK), svals, (const u32 *)ri, (const u32 *)run_start,
               (const u32 *)c.run_term, (const u32 *)kdoc, (const u32 *)pflag, (const u32 *)px, (const u32 *)T.unit_off, n_kept,
               T.post_doc, T.post_unit, post_beg, post_end);
    if (P) LAUNCH(ctx, cos_counts_kernel, ceil_div_u32(P, BLOCK), (const u32 *)post_beg, (const u32 *)post_end, P, T.post_cnt);

    // ---- n_d: the kept tokens of every document that are not stopwords
    u32 *nsx = a2.alloc<u32>(K1);
    u32 *ns = a2.alloc<u32>(K1);
    if (n_kept) LAUNCH(ctx, cos_nonstop_kernel, ceil_div_u32(n_kept, BLOCK), (const u32 *)run_of_tok, (const u32 *)c.run_term, n_kept, ns);
    device_scan_with_total(ctx, ArrIn{ns}, n_kept, nsx);
    LAUNCH(ctx, cos_doc_lengths_kernel, ceil_div_u32(D, BLOCK), (const u32 *)kdoc, n_kept, (const u32 *)nsx, D, c.n_d);

    // ---- the terms' text (term_len is part of the index: an array)
    if (V) LAUNCH(ctx, cos_term_len_kernel, ceil_div_u32(V, BLOCK), (const u32 *)term_run, (const u32 *)run_hlen, V, c.term_len);
    const u32 n_tcp = device_scan_count(ctx, ArrIn{c.term_len}, V, c.term_off);
    c.term_text.ensure(((size_t)n_tcp + 1) * 4, "the cosine index");
    c.tcp = (u32 *)c.term_text.p;
    if (V)
        LAUNCH(ctx, cos_term_text_kernel, ceil_div_u32(V, WAVES_PER_BLOCK), (const u32 *)cpu, (const u32 *)term_run,
               (const u32 *)run_hstart, (const u32 *)c.term_len, (const u32 *)c.term_off, V, c.tcp);

    T.n_units = V;
    T.P = P;
    cos_doc_order(ctx, T, D);
    timer.finish();
    c.build_ms = c.ms;
    c.n_docs = D;
    c.n_kept = n_kept;
    c.n_runs = n_runs;
    c.V = V;
    c.valid = true;
}

// the stems: the postings re-keyed by class (term_class[t], classes numbered by their smallest term id) and merged
static void cos_set_classes(east_hip_index *h, const int32_t *term_class, int32_t n_classes)
{
    CosState &c = cos_built(h);
    cos_withdraw_texts_matrix(h);
    cos_withdraw_terms(h);
    c.terms.bm_valid = c.cls.bm_valid = false;              // (bm25.h: its cached weights are those of one vector space)
    if (n_classes == 0) {                                   // back to the terms
        c.use_classes = false;
        return;
    }
    if (n_classes < 0 || (u32)n_classes > c.V || !term_class) east_throw(EAST_HIP_ERR_INVALID, "bad class map");
    for (u32 t = 0; t < c.V; t++)
        if (term_class[t] < 0 || term_class[t] >= n_classes) east_throw(EAST_HIP_ERR_INVALID, "a term's class is out of range");
    const u32 P = c.terms.P, D = c.n_docs, C = (u32)n_classes;
    CosUnits &U = c.cls;
    c.use_classes = false;
    U.w_valid[0] = U.w_valid[1] = false;
    const size_t K1 = (size_t)std::max(P, C) + 2;
    c.classes.ensure(K1 * 24 + (size_t)D * 4 + ((size_t)1 << 16), "the cosine index");
    Arena ac = c.classes.arena();
    U.unit_off = ac.alloc<u32>(K1);
    U.post_doc = ac.alloc<u32>(K1);
    U.post_unit = ac.alloc<u32>(K1);
    U.post_cnt = ac.alloc<u32>(K1);
    U.inv_perm = ac.alloc<u32>(K1);
    U.doc_off = ac.alloc<u32>((size_t)D + 1);
    Stats stats;
    // (a posting: the sort's two pairs of 12 bytes, fx, cos_doc_order's two pairs of 8, and 16 to spare)
    c.work.ensure(align256(((size_t)c.V + 1) * 4) + ((size_t)P + 2) * 60 + ((size_t)4 << 20), "the cosine index");
    Arena a = c.work.arena();
    Ctx ctx = handle_ctx(h, &a, &stats);
    u32 *d_tc = a.alloc<u32>((size_t)c.V + 1);
    SortBufs<u64> sb = sort_bufs_alloc<u64>(a, (size_t)P + 1);
    u32 *fx = a.alloc<u32>((size_t)P + 1);
    u32 Pc = 0;
    if (P) {
        HIP_CHECK(hipMemcpyAsync(d_tc, term_class, (size_t)c.V * 4, hipMemcpyHostToDevice, h->stream));
        LAUNCH(ctx, cos_class_keys_kernel, ceil_div_u32(P, BLOCK), (const u32 *)c.terms.post_unit, (const u32 *)c.terms.post_doc,
               (const u32 *)d_tc, P, sb.keys[0], sb.vals[0]);
        const int r = radix_sort_pairs<u64>(ctx, sb, P, 32 + std::max(1, bit_width_u32(C - 1)));
        Pc = device_scan_count(ctx, RunHeadIn<u64>{sb.keys[r], 0}, P, fx);
        LAUNCH(ctx, cos_class_merge_kernel, ceil_div_u32(P, BLOCK), (const u64 *)sb.keys[r], (const u32 *)sb.vals[r],
               (const u32 *)c.terms.post_cnt, (const u32 *)fx, P, U.post_doc, U.post_unit, U.post_cnt);
    }
    // (the postings of class u are [unit_off[u], unit_off[u + 1]): post_unit ascends)
    LAUNCH(ctx, ascending_offsets_kernel, ceil_div_u32((u64)C + 1, BLOCK), (const u32 *)U.post_unit, Pc, C, U.unit_off);
    U.n_units = C;
    U.P = Pc;
    cos_doc_order(ctx, U, D);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    c.use_classes = true;
}

// words (code points, prepared) -> term ids, -1 for a word that is not a term
static void cos_lookup(east_hip_index *h, const u32 *cps, const i64 *offsets, int32_t n_words, int32_t *out)
{
    CosState &c = cos_built(h);
    if (n_words < 0 || (n_words > 0 && (!offsets || !out))) east_throw(EAST_HIP_ERR_INVALID, "bad look-up arguments");
    if (n_words == 0) return;
    const std::vector<u32> off32 = ragged_offsets_u32(offsets, n_words, cps, "bad word offsets", "word offsets must not decrease");
    const u32 n_cps = off32[n_words];
    Stats stats;
    c.work.ensure(align256(((size_t)n_cps + 1) * 4) + align256(((size_t)n_words + 1) * 4) * 2 + 4096, "the cosine index");
    Arena a = c.work.arena();
    Ctx ctx = handle_ctx(h, &a, &stats);
    u32 *d_w = a.alloc<u32>((size_t)n_cps + 1), *d_off = a.alloc<u32>((size_t)n_words + 1);
    int32_t *d_out = a.alloc<int32_t>((size_t)n_words + 1);
    if (n_cps) HIP_CHECK(hipMemcpyAsync(d_w, cps, (size_t)n_cps * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, h->stream));
    LAUNCH(ctx, cos_lookup_kernel, ceil_div_u32((u32)n_words, BLOCK), (const u32 *)d_w, (const u32 *)d_off, (u32)n_words, c.B, c.mask,
           (const u64 *)c.run_key, c.n_runs, (const u32 *)c.run_term, (const u32 *)c.term_off, (const u32 *)c.term_len,
           (const u32 *)c.tcp, d_out);
    HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n_words * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

// where the weights and norms of weighting wt live (CosUnits::weights)
static void cos_weight_ptrs(CosUnits &U, u32 D, int wt, double **w, double **norm)
{
    const size_t wb = align256(((size_t)U.P + 1) * 8), nb = align256(((size_t)D + 1) * 8);
    if (U.weights.cap < 2 * (wb + nb)) {
        U.w_valid[0] = U.w_valid[1] = false;
        U.weights.ensure(2 * (wb + nb), "the cosine index");
    }
    *w = (double *)(U.weights.p + wt * (wb + nb));
    *norm = (double *)(U.weights.p + wt * (wb + nb) + wb);
}

// The weights and norms of weighting wt into their place (cos_weight_ptrs), unless they are there: two launches on the
// context's stream, the squares' scratch (P + 1 doubles) out of its arena.  The caller sets U.w_valid[wt] once it has
// waited for the stream.  Shared by the score call and the text-to-text cosine (cosine_texts.h): the same doubles.
static void cos_make_weights(Ctx &ctx, const CosState &c, CosUnits &U, int wt, double *w, double *norm)
{
    if (U.w_valid[wt]) return;
    const u32 D = c.n_docs;
    double *sq = ctx.arena->alloc<double>((size_t)U.P + 1);
    if (U.P)
        LAUNCH(ctx, cos_weights_kernel, ceil_div_u32(U.P, BLOCK), (const u32 *)U.post_doc, (const u32 *)U.post_unit,
               (const u32 *)U.post_cnt, (const u32 *)U.unit_off, (const u32 *)c.n_d, (const u32 *)U.inv_perm, U.P, D, wt, w, sq);
    LAUNCH(ctx, cos_norms_kernel, ceil_div_u32(D, WAVES_PER_BLOCK), (const double *)sq, (const u32 *)U.doc_off, D, norm);
}

static void cos_score(east_hip_index *h, const int32_t *q_ids, const i64 *q_offsets, i64 q_len, int32_t K, int32_t weighting,
                      double *out)
{
    CosState &c = cos_built(h);
    if (K < 0 || weighting < 0 || weighting > 1 || (K > 0 && !q_offsets)) east_throw(EAST_HIP_ERR_INVALID, "bad score arguments");
    if (K == 0) return;
    const char *bad_offsets = "q_offsets must start at 0 and end at q_len";
    if (q_offsets[K] != q_len || q_len < 0) east_throw(EAST_HIP_ERR_INVALID, bad_offsets);
    const std::vector<u32> off32 = ragged_offsets_u32(q_offsets, K, q_ids, bad_offsets, "q_offsets must not decrease");
    CosUnits &U = c.use_classes ? c.cls : c.terms;
    for (i64 i = 0; i < q_len; i++)
        if (q_ids[i] < -1 || (q_ids[i] >= 0 && (u32)q_ids[i] >= U.n_units))
            east_throw(EAST_HIP_ERR_INVALID, "a query id is neither -1 nor a unit of the vector space");
    c.table_valid = false;
    const u32 D = c.n_docs, total = (u32)q_len;
    const size_t b_ids = align256(((size_t)total + 1) * 4), b_off = align256(((size_t)K + 1) * 4),
                 b_qw = align256(((size_t)total + 1) * 8), table = (size_t)K * D * 8;
    c.score.ensure(b_ids + b_off + b_qw + table, "the cosine index");
    int32_t *d_ids = (int32_t *)c.score.p;
    u32 *d_off = (u32 *)(c.score.p + b_ids);
    double *d_qw = (double *)(c.score.p + b_ids + b_off), *d_out = (double *)(c.score.p + b_ids + b_off + b_qw);
    double *w = nullptr, *norm = nullptr;
    cos_weight_ptrs(U, D, weighting, &w, &norm);
    Stats stats;
    Arena a = c.text.arena();             // (the build's first scratch: 6 bytes and more per byte of text, P <= bytes / 4)
    Ctx ctx = handle_ctx(h, &a, &stats);
    ConsumerTimer timer(h, c);
    cos_make_weights(ctx, c, U, weighting, w, norm);
    if (total) HIP_CHECK(hipMemcpyAsync(d_ids, q_ids, (size_t)total * 4, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(d_off, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (total)
        LAUNCH(ctx, cos_query_weights_kernel, ceil_div_u32(total, BLOCK), (const int32_t *)d_ids, (const u32 *)d_off, (u32)K, total,
               U.n_units, d_qw);
    LAUNCH(ctx, cos_score_kernel, std::min<u32>((u32)K, 1u << 16), (const int32_t *)d_ids, (const u32 *)d_off, (const double *)d_qw,
           (u32)K, (const u32 *)U.unit_off, (const u32 *)U.post_doc, (const double *)w, (const double *)norm, D, d_out);
    timer.stop();                           // (the time is the launches': the copy of the table is not in it)
    if (out) HIP_CHECK(hipMemcpyAsync(out, d_out, table, hipMemcpyDeviceToHost, h->stream));     // (null: the table stays on the device, graph.h)
    timer.finish();
    c.score_ms = c.ms;
    U.w_valid[weighting] = true;
    c.table = d_out;
    c.table_K = (u32)K;
    c.table_valid = true;
}

extern "C" {

int east_hip_cosine_build_texts(east_hip_handle_t h, const uint8_t *bytes, int64_t n_bytes, const int64_t *text_offsets,
                                int32_t n_docs, const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                                const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                                int32_t n_hi_upper, const uint32_t *stop_cps, const int64_t *stop_offsets, int32_t n_stop)
{
    return guarded([&] {
        cos_build(h, host_texts_joined(bytes, n_bytes, text_offsets, n_docs), UnicodeTablesHost{cp_class, cp_upper, word_hi, digit_hi, hi_upper_from, hi_upper_to, n_hi_upper}, stop_cps, stop_offsets, n_stop);
    });
}

int east_hip_cosine_build_texts_v(east_hip_handle_t h, const uint8_t *const *texts, const int64_t *lengths, int32_t n_docs,
                                  const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                                  const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                                  int32_t n_hi_upper, const uint32_t *stop_cps, const int64_t *stop_offsets, int32_t n_stop)
{
    return guarded([&] {
        cos_build(h, host_texts_separate(texts, lengths, n_docs), UnicodeTablesHost{cp_class, cp_upper, word_hi, digit_hi, hi_upper_from, hi_upper_to, n_hi_upper}, stop_cps, stop_offsets, n_stop);
    });
}

int east_hip_cosine_info(east_hip_handle_t h, int64_t *out, int32_t cap)
{
    if (!h || !out || cap < 0) return EAST_HIP_ERR_INVALID;
    const CosState *c = consumer_peek<CosState>(h);
    const bool b = c && c->valid;
    const int64_t v[10] = {b ? 1 : 0,
                           b ? (int64_t)c->n_docs : 0,
                           b ? (int64_t)c->n_kept : 0,
                           b ? (int64_t)c->n_runs : 0,
                           b ? (int64_t)c->V : 0,
                           b && c->use_classes ? (int64_t)c->cls.n_units : 0,
                           b ? (int64_t)(c->use_classes ? c->cls.P : c->terms.P) : 0,
                           b ? (int64_t)c->attempts : 0,
                           b ? (int64_t)(c->build_ms * 1000.0) : -1,
                           b && c->score_ms >= 0.f ? (int64_t)(c->score_ms * 1000.0) : -1};
    for (int i = 0; i < 10 && i < cap; i++) out[i] = v[i];
    return EAST_HIP_OK;
}

int east_hip_cosine_get_terms(east_hip_handle_t h, int64_t *offsets, uint32_t *cps, int64_t *n_cps)
{
    return guarded([&] {
        CosState &c = cos_built(h);
        std::vector<u32> off((size_t)c.V + 1);
        HIP_CHECK(hipMemcpyAsync(off.data(), c.term_off, off.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (n_cps) *n_cps = off[c.V];
        if (offsets)
            for (u32 t = 0; t <= c.V; t++) offsets[t] = off[t];
        if (cps && off[c.V]) {
            HIP_CHECK(hipMemcpyAsync(cps, c.tcp, (size_t)off[c.V] * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    });
}

int east_hip_cosine_set_classes(east_hip_handle_t h, const int32_t *term_class, int32_t n_classes)
{
    return guarded([&] { cos_set_classes(h, term_class, n_classes); });
}

int east_hip_cosine_lookup(east_hip_handle_t h, const uint32_t *cps, const int64_t *offsets, int32_t n_words, int32_t *ids)
{
    return guarded([&] { cos_lookup(h, cps, offsets, n_words, ids); });
}

int east_hip_cosine_score_table(east_hip_handle_t h, const int32_t *q_ids, const int64_t *q_offsets, int64_t q_len,
                                int32_t n_keyphrases, int32_t weighting, double *out)
{
    return guarded([&] { cos_score(h, q_ids, q_offsets, q_len, n_keyphrases, weighting, out); });
}

int east_hip_debug_set_term_hash_bits(int bits)
{
    if (bits < 0 || bits > COS_HASH_BITS) return EAST_HIP_ERR_INVALID;
    knobs_update([&](Knobs &k) { k.term_hash_bits = bits; });
    return EAST_HIP_OK;
}

}  // extern "C"
