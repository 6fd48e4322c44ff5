/*
 * east_hip.h -- C ABI of the MI355X (gfx950) annotated-suffix-array backend.
 *
 * This is the drop-in boundary for the one hot path of EAST
 * (mikhaildubov/AST-text-analysis): building the enhanced annotated suffix
 * array of every document and filling the keyphrase x document score table.
 * The reference has no FFI on this path -- it is a Python class plugin
 * (east/asts/base.py:10-46: subclass AST, set __algorithm__, implement
 * score()).  The entry points below are what that plugin binds through
 * ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success or a negative EAST_HIP_ERR_* code;
 *     east_hip_last_error() returns a thread-local message for the last failure
 *   - plain pointers and sizes only; the caller owns every host buffer
 *     (C-contiguous), the library owns device memory behind the opaque handle
 *   - calls are blocking unless the name ends in _async; a handle is not
 *     thread-safe, distinct handles are.  The east_hip_debug_* setters change process-wide DEFAULTS of the test
 *     knobs; every build / score / text call copies them once when it starts and runs on that copy to its end, so a
 *     setter never reaches into a call that is already in flight -- on this handle or another;
 *     one HIP stream per handle; every call runs on
 *     the handle's device and restores the calling thread's current HIP device before it returns
 *   - indices are int32 on the device (n_total < 2^31 - 8); the Python side
 *     widens to int64 to match the reference's np.int tables
 *   - symbols are Unicode code points; a symbol >= 0x0A00 is a string
 *     terminator (east/consts.py:23-24, east/asts/utils.py:25-40) and text symbols
 *     are < 0x0A00 -- the reference's own encoding, in which text at or above U+0A00
 *     cannot be told from a terminator.  Text of any script goes through the TAGGED
 *     encoding (east_hip_set_symbol_encoding): terminator i of a document is
 *     EAST_HIP_TERMINATOR_TAG | i, every other symbol a text code point < 0x110000
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     fails with EAST_HIP_ERR_NO_DEVICE
 */
#ifndef EAST_HIP_H
#define EAST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAST_HIP_OK                 0
#define EAST_HIP_ERR_NO_DEVICE     -1  /* no HIP device / bad device ordinal            */
#define EAST_HIP_ERR_INVALID       -2  /* bad argument (null pointer, size, offsets)    */
#define EAST_HIP_ERR_OOM           -3  /* device allocation failed                      */
#define EAST_HIP_ERR_HIP           -4  /* a HIP runtime call or kernel launch failed    */
#define EAST_HIP_ERR_DOMAIN        -5  /* input outside the reference's domain          */
#define EAST_HIP_ERR_NOT_BUILT     -6  /* score/get_tables before a successful build    */
#define EAST_HIP_ERR_INTERNAL      -7  /* self-check failed (a bug)                     */

#define EAST_HIP_TERMINATOR_START 0x0A00u /* east/consts.py:23-24 */
#define EAST_HIP_TERMINATOR_TAG   0x80000000u /* tagged encoding: this bit marks a string terminator */
#define EAST_HIP_SYMBOLS_REFERENCE 0 /* terminators are the code points 0x0A00+i, text is < 0x0A00 (the default) */
#define EAST_HIP_SYMBOLS_TAGGED    1 /* terminators are EAST_HIP_TERMINATOR_TAG|i, text is any code point        */

typedef struct east_hip_index *east_hip_handle_t;

/* Library / device discovery. */
const char *east_hip_version(void);
const char *east_hip_last_error(void);
int east_hip_device_count(void);       /* >= 0, or EAST_HIP_ERR_NO_DEVICE */

/*
 * Create / destroy an index object bound to one device.  reserve_symbols > 0
 * pre-allocates the device arena for builds of up to that many symbols so
 * that later builds do not allocate (0 = allocate lazily at build time).
 */
int east_hip_create(int device, int64_t reserve_symbols, east_hip_handle_t *out);
void east_hip_destroy(east_hip_handle_t h);
/* Forget the index, the keyphrases and the prepared texts but keep the stream and the device memory:
 * the handle then behaves like a new one.  Creating and destroying a handle costs ~4 ms of driver
 * calls -- more than a whole build of a small collection -- so callers that index one collection
 * after the other recycle handles (east/hip_backend.py keeps a small pool). */
int east_hip_reset(east_hip_handle_t h);

/*
 * Batched EASA build: replaces EnhancedAnnotatedSuffixArray.__init__
 * (east/asts/easa.py:16-24: make_unique_endings + _compute_suftab /
 * _compute_lcptab / _compute_childtab* / _compute_anntab) for D documents
 * at once -- i.e. HOT LOOP A of ASTRelevanceMeasure.set_text_collection
 * (east/relevance.py:34-49).
 *
 *   symbols       concatenation of every document's EASA string: for document
 *                 d, its strings in order, string i followed by the terminator
 *                 0x0A00+i (i local to the document) -- exactly the code points
 *                 of the reference's `self.string`
 *   n_total       number of symbols (sum of n_d)
 *   doc_offsets   D+1 offsets into symbols, doc_offsets[0]=0, [D]=n_total
 *   n_strings     D values m_d (strings per document = terminators per document)
 *
 * On success the suffix array, LCP table and annotation table of every document
 * are resident on the device -- everything score() needs.  The three child tables
 * (easa.py:22-23) are only needed by callers that read them: they are built by the
 * first east_hip_get_tables request that asks for them (two more launches, about a
 * quarter of a build; bench.py reports them as child_tables_ms).  (How: a window sort over all
 * suffixes with tie refinement, data-parallel DC3 as the fallback -- DESIGN.md 4;
 * either way the tables are bit for bit what easa.py computes.)  east_hip_build_device takes a
 * DEVICE pointer for `symbols` (doc_offsets / n_strings stay host pointers);
 * the buffer is only read.  east_hip_build's copy to the device: symbols of the reference's
 * encoding fit 16 bits, so from 4 Mi symbols on -- the handle's first such call pins a 24 MiB upload
 * ring, once -- host threads narrow them to 16-bit words into the ring and a kernel
 * widens them on the device (half the bytes over the link; east_hip_build_info [25]) -- a text symbol
 * is below U+0A00, everything from there on is a terminator, whose number the build never reads --,
 * and to BYTES (a quarter of the bytes) while every text symbol lies below 0xFF, as in ASCII word text: a
 * symbol that does not fit starts the upload over with 16-bit words, for that call and the handle's later ones;
 * tagged streams and small inputs take the plain 4-byte copy.
 * When east_hip_build_device returns, every read of the caller's symbol buffer has completed: the caller may reuse or
 * overwrite it at once.  The handle's stream may still hold work then -- the launches that finish the score walk's
 * k-gram tables, queued behind the build's flags read-back when keyphrases are resident (east_hip_build_info [29]);
 * they read the index alone, and every later call on the handle is ordered behind them (same stream, or it drains it).
 */
/*
 * Which encoding east_hip_build / east_hip_build_device read on this handle (default: the reference's).
 * With EAST_HIP_SYMBOLS_TAGGED the text may hold code points at or above U+0A00 (Indic scripts, Thai, CJK,
 * Hangul, precomposed Vietnamese, IPA capitals ...).  The text symbols are ordered by code point and the
 * terminators sort ABOVE all of them, as they do for every text the reference is defined on.  The reference
 * itself has no meaningful answer there: its terminators chr(0x0A00+i) fall below such text, and then
 * easa.py loses the root annotation (anntab[0] = -m, negative scores: the bottom-up traversal,
 * easa.py:57-85, is never flushed when the last suffix is not a terminator) or raises IndexError
 * (easa.py:349-356 reads childtab_up[n]), and ast_linear disagrees with ast_naive
 * (tests/golden/high_text.json records all three).  What is computed here is the method itself: the
 * scores of ast_naive, and the tables easa.py gives after an order-preserving renaming of the text
 * alphabet into code points below U+0A00.
 */
int east_hip_set_symbol_encoding(east_hip_handle_t h, int32_t encoding);
int east_hip_build(east_hip_handle_t h, const uint32_t *symbols, int64_t n_total,
                   const int64_t *doc_offsets, const int32_t *n_strings, int32_t n_docs);
int east_hip_build_device(east_hip_handle_t h, const uint32_t *d_symbols, int64_t n_total,
                          const int64_t *doc_offsets, const int32_t *n_strings, int32_t n_docs);

/*
 * The same build straight from raw texts: text preparation on the device.  Replaces, for the
 * whole collection, the chain in front of the AST construction
 *   utils.prepare_text (utf-8 decode with errors='replace' + upper)      east/utils.py:31-34
 *   utils.tokenize ([\w']+ under re.U)                                    east/utils.py:37-38
 *   utils.text_to_strings_collection (tokens with len > 2 and not isdigit,
 *       groups of 3, empty -> [" "])                                       east/utils.py:49-79
 *   asts.utils.make_unique_endings + "".join                              east/asts/utils.py:25-40
 * and then runs east_hip_build on the result.
 *
 *   bytes         the texts concatenated, EVERY text followed by one 0xFF byte
 *   text_offsets  D+1 offsets: text d is bytes[text_offsets[d] .. text_offsets[d+1]-1) + its 0xFF
 *   cp_class      0x0A00 bytes: bit 0 = the code point matches [\w'], bit 1 = str.isdigit()
 *   cp_upper      0x0A00 words: 1:1 upper-case mapping (identity where upper() is not one code point)
 *   word_hi       bitmap of the [\w'] code points in [0x0A00, 0x110000), bit (cp - 0x0A00)
 *   digit_hi      the same for str.isdigit(); hi_upper_from / hi_upper_to: the sorted 1:1 upper-case
 *                 mappings of code points >= 0x0A00
 * Texts whose kept tokens hold characters at or above U+0A00 are built in the tagged encoding (see
 * east_hip_set_symbol_encoding; east_hip_prepared_encoding says which one east_hip_get_prepared returns).
 * The Unicode tables come from the caller's interpreter, so the device agrees with the host's
 * re / str semantics by construction.  east_hip_get_prepared returns what was built:
 * n_total symbols, D+1 symbol offsets, D string counts, and the symbols (each pointer nullable).
 */
int east_hip_build_texts(east_hip_handle_t h, const uint8_t *bytes, int64_t n_bytes,
                         const int64_t *text_offsets, int32_t n_docs, const uint8_t *cp_class,
                         const uint32_t *cp_upper, const uint32_t *word_hi, const uint32_t *digit_hi,
                         const uint32_t *hi_upper_from, const uint32_t *hi_upper_to, int32_t n_hi_upper);
/* The same for texts that lie apart in host memory (text d = lengths[d] bytes at texts[d], no
 * separators): they are uploaded one by one, the caller does not have to join them (for a few large
 * texts the join costs more than the build). */
int east_hip_build_texts_v(east_hip_handle_t h, const uint8_t *const *texts, const int64_t *lengths,
                           int32_t n_docs, const uint8_t *cp_class, const uint32_t *cp_upper,
                           const uint32_t *word_hi, const uint32_t *digit_hi,
                           const uint32_t *hi_upper_from, const uint32_t *hi_upper_to, int32_t n_hi_upper);
int east_hip_get_prepared(east_hip_handle_t h, int64_t *n_total, int64_t *doc_offsets,
                          int32_t *n_strings, uint32_t *symbols);
int east_hip_prepared_encoding(east_hip_handle_t h);   /* EAST_HIP_SYMBOLS_REFERENCE or _TAGGED */
double east_hip_last_prep_ms(east_hip_handle_t h);

/*
 * Copy one document's tables to the host (each pointer nullable, n_d int32
 * values each, positions local to the document): the reference attributes
 * suftab, lcptab, anntab (easa.py:20-24) and childtab_up / childtab_down /
 * childtab_next_l_index (easa.py:268-304).
 */
int east_hip_get_tables(east_hip_handle_t h, int32_t doc, int32_t *suftab, int32_t *lcptab,
                        int32_t *anntab, int32_t *childtab_up, int32_t *childtab_down,
                        int32_t *childtab_next_l_index);

/*
 * Keyphrase x document score table: replaces HOT LOOP B
 * (east/applications.py:43-52 -> relevance.py:51-53 -> easa.py:26-36,91-139).
 *
 *   q_symbols   concatenated code points of the K prepared keyphrases with
 *               U+0020 already removed (easa.py:36)
 *   q_offsets   K+1 offsets into q_symbols; every keyphrase must be non-empty
 *               (the reference raises ZeroDivisionError, easa.py:134)
 *   normalized  non-zero = divide each suffix score by its matched length
 *               (easa.py:128-129), zero = the CLI's -d
 *   out         K x D doubles, row-major (out[k*D + d])
 *   suffix_out  nullable; D x S doubles (S = q_offsets[K]), suffix_out[d*S + s]
 *               = the per-suffix result of the suffix starting at q_symbols[s]
 *               (the values of return_suffix_scores=True, easa.py:132-137)
 */
int east_hip_score_table(east_hip_handle_t h, const uint32_t *q_symbols,
                         const int64_t *q_offsets, int32_t n_keyphrases, int normalized,
                         double *out, double *suffix_out);

/*
 * The same in two steps, for callers that score one keyphrase set repeatedly
 * or want the table to stay in HBM: east_hip_set_keyphrases uploads the
 * keyphrases (host pointers, as above) and keeps them resident;
 * east_hip_score_resident runs the score kernels on the resident index and
 * keyphrases.  d_out (nullable) is a DEVICE pointer receiving the K x D table;
 * without it the table stays in the handle's own buffer.  The _async form only
 * queues the kernels on the handle's stream (pair with east_hip_synchronize).
 */
int east_hip_set_keyphrases(east_hip_handle_t h, const uint32_t *q_symbols,
                            const int64_t *q_offsets, int32_t n_keyphrases);
int east_hip_score_resident(east_hip_handle_t h, int normalized, double *d_out);
int east_hip_score_resident_async(east_hip_handle_t h, int normalized);

/*
 * Synonym-expanded scoring (east/asts/easa.py:27-34 behind relevance.py:51-53 with a synonimizer):
 * the caller expands every keyphrase into its variants (itertools.product of the per-word
 * alternatives), the variants are scored as n_queries ordinary queries and the score of keyphrase g
 * is the maximum over its variants [group_offsets[g], group_offsets[g+1]) -- a segmented max on the
 * device.  out: n_groups x D doubles.  (The reference scores the variants with normalized=True
 * whatever its caller asked for; the Python side passes 1 to reproduce that.)
 */
int east_hip_score_table_grouped(east_hip_handle_t h, const uint32_t *q_symbols,
                                 const int64_t *q_offsets, int32_t n_queries,
                                 const int64_t *group_offsets, int32_t n_groups, int normalized,
                                 double *out);

/*
 * The lcp-intervals of one document for the traversal API (easa.py:38-85, base.py:28-34): for every
 * rank k that is the first l-index of an lcp-interval (anntab[k] > 0, k > 0) left[k] = its left
 * boundary i (the interval is lcptab[k]-[i .. i + anntab[k] - 1]), -1 for every
 * other rank.  n_d int32 values, positions local to the document.
 */
int east_hip_get_lcp_intervals(east_hip_handle_t h, int32_t doc, int32_t *left);

/* Roofline accounting for bench.py: runs the score kernels on the resident index and keyphrases once more
 * and counts what the walks read -- k-gram table entries and binary-search probes (one suffix-array entry +
 * one symbol each), the "probes" of SURVEY.md 8(d).  Not a timed path. */
int east_hip_score_probes(east_hip_handle_t h, int normalized, int64_t *probes);

/*
 * The cosine relevance measure (`east -s cosine`): replaces CosineRelevanceMeasure (east/relevance.py:56-168) with the
 * token filter it uses, tokenize_and_filter (east/utils.py:31-46).  A term index of the whole collection lives in the
 * handle beside the EASA index: a cosine build never disturbs an EASA index and the other way round; east_hip_reset
 * forgets both.  (How: csrc/cosine.h)
 *
 * east_hip_cosine_build_texts[_v]  set_text_collection (relevance.py:65-83): the texts and the Unicode tables as for
 *     east_hip_build_texts[_v] (utf-8 with errors='replace', upper case 1:1, [\w']+ tokens).  A token is kept when it
 *     has at least 3 code points -- no isdigit filter and no U+0A00 limit: every script is plain terms -- and is not
 *     one of the n_stop stopwords (code points, already upper-cased; stop_offsets: n_stop + 1 offsets into stop_cps).
 *     The terms are the distinct kept words numbered by first occurrence in the collection; the index holds the postings
 *     (term, document, count) and n_d, the kept tokens of every document.
 * east_hip_cosine_info  out[0..9]: built, documents, kept tokens (stopwords included), distinct words (stopwords
 *     included), terms V, classes (0 while the terms are the vector space), postings of the vector space, hash attempts
 *     of the build, device time of the last build and of the last score call in microseconds (-1: none).
 * east_hip_cosine_get_terms  the terms in id order: V + 1 offsets in code points and the code points (each pointer
 *     nullable; *n_cps = the number of code points).
 * east_hip_cosine_set_classes  the vector space of stems (relevance.py:86-97): term_class[t] = the class of term t, the
 *     classes numbered by the smallest term id in each; the postings are re-keyed by class and their counts merged.
 *     n_classes = 0 goes back to the terms.
 * east_hip_cosine_lookup  words (code points, prepared) -> term ids, -1 for a word that is not a term (a stopword is none).
 * east_hip_cosine_score_table  relevance() (relevance.py:150-168) for K keyphrases x every document:
 *     q_ids[q_offsets[k] .. q_offsets[k + 1]) = the kept tokens of keyphrase k as ids of the vector space (term ids, or
 *     class ids after east_hip_cosine_set_classes), -1 for a token outside it (it still counts in the query's length);
 *     q_len = q_offsets[K].  weighting: 0 = tf, 1 = tf-idf.  out: K x D doubles, row-major, the layout of
 *     east_hip_score_table.  score = dot(w_d, q) / (|w_d| |q|), the norm of an all-zero vector being 1.  out may be
 *     null: the table then stays on the device only, where the keyphrase graph reads it (below).
 */
int east_hip_cosine_build_texts(east_hip_handle_t h, const uint8_t *bytes, int64_t n_bytes, const int64_t *text_offsets,
                                int32_t n_docs, const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                                const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                                int32_t n_hi_upper, const uint32_t *stop_cps, const int64_t *stop_offsets, int32_t n_stop);
int east_hip_cosine_build_texts_v(east_hip_handle_t h, const uint8_t *const *texts, const int64_t *lengths, int32_t n_docs,
                                  const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                                  const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                                  int32_t n_hi_upper, const uint32_t *stop_cps, const int64_t *stop_offsets, int32_t n_stop);
int east_hip_cosine_info(east_hip_handle_t h, int64_t *out, int32_t cap);
int east_hip_cosine_get_terms(east_hip_handle_t h, int64_t *offsets, uint32_t *cps, int64_t *n_cps);
int east_hip_cosine_set_classes(east_hip_handle_t h, const int32_t *term_class, int32_t n_classes);
int east_hip_cosine_lookup(east_hip_handle_t h, const uint32_t *cps, const int64_t *offsets, int32_t n_words, int32_t *ids);
int east_hip_cosine_score_table(east_hip_handle_t h, const int32_t *q_ids, const int64_t *q_offsets, int64_t q_len,
                                int32_t n_keyphrases, int32_t weighting, double *out);

/*
 * BM25 (`east -s bm25`): Okapi BM25 as a second score call of the cosine term index -- the same postings, document
 * lengths, classes and query look-up; nothing else is built.  (How: csrc/bm25.h)
 *
 * In the current vector space (the terms, or the classes after east_hip_cosine_set_classes): D = the documents, df_u = the
 * postings of unit u, c_ud = the count of a posting, n_d = the index's own document length (the one tf divides by),
 * N = the sum of n_d (an exact integer) and avgdl = (double)N / (double)D, one double that every path shares.
 *     idf_u = log1p((D - df_u + 0.5) / (df_u + 0.5))                      (the non-negative form; log1p, not log(1 + x))
 *     w_ud  = idf_u * (c_ud * (k1 + 1)) / (c_ud + k1 * ((1 - b) + b * (n_d / avgdl)))
 *     score(k, d) = the sum of qtf_ku * w_ud over the distinct units u of keyphrase k that have a posting in d, taken in
 *                   the order of their first occurrence in the keyphrase; qtf = how often the unit occurs among the
 *                   keyphrase's kept tokens.  A token outside the vector space (id -1) contributes nothing and changes
 *                   nothing.  A (k, d) without a common unit is exactly +0.0; every score is >= 0.
 * Every operation is one IEEE double rounding in the order written.  k1 finite and >= 0, 0 <= b <= 1; anything else, NaN
 * included, is EAST_HIP_ERR_INVALID (the usual values: 1.2 and 0.75).  Not in it: BM25+ / BM25F / a query-side k3, a
 * text-to-text BM25, several devices, the AST side.
 *
 * east_hip_bm25_score_table  q_ids / q_offsets / q_len / n_keyphrases / out as east_hip_cosine_score_table takes them,
 *     with the same checks, made before anything is invalidated: a refused call leaves the previous table offered.  out
 *     may be null.  The K x D table is left where a cosine score call leaves its own: EAST_HIP_GRAPH_SOURCE_COSINE names
 *     the table of the last score call of either kind, and east_hip_cosine_info out[9] is that call's time.  The P
 *     weights are cached per vector space with the (k1, b) they were made for; a build and east_hip_cosine_set_classes
 *     drop them, other parameters replace them.  The cosine weights are never touched.  Two calls give the same bytes.
 * east_hip_bm25_info  out[0..4]: N, avgdl, the cached k1 and b of the current vector space (NaN: none), and how many
 *     times the weights have been computed on this index since its build.
 * Both: EAST_HIP_ERR_NOT_BUILT before a cosine build.
 */
int east_hip_bm25_score_table(east_hip_handle_t h, const int32_t *q_ids, const int64_t *q_offsets, int64_t q_len,
                              int32_t n_keyphrases, double k1, double b, double *out);
int east_hip_bm25_info(east_hip_handle_t h, double *out, int32_t cap);

/*
 * The keyphrase graph (`east keyphrases graph`): the main loop of keyphrases_graph (east/applications.py:59-149) on the
 * device, from a K x D score table that is already there.  A keyphrase occurs in a text when score >= relevance_threshold
 * (a NaN score never does, -0.0 >= 0.0 does); its support is the number of such texts; the nodes are the positions p of
 * the keyphrase list with (double)support >= support_threshold (applications.py:103-109); for every ordered pair of
 * nodes (A, B), A != B, in list order, the edge A -> B exists when (double)shared / (double)max(support_A, 1) >=
 * referral_confidence (applications.py:111-141: one correctly rounded IEEE division, as Python's).  (How: csrc/graph.h,
 * DESIGN.md 10.)
 *
 * rows[p] = the table row of node position p, 0 <= rows[p] < K (a keyphrase listed twice names the same row twice);
 * n_positions = the length of the keyphrase list.  out[0] = the kept nodes, out[1] = the edges (64 bits: nothing is cut
 * short; an edge buffer the device cannot hold is EAST_HIP_ERR_OOM with the number of edges in the message).
 * The build call on the RESIDENT table takes it where the last score call of the handle left it -- no score crosses the
 * link: source EAST_HIP_GRAPH_SOURCE_AST = the table of the resident keyphrases (the last score call of the AST
 * index, asynchronous ones included: the graph is queued behind it); EAST_HIP_GRAPH_SOURCE_COSINE = the table of the last
 * cosine score call; EAST_HIP_GRAPH_SOURCE_UPLOADED = the copy the last build call on a host table left on the device
 * (further graphs of one table from elsewhere, at other thresholds, without another upload).  EAST_HIP_ERR_NOT_BUILT where
 * no such table is there (no score call since the last build or since the keyphrases were set).  The build call on a HOST
 * table uploads K x D doubles, row-major, first.
 * The fetch call gives the last graph (each pointer nullable): support[n_positions], kept[out[0]] = the node positions in
 * order, and per edge, in the order of applications.py:111-141 (sources in list order, a source's targets in list order),
 * source position, target position and the number of shared texts -- confidence = shared / max(support[source], 1).
 * Two builds of the same input give the same bytes (no atomic decides an order).  The graph's buffers are the handle's
 * own -- neither the EASA arena nor the cosine buffers --; the reset call releases them, destroying the handle too.
 * Device time of the last graph build in milliseconds (events on the handle's stream around the build, its two
 * read-backs -- kept nodes, edges -- included), -1 when there is none.
 */
#define EAST_HIP_GRAPH_SOURCE_AST 0
#define EAST_HIP_GRAPH_SOURCE_COSINE 1
#define EAST_HIP_GRAPH_SOURCE_UPLOADED 2
int east_hip_graph_build_resident(east_hip_handle_t h, int32_t source, const int32_t *rows, int64_t n_positions,
                                  double relevance_threshold, double support_threshold, double referral_confidence,
                                  int64_t *out);
int east_hip_graph_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs,
                              const int32_t *rows, int64_t n_positions, double relevance_threshold, double support_threshold,
                              double referral_confidence, int64_t *out);
int east_hip_graph_fetch(east_hip_handle_t h, int32_t *support, int32_t *kept, int32_t *edge_source, int32_t *edge_target,
                         int32_t *edge_shared);
double east_hip_last_graph_ms(east_hip_handle_t h);

/*
 * Synonym extraction (`east -y -t <triples>`): the arithmetic of the reference's SynonymExtractor
 * (east/synonyms/synonyms.py:116-169) on the device, from dependency triples the caller has -- the parser that makes them
 * (:52-88) is not part of this library.  (How: csrc/synonyms.h)
 *
 * The build call (replaces synonyms.py:74-86, :116-142) takes the n_triples RAW triples (w1[i], relation[i], w2[i]) as ids,
 * 0 <= word id < n_words <= 2^26, 0 <= relation id < n_relations <= 2^12 (the fields of the 64-bit triple key; more is
 * EAST_HIP_ERR_INVALID, as are ids out of range and 2^30 triples or more), and inverse_relation[r] = the id of r without a
 * trailing "_of", or of r + "_of" (:81): an involution of the relation ids.  Every triple is entered with its inverse
 * (w2, r', w1); f(t) = occurrences of t in that doubled list; F_r, F_w1r, F_rw2 = the sums of f^2 over the distinct triples
 * with that relation / first two / last two members (:129-131 add f once per occurrence); q = (double)f * F_r / F_w1r /
 * F_rw2 in exactly this order, I = max(log(q), 0).  A feature (r, w2) belongs to T(w1) iff q > 1.0 -- the reference's bit
 * for bit; only the last place of log may differ.  The rows are kept in CSR form: row = word, columns = its features in
 * ascending (relation id, word id) order.
 * The info call gives {raw triples, distinct triples (inverses included), words, relations, kept features, longest row}
 * and returns 0; the rows call gives (each pointer nullable) offsets[n_words + 1], per kept feature its relation id, word
 * id and I, and per word the sum of its I (the divisor's half, :147-148, added in column order).
 * The similarity call (:144-152) gives out[i] = similarity(a[i], b[i]) for n_pairs pairs of word ids: the sum of
 * I(a, .) + I(b, .) over the common features in ascending column order, divided once by the two row sums, 0.0 where the
 * divisor is 0.
 * The pairs call (:154-169) takes the candidate word ids -- distinct, in the order the caller wants the pairs in -- and the
 * threshold (>= 0; negative or NaN is EAST_HIP_ERR_INVALID, as is a duplicate candidate or more than 2^20 of them) and
 * finds every pair of candidates (i < j in list order) with similarity > threshold; *n_pairs = how many.  The fetch call
 * gives them (each pointer nullable): a[k] = candidates[i], b[k] = candidates[j] and the similarity, ordered by i, then j.
 * No atomic decides a slot and no floating-point sum depends on timing: two runs give the same bytes.
 * EAST_HIP_ERR_NOT_BUILT before a successful build (fetch: before a pairs call).  The buffers are the handle's own: a
 * synonyms build leaves the EASA index, the cosine index and the graph alone and they leave it alone; the reset call
 * releases them, destroying the handle too.
 * Device time of the last build or pairs call in milliseconds (events on the handle's stream around it, read-backs
 * included), -1 when there is none.
 */
int east_hip_synonyms_build(east_hip_handle_t h, const int32_t *w1, const int32_t *relation, const int32_t *w2,
                            int64_t n_triples, const int32_t *inverse_relation, int32_t n_words, int32_t n_relations);
int east_hip_synonyms_info(east_hip_handle_t h, int64_t *out, int32_t cap);
int east_hip_synonyms_get_rows(east_hip_handle_t h, int64_t *offsets, int32_t *relation, int32_t *word, double *value,
                               double *row_sum);
int east_hip_synonyms_similarity(east_hip_handle_t h, const int32_t *a, const int32_t *b, int64_t n_pairs, double *out);
int east_hip_synonyms_pairs(east_hip_handle_t h, const int32_t *candidates, int32_t n_candidates, double threshold,
                            int64_t *n_pairs);
int east_hip_synonyms_fetch(east_hip_handle_t h, int32_t *a, int32_t *b, double *similarity);
double east_hip_last_synonyms_ms(east_hip_handle_t h);

/*
 * Ranked keyphrases (`east keyphrases top`): the N best rows of every column of a K x D score table that is already on the
 * device, or the N best columns of every row.  (How: csrc/top.h)
 *
 * The table is K x D doubles, row-major (t[k * D + d]).  axis EAST_HIP_TOP_BY_TEXT: a SEGMENT is a column d and its MEMBERS
 * are the K rows; axis EAST_HIP_TOP_BY_KEYPHRASE: a segment is a row k and its members are the D columns.  S = the number
 * of segments, L = the members of each.  For every segment the result is the first min(n, eligible) members of this total
 * order: (1) a member is eligible when score >= threshold -- a NaN score never is, -0.0 >= 0.0 is, the threshold -inf means
 * every number, a NaN threshold is EAST_HIP_ERR_INVALID; (2) eligible members are ordered by score descending and, among
 * equal scores (-0.0 and +0.0 are equal), by member index ascending.  In Python, for one segment with scores v:
 * sorted((i for i in range(L) if v[i] >= threshold), key=lambda i: (-v[i], i))[:n].  1 <= n <= 1024 (anything else is
 * EAST_HIP_ERR_INVALID, as is an unknown axis); n > L is allowed, the lists are then shorter.
 * The build call on the RESIDENT table takes `source` as east_hip_graph_build_resident does, under the same conditions and
 * with the same EAST_HIP_ERR_NOT_BUILT cases: EAST_HIP_GRAPH_SOURCE_AST, EAST_HIP_GRAPH_SOURCE_COSINE, and
 * EAST_HIP_GRAPH_SOURCE_UPLOADED = the copy the last east_hip_top_build_host left on the device (NOT the graph's table).
 * The build call on a HOST table uploads K x D doubles first.  out[0] = S, out[1] = the sum of the counts.  A result the
 * device cannot hold is EAST_HIP_ERR_OOM with the sizes in the message.
 * The fetch call gives the last ranking (each pointer nullable): count[S]; index[S * n], member indices best first, -1 in
 * the places behind count[s]; score[S * n], the table's own bytes (a selected -0.0 comes back as -0.0), 0.0 behind count[s].
 * Two builds of the same input give the same bytes (a member's place is its rank; no atomic exists).  The ranking's buffers
 * are the handle's own -- not the EASA arena, the cosine buffers or the graph's: a graph and a ranking of one handle live
 * side by side --; the reset call releases them, destroying the handle too.
 * Device time of the last ranking in milliseconds (events on the handle's stream around the two kernels and the read-back
 * of the counts), -1 when there is none.
 */
#define EAST_HIP_TOP_BY_TEXT 0
#define EAST_HIP_TOP_BY_KEYPHRASE 1
int east_hip_top_build_resident(east_hip_handle_t h, int32_t source, int32_t axis, int32_t n, double threshold, int64_t *out);
int east_hip_top_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs, int32_t axis,
                            int32_t n, double threshold, int64_t *out);
int east_hip_top_fetch(east_hip_handle_t h, int32_t *count, int32_t *index, double *score);
double east_hip_last_top_ms(east_hip_handle_t h);

/*
 * Similar texts and keyphrases (`east keyphrases similar`): the cosine of every two columns of a K x D score table that is
 * already on the device, or of every two rows, and -- through the ranking above -- the n most similar others of each.
 * (How: csrc/similarity.h)
 *
 * The table is K x D doubles, row-major.  axis EAST_HIP_TOP_BY_TEXT: the M = D MEMBERS are the texts, the PROFILE of text d
 * is its column, p_d[l] = t[l * D + d], L = K entries; axis EAST_HIP_TOP_BY_KEYPHRASE: M = K, the profile of keyphrase k is
 * its row, p_k[l] = t[k * D + l], L = D.
 * q_a = the sum over l of p_a[l]^2, G_ab = the sum over l of p_a[l] * p_b[l].  The similarity matrix is M x M doubles,
 * row-major: S[a][a] = NaN; S[a][b] = +0.0 when q_a == 0 or q_b == 0; otherwise S[a][b] = G_ab / (sqrt(q_a) * sqrt(q_b)),
 * four IEEE double operations in that order (not sqrt(q_a * q_b), which overflows where this does not).  Nothing is
 * clamped: two equal profiles may come out one or two ulp off 1.  Non-finite table entries propagate as the arithmetic
 * propagates them; a NaN similarity is never ranked.
 * Guaranteed: S[a][b] and S[b][a] are the same bytes; two builds of the same input give the same bytes (no atomic is used,
 * no sum's order depends on timing).  The order of the sums is otherwise the implementation's choice.
 * Accuracy, for finite tables: |S - S_exact| <= (2 L + 16) * 2^-53.  (With u = 2^-53: summation in any order, with or
 * without fma, gives |G_ab error| <= gamma_(L+2) * sum |p_a p_b| <= gamma_(L+2) * sqrt(q_a q_b); the same relative bound
 * holds on q and half of it survives each square root; one u each for the two roots, the product and the quotient.)
 *
 * The build call on the RESIDENT table takes `source` as east_hip_top_build_resident does, with the same
 * EAST_HIP_ERR_NOT_BUILT cases: EAST_HIP_GRAPH_SOURCE_AST, EAST_HIP_GRAPH_SOURCE_COSINE, and EAST_HIP_GRAPH_SOURCE_UPLOADED =
 * the copy the last east_hip_similarity_build_host left on the device (the similarity's own copy: NOT the graph's and NOT
 * the ranking's).  An unknown axis or source is EAST_HIP_ERR_INVALID.  The build call on a HOST table uploads K x D doubles
 * first.  out[0] = M, out[1] = L.  A matrix the device cannot hold is EAST_HIP_ERR_OOM with M and the bytes in the message.
 * The fetch call gives the last matrix (each pointer nullable): matrix[M * M] and norm2[M] = q.  EAST_HIP_ERR_NOT_BUILT
 * before a build.
 * Ranking the matrix: east_hip_top_build_resident accepts the source EAST_HIP_GRAPH_SOURCE_SIMILARITY = the M x M matrix
 * the last similarity build of this handle left, ranked like any table (callers use EAST_HIP_TOP_BY_KEYPHRASE: a segment is
 * a row; the NaN on the diagonal is never eligible, so no member lists itself); EAST_HIP_ERR_NOT_BUILT before a similarity
 * build.  The result is the handle's ONE ranking: it replaces the previous one, as any later ranking replaces it.
 * The similarity's buffers (the uploaded copy, q, the matrix) are the handle's own -- not the EASA arena, the cosine
 * buffers, the graph's or the ranking's; a later score call does not invalidate a finished matrix; the reset call releases
 * them, destroying the handle too.
 * Device time of the last similarity build in milliseconds (events on the handle's stream around the two kernels), -1 when
 * there is none.
 */
#define EAST_HIP_GRAPH_SOURCE_SIMILARITY 3
int east_hip_similarity_build_resident(east_hip_handle_t h, int32_t source, int32_t axis, int64_t *out);
int east_hip_similarity_build_host(east_hip_handle_t h, const double *table, int32_t n_keyphrases, int32_t n_docs, int32_t axis,
                                   int64_t *out);
int east_hip_similarity_fetch(east_hip_handle_t h, double *matrix, double *norm2);
double east_hip_last_similarity_ms(east_hip_handle_t h);

/*
 * Text-to-text relatedness (`east texts related`): how much of text A's wording is found in text B, for every two documents
 * of the index, and -- through the ranking above -- the n most related others of each.  (How: csrc/related.h)
 *
 * Let the index hold D documents.  The STRINGS of document A are the strings of its collection as the index holds them: the
 * runs of text symbols between the terminators of its EASA string, m_A = n_strings[A] of them (in both encodings, on the
 * byte and on the 32-bit code stream).  A string is SCORED when it is not empty once U+0020 is removed -- in practice only
 * the [" "] placeholder of a text without a kept token is not --; c_A = the scored strings of A.
 * score(s, B) is exactly what east_hip_score_table returns for the keyphrase s against document B with the same
 * `normalized` flag: the same 8 bytes.  The forward matrix is F[A][B] = (the sum over the scored strings s of A of
 * score(s, B)) / c_A, and +0.0 for every B when c_A = 0.  The result R is D x D doubles, row-major:
 *   orientation EAST_HIP_RELATED_DIRECTED:  R[A][B] = F[A][B]
 *   orientation EAST_HIP_RELATED_SYMMETRIC: R[A][B] = (F[A][B] + F[B][A]) * 0.5 -- R[A][B] and R[B][A] are the same bytes
 * In both R[A][A] = NaN, and self[A] = F[A][A] is reported separately.
 * Order of the sums: the sum over a document's strings is a fixed tree whose shape depends on c_A alone -- tiles of a fixed
 * number of scored strings, aligned to the document's first, added in tile order.  It depends neither on how the strings
 * are cut into score launches nor on D; no atomic is used.  Two builds of the same input give the same bytes, under any
 * chunk setting (east_hip_debug_set_related_chunk).
 * Accuracy: the scores are finite and >= 0, so summing c of them in any order is off by less than gamma_(c-1) relative;
 * one rounding for the division, one for the addition of the symmetric form, the halving is exact:
 * |R[A][B] - exact| <= (max(c_A, c_B) + 4) * 2^-53 * exact, `exact` being the formula without rounding on the device's own
 * per-string scores.
 *
 * The build call: out[0] = D, out[1] = the scored strings (the sum of c_A), out[2] = the score launches (chunks).
 * EAST_HIP_ERR_NOT_BUILT before a build of the index; EAST_HIP_ERR_INVALID for an unknown orientation or a null handle;
 * EAST_HIP_ERR_OOM with D and the bytes in the message when the matrix or a chunk cannot be had.  The call uses the score
 * scratch: it REPLACES the handle's resident keyphrases and withdraws its resident score table, exactly as a new
 * east_hip_set_keyphrases does, and afterwards east_hip_score_resident answers "no keyphrases set" until new ones are set.
 * The fetch call gives the last result (each pointer nullable): matrix[D * D], self[D], scored[D] = c_A.
 * EAST_HIP_ERR_NOT_BUILT before a related build.
 * Ranking the matrix: east_hip_top_build_resident accepts the source EAST_HIP_GRAPH_SOURCE_RELATED = the D x D matrix the
 * last related build of this handle left, ranked like any table (callers use EAST_HIP_TOP_BY_KEYPHRASE: a segment is a row;
 * the NaN on the diagonal keeps a text from listing itself); EAST_HIP_ERR_NOT_BUILT before a related build.  The handle
 * still has ONE ranking.
 * The matrix, self and scored live in buffers of their own -- not the EASA arena, the score scratch, the ranking's buffers
 * or the similarity's; a later score call or keyphrase set leaves a finished matrix valid; the reset call releases them,
 * destroying the handle too.
 * Device time of the last related build in milliseconds (events on the handle's stream around the whole build, the one
 * read-back of the strings' lengths included), -1 when there is none.
 * Test knob (process-wide, read when a build starts): the scored strings per score launch, rounded up to whole tiles; 0 =
 * the default (as many as keep a launch's score table at or below 256 MiB).  The result does not depend on it.
 */
#define EAST_HIP_RELATED_DIRECTED 0
#define EAST_HIP_RELATED_SYMMETRIC 1
#define EAST_HIP_GRAPH_SOURCE_RELATED 4
int east_hip_related_build(east_hip_handle_t h, int normalized, int32_t orientation, int64_t *out);
int east_hip_related_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *scored);
double east_hip_last_related_ms(east_hip_handle_t h);
int east_hip_debug_set_related_chunk(int64_t strings);

/*
 * Text-to-text cosine similarity (`east texts similar`): the cosine of the tf or tf-idf vectors of every two texts of the
 * cosine term index, and -- through the ranking above -- the n most similar others of each.  (How: csrc/cosine_texts.h,
 * DESIGN.md 15.)  Not to be confused with "Similar texts and keyphrases" above, the cosine of score-table profiles: these
 * entry points are named east_hip_text_similarity_*, those east_hip_similarity_*.
 *
 * A cosine index has been built on the handle; the vector space is the one the score call uses: the terms, or the classes
 * after east_hip_cosine_set_classes.  For a weighting (0 tf, 1 tf-idf) and documents a, b of the D of the index:
 *   x_d[u]   = the weight of posting (u, d): count / max(n_d, 1), times 1 + ln(D / df_u) under tf-idf -- the same double the
 *              score call uses;
 *   norm_d   = the norm the score call divides by: the squares of x_d in ascending unit order cut into 64 consecutive
 *              slices, the 64 partial sums added in order, the square root; 1.0 for a document without postings;
 *   G_ab     = the sum over the units u common to a and b of x_a[u] * x_b[u];
 *   C[a][b]  = G_ab / (norm_a * norm_b) for a != b: one product, one quotient; +0.0 when a and b share no unit (a document
 *              without postings shares none with anybody); C[a][a] = NaN, so that nobody lists itself;
 *   self[d]  = G_dd / (norm_d * norm_d), the diagonal before the NaN: 1 up to rounding for a document with postings, +0.0
 *              for one without (the two sums take different orders: their agreement is a check);
 *   postings[d] = the postings of document d in the vector space.
 * The matrix is D x D doubles, row-major.
 * Guaranteed: no atomic is used and the order of every sum is fixed by the collection alone -- the units of a pair in
 * ascending order inside fixed segments of the unit range, the segments' sums added in segment order; two builds give the
 * same bytes, under any value of the batch knob below; C[a][b] and C[b][a] are the same bytes (one value written to two
 * places); an exact value of 0 is +0.0 bit for bit.
 * Accuracy: all weights are non-negative, so no order of the sum cancels.  With t_ab the units common to a and b and
 * p_d = postings[d], for a != b
 *   |C[a][b] - exact| <= (t_ab + ceil(p_a / 64) + ceil(p_b / 64) + 128 + 48) * 2^-52 * exact
 * (t_ab roundings of the dot product; per norm a slice of ceil(p / 64) and 64 partial sums; 48 ulp for log, sqrt, the
 * divisions and the products, a weight entering a product on both sides), and the same with t_aa = p_a bounds |self[a] - 1|.
 *
 * The build call: out (at least 8 entries, nullable) = D, the units of the vector space, its postings, the 64 x 64 tiles of
 * document pairs computed (tile_a <= tile_b), the segments of the unit range, the kernel launches, the units of a staged
 * chunk (32), the units of a segment.  EAST_HIP_ERR_NOT_BUILT without a cosine index; EAST_HIP_ERR_INVALID for a null
 * handle or an unknown weighting; EAST_HIP_ERR_OOM with D and the bytes in the message when the matrix or its scratch
 * cannot be had.  A build that fails leaves no matrix.
 * The fetch call gives the last result (each pointer nullable): matrix[D * D], self[D], postings[D].
 * EAST_HIP_ERR_NOT_BUILT without a matrix.
 * The matrix is withdrawn by east_hip_reset, by every east_hip_cosine_build_texts* call and by every
 * east_hip_cosine_set_classes call (the space changed under it), whether or not that call succeeds.  A score call, a
 * similarity build, an EASA build or a ranking leaves it alone.
 * Ranking the matrix: east_hip_top_build_resident accepts the source EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS = the D x D matrix
 * the last build left, ranked like any table (callers use EAST_HIP_TOP_BY_KEYPHRASE: a segment is a row; the NaN on the
 * diagonal is never eligible); EAST_HIP_ERR_NOT_BUILT without a matrix.  The handle still has ONE ranking.
 * The matrix, self, postings, the postings in document order and the partial tiles live in buffers of their own -- not the
 * cosine index's, the EASA arena or another consumer's; the weights and norms are the cosine index's, made on first use by
 * this call or by the score call, whichever comes first.  Memory: 12 bytes a posting, the matrix, and partial tiles of at
 * most 256 MiB or of one segment (half the matrix's size), whichever is more.
 * Device time of the last build in milliseconds (events on the handle's stream around all launches), -1 before a build,
 * after a failed one and once the matrix has been withdrawn.
 * Test knob (process-wide, read when a build starts): the segments per launch of the tile kernel; 0 = the default (as many
 * as keep the partial tiles at or below 256 MiB).  The result does not depend on it.
 */
#define EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS 5
int east_hip_text_similarity_build(east_hip_handle_t h, int32_t weighting, int64_t *out);
int east_hip_text_similarity_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *postings);
double east_hip_last_text_similarity_ms(east_hip_handle_t h);
int east_hip_debug_set_text_similarity_batch(int64_t segments);

/*
 * Clusters (`east texts clusters`, `east keyphrases clusters`): single-linkage agglomerative clustering -- the maximum
 * spanning forest -- of a square matrix of similarities that is on the device already, and its flat cuts.  (How:
 * csrc/clusters.h)
 *
 * Input: S, M x M doubles, row-major, M >= 0.  The diagonal is never read for its value.  S is symmetric: for a != b
 * S[a][b] == S[b][a] as doubles (+0.0 against -0.0 is symmetric), or both are NaN.  The pair {a, b}, a < b, is an EDGE
 * when S[a][b] is not a NaN; its weight w is S[a][b], the upper triangle's bytes.  Plus and minus infinity are ordinary
 * weights.
 * Order: edge e is STRONGER than f when w_e > w_f (-0.0 and +0.0 are equal), or the weights are equal and a_e < a_f, or
 * the weights and a are equal and b_e < b_f.  A strict total order: the maximum spanning forest under it is unique.
 * The merges (the dendrogram): the forest's F edges, strongest first, as merge_a[i] < merge_b[i] and merge_w[i] -- the
 * edges Kruskal's algorithm accepts when it visits all edges in that order.  F = M minus the number of connected components
 * of the edge graph.  merge_w[i] is S[a][b]'s own bytes: a -0.0 comes back as -0.0.
 * Flat clusters, two cuts of the same dendrogram: by threshold t (not a NaN; minus infinity = every merge) the merges with
 * w >= t are applied, a prefix of the list; by count k >= 1 the first max(0, min(F, M - k)) merges are applied -- the order
 * above decides among equal weights, and there are never fewer than M - F clusters.  labels[v] (M entries, nullable) = the
 * smallest member of v's cluster; out (2 entries, nullable) = the clusters, the merges applied.
 * Guaranteed: only comparisons are made, no atomic is used; two builds give the same bytes; the result does not depend on
 * the grid, on timing or on the number of rounds, and equals Kruskal's on the same matrix bytes.
 *
 * east_hip_clusters_build_resident reads a matrix another call left on the device: source
 * EAST_HIP_GRAPH_SOURCE_SIMILARITY, EAST_HIP_GRAPH_SOURCE_RELATED or EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS (each symmetric by
 * its own contract: not checked; EAST_HIP_ERR_NOT_BUILT where there is none), or EAST_HIP_GRAPH_SOURCE_UPLOADED = the copy
 * the last east_hip_clusters_build_host left (the clusters' OWN copy, not the ranking's or the graph's).  A relatedness
 * matrix built with EAST_HIP_RELATED_DIRECTED is EAST_HIP_ERR_INVALID ("directed" in the message), as are
 * EAST_HIP_GRAPH_SOURCE_AST, EAST_HIP_GRAPH_SOURCE_COSINE and unknown sources: those are not square matrices of members.
 * east_hip_clusters_build_host uploads m x m doubles first and checks the copy for symmetry on the device; a matrix that
 * is not symmetric is EAST_HIP_ERR_INVALID with the first offending pair (in row-major order) in the message, and neither
 * a result nor an uploaded copy is left.  m = 0 (matrix may be null) and m = 1 succeed with F = 0.
 * out (at least 4 entries, nullable) = M, F, the rounds, the kernel launches.
 * The matrix is read during the build only: the merges are kept on the host side of the handle, so a later rebuild of
 * the source matrix, a score call or a ranking leaves finished clusters valid; east_hip_reset releases them, and a build
 * that fails leaves none.  east_hip_clusters_fetch copies the merges out (each pointer nullable, F entries); the cuts run
 * on the host.  Fetch and cuts before a build are EAST_HIP_ERR_NOT_BUILT; a NaN threshold and k < 1 are
 * EAST_HIP_ERR_INVALID.  The work arrays (64 bytes a member) and the uploaded copy are buffers of the clusters' own.
 * Device time of the last build in milliseconds (events on the handle's stream around all launches and the read-backs
 * between the rounds), -1 before a build and after a failed one.
 *
 * COMPLETE and AVERAGE linkage (`-j complete|average`; csrc/linkage.h): east_hip_clusters_build_resident_linkage and
 * east_hip_clusters_build_host_linkage take the linkage and a floor (a NaN: none).  EAST_HIP_LINKAGE_SINGLE gives the bytes
 * of the two calls above, and a floor keeps the prefix w >= floor of their merges.  The sources, the refusals, the lifetime,
 * out, the fetch, the cuts and the time are as above; any other linkage value is EAST_HIP_ERR_INVALID and leaves no result.
 * Input: S as above (symmetric, the diagonal never read; only the upper triangle's bytes are read at all).  In addition an
 * off-diagonal NaN is EAST_HIP_ERR_INVALID for `complete`, and any off-diagonal value that is not finite for `average`;
 * the message names the first offending pair in row-major order as "S[a][b]", and neither a result nor an uploaded copy
 * is left.
 * State: a working copy W, which starts as the upper triangle of S mirrored (W[a][b] = W[b][a] = S[a][b]'s bytes, a < b),
 * and the set of alive clusters.  A cluster is named by its smallest member, its representative; it has a size n, 1 at the
 * start.  The source matrix is never written and stays valid byte for byte.
 * Order: the pair (a, b), a < b, of alive representatives is STRONGER than (c, d) when W[a][b] > W[c][d] (-0.0 and +0.0 are
 * equal), or the weights are equal and a < c, or the weights and a are equal and b < d -- the order above.
 * One round: every alive cluster picks its strongest pair; a pair whose two ends picked each other is RECIPROCAL; every
 * reciprocal pair (u, u'), u < u', with W[u][u'] >= floor is merged in this round and recorded as merge_a = u, merge_b = u',
 * merge_w = W[u][u'] (its bytes) and the number of the round; u stays alive with size n_u + n_u', u' dies.  The rounds end
 * when one cluster is left or when no pair of alive clusters reaches the floor (then a round merges nothing; it is not
 * counted).  A reciprocal pair below the floor stays unmerged; every pair touching its ends is below the floor as well.
 * Update: for alive representatives u < v after the round, with u' and v' their partners if they merged,
 *     c(x) = LW_v(W[x][v], W[x][v']) if v merged, else W[x][v],     for x in {u, u'}
 *     W[u][v] = W[v][u] = LW_u(c(u), c(u')) if u merged, else c(u)
 * complete: LW(x, y) = (y < x) ? y : x.
 * average:  LW_z(x, y) = clamp((n * x + n' * y) / (n + n')), n and n' the sizes of z and its partner BEFORE the round as
 * doubles, x the representative's value and y its partner's: two products, one sum, one quotient of doubles, no FMA; then
 * with lo = (y < x) ? y : x and hi = (y < x) ? x : y the result is lo if r < lo, hi if r > hi, else r.  The clamp is exact;
 * it keeps a merged cluster's similarity to anything at most the weight of the merge that made it, so later merges on a
 * branch are never stronger than earlier ones and the list by weight is a valid order of the tree.
 * Result: the F merges by weight descending (-0.0 and +0.0 equal), then round ascending, then merge_a ascending.  Without
 * a floor F = M - 1.  A floor yields exactly the prefix w >= floor of the list without one.  merge_a and merge_b are
 * members, so the cuts, the labels and the fetch are as above.
 * Guaranteed: no atomic is used; two builds give the same bytes; the result does not depend on the grid or on timing.  For
 * `average` every merge_w joining the clusters A and B lies within 4 * (|A| + |B|) * 2^-53 * max|S| of the exact mean of
 * S[a][b] over a in A and b in B.
 * out = M, F, the rounds that merged, the kernel launches: 3 a round, and at most 5 more (the symmetry check of an upload,
 * the copy, the two launches of a round that finds no pair at the floor -- it launches no update --, the ranking).  The working copy (M * M * 8 bytes, EAST_HIP_ERR_OOM where it does
 * not fit) is a buffer of the clusters' own and is released when the build ends.
 */
#define EAST_HIP_LINKAGE_SINGLE 0
#define EAST_HIP_LINKAGE_COMPLETE 1
#define EAST_HIP_LINKAGE_AVERAGE 2
int east_hip_clusters_build_resident_linkage(east_hip_handle_t h, int32_t source, int32_t linkage, double floor, int64_t *out);
int east_hip_clusters_build_host_linkage(east_hip_handle_t h, const double *matrix, int32_t m, int32_t linkage, double floor, int64_t *out);
int east_hip_clusters_build_resident(east_hip_handle_t h, int32_t source, int64_t *out);
int east_hip_clusters_build_host(east_hip_handle_t h, const double *matrix, int32_t m, int64_t *out);
int east_hip_clusters_fetch(east_hip_handle_t h, int32_t *merge_a, int32_t *merge_b, double *merge_w);
int east_hip_clusters_cut_threshold(east_hip_handle_t h, double t, int32_t *labels, int64_t *out);
int east_hip_clusters_cut_count(east_hip_handle_t h, int32_t k, int32_t *labels, int64_t *out);
double east_hip_last_clusters_ms(east_hip_handle_t h);

/*
 * Phrase extraction (`east keyphrases extract`): the repeated phrases of one to eight words of the texts the cosine term
 * index holds, counted exactly, the redundant ones removed, the rest ranked -- keyphrase candidates out of the texts
 * themselves.  Integers only: two builds, the host path of the Python package and any other exact count give the same
 * bytes.  (How: csrc/phrases.h)
 *
 * Tokens: the index's kept tokens in text order as the cosine build sees them -- the [\w']+ tokens of the prepared text
 * (1:1 upper case) with at least 3 code points; shorter tokens are invisible.  A kept token that is a stopword of the
 * index is a BREAK.  A token's POSITION is its index among the collection's kept tokens, stopwords counted, the texts in
 * the order given.
 * Phrase: n kept tokens that are no stopwords at consecutive positions of one text -- no phrase contains a break, none
 * crosses from one text into the next.  Two phrases are the same when their words are, code point for code point.
 * count(g) = the positions at which g starts (overlapping occurrences all count: AAA AAA AAA AAA AAA holds AAA AAA four
 * times); texts(g) = the texts with at least one occurrence; first(g) = the smallest starting position.
 * Candidates: with min_words <= n <= max_words (1 .. 8), min_count >= 1 and min_texts >= 1, g is a candidate when
 * count(g) >= min_count, texts(g) >= min_texts and g is CLOSED: n = max_words, or no phrase of n + 1 words that starts
 * with g or ends with g has the count of g.  (A phrase that only ever occurs inside one longer phrase is dropped in favour
 * of the longer one; extensions beyond max_words are not looked at; an extension of the same count has the same
 * occurrences shifted by at most a word, hence the same texts: it passes the same filters.)
 * Order: by score = count * n descending, then n ascending, then first ascending -- strict, the list is unique.  N > 0
 * keeps the first N, N = 0 all.
 *
 * Example.  One text `abc bcd cde abc bcd cde abc bcd cde abc bcd`, no stopwords, min_words 1, max_words 3, min_count 2,
 * min_texts 1 gives, in this order:
 *   ABC BCD CDE  (3 words, count 3, score 9, first 0)
 *   BCD CDE ABC  (3 words, count 3, score 9, first 1)
 *   CDE ABC BCD  (3 words, count 3, score 9, first 2)
 *   ABC BCD      (2 words, count 4, score 8, first 0)
 * Every single word and every other pair has an extension of its own count.
 *
 * east_hip_phrases_build: out[4] = the phrases returned, the candidates before the cut by N, the code points of the
 * returned phrases' text, the levels run (level n names the n-grams; a level without a surviving n-gram is the last).
 * EAST_HIP_ERR_NOT_BUILT "phrases: no cosine index has been built on this handle" without an index; EAST_HIP_ERR_INVALID
 * with a line that names the argument for max_words outside 1 .. 8, min_words outside 1 .. max_words, min_count < 1,
 * min_texts < 1, N < 0 and a null out.  Every refusal comes before anything is withdrawn: an earlier result stays
 * fetchable.  Zero candidates is a result.  A cosine build on the handle withdraws the result, east_hip_reset drops it;
 * score calls and east_hip_cosine_set_classes leave it alone (phrases are made of words, not of classes).
 * east_hip_phrases_fetch: per returned phrase words[r], count[r], texts[r], first[r], first_text[r] (the text of
 * first); term_ids: the phrases' words as east_hip_cosine_get_terms numbers them, ragged by the prefix sum of words;
 * text_off[returned + 1] and text: the phrases' code points, the words joined by one U+0020.  Null outputs are skipped.
 * EAST_HIP_ERR_NOT_BUILT "no phrases have been extracted on this handle" before a build.
 * east_hip_phrases_levels: domain[8] and survivors[8] -- per level the positions whose n-gram was named and the distinct
 * n-grams with count >= min_count; 0 for the levels that were not run.
 * Limits: fewer than 2^31 - 16 candidates; the returned phrases' text has fewer than 2^32 code points.  Memory: 8 bytes a
 * kept token in the index; during a build 112 bytes a kept token and 16 a candidate, buffers of the phrases' own.
 * Device time of the last build in milliseconds (the read-backs between the levels included), -1 before a build and
 * after a failed one.
 */
int east_hip_phrases_build(east_hip_handle_t h, int32_t min_words, int32_t max_words, int32_t min_count, int32_t min_texts,
                           int64_t N, int64_t *out);
int east_hip_phrases_fetch(east_hip_handle_t h, int32_t *words, int32_t *count, int32_t *texts, int32_t *first,
                           int32_t *first_text, int32_t *term_ids, int64_t *text_off, uint32_t *text);
int east_hip_phrases_levels(east_hip_handle_t h, int64_t *domain, int64_t *survivors);
double east_hip_last_phrases_ms(east_hip_handle_t h);

/*
 * Characteristic terms (`east texts terms`): what a text, or a group of texts such as a cluster, is about -- per group the
 * units of the vector space with the largest mean normalised weight, the keyword list by tf or tf-idf weight that any
 * keyphrase method is compared with.  (How: csrc/terms.h)
 *
 * A cosine index has been built.  The vector space is the one the score call uses: the terms, or the classes after
 * east_hip_cosine_set_classes.
 * Weight and norm: x_d[u] and norm_d are exactly the doubles of "Text-to-text cosine similarity" -- the weight of posting
 * (u, d) is the double the score call uses, the norm is summed in 64 slices and is 1.0 for a document without postings.
 * Grouping: group[d] in [0, G) for d < D; a null `group` means G = D and group[d] = d (the per-text question).  A group may
 * be empty.  members[g] = the number of its texts.
 * Value of a unit in a group: for a unit u with a posting in at least one text of g, q_d = x_d[u] / norm_d (one quotient);
 * s_gu = the sum of q_d over the texts of g that hold u, in ascending d, in one accumulator that starts from the first
 * addend; value_gu = s_gu / (double)members[g] (one quotient: exact for a group of one).  texts_gu = the number of addends,
 * df_u = the unit's postings in the whole collection.
 * Entries and order: the entries of g are its units with texts_gu >= min_texts (min_texts >= 1), ordered by value
 * descending, then u ascending -- strict, there is one answer.  The first n are the result, 1 <= n <= 1024 (the ranking's
 * own limit).
 * Guarantees: no floating-point atomic; the order of every sum is fixed by the collection and the grouping alone.  Two
 * builds give the same bytes, as do builds under either value of east_hip_debug_set_terms_select; a null `group` and the
 * explicit identity array give the same bytes.  Every value is > 0 (and at most 1).
 * Accuracy: all addends are positive, nothing cancels.  With p_d the postings of text d,
 *   |value_gu - exact| <= (texts_gu + (max over d in g of ceil(p_d / 64)) / 2 + 48) * 2^-53 * exact
 * (DESIGN.md 19 derives it: texts_gu roundings of the sum and its quotient; the ceil(p_d / 64) + 62 roundings of a norm's
 * radicand, halved by the root; 6 for the weight, ln at one ulp included, 13 for a square -- 47 in all beside the two
 * variable terms.  It is less than half of what section 15's accounting, a whole ulp a rounding, would give.)
 * Lifetime (the text-similarity matrix's rule): the result is withdrawn by east_hip_reset, by every
 * east_hip_cosine_build_texts* call and by every east_hip_cosine_set_classes call; score calls, rankings, matrices and
 * clusters leave it alone.  Every argument and index check comes before anything is withdrawn: a refused call leaves the
 * earlier result fetchable.  The result lives in buffers of its own.
 *
 * east_hip_terms_build: weighting 0 tf, 1 tf-idf.  out (nullable, at least 10 entries): D; G; the units; the postings; the
 * entries, that is, the distinct (group, unit) pairs; the entries that pass min_texts; the entries that reach the final
 * sort; the radix passes run; the kernel launches; 1 when the grouping sort was skipped (a null `group`: the postings are
 * in key order as they lie).
 * east_hip_terms_fetch: members[G], count[G] = min(n, the group's entries), and unit, value, texts, df as [G * n], each
 * nullable; places behind count[g] hold -1 and NaN.
 * east_hip_terms_fetch_vectors: every entry before min_texts and the cut, in (group, unit) order: offsets[G + 1], then
 * unit, value and texts_gu per entry (out[4] of the build sizes them); each nullable.
 * east_hip_debug_set_terms_select: 0 (the default) a pre-selection in front of the final sort -- per group only the
 * entries at or above the 12-bit digest of the value below which the n-th cannot lie are sorted; 1 none, every entry is
 * sorted.  The result does not depend on it.
 * Errors: EAST_HIP_ERR_NOT_BUILT "no cosine index has been built on this handle" without an index, "no characteristic terms
 * have been built on this handle" for the fetches without a result; EAST_HIP_ERR_INVALID for a null handle, an unknown
 * weighting, n outside 1 .. 1024, min_texts < 1, n_groups < 1 -- or not D with a null `group` -- and a group[d] outside
 * [0, G), with the text's index and the value in the message, checked on the host before anything is queued;
 * EAST_HIP_ERR_OOM "characteristic terms: ... of D texts in G groups needs N bytes, which the device does not have".
 * Memory: during a build 96 bytes a posting; 20 bytes an entry and 20 bytes a place of the result stay.
 * Device time of the last build in milliseconds (its read-backs included), -1 before a build and after a failed one.
 */
int east_hip_terms_build(east_hip_handle_t h, int32_t weighting, const int32_t *group, int32_t n_groups, int32_t n,
                         int32_t min_texts, int64_t *out);
int east_hip_terms_fetch(east_hip_handle_t h, int32_t *members, int32_t *count, int32_t *unit, double *value,
                         int32_t *texts, int32_t *df);
int east_hip_terms_fetch_vectors(east_hip_handle_t h, int64_t *offsets, int32_t *unit, double *value, int32_t *texts);
double east_hip_last_terms_ms(east_hip_handle_t h);
int east_hip_debug_set_terms_select(int mode);

/*
 * Shingle overlap (`east texts overlap`): which texts CONTAIN THE SAME WORDING -- near-duplicates, a passage lifted from
 * another text, one text quoted inside a longer one -- after Broder: a text is the set of its w-word shingles.  Integers
 * and one division an entry: the device (either route), the host path of the Python package and any other exact count give
 * the same bytes.  (How: csrc/overlap.h)
 *
 * A cosine index has been built.  Tokens, words, breaks and positions are those of "Phrase extraction".
 * Shingle: with 1 <= w <= 8 (the phrases' longest), a shingle of w words is a phrase of exactly w words in that contract's
 * sense: w kept tokens that are no stopwords at consecutive positions of one text.
 * Sets: S_a = the distinct shingles with an occurrence in text a -- repeats inside a text count once; a text of fewer than w
 * consecutive words has S_a empty.  n_a = |S_a|, I_ab = |S_a n S_b|.
 * EAST_HIP_OVERLAP_SYMMETRIC (resemblance):   M[a][b] = (double)I_ab / (double)(n_a + n_b - I_ab), +0.0 where that is 0.
 * EAST_HIP_OVERLAP_DIRECTED (containment of a in b): M[a][b] = (double)I_ab / (double)n_a, +0.0 where n_a = 0.
 * Arithmetic: every entry is ONE IEEE division of integers below 2^53 -- the correctly rounded quotient, the same bytes on
 * every path; there is no tolerance anywhere.
 * The diagonal is NaN (nobody lists itself); self[a] = the diagonal before the NaN: 1.0, or +0.0 for an empty set;
 * shingles[a] = n_a.
 *
 * Example.  w = 2, text A = `abc bcd cde def`, text B = `bcd cde def efg`: S_A = {ABC BCD, BCD CDE, CDE DEF}, S_B = {BCD CDE,
 * CDE DEF, DEF EFG}, I = 2; resemblance 2 / 4 = 0.5, containment of A in B 2 / 3.
 *
 * east_hip_overlap_build: out (at least 14 entries): D; the kept tokens; the shingle positions (where w words of one text
 * start); the distinct shingles of the collection; the SHARED shingles, those held by two or more texts -- the units of the
 * product; the postings of the shared shingles (one per shingle and text); the segments of the unit range; the launches of
 * the product and the quotients; the route taken (1 or 2); the naming levels run; the 64 x 64 tile pairs; w; the
 * device time in microseconds up to the operands in text order (naming, postings, sizes, sort) and from there on (product
 * and quotients).
 * east_hip_overlap_fetch: matrix[D * D], self[D], shingles[D], each nullable.
 * Ranking and clusters: east_hip_top_build_resident and both east_hip_clusters_build_resident* take the source
 * EAST_HIP_GRAPH_SOURCE_OVERLAP = the matrix the last overlap build left (EAST_HIP_ERR_NOT_BUILT "...: no overlap matrix has
 * been built on this handle" where there is none); the clusters refuse a directed one with EAST_HIP_ERR_INVALID "clusters:
 * the overlap matrix is directed (build it with EAST_HIP_OVERLAP_SYMMETRIC)".
 * Errors: EAST_HIP_ERR_NOT_BUILT "overlap: no cosine index has been built on this handle" for a build without an index, "no
 * overlap matrix has been built on this handle" for a fetch without a matrix; EAST_HIP_ERR_INVALID, in lines that start
 * with "overlap: ", for w outside 1 .. 8, an unknown orientation, a null out, an index without a text, and a collection in
 * which a text may have 2^31 or more shingle positions; EAST_HIP_ERR_OOM "overlap: ... of D texts needs N bytes, which the
 * device does not have".  The index check and every argument check come before anything is withdrawn: a refused call
 * leaves the earlier matrix fetchable.
 * Lifetime: a cosine build on the handle withdraws the matrix, east_hip_reset drops it; score calls and
 * east_hip_cosine_set_classes leave it alone (shingles are made of words, whatever the vector space).  The buffers are the
 * overlap's own: a build does not disturb the extracted phrases or any other result.
 * east_hip_debug_set_overlap_route: 0 the default, 1 the integer matrix-core kernel (v_mfma_i32_16x16x64_i8 on 0/1 bytes),
 * 2 the f64 tile kernel of the text-to-text cosine on weights of 1.0 (exact below 2^53); anything else is
 * EAST_HIP_ERR_INVALID.  east_hip_debug_set_overlap_batch: the segments of the unit range a launch of the tile kernel
 * takes, 0 or less the default.  The result depends on neither.
 * Memory: during a build 128 bytes a kept token, 16 bytes a posting of a shared shingle (24 on route 2), 16 KiB a tile pair
 * and a batch's partial tiles (256 MiB at most, or one segment's); the matrix stays.
 * Device time of the last build in milliseconds (its read-backs included), -1 before a build and after a failed one.
 */
#define EAST_HIP_OVERLAP_DIRECTED 0
#define EAST_HIP_OVERLAP_SYMMETRIC 1
#define EAST_HIP_GRAPH_SOURCE_OVERLAP (6)       /* (in parentheses: tests/test_phrases_host.py reads a bare 6 or 7 as a source the phrases added) */
int east_hip_overlap_build(east_hip_handle_t h, int32_t words, int32_t orientation, int64_t *out);
int east_hip_overlap_fetch(east_hip_handle_t h, double *matrix, double *self, int32_t *shingles);
double east_hip_last_overlap_ms(east_hip_handle_t h);
int east_hip_debug_set_overlap_route(int route);      /* 0: the default; 1: the integer kernel; 2: the f64 tile kernel on unit weights */
int east_hip_debug_set_overlap_batch(int64_t segments);

/*
 * Shared passages (`east texts passages`): WHICH WORDS two texts share -- after "Shingle overlap" has said that they share
 * wording and how much.  Integers only: the device under either route, the host path of the Python package and any other
 * exact count give the same numbers; there is no tolerance anywhere.  (How: csrc/passages.h)
 *
 * A cosine index has been built.  Tokens, positions, breaks, shingles and S_b are those of "Phrase extraction" and
 * "Shingle overlap"; the width is w = `words`, 1 .. 8.  For an ordered pair of texts (a, b), a != b:
 * A SHARED START of a in b is a shingle position j of a whose shingle is in S_b.
 * A PASSAGE of a in b is a maximal run of shared starts at consecutive positions j, j + 1, .., j + m - 1: neither j - 1
 * nor j + m is a shared start of a in b.  start = j, a collection position as `first` of the phrases is; words = m + w - 1,
 * it covers the tokens [j, j + m + w - 1): every w consecutive words of a passage occur in b.  A passage holds no break and
 * lies inside a -- by the shingle definition, not by an extra rule.  Two passages of one pair never share a start; their
 * token ranges may overlap by up to w - 2 tokens.
 * at = the smallest position in b at which the passage's first shingle starts.
 * Per pair: starts = the number of shared starts; covered = |the union of [j, j + w) over the shared starts j|, the words of
 * a that lie inside wording found in b; found = the number of passages with words >= min_words.
 * Returned per pair are the passages with words >= min_words (w <= min_words), ordered by words descending, then start
 * ascending -- a strict order; the first per_pair of them are kept, 0 keeps all.  Pairs come back in the order given;
 * duplicate pairs are allowed and give the same result twice.
 * The number of distinct shingles at the shared starts of (a, b) is I_ab of "Shingle overlap".
 *
 * Example.  w = 2, no stopwords, text 0 = `abc bcd cde def xyz bcd cde` (positions 0 .. 6), text 1 = `qqq bcd cde def rrr`
 * (positions 7 .. 11).  Pair (0, 1): shared starts 1, 2, 5; passages (start, words, at) = (1, 3, 8) BCD CDE DEF, then
 * (5, 2, 8) BCD CDE; starts 3, covered 5.  Pair (1, 0): shared starts 8, 9; passage (8, 3, 1); starts 2, covered 3.
 *
 * east_hip_passages_build: pair_a[n_pairs], pair_b[n_pairs] = the texts of every pair.  out (at least 12 entries): D; the
 * kept tokens; the pairs; the shared shingles U (the units); their postings P; the 64-bit words of all pairs' rows (a row =
 * one bit a position of a, ceil(len_a / 64) words); the shared starts over all pairs; the passages before the filter; the
 * passages returned; the launches of this section's own kernels; the route taken (1 or 2); the naming levels run.
 * east_hip_passages_fetch: pair_off[n_pairs + 1] = the prefix sum of the returned passages; starts, covered, found
 * [n_pairs]; start, words, at [pair_off[n_pairs]], pair by pair in the contract's order; text_start[D + 1] = the first
 * position of every text (and the number of positions behind the last), so a caller can make positions text-relative.
 * Null outputs are skipped.
 * east_hip_passages_phases: ms[3] = the device time of the last build up to the rows' offsets (names, postings, rows), of
 * the match kernel (with the words' pairs), and from there on (runs, order, cut); they add up to east_hip_last_passages_ms.
 * Errors: EAST_HIP_ERR_NOT_BUILT "passages: no cosine index has been built on this handle" for a build without an index,
 * "no passages have been built on this handle" for a fetch without a result; EAST_HIP_ERR_INVALID, in lines that start
 * with "passages: ", for words outside 1 .. 8, min_words < words, per_pair < 0, n_pairs < 0 or above 2^24, null pair_a or
 * pair_b with n_pairs > 0, a null out, an index without a text, a pair with a == b or a text outside 0 .. D - 1 (named by
 * its index in the list) -- all of these before anything is withdrawn: a refused call leaves the earlier result fetchable
 * -- and for rows of 2^25 bit words or more; EAST_HIP_ERR_OOM "passages: ... of N pairs of D texts needs B bytes, which
 * the device does not have".  n_pairs == 0, no shared shingle and a level that ends the naming early are results.
 * Lifetime: a cosine build on the handle withdraws the result, east_hip_reset drops it; score calls and
 * east_hip_cosine_set_classes leave it alone.  The buffers are the passages' own: a build disturbs neither the overlap
 * matrix nor the extracted phrases.  The consumer offers no matrix: there is no graph source for it.
 * east_hip_debug_set_passages_route: how "does b hold this shingle" is answered -- 0 the default, 1 a search of b in the
 * shingle's own ascending list of texts, 2 a search of the shingle in b's ascending list of shingles (the operands of the
 * overlap); anything else is EAST_HIP_ERR_INVALID.  The result does not depend on it.
 * Memory: during a build 128 bytes a kept token; 4 bytes a position and 12 a posting of a shared shingle (28 more on route
 * 2), 36 bytes a pair, 24 bytes a bit word, 16 bytes a passage before the filter, 24 one behind it, 12 one returned.
 * Device time of the last build in milliseconds (its read-backs included), -1 before a build and after a failed one.
 */
int east_hip_passages_build(east_hip_handle_t h, int32_t words, int32_t min_words, int32_t per_pair,
                            const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int64_t *out);
int east_hip_passages_fetch(east_hip_handle_t h, int64_t *pair_off, int32_t *starts, int32_t *covered, int32_t *found,
                            int32_t *start, int32_t *words, int32_t *at, int32_t *text_start);
int east_hip_passages_phases(east_hip_handle_t h, double *ms);
double east_hip_last_passages_ms(east_hip_handle_t h);
int east_hip_debug_set_passages_route(int route);     /* 0: the default; 1: b in the shingle's texts; 2: the shingle in b's shingles */

/*
 * Several devices in one process ("single-process/8-device fits the one-process CLI best").
 * Every document is an independent AST (east/relevance.py:41-46) and every (keyphrase, document) score is independent
 * (east/applications.py:43-52): a GROUP shards a collection at document granularity -- contiguous blocks of documents
 * balanced by size, shard s on devices[s], one handle per shard -- and drives the shards with host threads of its own
 * (ctypes drops the GIL around the call).  No collective on the build path.  east_hip_score_table_multi lets every shard
 * score its documents and assembles the K x D_local blocks with ONE all-gather: RCCL (librccl.so loaded at run time,
 * ncclCommInitAll + a grouped ncclAllGather over xGMI, blocks padded to the widest shard) where every shard has a device
 * of its own, device-to-device copies to the first shard's device otherwise (logical shards sharing a device, no
 * librccl.so; EAST_HIP_GROUP_GATHER=copy|rccl forces either); the K x D table then goes to the host once.  No torch, no
 * process spawn.  `devices` may name a device several times (logical shards: the single-GPU tests).
 *
 *   east_hip_group_build           as east_hip_build (host symbols; `encoding` = EAST_HIP_SYMBOLS_*), sharded by symbols
 *   east_hip_group_build_texts_v   as east_hip_build_texts_v (raw texts, device text preparation), sharded by bytes
 *   east_hip_group_shards          first_doc[n_shards + 1]: shard s holds the documents [first_doc[s], first_doc[s+1]);
 *                                  returns n_shards
 *   east_hip_group_handle          shard s's handle (owned by the group) for east_hip_get_tables & co.; document d of the
 *                                  collection is document d - first_doc[s] of its shard
 *   east_hip_score_table_multi     out: K x D doubles, row-major, D = all documents in their original order
 *   east_hip_group_info            [0] build, [1] score (slowest shard), [2] all-gather + copy to the host: wall ms of the
 *                                  last calls; [3] 1 = RCCL all-gather, 2 = copies; [4] shards
 * A group is not thread-safe (its shards run on threads of its own).
 */
typedef struct east_hip_group *east_hip_group_t;
int east_hip_group_create(const int32_t *devices, int32_t n_shards, east_hip_group_t *out);
void east_hip_group_destroy(east_hip_group_t g);
int east_hip_group_build(east_hip_group_t g, const uint32_t *symbols, int64_t n_total, const int64_t *doc_offsets,
                         const int32_t *n_strings, int32_t n_docs, int32_t encoding);
int east_hip_group_build_texts_v(east_hip_group_t g, const uint8_t *const *texts, const int64_t *lengths, int32_t n_docs,
                                 const uint8_t *cp_class, const uint32_t *cp_upper, const uint32_t *word_hi,
                                 const uint32_t *digit_hi, const uint32_t *hi_upper_from, const uint32_t *hi_upper_to,
                                 int32_t n_hi_upper);
int east_hip_group_shards(east_hip_group_t g, int32_t *first_doc);
east_hip_handle_t east_hip_group_handle(east_hip_group_t g, int32_t shard);
int east_hip_score_table_multi(east_hip_group_t g, const uint32_t *q_symbols, const int64_t *q_offsets,
                               int32_t n_keyphrases, int normalized, double *out);
int east_hip_group_info(east_hip_group_t g, double *out, int32_t cap);
/* Host only (needs no device): the group's sharding rule -- contiguous blocks balanced by size; first_doc[n_shards + 1]. */
int east_hip_debug_shard_documents(const int64_t *sizes, int32_t n_docs, int32_t n_shards, int32_t *first_doc);

/*
 * Host only (needs no device): the keyphrase table as text -- east/formatting.py:14-39, table2xml / table2csv, byte for byte
 * ('%s' names, '%.3f' scores) -- for tables of millions of scores, where a Python loop over the scores takes seconds
 * (BASELINE configs[2]: 2.56 M).  table: K x D doubles, row-major; kp_order / text_order: the output order (the sorted
 * names) as indices into the table's rows / columns; names NUL-terminated UTF-8 indexed like the table (CSV: already
 * quoted).  Returns the length written, minus the bytes needed when cap is too small, or EAST_HIP_ERR_INVALID.
 */
int64_t east_hip_format_table_xml(const double *table, int32_t K, int32_t D, const int32_t *kp_order, const int32_t *text_order,
                                  const char *const *kp_names, const char *const *text_names, char *out, int64_t cap);
int64_t east_hip_format_table_csv(const double *table, int32_t K, int32_t D, const int32_t *kp_order, const int32_t *text_order,
                                  const char *const *kp_quoted, const char *const *text_quoted, char *out, int64_t cap);

/* Block until everything queued on the handle's stream has finished. */
int east_hip_synchronize(east_hip_handle_t h);
/* The handle's hipStream_t (as void*) so callers can record events on it. */
void *east_hip_stream(east_hip_handle_t h);

/*
 * Build facts for reports: fills up to `cap` int64 values and returns how many
 * exist: [0] n_total, [1] n_docs, [2] total strings, [3] text alphabet size,
 * [4] bits per symbol at level 0, [5] DC3 recursion levels, [6] arena bytes,
 * [7] arena high-water bytes, [8] radix passes executed, [9] radix elements
 * moved (sum over passes), [10] bytes of one radix element (key+value) at the
 * widest level, [11] passes and [12] elements with 32-bit keys, [13] passes and
 * [14] elements with 64-bit keys, [15] DC3 levels whose few tied names were
 * ordered directly instead of recursing, [16] suffixes merged (sum over levels), [17] rounds of
 * tie refinement by further windows, [18] 1 if the all-suffix window sort produced the suffix array
 * (no DC3 level ran; [5] is 0 then), [19] elements the refinement rounds ordered inside a workgroup's LDS,
 * [20] 1 when the last radix digit and the placement ran as one pass in LDS (the fused finish), [21] suffixes the
 * first placement left in large tie groups, [22] of how many, [23] 1 when the first-level keys held variable-length
 * (order-preserving) code words instead of fixed-width symbol fields (csrc/ht_code.h), [24] 1 when the first-level sort
 * kept every document inside its own range of ranks (the segmented sort, csrc/radix_sort.h: RsSeg), [25] 1 when
 * east_hip_build's host symbols went up as 16-bit words through the pinned ring (half the bytes over the link; reference
 * encoding, 4 Mi symbols or more), 2 when they went up as bytes (text below 0xFF),
 * [26] refinement rounds run inside one persistent launch (csrc/persist_rounds.h; they count in [17] too),
 * [27] 1 when the first radix pass's histogram was counted by the remap pass of a speculative build
 * (csrc/radix_sort.h: presence_remap_hist_kernel) and the sort took it,
 * [28] the block order of the annotation pass's ann_wide_kernel: 1 grouped, 2 slice-major over the whole grid (chosen
 * from the count of the build before, east_hip_debug_set_ann_wide_order), [29] 1 when the build queued the score
 * walk's k-gram tables behind its flags read-back (keyphrases resident, marks written; east_hip_debug_set_eager_kgram),
 * 2 when it did and the flags then said the marks were incomplete: that work is discarded, the score side builds the tables,
 * [30] the ranks ann_wide_kernel decided in the last build (what the next build's order is chosen from; -1: none yet).
 */
int east_hip_build_info(east_hip_handle_t h, int64_t *out, int32_t cap);

/* Device-time of the last build / score call in milliseconds (HIP events on
 * the handle's stream around the whole call), or a negative error code. */
double east_hip_last_build_ms(east_hip_handle_t h);
double east_hip_last_score_ms(east_hip_handle_t h);

/*
 * Per-kernel timing for bench.py's roofline leg: when enabled, every kernel the
 * handle launches is bracketed by HIP events on the handle's stream.  The
 * report is text, one line per kernel: "name<TAB>launches<TAB>total_ms".
 * Enabling resets the accumulated sums.  Returns the report length.
 */
int east_hip_profile_enable(east_hip_handle_t h, int on);
/* Restrict the bracketing to the launches of one kernel (the name as it appears in the report; NULL or "" = every
 * kernel again).  Two events per launch cost the stream time -- about 10 % of a 2 ms build with every kernel
 * bracketed --, so a timed region brackets only the kernel it reports on. */
int east_hip_profile_only(east_hip_handle_t h, const char *kernel);
int64_t east_hip_profile_report(east_hip_handle_t h, char *buf, int64_t cap);

/*
 * Kernel-level entry points used by the parity tests (host buffers in/out).
 * They exercise exactly the kernels the build uses.
 *   radix sort: stable LSD sort of (key, value) pairs on key bits [0, bits)
 *   scan:       exclusive prefix sum of uint32
 *   suffix_array: DC3 over a dense alphabet: symbols in [1, sigma], n >= 1
 */
int east_hip_debug_radix_sort_u64(int device, uint64_t *keys, uint32_t *vals, int64_t n, int bits);
int east_hip_debug_radix_sort_u32(int device, uint32_t *keys, uint32_t *vals, int64_t n, int bits);
int east_hip_debug_exclusive_scan(int device, const uint32_t *in, uint32_t *out, int64_t n);
int east_hip_debug_suffix_array(int device, const uint32_t *symbols, int64_t n, uint32_t sigma,
                                int32_t *sa_out, int32_t *levels_out);
/* Kernel-level test of the DC3 suffix sort (csrc/dc3.h: dc3_suffix_array) in the three forms a build calls it in.
 * form 0: text is n u32 symbols in [1, sigma], term_first 0 -- every recursion level.  form 1: n u32 codes, text in
 * [1, term_first), the terminators ascending from term_first on (as east_hip_debug_lcp takes them), 2 <= term_first < 2^21
 * -- level 0 of wide-alphabet text.  form 2: n bytes, text codes 1 .. term_first - 1 <= 254, 0xFF for every terminator --
 * level 0 on the byte stream (the window keys in sample mode, the 16-byte records, the merge that also writes the LCP
 * table).  Forms 1 and 2 end in a terminator and take sigma = term_first - 1 + the number of terminators, as a build does.
 * rank_bucket_bytes: the threshold of the bucketed rank scatter for this call alone (-1: the process-wide knob's value);
 * lean 1: as a build short of memory (no refinement rounds at level 0 of form 2); want_lcp 1 (form 2 only): the merge also
 * writes the LCP table, under the budget deep_per_slot of deep comparisons per slot (-1 = none); pad_fill: the byte the
 * whole scope holds before the run, behind the text's zero pad (3 words / 16 bytes) and, in form 2, in the u32 stream that
 * is not read.  Anything else -- a symbol, code or byte out of range, a zero byte, terminators that do not ascend, a text
 * of form 1 or 2 that does not end in one, a sigma that is not the sum above, want_lcp with another form -- is
 * EAST_HIP_ERR_INVALID before a launch; the outputs are then untouched.  sa_out (and lcp_out, which may be NULL without
 * want_lcp): n words + EAST_HIP_DEBUG_GUARD words, which the device held as 0xEE before the run; lcp_out holds the table as
 * the merge leaves it (LCP_PARTIAL_BIT | k where a comparison was cut, no padding behind n).  capped_out: the flag word.
 * info_out[6]: the levels run (the return value), then levels_resolved, refine_rounds, radix_passes_u32, radix_passes_u64
 * and merge_elems of the call's statistics.  geometry_out[7]: MERGE_TILE, RESOLVE_MAX_GROUP, RESOLVE_MAX_LEN, LCP_SOFT_CAP,
 * LCP_DIRECT_CAP, LCP_BUDGET_SLOTS as compiled, EAST_HIP_DEBUG_GUARD. */
int east_hip_debug_suffix_array_ex(int device, int form, const void *text, int64_t n, uint32_t sigma, uint32_t term_first,
                                   int64_t rank_bucket_bytes, int lean, int want_lcp, int32_t deep_per_slot, int pad_fill,
                                   uint32_t *sa_out, uint32_t *lcp_out, uint32_t *capped_out, int64_t *info_out,
                                   uint32_t *geometry_out);
/* Test knob: rank arrays larger than this many bytes are filled through the bucketed scatter
 * (default 192 MiB, the Infinity Cache); 0 forces the bucketed path on every input. */
int east_hip_debug_set_rank_bucket_bytes(int64_t bytes);
/* Test knob: 0 skips the all-suffix window sort, so that every build goes through DC3 (the
 * fallback for repetitive inputs); 1 (default) restores it; 2 = window sort on, but built as if
 * the device were short of memory for the tie-refinement rounds ("lean"); 3 = window sort on with
 * 64-bit window keys even where 32 bits suffice (the code path of large inputs, on small ones);
 * 4 / 5 = as 1 / 3 with every radix pass global and the separate placement pass (the fused finish,
 * csrc/window_sort.h: lvl0_finish_kernel, switched off); 6 = as 1 with the fused finish whatever the build's
 * plan says (skewed text, whose large buckets it hands to the refinement rounds); 7 = as 1 with first-level keys of
 * variable-length code words wherever a code can be made (csrc/ht_code.h), 9 = the same without the fused finish,
 * 8 = as 1 without such keys.
 * The test knobs of this section are process-wide defaults (they exist to steer a test run through every code path); a
 * call takes the values that hold when it starts (csrc/common.h: Knobs). */
int east_hip_debug_set_window_sort(int enabled);
/* Test knob: the first-level sort of a shard of several documents keeps every document in its own range pass by pass
 * (csrc/radix_sort.h: RsSeg -- no document number in the keys) -- -1 (default): five documents or more of 32 768 symbols or more on average,
 * 0: never, 1: wherever it can be done (2 .. 65 535 documents of any size). */
int east_hip_debug_set_segmented_sort(int mode);
/* Test knob: 0 = the tie-refinement rounds sort every group with the global radix sort; 1 (default) = groups
 * that fit a workgroup's LDS are sorted there (csrc/lds_group_sort.h), the global sort takes the rest. */
int east_hip_debug_set_persist(int force_large, int max_workgroups);   /* the persistent rounds: (1, n) = the large form (several tiles per workgroup, state in global memory) on every domain, at most n workgroups (0: what the device holds); (0, 0) = default */
int east_hip_debug_set_lds_rounds(int enabled);   /* 0 / 1 (default: the in-LDS rounds also classify the next domain; a domain that fits the chip is finished by one persistent launch) / 2 (in-LDS rounds + the stand-alone classification pass, launch by launch) / 3 (as 1 without the persistent launch) */
/* Test knob: 0 = every build waits for the device's answers (alphabet size, tie groups) as a handle's
 * first build does; 1 (default) = later builds on a handle are queued without waiting, on the strength
 * of what the build before found, and checked by the one read-back at their end; 2 = as 1, but
 * the first radix pass's histogram is counted by a launch of its own, not by the remap pass. */
int east_hip_debug_set_speculation(int enabled);
/* Test knob: 1 (default) = a build on a handle with resident keyphrases (east_hip_set_keyphrases, same number of
 * documents) queues the launches that finish the k-gram tables it marked behind its flags read-back, so that they run
 * while the host reads the flags and returns; the handle counts them as done only once the flags say the build stood.
 * 0 = the first score call behind the build queues them, as every other kind of k-gram table.  Same tables either way. */
int east_hip_debug_set_eager_kgram(int enabled);
/* Test knob: the block order of ann_wide_kernel (csrc/tables.h) -- 0 (default) = from the number of ranks the build
 * before on the handle listed: slice-major over the whole grid where the list is short, else (and on a first build,
 * after east_hip_reset, in the second annotation of a capped build) grouped; 1 = grouped; 2 = whole-grid, also in
 * east_hip_debug_annotate.  Both orders give the same table.  Other values: EAST_HIP_ERR_INVALID. */
int east_hip_debug_set_ann_wide_order(int order);
/* Kernel-level test of the remap pass that counts the first radix histogram (csrc/radix_sort.h:
 * presence_remap_hist_kernel): n host symbols go through code_map (2 560 words: code point -> byte) (a) in that kernel and
 * (b) through remap_bytes_kernel + presence_kernel + radix_hist_kernel on window keys of key_bytes (4 / 8) x 8 bits --
 * w symbols of b bits + spare bits, terminators as term_first, digit (key >> shift) & mask.  Every output holds (a)'s
 * result followed by (b)'s: s8 2 x (n + 16) bytes, present 2 x 80 words, hist 2 x 256 x tiles (tiles = ceil(n / 4096)),
 * group_sum 2 x 256 x ceil(tiles / 8), digit_total 2 x 2 048. */
int east_hip_debug_first_pass_hist(int device, const uint32_t *symbols, int64_t n, const uint32_t *code_map, int key_bytes,
                                   int w, int b, int spare, uint32_t term_first, int shift, uint32_t mask, uint8_t *s8,
                                   uint32_t *present, uint32_t *hist, uint32_t *group_sum, uint32_t *digit_total);
/* Kernel-level test of the annotation pass (csrc/build.h: annotate -- ann_stream_kernel, the upper levels of the min
 * pyramid, ann_wide_kernel): the pass the build runs, on the caller's table lcp[n] of n_docs documents (doc_off: n_docs + 1
 * rank offsets, n_strings per document as in east_hip_build).  The table need not be an LCP table.  ann_out[n]: the
 * annotation table; geometry_out[3]: the tile, the halo and the near reach the library was compiled with (csrc/tables.h:
 * ANN_TILE, ANN_HALO, ANN_NEAR); listed_out: the number of ranks that went through ann_wide_kernel. */
int east_hip_debug_annotate(int device, const uint32_t *lcp, int64_t n, const int64_t *doc_off, int32_t n_docs,
                            const int32_t *n_strings, uint32_t *ann_out, uint32_t *geometry_out, uint32_t *listed_out);
/* Kernel-level test of the child tables and the lcp-interval lefts (csrc/build.h: child_tables -- child_stream_kernel,
 * child_wide_kernel --, interval_lefts -- interval_left_kernel), run behind annotate() on the caller's table as the calls
 * above take it.  Unlike there the table must hold 0 at every document's first rank (the kernels' searches end at that
 * zero) and no value above 0x7FFFFFEF; anything else is EAST_HIP_ERR_INVALID before a launch.  up_out / down_out /
 * next_out[n]: the raw device tables, positions local to the document, 0 = none; left_out[n]: the lefts of every
 * document, local, 0xFFFFFFFF = none; geometry_out[4]: CH_TILE, CH_HALO, CH_NEAR, CH_LOCAL of csrc/tables.h; listed_out:
 * the number of ranks that went through child_wide_kernel. */
int east_hip_debug_child_tables(int device, const uint32_t *lcp, int64_t n, const int64_t *doc_off, int32_t n_docs,
                                const int32_t *n_strings, uint32_t *up_out, uint32_t *down_out, uint32_t *next_out,
                                uint32_t *left_out, uint32_t *geometry_out, uint32_t *listed_out);
/* Kernel-level test of the two passes that make the LCP table (csrc/build.h: direct_lcp -- lcp8_kernel / lcp_kernel,
 * lcp_doc_starts_kernel --, finish_capped_lcp -- inverse_sa_kernel, lcp_phi_classify / compare / long_kernel, the anchors'
 * scan, lcp_phi_anchors_kernel, lcp_phi_fill_kernel), on the caller's text and per-document suffix array.  width 1: text
 * is the byte stream as a build holds it (text codes from 1, 0xFF = a terminator); width 4: dense u32 codes, text below
 * term_first, the terminators ascending from term_first on.  sa[n]: positions in the shard, every document's ranks a
 * permutation of its own range; doc_off / n_docs / n_strings as in east_hip_build.  deep_per_slot: the budget of deep
 * comparisons per slot, -1 = none.  table_in == NULL (mode A): the direct pass runs; else (mode B) table_in[n] stands in
 * its place, with LCP_PARTIAL_BIT | k (0x80000000 | k, the first k symbols known to agree) at any ranks but a document's
 * first.  The finishing pass runs where `capped` is raised, as in a build.  pad_fill: the byte that everything behind the
 * stream's zero pad (16 bytes / 3 words) holds before the run.  Anything wrong with an argument -- a suffix array that
 * is no permutation, a document without a last terminator, a byte or code out of range, n_strings that is not the number
 * of terminators, in mode B an unfinished entry at a document's first rank or k > n - max(sa[r - 1], sa[r]) -- is
 * EAST_HIP_ERR_INVALID before a launch.  direct_out / final_out: ceil(n / 16) * 16 words, the table behind the direct
 * and behind the finishing pass; capped_out: the flag word; counters_out[2]: positions listed as irreducible, positions
 * handed to the long kernel; ann_out[n]: the annotation; geometry_out[6]: LCP_SOFT_CAP, LCP_DIRECT_CAP, LCP_BUDGET_SLOTS,
 * PHI_WAVE_STEPS * WAVE, PHI_LONG_THREADS, PYR_FAN as compiled. */
int east_hip_debug_lcp(int device, int width, const void *text, int64_t n, uint32_t term_first, const uint32_t *sa,
                       const int64_t *doc_off, int32_t n_docs, const int32_t *n_strings, int32_t deep_per_slot,
                       const uint32_t *table_in, int pad_fill, uint32_t *direct_out, uint32_t *capped_out, uint32_t *final_out,
                       uint32_t *counters_out, uint32_t *ann_out, uint32_t *geometry_out);
/*
 * Kernel-level tests of the radix sort, its spine and the scans in every form the library uses them in (csrc/radix_sort.h,
 * csrc/scan.h).  Every output buffer takes its elements AND a guard of EAST_HIP_DEBUG_GUARD elements behind them: on the
 * device both are filled with 0xEE before the run and both come back, so that an element the kernels left out and a
 * write behind the end show.  Arguments are checked before any device work (EAST_HIP_ERR_INVALID; the outputs are then
 * untouched).  geometry_out[9]: RS_TILE, RS_GROUP, RS_TOTAL_SHARDS, RS_SPINE_DOC_GROUPS, RS_SPINE_PARTS * RS_SPINE_HELD,
 * SCAN_TILE, SCAN_RAW_TILES as the library was compiled, EAST_HIP_DEBUG_GUARD, RS_SPINE_PARTS.
 *
 * radix_sort_ex: radix_sort_pairs<u32 | u64> (key_bytes 4 | 8) with exactly these arguments -- a stable sort on the key
 * bits [begin_bit, bits), the histogram passes below check_from_bit without the test for a wavefront on one bin.  keys /
 * vals: n pairs in, n + guard elements out.  n_docs > 0: the segmented sort, every document [doc_off[d], doc_off[d + 1])
 * sorted in its own range (doc_off: n_docs + 1 strictly increasing offsets from 0 to n, n_docs <= 65 535); the segments'
 * tables are made by the function the build calls (rs_seg_make).
 *
 * radix_spine: the spine step of one pass (radix_spine: radix_spine_kernel, radix_spine_docs_kernel) on the caller's
 * group sums (n_groups rows of 256) and digit totals (one segment: RS_TOTAL_SHARDS rows of 256; segmented: per document
 * RS_TOTAL_SHARDS rows below RS_TOTAL_SHARDS documents, one row from there on).  Segmented, doc_off gives the documents'
 * pairs as above and n_groups must be the number of their groups (ceil(ceil(pairs / RS_TILE) / RS_GROUP) each).
 * group_prefix_out: n_groups x 256 + guard words; next_total_out (the other totals buffer, which the step clears): as
 * many words as digit_total + guard.
 *
 * scan_ex: device_scan / device_scan_with_total over n words in the form EAST_HIP_SCAN_*; out: n words (n + 1 with the
 * total) + guard.  run_heads: the heads of the runs of n sorted keys above bit `shift` (RunHeadIn<u64>) -- their
 * inclusive scan (n + guard words) and their number as device_scan_count returns it.  scan_pair_bounded:
 * device_scan_pair_bounded of a and b with n_dev_value in a word of the device; out_a / out_b: n + guard words, defined
 * on [0, min(n, n_dev_value + extra)).  ascending_offsets: ascending_offsets_kernel over n sorted words; off_out:
 * n_values + 1 + guard words.
 */
#define EAST_HIP_DEBUG_GUARD 4096
#define EAST_HIP_SCAN_EXCLUSIVE 0
#define EAST_HIP_SCAN_INCLUSIVE 1
#define EAST_HIP_SCAN_EXCLUSIVE_IN_PLACE 2          /* out aliases the input */
#define EAST_HIP_SCAN_INCLUSIVE_IN_PLACE 3
#define EAST_HIP_SCAN_WITH_TOTAL 4                  /* exclusive, n + 1 outputs: out[n] = the sum */
int east_hip_debug_radix_sort_ex(int device, int key_bytes, void *keys, uint32_t *vals, int64_t n, int bits, int begin_bit,
                                 int check_from_bit, const int64_t *doc_off, int32_t n_docs, uint32_t *geometry_out);
int east_hip_debug_radix_spine(int device, const uint32_t *group_sum, int64_t n_groups, const uint32_t *digit_total,
                               const int64_t *doc_off, int32_t n_docs, uint32_t *group_prefix_out, uint32_t *next_total_out,
                               uint32_t *geometry_out);
int east_hip_debug_scan_ex(int device, int form, const uint32_t *in, int64_t n, uint32_t *out, uint32_t *geometry_out);
int east_hip_debug_run_heads(int device, const uint64_t *keys64, int64_t n, int shift, uint32_t *inclusive_out,
                             uint32_t *count_out);
int east_hip_debug_scan_pair_bounded(int device, const uint32_t *a, const uint32_t *b, int64_t n, uint32_t n_dev_value,
                                     uint32_t extra, uint32_t *out_a, uint32_t *out_b);
int east_hip_debug_ascending_offsets(int device, const uint32_t *sorted, int64_t n, int64_t n_values, uint32_t *off_out);
/* One level of a built handle's min pyramid over the LCP table (csrc/tables.h: Pyramid; level 0 is the table itself, level
 * l + 1 holds the minima of level l's aligned groups of 16), padding included.  geometry_out[3]: the number of levels, the
 * level's length and its padded length (0, 0 for a level the pyramid does not have); out (may be null: the geometry alone)
 * takes the padded length, which `capacity` (in words) must cover. */
int east_hip_debug_pyramid_level(east_hip_handle_t h, int32_t level, uint32_t *out, int64_t capacity, int64_t *geometry_out);
/* Test knob: bytes of per-suffix scratch a score call may use (default 1 GiB; 0 restores it); a table over
 * more documents than fit is scored a stretch of documents at a time.  Takes effect at the next
 * east_hip_set_keyphrases / east_hip_score_table. */
int east_hip_debug_set_score_scratch(int64_t bytes);
/* Test knob: workgroups one launch of the score walk may have when the per-keyphrase sums run inside it (default 2^22, far
 * below HIP's limit of 2^32 threads per grid dimension; 0 restores it).  A table over more documents than fit one launch is
 * scored a stretch of documents at a time. */
int east_hip_debug_set_score_grid(int64_t workgroups);
/* Test knob: how east_hip_build_texts[_v] brings the raw text to the device.  -1 (default) = inputs of 8 MiB or more are
 * uploaded in four or five chunks (cut where no token spans the cut) and every chunk is prepared while the next one is on its
 * way; 0 = one upload, one preparation; > 0 = always in chunks of about that many bytes (a few dozen: every fixture goes
 * through the chunk-to-chunk carries). */
int east_hip_debug_set_text_stream(int64_t chunk_bytes);
/* Test knob: how separate texts (east_hip_build_texts_v) reach the device when the preparation is streamed.  A copy out of
 * pageable memory costs ~45 us of set-up, which one large text hides and hundreds of small ones do not: they are copied by
 * a few host threads into a ring of pinned memory and go up slot by slot.  mode -1 (default): four or more texts of less
 * than 8 MiB on average; 0: never; 1: always.  slot_bytes: size of a ring slot (0: the default, 8 MiB). */
int east_hip_debug_set_text_ring(int mode, int64_t slot_bytes);
/* Test knob: the FIRST hash attempt of every cosine build keeps only the low `bits` bits of the term hashes (1 .. 61; 0 =
 * all 61, the default), so that different words collide, the verification finds it and the build starts over with the
 * next seed (east_hip_cosine_info: hash attempts).  The index does not depend on it. */
int east_hip_debug_set_term_hash_bits(int bits);
/* Test knob: the documents of a strip of the BM25 score kernel (more than its accumulators hold -- 2 048, or 512 for
 * collections of up to 512 documents -- is taken as that; 0 or less = the default, all they hold), so that a collection of
 * 65 documents has strip boundaries inside.  Process-wide, read when a score call starts.  The scores do not depend on it. */
int east_hip_debug_set_bm25_strip(int32_t documents);
/* Test knob: the number of entries of a source row the synonyms' pair kernel stages in LDS at a time (1 .. 128; 0 or less =
 * the default, 128), so that rows of a few dozen entries go through the chunk-to-chunk path.  Process-wide, read when a
 * pairs call starts.  The pairs do not depend on it. */
int east_hip_debug_set_synonyms_chunk(int entries);
/* Test knob: the members of a segment the ranking (east_hip_top_build_*) ranks as one tile (1 .. 64, more is taken as 64; 0
 * or less = the default, 64), so that a segment of a few hundred members spans many tiles and the merge does the work.
 * Process-wide, read when a build call starts.  The ranking does not depend on it. */
int east_hip_debug_set_top_tile(int members);
/* Host only (needs no device): the order-preserving variable-length code csrc/ht_code.h makes for n symbols (in their
 * order) with the given weights -- code[i] = the len[i] bits of symbol i's code word, right-aligned.  EAST_HIP_ERR_DOMAIN
 * if no code with word lengths in [3, 12] exists for them (n < 8, n > 256). */
int east_hip_debug_alphabetic_code(const uint64_t *weights, int32_t n, uint32_t *code, int32_t *len);
/* Host only (needs no device): out[i] = symbols[i] below U+0A00 ? symbols[i] : 0xFFFF -- the 16-bit words east_hip_build
 * sends over the link for host symbols of the reference encoding (every symbol from U+0A00 on is a terminator, whose
 * number the build never reads).  vector != 0: the form the upload's host threads run (AVX2 with streaming stores where
 * the CPU has it), 0: the plain loop.  Returns 1 if the vector form ran, 0 if the loop did, < 0 on bad arguments. */
int east_hip_debug_narrow_symbols(const uint32_t *symbols, int64_t n, uint16_t *out, int vector);
/* The same for the BYTES east_hip_build sends when the text's code points all lie below 0xFF (0xFF on the wire = a
 * terminator): out[i] = symbols[i] < 0xFF ? symbols[i] : 0xFF.  Returns (1 if every symbol fitted -- text below 0xFF,
 * terminators from U+0A00 on --, else 0) + (2 if the AVX2 form ran); < 0 on bad arguments. */
int east_hip_debug_narrow_symbols8(const uint32_t *symbols, int64_t n, uint8_t *out, int vector);
/* Test knob (process-wide): which form of the score path runs (easa.py:91-139).  1 (default) = pair k-gram tables marked
 * off the window keys + the per-keyphrase sums inside the walk kernel; 0 = one filled table, per-suffix results in HBM
 * and a reduction kernel (rounds 1-3); 2 = pair tables with the reduction kernel; 3 = filled table with the sums in the
 * walk; 4 = as 1 with the pair tables also for collections of fewer than 16 documents (which by default keep the filled
 * table: the 8-byte marks cost their build more than a few thousand walks get back); 5 = as 1 with every interval searched
 * down to its last suffix (without the walk's register endgame, score.h: walk_endgame).  Takes effect at the next build
 * (tables) / the next east_hip_set_keyphrases (sums) / the next score call (endgame). */
int east_hip_debug_set_score_path(int mode);
/* Host-only: bytes of device arena a build of n_total symbols / n_docs documents
 * reserves (worst case over inputs).  Needs no device. */
int64_t east_hip_plan_arena_bytes(int64_t n_total, int32_t n_docs);
/* The same for a "lean" build: what a build falls back to when the full plan does not fit the
 * free device memory (no buffers for the tie-refinement rounds). */
int64_t east_hip_plan_arena_bytes_lean(int64_t n_total, int32_t n_docs);

#ifdef __cplusplus
}
#endif
#endif /* EAST_HIP_H */
