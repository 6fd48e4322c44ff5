/*
 * TEST INFRASTRUCTURE ONLY -- linear-time checkers of a built index.
 *
 * The faithful restatement in easa_oracle.c builds every table the way the
 * reference does; its annotation pass (util_index lookups) is quadratic on
 * deep suffix trees and its DC3 is a single core's work.  These functions
 * instead CHECK given tables against their definitions in O(n), with int32
 * scratch (n < 2^31 by the library's ABI), so that inputs of 2^24 .. 2^29
 * symbols and trees thousands of levels deep are checked in full:
 *
 *   suftab  a permutation, and for every rank r
 *           (s[SA[r-1]], rank[SA[r-1]+1]) < (s[SA[r]], rank[SA[r]+1]),
 *           the rank past the end being -1 (Burkhardt & Kaerkkaeinen): this
 *           alone proves the order, no suffix array is built;
 *   lcptab  Kasai et al. from the verified suffix array;
 *   anntab  NSV(k) - PSV(k) at the first l-index k of every lcp-interval,
 *           0 elsewhere, n - m at rank 0 (one monotonic-stack pass);
 *   left    PSV(k) at those k > 0, -1 elsewhere (east_hip_get_lcp_intervals);
 *   childtab_up / _down / _next_l_index   the stack scans of easa_childtab
 *           and easa_next_l_index, each value compared once it is final.
 *
 * Every check reports the lowest failing rank.  The multi-document forms take
 * the documents concatenated (tables in document-local numbering, at the
 * documents' offsets) and report the lowest failing document; they and the
 * batched score walk split their work over documents with at most 16 threads.
 */
#include <omp.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef int64_t i64;
typedef int32_t i32;
typedef uint64_t u64_t;

enum { T_SA = 0, T_LCP = 1, T_ANN = 2, T_UP = 3, T_DOWN = 4, T_NEXT = 5, T_LEFT = 6 };

double easa_score_fast(const uint32_t *sym, i64 n, i64 m, const i64 *suftab,
                       const uint32_t *q, i64 qlen, int normalized,
                       double *suffix_scores, i64 *probes, int *err);

static int n_threads(void)
{
    int t = omp_get_max_threads();             /* (OMP_NUM_THREADS, when set) */
    return t < 1 ? 1 : (t > 16 ? 16 : t);
}

/* a growable int32 stack of records of `w` fields */
typedef struct { i32 *v; i64 sp, cap; int w; } stk_t;

static int stk_push(stk_t *s, const i32 *rec)
{
    if (s->sp == s->cap) {
        i64 cap = s->cap ? s->cap * 2 : 4096;
        i32 *v = (i32 *)realloc(s->v, (size_t)cap * s->w * sizeof(i32));
        if (!v) return -1;
        s->v = v; s->cap = cap;
    }
    memcpy(s->v + s->sp * s->w, rec, (size_t)s->w * sizeof(i32));
    s->sp++;
    return 0;
}

static i32 *stk_top(stk_t *s) { return s->v + (s->sp - 1) * s->w; }

static void lowest(i64 *bad, i64 r) { if (r < *bad) *bad = r; }

/* The rank-pair check and Kasai are bound by the latency of scattered reads: the loops ask for them PF iterations ahead
 * (half as far for reads whose address comes from an earlier one). */
#define PF 32

/* suffix array: `rank` (n + 1 int32) receives the inverse permutation.  Returns the lowest failing rank, n if none; an
 * entry that occurs twice fails at the lower of its ranks. */
i64 lin_check_suftab(const uint32_t *sym, i64 n, const i64 *sa, i32 *rank)
{
    i64 bad = n;
#pragma omp parallel for num_threads(n_threads())
    for (i64 i = 0; i <= n; i++) rank[i] = -1;
#pragma omp parallel for num_threads(n_threads()) reduction(min : bad)
    for (i64 r = 0; r < n; r++) {
        if (r + PF < n && (u64_t)sa[r + PF] < (u64_t)n) __builtin_prefetch(&rank[sa[r + PF]], 1);
        i64 p = sa[r];
        if (p < 0 || p >= n) { if (r < bad) bad = r; continue; }
#pragma omp atomic write
        rank[p] = (i32)r;
    }
    if (bad < n) return bad;
    i64 unwritten = n;                         /* n entries in [0, n) that reach every position: a permutation */
#pragma omp parallel for num_threads(n_threads()) reduction(min : unwritten)
    for (i64 p = 0; p < n; p++)
        if (rank[p] == -1 && p < unwritten) unwritten = p;
    if (unwritten < n) {                       /* (not one: the lowest rank whose entry occurs at another rank as well) */
#pragma omp parallel for num_threads(n_threads()) reduction(min : bad)
        for (i64 r = 0; r < n; r++) {
            i64 w = rank[sa[r]];
            if (w != r) { i64 lo = w < r ? w : r; if (lo < bad) bad = lo; }
        }
        return bad;
    }
#pragma omp parallel for num_threads(n_threads()) reduction(min : bad)
    for (i64 r = 1; r < n; r++) {
        if (r + PF < n) { i64 c = sa[r + PF]; __builtin_prefetch(&sym[c]); __builtin_prefetch(&rank[c + 1]); }
        i64 a = sa[r - 1], b = sa[r];
        if (sym[a] > sym[b] || (sym[a] == sym[b] && rank[a + 1] >= rank[b + 1])) { if (r < bad) bad = r; }
    }
    return bad;
}

/* lcp[r] = length of the common prefix of the suffixes at ranks r - 1 and r (0 at r = 0), by Kasai from a VERIFIED
 * suffix array and its inverse.  The text is cut into one stretch per thread; each starts from h = 0 (h is only a
 * lower bound that saves comparisons). */
i64 lin_check_lcptab(const uint32_t *sym, i64 n, const i64 *sa, const i32 *rank, const i64 *lcp)
{
    i64 bad = n;
    if (n > 0 && lcp[0] != 0) bad = 0;
    int T = n_threads();
    if (n < (1 << 16)) T = 1;
#pragma omp parallel for num_threads(T) reduction(min : bad) schedule(static, 1)
    for (int c = 0; c < T; c++) {
        i64 h = 0, end = n * (c + 1) / T;
        for (i64 i = n * c / T; i < end; i++) {
            if (i + PF < end) {
                i64 rp = rank[i + PF];
                __builtin_prefetch(&lcp[rp]);
                if (rp > 0) __builtin_prefetch(&sa[rp - 1]);
            }
            if (i + PF / 2 < end) {
                i64 rp = rank[i + PF / 2];
                if (rp > 0) __builtin_prefetch(&sym[sa[rp - 1]]);
            }
            i64 r = rank[i];
            if (r == 0) { h = 0; continue; }
            i64 j = sa[r - 1];
            while (i + h < n && j + h < n && sym[i + h] == sym[j + h]) h++;
            if (lcp[r] != h && r < bad) bad = r;
            if (h > 0) h--;
        }
    }
    return bad;
}

/* anntab and left from a VERIFIED lcp table: the bottom-up traversal of the lcp-intervals (Abouelhoda et al.).  The
 * interval <l, lb, rb> pushed at rank f has f as its first l-index and lb as PSV(f); it closes at NSV(f) = rb + 1.
 * Either table may be NULL.  Returns the lowest failing rank (n if none) in *bad_ann / *bad_left. */
int lin_check_anntab(const i64 *lcp, i64 n, i64 m, const i64 *ann, const i64 *left, i64 *bad_ann, i64 *bad_left)
{
    stk_t s = {0, 0, 0, 3};                    /* <l, lb, f> */
    i64 ba = n, bl = n;
    i32 root[3] = {0, 0, 0};
    if (stk_push(&s, root)) return -1;
    for (i64 k = 1; k <= n; k++) {
        i64 v = k < n ? lcp[k] : 0, lb = k - 1;
        while (s.sp > 1 && v < stk_top(&s)[0]) {
            const i32 *t = stk_top(&s);
            i64 f = t[2], b = t[1];
            if (ann && ann[f] != k - b) lowest(&ba, f);
            if (left && left[f] != b) lowest(&bl, f);
            lb = b;
            s.sp--;
        }
        if (k == n) break;
        if (v > stk_top(&s)[0]) {
            i32 rec[3] = {(i32)v, (i32)lb, (i32)k};
            if (stk_push(&s, rec)) { free(s.v); return -1; }
        } else {                               /* not the first l-index of an interval */
            if (ann && ann[k] != 0) lowest(&ba, k);
            if (left && left[k] != -1) lowest(&bl, k);
        }
    }
    if (n > 0) {
        if (ann && ann[0] != n - m) lowest(&ba, 0);
        if (left && left[0] != -1) lowest(&bl, 0);
    }
    free(s.v);
    *bad_ann = ba; *bad_left = bl;
    return 0;
}

/* childtab up / down (easa_childtab's scan; down[x] is final once x leaves the stack) and next_l_index (easa_next_l_index's
 * scan: x is popped either by an equal value, next[x] = i, or by a smaller one, next[x] = 0).  Any table may be NULL. */
int lin_check_childtab(const i64 *lcp, i64 n, const i64 *up, const i64 *down, const i64 *next,
                       i64 *bad_up, i64 *bad_down, i64 *bad_next)
{
    i64 bu = n, bd = n, bn = n;
    /* (both scans of easa_oracle.c start from a stack holding rank 0 and process i = 0 against it; what that leaves is
     * a stack holding rank 0, up[0] = next[0] = 0 for now, and the scans go on from i = 1) */
    if (n > 0 && up && up[0] != 0) lowest(&bu, 0);
    if (n > 0 && (up || down)) {
        stk_t s = {0, 0, 0, 2};                /* <index, down so far> */
        i32 first[2] = {0, 0};
        i64 last = -1;
        if (stk_push(&s, first)) return -1;
        for (i64 i = 1; i < n; i++) {
            while (s.sp > 1 && lcp[i] < lcp[stk_top(&s)[0]]) {
                const i32 *t = stk_top(&s);
                last = t[0];
                if (down && down[last] != t[1]) lowest(&bd, last);
                s.sp--;
                i32 *u = stk_top(&s);
                if (lcp[i] <= lcp[u[0]] && lcp[u[0]] != lcp[last]) u[1] = (i32)last;
            }
            if (up && up[i] != (last != -1 ? last : 0)) lowest(&bu, i);
            last = -1;
            i32 rec[2] = {(i32)i, 0};
            if (stk_push(&s, rec)) { free(s.v); return -1; }
        }
        for (i64 e = 0; e < s.sp; e++) {
            const i32 *t = s.v + e * 2;
            if (down && down[t[0]] != t[1]) lowest(&bd, t[0]);
        }
        free(s.v);
    }
    if (n > 0 && next) {
        stk_t s = {0, 0, 0, 1};
        i32 first = 0;
        if (stk_push(&s, &first)) return -1;
        for (i64 i = 1; i < n; i++) {
            while (s.sp > 1 && lcp[i] < lcp[*stk_top(&s)]) {
                i64 x = *stk_top(&s);
                if (next[x] != 0) lowest(&bn, x);
                s.sp--;
            }
            if (s.sp > 0 && lcp[i] == lcp[*stk_top(&s)]) {
                i64 x = *stk_top(&s);
                if (next[x] != i) lowest(&bn, x);
                s.sp--;
            }
            i32 rec = (i32)i;
            if (stk_push(&s, &rec)) { free(s.v); return -1; }
        }
        for (i64 e = 0; e < s.sp; e++)
            if (next[s.v[e]] != 0) lowest(&bn, s.v[e]);
        free(s.v);
    }
    *bad_up = bu; *bad_down = bd; *bad_next = bn;
    return 0;
}

/* every given table of one document; returns 0 (all agree), 1 (*table, *rank: the first failure) or -1 (no memory).
 * The suffix array and the lcp table must be given when anything after them is: the later checks build on them --
 * unless `lcp_verified`: then sa is NULL and lcp, checked before, is only the base of the others.  Within a document the
 * work runs on several threads (inside the multi-document loop: on the loop's one). */
static int check_doc(const uint32_t *sym, i64 n, i64 m, const i64 *sa, const i64 *lcp, int lcp_verified, const i64 *ann,
                     const i64 *up, const i64 *down, const i64 *next, const i64 *left, i64 *table, i64 *rank)
{
    i64 bad[7];
    int oom = 0;
    for (int t = 0; t < 7; t++) bad[t] = n;
    if (sa) {
        i32 *inv = (i32 *)malloc(((size_t)n + 1) * sizeof(i32));
        if (!inv) return -1;
        bad[T_SA] = lin_check_suftab(sym, n, sa, inv);
        if (bad[T_SA] == n && lcp) bad[T_LCP] = lin_check_lcptab(sym, n, sa, inv, lcp);
        free(inv);
    }
    if (bad[T_SA] == n && bad[T_LCP] == n && lcp && (sa || lcp_verified)) {
#pragma omp parallel sections num_threads(n_threads() < 2 ? 1 : 2)
        {
#pragma omp section
            if ((ann || left) && lin_check_anntab(lcp, n, m, ann, left, &bad[T_ANN], &bad[T_LEFT])) oom = 1;
#pragma omp section
            if ((up || down || next) && lin_check_childtab(lcp, n, up, down, next, &bad[T_UP], &bad[T_DOWN], &bad[T_NEXT]))
                oom = 1;
        }
    }
    if (oom) return -1;
    for (int t = 0; t < 7; t++) {
        if (bad[t] < n) { *table = t; *rank = bad[t]; return 1; }
    }
    return 0;
}

/* D documents at doc_off[0..D] of the concatenated symbols and tables.  fail[3] = <document, table, rank> of the lowest
 * failing document.  Returns 0, 1 (a failure) or -1 (no memory). */
int lin_check_tables(const uint32_t *sym, const i64 *doc_off, const i64 *n_strings, i64 D,
                     const i64 *sa, const i64 *lcp, int lcp_verified, const i64 *ann, const i64 *up, const i64 *down,
                     const i64 *next, const i64 *left, i64 *fail)
{
    i64 first = D, ft = 0, fr = 0;
    int oom = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads())
    for (i64 d = 0; d < D; d++) {
        i64 o = doc_off[d], n = doc_off[d + 1] - doc_off[d], t = 0, r = 0;
#define AT(p) ((p) ? (p) + o : NULL)
        int rc = check_doc(sym + o, n, n_strings[d], AT(sa), AT(lcp), lcp_verified, AT(ann), AT(up), AT(down), AT(next), AT(left), &t, &r);
#undef AT
#pragma omp critical
        {
            if (rc < 0) oom = 1;
            if (rc == 1 && d < first) { first = d; ft = t; fr = r; }
        }
    }
    if (oom) return -1;
    if (first == D) return 0;
    fail[0] = first; fail[1] = ft; fail[2] = fr;
    return 1;
}

/* the interval-narrowing score walk (easa_score_fast) of K queries in D documents: out[k * D + d], and when `suf` is
 * given the per-suffix results of document d at suf[d * q_off[K] + q_off[k] ..].  A query of length 0 scores 0 with its
 * entry counted in *n_empty (the reference raises ZeroDivisionError). */
int lin_score_table(const uint32_t *sym, const i64 *doc_off, const i64 *n_strings, i64 D, const i64 *sa,
                    const uint32_t *q, const i64 *q_off, i64 K, int normalized, double *out, double *suf,
                    i64 *n_empty)
{
    i64 empty = 0, total = q_off[K];
#pragma omp parallel for schedule(dynamic, 16) num_threads(n_threads()) reduction(+ : empty)
    for (i64 e = 0; e < K * D; e++) {
        i64 d = e / K, k = e % K, o = doc_off[d];
        int err = 0;
        out[k * D + d] = easa_score_fast(sym + o, doc_off[d + 1] - o, n_strings[d], sa + o, q + q_off[k],
                                         q_off[k + 1] - q_off[k], normalized, suf ? suf + d * total + q_off[k] : NULL,
                                         NULL, &err);
        empty += err;
    }
    if (n_empty) *n_empty = empty;
    return 0;
}
