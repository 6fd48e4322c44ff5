"""gpu tier: the score walk and its k-gram tables against the exact model, exhaustively.

Every comparison is of the WHOLE (K, D) table and the WHOLE (D, S) per-suffix array, bit for bit, normalized and not,
through the plain call (with and without the per-suffix results) and through set_keyphrases + score_resident.  The
keyphrases are all sequences up to a length beyond the table depth over the text alphabet and a symbol absent from the
corpus (+ terminator code points and values that are no code points), so every k-gram a walk can read is read.  The
reference is tests/score_exact.py, a dict of substring counts (pinned to the reference's fixtures and to the oracle in
tests/test_score_exact_host.py, which also asserts what every case here is for); on the large collections it is the
oracle's interval walk over a suffix array that check_tables has verified, plus the model on whole documents.

Every case asserts which table kernels ran (the launches as the library's profiler names them) and the alphabet the build
found; the depth of the tables follows from the alphabet and the sizes by the constants of csrc/build.h and
csrc/score_host.h (score_exact.marked_k / small_k restate them; the host file asserts the values).
"""
import numpy as np
import pytest

import score_exact as sx

pytestmark = pytest.mark.gpu

MODES = (1, 0, 2, 3, 4, 5)                  # east_hip_debug_set_score_path
FUSED_MODES = (1, 3, 4, 5)                  # the per-keyphrase sums inside the walk (keyphrases of at most 256 symbols)
PAIR_MODES = (1, 2, 4, 5)                   # the pair layout where the build marks the tables (4: also below 16 documents)
MARK, SEARCH, FILL = "kgram_mark_kernel", "kgram_search_kernel", "kgram_fill_kernel"    # (the tiled marking kernel goes by the same name)
PAIRS_END, UPPER = "kgram_pairs_end_kernel", "kgram_upper_kernel"
CHUNKS = ("kgram_chunk_min_kernel", "kgram_chunk_suffix_kernel", "kgram_chunk_fill_kernel")
TABLE_KERNELS = (MARK, SEARCH, FILL, PAIRS_END, UPPER) + CHUNKS
PAIR_KERNELS = (PAIRS_END, FILL, UPPER)
WALK, REDUCE = "score_walk_kernel", "score_reduce_kernel"
SINGLE_DOCUMENT = ("random_alone", "markov_alone", "one_letter_alone", "period3_alone", "search_kernel")


class _Knobs(object):
    """The process-wide debug knobs a case sets; back to the defaults on the way out, whatever happened on the way in.
    Speculation is off unless a case asks for it: a HipIndex may be a recycled handle, which builds on the guesses of
    whoever had it before -- no planning sample, so repetitive text is not recognised and the build of a small input marks
    no tables: another path every other time (east/hip_backend.py: HipIndex.__init__)."""

    def __init__(self, hip, score_path=1, window_sort=1, speculation=0):
        self.lib = hip.load()
        self.want = ((self.lib.east_hip_debug_set_score_path, score_path, 1), (self.lib.east_hip_debug_set_window_sort, window_sort, 1),
                     (self.lib.east_hip_debug_set_speculation, speculation, 1))

    def __enter__(self):
        try:
            for fn, value, _ in self.want:
                assert fn(value) == 0, (fn.__name__, value)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        rcs = [fn(default) for fn, _, default in self.want]        # (all of them, then the verdict)
        assert rcs == [0] * len(rcs), rcs
        return False


def _assert_equal(got, want, what, names=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(i) for i in np.argwhere(got != want)[0])
        raise AssertionError("%s: %d of %d entries differ, the first at %s: %r, want %r%s" % (
            what, int((got != want).sum()), got.size, at, got[at], want[at], names(at) if names else ""))


def _resident_table(index, qs, qo, norm):
    import torch
    out = torch.zeros((qo.size - 1, index.n_docs), dtype=torch.float64, device="cuda:%d" % index.device)
    index.set_keyphrases(qs, qo)
    index.score_resident(norm, out.data_ptr())
    return out.cpu().numpy()


def _build(hip, case):
    sym, off, ms = case.input()
    index = hip.HipIndex()
    index.build(sym, off, ms)
    info = index.info()
    assert info["sigma_text"] == case.sigma_t and info["n_docs"] == len(case.docs)
    return index, (sym, off, ms)


def _score_all(index, kps, refs, what, docs=None):
    """The three ways of asking for a table against refs[normalized] = (table, per-suffix array) -- of all documents, or of
    the documents `docs`.  Returns {normalized: (table, suffix)} as the device gave them."""
    qs, qo = sx.pack(kps)
    got = {}
    for norm in (True, False):
        table, suf = index.score_table(qs, qo, norm, want_suffix=True)
        got[norm] = (table, suf)
        if refs is not None:
            want, want_suf = refs[norm]
            pick_t = table if docs is None else table[:, docs]
            pick_s = suf if docs is None else suf[docs]
            _assert_equal(pick_s, want_suf, "%s: per-suffix results (normalized=%s)" % (what, norm),
                          lambda at: " (document %d, suffix %d of keyphrase %r)" % (
                              at[0], at[1] - qo[np.searchsorted(qo, at[1], side="right") - 1],
                              kps[int(np.searchsorted(qo, at[1], side="right")) - 1]))
            _assert_equal(pick_t, want, "%s: table (normalized=%s)" % (what, norm),
                          lambda at: " (keyphrase %r, document %d)" % (kps[at[0]], at[1]))
        _assert_equal(index.score_table(qs, qo, norm), table, "%s: the plain call (normalized=%s)" % (what, norm))
        _assert_equal(_resident_table(index, qs, qo, norm), table, "%s: score_resident (normalized=%s)" % (what, norm))
    return got


def _ran(report):
    return set(name for name in report if name in TABLE_KERNELS)


# ---- small collections: the score side builds the tables itself -----------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sx.small_cases(), ids=repr)
def test_small_collection_equals_the_model(hip, case, mode):
    """At most 65 536 symbols: tables of k <= 3 levels by the marking kernel (one document / tiled), or by binary search
    for one long document, then kgram_fill_kernel; no tables for more than 254 text symbols (u32 stream).  The periodic
    text of the packing case counts as repetitive: the build marks its tables, small as it is (4 levels)."""
    k = case.plans[0][0]
    n_docs = len(case.docs)
    with _Knobs(hip, score_path=mode, window_sort=case.window_sort):
        index, (sym, off, ms) = _build(hip, case)
        try:
            # (the u32 symbol stream goes through DC3 whatever the knob says)
            assert bool(index.info()["window_sorted"]) == (case.window_sort != 0 and case.sigma_t <= 254)
            index.profile_enable(True)
            refs = {norm: case.tables(norm) for norm in (True, False)}
            _score_all(index, case.keyphrases(), refs, "%s, mode %d" % (case, mode))
            report = index.profile_report()
            # the tables: k follows from sigma_t (asserted by _build) and the sizes (score_exact.small_k); which kernel
            # makes them from the number of documents and their length
            if k == 0:
                want = set()
            elif case.marked:
                want = set(PAIR_KERNELS if mode == 4 else CHUNKS)
            elif sym.size // n_docs >= 256 * case.A ** k:
                want = {SEARCH}
            else:
                want = {MARK, FILL}
            assert _ran(report) == want, (case, mode, sorted(report))
            assert (case.name == "search_kernel") == (want == {SEARCH})
            # (the profiler has one name for kgram_mark_kernel and its tiled form: one document takes the first, several
            # the second -- which of the two a case is there for is said here)
            assert (n_docs == 1) == (case.name in SINGLE_DOCUMENT), (case, n_docs)
            assert report.get(MARK, (0, 0))[0] <= 1 and report.get(FILL, (0, 0))[0] <= 1       # built once per index
            assert (REDUCE in report) == (mode not in FUSED_MODES), (case, mode, sorted(report))
            if case.with_long is not None:
                # one keyphrase of 257 symbols: no workgroup can take it whole, every sum goes to the reduction kernel
                index.profile_enable(True)
                model = [case.document(d) for d in range(n_docs)]
                refs = {norm: sx.score_tables(model, case.with_long, norm) for norm in (True, False)}
                _score_all(index, case.with_long, refs, "%s + 257 symbols, mode %d" % (case, mode))
                report = index.profile_report()
                assert REDUCE in report and report[REDUCE][0] == report[WALK][0], (mode, report)
        finally:
            index.profile_enable(False)
            index.close()


# ---- just above the small-input limit of the window sort: the build marks the tables off its keys --------------
def _oracle_refs(oracle, index, inp, kps):
    """{normalized: (table, per-suffix array)} by the oracle's interval walk over the index's suffix arrays, which
    check_tables verifies first (rank-pair condition, linear time): the library is not its own reference."""
    sym, off, ms = inp
    sa = np.concatenate([index.tables(d, names=("suftab",))["suftab"] for d in range(ms.size)])
    oracle.check_tables(sym, off, ms, {"suftab": sa})
    qs, qo = sx.pack(kps)
    # (the oracle takes a terminator code point in a query for the terminator; the library takes it for an absent symbol)
    text = qs < sx.TERMINATOR_START
    qs = np.where(text, qs, np.uint32(1))
    return {norm: oracle.score_table_fast(sym, off, ms, sa, qs, qo, norm, want_suffix=True) for norm in (True, False)}


def _own_table_kernels(case):
    """What the score side runs where the build marked nothing (csrc/score_host.h: ensure_kgram)."""
    sym, _, ms = case.input()
    k = sx.small_k(case.sigma_t, sym.size, ms.size)
    assert (k, False) in case.plans
    return (SEARCH,) if sym.size // ms.size >= 256 * case.A ** k else (MARK, FILL)


def _marked_case(hip, oracle, case, mode, window_sort, want_kernels, model_docs, ht=False):
    """ht: the build makes its first-level keys of variable-length code words (window sort 7 and an alphabet of 7 text
    symbols or more, csrc/build.h: prepare_ht_code) -- the sort then marks nothing."""
    with _Knobs(hip, score_path=mode, window_sort=window_sort):
        index, inp = _build(hip, case)
        try:
            info = index.info()
            assert bool(info["window_sorted"]) == (window_sort != 0), info
            assert bool(info["ht_keys"]) == ht, info
            index.profile_enable(True)
            kps = case.keyphrases()
            what = "%s, mode %d, window sort %d" % (case, mode, window_sort)
            got = _score_all(index, kps, _oracle_refs(oracle, index, inp, kps), what)
            report = index.profile_report()
            assert _ran(report) == set(want_kernels), (what, sorted(report))
            for name in want_kernels:
                assert report[name][0] == 1, (what, name, report[name])
            assert (REDUCE in report) == (mode not in FUSED_MODES), (what, sorted(report))
            # the model on whole documents
            for norm in (True, False):
                want, want_suf = case.tables_of(model_docs, norm)
                _assert_equal(got[norm][0][:, model_docs], want, "%s: table against the model (%s)" % (what, norm))
                _assert_equal(got[norm][1][model_docs], want_suf, "%s: per-suffix results against the model (%s)" % (what, norm))
        finally:
            index.profile_enable(False)
            index.close()


@pytest.mark.parametrize("mode", [1, 2, 5, 0, 3])
def test_marked_pair_tables_equal_the_model(hip, oracle, mode):
    """38 documents (17 of 4 200 symbols, 21 of a few) over 6 letters, window sort 8 (no variable-length keys: they would take the
    marks away): A = 8, k = 4, 4 096 bins.  16 documents or more: the pair layout (modes 1, 2, 5) with the upper tables
    (8 + 1 + 64 + 1 words) staged in LDS; modes 0 and 3: the filled layout, by chunks."""
    case = sx.marked_cases()["pairs"]
    assert len(case.docs) >= 16 and case.plans[0] == (4, True)
    _marked_case(hip, oracle, case, mode, 8, PAIR_KERNELS if mode in PAIR_MODES else CHUNKS, [3, 35])


@pytest.mark.parametrize("window_sort", [8, 0, 7])
def test_marked_pair_tables_with_long_runs_of_empty_buckets(hip, oracle, window_sort):
    """A periodic and a one-letter document among random ones: runs of hundreds of empty entries behind a bucket.  Behind
    DC3 the score side builds its own tables (2 levels); window sort 7 changes nothing for six letters (see below)."""
    case = sx.marked_cases()["pairs_runs"]
    _marked_case(hip, oracle, case, 1, window_sort, PAIR_KERNELS if window_sort else _own_table_kernels(case), [15, 16])


@pytest.mark.parametrize("mode", [1, 0, 3, 4])
def test_marked_tables_of_three_documents_equal_the_model(hip, oracle, mode):
    """Fewer than 16 documents: the filled layout by the three chunk kernels (4 chunks of 1 024 entries); mode 4 forces the
    pair layout."""
    case = sx.marked_cases()["chunks"]
    assert len(case.docs) < 16 and (4, mode == 4) in case.plans
    _marked_case(hip, oracle, case, mode, 8, PAIR_KERNELS if mode == 4 else CHUNKS, [0, 2])


@pytest.mark.parametrize("window_sort", [0, 7])
@pytest.mark.parametrize("which", ["pairs", "chunks"])
def test_large_input_with_tables_of_the_score_side(hip, oracle, which, window_sort):
    """The same collections by DC3 (nothing marked): the score side builds tables of k = 2 / 3 levels over a large input.
    Window sort 7 asks for variable-length keys wherever a code can be made; none is made for fewer than 7 text symbols
    (csrc/build.h: prepare_ht_code, sigma_t + 1 < 8), so these collections over 6 letters get fixed-length keys and the
    build marks their tables as ever.  The collections over 21 and 30 letters below do get a code."""
    case = sx.marked_cases()[which]
    assert case.sigma_t + 1 < 8
    marked = PAIR_KERNELS if which == "pairs" else CHUNKS
    _marked_case(hip, oracle, case, 1, window_sort, marked if window_sort else _own_table_kernels(case), [3, 35] if which == "pairs" else [0, 2])


@pytest.mark.parametrize("window_sort", [8, 0, 7])
def test_more_than_256_chunks(hip, oracle, window_sort):
    """One document of 140 000 symbols over 21 letters: A = 23, k = 4, 279 841 bins = 274 chunks -- the suffix minima of
    the chunks take two rounds of kgram_chunk_suffix_kernel's loop.  DC3, and window sort 7 (variable-length keys: the
    sort marks nothing): the score side's own tables, k = 2 -- 529 entries, found by binary search in a document this long."""
    case = sx.large_case("chunks_274")
    own = _own_table_kernels(case)
    assert own == (SEARCH,) and case.sigma_t + 1 >= 8
    _marked_case(hip, oracle, case, 1, window_sort, CHUNKS if window_sort == 8 else own, [0], ht=window_sort == 7)


@pytest.mark.parametrize("window_sort", [8, 0, 7])
def test_bins_limit_and_upper_tables_from_global_memory(hip, oracle, window_sort):
    """One document of 530 000 symbols over 30 letters, mode 4 (pairs for fewer than 16 documents): A = 32, k = 4,
    bins = 2^20 = KGRAM_KEYS_MAX_BINS exactly; the upper tables take 32 + 1 + 1 024 + 1 = 1 058 words, more than
    KG_UP_LDS_WORDS, so the levels 1 and 2 are read from global memory.  DC3, and window sort 7 (variable-length keys: the
    sort marks nothing): the score side's own tables over a large input, k = 3, 32 768 bins."""
    case = sx.large_case("bins_limit")
    own = _own_table_kernels(case)
    assert own == (MARK, FILL) and case.sigma_t + 1 >= 8
    _marked_case(hip, oracle, case, 4, window_sort, PAIR_KERNELS if window_sort == 8 else own, [0], ht=window_sort == 7)


@pytest.mark.parametrize("name", ["mixed_sigma3", "packing"])
def test_default_speculation_on_a_handle_of_its_own(hip, name):
    """Every case above builds with speculation off, to pin its path on handles that may be recycled.  Here the default:
    speculation on, a handle that is nobody's leftover (reserve_symbols keeps it out of the pool).  Its first build waits
    for the alphabet and takes its planning sample; the second, of the same input, runs on the guesses of the first -- the
    same tables by the same kernels (the repetitive text of the packing case stays on the persistent rounds), the same
    scores."""
    case = [c for c in sx.small_cases() if c.name == name][0]
    sym, off, ms = case.input()
    with _Knobs(hip, speculation=1):
        index = hip.HipIndex(reserve_symbols=int(sym.size))
        try:
            refs = {norm: case.tables(norm) for norm in (True, False)}
            for build in (1, 2):
                index.build(sym, off, ms)
                assert index.info()["sigma_text"] == case.sigma_t and index.info()["window_sorted"]
                index.profile_enable(True)
                _score_all(index, case.keyphrases(), refs, "%s, build %d with speculation" % (case, build))
                assert _ran(index.profile_report()) == set(CHUNKS if case.marked else (MARK, FILL)), (case, build)
        finally:
            index.profile_enable(False)
            index.close()
