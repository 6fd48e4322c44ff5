"""gpu tier: the parity tests proper.  Everything goes through the C ABI
(east.hip_backend -> libeast_hip.so); the checker is the committed golden
fixtures (generated from the imported reference) and the CPU oracle.

Bar: suffix array, LCP, annotation and child tables bit-exact; scores are
compared with == (bit-equal) where the fixtures hold them and the required
tolerance 1e-6 is asserted as well.
"""
import os

import numpy as np
import pytest

from conftest import load_golden, word_stream

pytestmark = pytest.mark.gpu


_PATH_KNOB = {"window_sort": 1, "window_sort_unfused": 4, "window_sort_ht": 7, "window_sort_ht_unfused": 9, "dc3_only": 0,
              "window_sort_seg": 1, "window_sort_seg_unfused": 4, "window_sort_seg_ht": 7}
_CURRENT = {"knob": 1, "seg": 0}          # the knobs of the running test (tests that check which path a build took)


@pytest.fixture(autouse=True, params=list(_PATH_KNOB))
def suffix_sort_path(request, hip):
    """Every parity test runs eight times: through the all-suffix window sort as it ships (the last radix
    digit ordered in LDS by the fused finish), through the same sort with every pass global and the separate
    placement pass, through the window sort with first-level keys of variable-length code words wherever a code can
    be made (csrc/ht_code.h; by itself the build only takes them for text they pay on) with and without the fused
    finish, with the window sort switched off, so that DC3 -- the fallback for repetitive inputs -- stays covered on
    every input as well, and (the `_seg` paths) through the segmented first-level sort -- every document sorted inside
    its own range, no document number in the keys (csrc/radix_sort.h: RsSeg; by itself the build takes it for a few
    large documents) -- wherever a shard holds 2 .. 65 535 documents.
    (Tests that read `suffix_sort_path` get "window_sort" for the first two.)"""
    lib = hip.load()
    seg = "_seg" in request.param
    assert lib.east_hip_debug_set_window_sort(_PATH_KNOB[request.param]) == 0
    assert lib.east_hip_debug_set_segmented_sort(1 if seg else -1) == 0
    _CURRENT["knob"] = _PATH_KNOB[request.param]
    _CURRENT["seg"] = int(seg)
    # (the variants with variable-length keys / segments get their own names: the checks of WHICH passes ran do not apply)
    yield "window_sort" if request.param in ("window_sort", "window_sort_unfused") else request.param
    assert lib.east_hip_debug_set_window_sort(1) == 0
    assert lib.east_hip_debug_set_segmented_sort(-1) == 0
    _CURRENT["knob"] = 1
    _CURRENT["seg"] = 0


TABLES = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")
TOL = 1e-6


def _raw_path(request):
    """The parametrisation of the running test as the autouse fixture got it (suffix_sort_path folds two of them)."""
    return request.node.callspec.params["suffix_sort_path"]


def _only_paths(request, *paths):
    """Full-size cases pay for a CPU oracle of tens of seconds: they run on the named paths and skip the others."""
    if _raw_path(request) not in paths:
        pytest.skip("full-size case: runs on %s only" % " / ".join(paths))


def _three_paths(request, *others):
    """Cases of ten seconds and more run on window_sort, on dc3_only and on ONE of `others` -- picked by the test's name:
    another one for every test, the same one every run -- instead of on five to eight paths (the gpu tier is bounded by
    the driver's step budget; the cases under a second keep all eight)."""
    import zlib
    raw = _raw_path(request)
    if raw in ("window_sort", "dc3_only"):
        return
    pick = others[zlib.crc32(request.node.originalname.encode()) % len(others)]
    if raw != pick:
        pytest.skip("full-size case: runs on window_sort / dc3_only / %s" % pick)


def _check_case(base, case):
    ast = base.AST.get_ast(case["strings"])
    assert [ord(c) for c in ast.string] == case["string"]
    for name in TABLES:
        got = getattr(ast, name)
        assert got.dtype == np.int64
        assert got.tolist() == case[name], (name, case["strings"])
    for q in case["queries"]:
        for mode, norm in (("normalized", True), ("denormalized", False)):
            total, suffixes = ast.score(q["query"], normalized=norm, return_suffix_scores=True)
            assert abs(total - q[mode]) <= TOL
            assert total == q[mode], (case["strings"], q["query"], mode, total, q[mode])
            assert ast.score(q["query"], normalized=norm) == q[mode]
            qq = q["query"].replace(" ", "")
            want = q["suffix_" + mode]
            # the reference returns a dict keyed by suffix text: repeated suffixes collapse to the last
            expect = {qq[i:]: want[i] for i in range(len(qq))}
            assert suffixes == expect


def test_readme_example(hip):
    from east.asts import base
    case = load_golden("readme_example.json")
    _check_case(base, case)
    ast = base.AST.get_ast(["XABXAC", "HI"])
    assert ast.score("ABCI") == 0.1875          # README.rst:151
    assert ast.score("NOPE") == 0               # README.rst:152


def test_reference_unit_test_case(hip):
    """tests/asts/test_base.py:13-24: every algorithm name gives identical scores."""
    from east.asts import base
    case = load_golden("test_base_case.json")
    _check_case(base, case)
    for alg in ("easa", "easa_hip", "ast_linear", "ast_naive"):
        ast = base.AST.get_ast(case["strings"], alg)
        for q in case["queries"]:
            assert ast.score(q["query"], normalized=True) == q["normalized"]
            assert ast.score(q["query"], normalized=False) == q["denormalized"]


def test_fuzz_fixtures(hip):
    from east.asts import base
    for case in load_golden("fuzz_small.json")["cases"]:
        _check_case(base, case)


def test_factory_errors(hip):
    from east import exceptions
    from east.asts import base
    with pytest.raises(exceptions.EmptyStringsCollectionException):
        base.AST.get_ast([])
    with pytest.raises(exceptions.NoSuchASTAlgorithm):
        base.AST.get_ast(["A"], "no_such")
    assert base.AST.get_ast(["中文AB"]).score("中文") > 0        # (text of any script: test_text_above_the_terminator_base_*)
    with pytest.raises(ZeroDivisionError):
        base.AST.get_ast(["AB"]).score(" ")


def _table_equal(got, want):
    assert set(got) == set(want)
    for kp in want:
        assert set(got[kp]) == set(want[kp])
        for t in want[kp]:
            assert abs(got[kp][t] - want[kp][t]) <= TOL
            assert got[kp][t] == want[kp][t], (kp, t, got[kp][t], want[kp][t])


@pytest.mark.parametrize("fixture", ["sample_table.json", "hse_config1.json", "zipf_docs.json", "prose_like_docs.json"])
def test_keyphrases_table_fixtures(hip, fixture):
    """BASELINE config 1 (30 HSE docs x 10 keyphrases), the XABXAC sample and the
    natural-language-like docs scored by ast_linear: the batched build + batched score."""
    from east import applications, relevance
    g = load_golden(fixture)
    texts = {k: v.encode("utf-8") for k, v in g["texts"].items()}
    for mode, norm in (("normalized", True), ("denormalized", False)):
        measure = relevance.ASTRelevanceMeasure("easa", norm)
        table = applications.keyphrases_table(g["keyphrases"], texts, measure)
        _table_equal(table, g[mode])
        if "sum_" + mode in g:
            assert abs(sum(v for row in table.values() for v in row.values()) - g["sum_" + mode]) < 1e-9
        # per-pair surface (relevance.py:51-53) agrees with the batched table
        from east import utils
        names = list(texts.keys())
        for kp in g["keyphrases"][:3]:
            for j in (0, len(names) - 1):
                assert measure.relevance(utils.prepare_text(kp), j) == g[mode][kp][names[j]]


def test_hse_per_doc_tables(hip):
    """Per-document tables out of ONE batched build equal the reference's per-document ASTs."""
    from east import relevance
    g = load_golden("hse_config1.json")
    names = list(g["texts"].keys())
    measure = relevance.ASTRelevanceMeasure()
    measure.set_text_collection([g["texts"][k].encode("utf-8") for k in names])
    for d, name in enumerate(names):
        want = g["per_doc"][name]
        t = measure.index.tables(d)
        assert len(t["suftab"]) == want["n"]
        assert t["suftab"][:8].tolist() == want["suftab_head"]
        assert int(sum(int(x) * (i + 1) for i, x in enumerate(t["suftab"]))) == want["suftab_sum"]
        assert int(t["lcptab"].sum()) == want["lcptab_sum"] and int(t["lcptab"].max()) == want["max_lcp"]
        assert int(t["anntab"].sum()) == want["anntab_sum"]


def _random_collections(rng, n_docs, alphabet, max_strings=8, max_len=14):
    docs = []
    for _ in range(n_docs):
        m = int(rng.integers(1, max_strings + 1))
        sc = ["".join(rng.choice(list(alphabet), size=int(rng.integers(0, max_len + 1)))) for _ in range(m)]
        if sum(map(len, sc)) == 0:
            sc[0] = alphabet[0]
        docs.append(sc)
    return docs


FUZZ_SEEDS = {"AB": 101, "ABC": 202, "ABCDEFGH": 303, "AB C": 404, "АБВГДЕЖЗ": 505}


@pytest.mark.parametrize("alphabet", list(FUZZ_SEEDS))
def test_fuzz_multidoc_vs_oracle(hip, oracle, alphabet):
    """Random small corpora: every table of every document and the K x D scores vs the oracle's
    faithful port (sibling-chain walk), normalized and denormalized."""
    from east import relevance
    rng = np.random.default_rng(FUZZ_SEEDS[alphabet])         # (fixed: hash() is randomized per process)
    for it in range(6):
        docs = _random_collections(rng, int(rng.integers(1, 9)), alphabet)
        measure = relevance.ASTRelevanceMeasure()
        measure.set_strings_collections(docs)
        oracles = [oracle.OracleEASA(sc) for sc in docs]
        for d, o in enumerate(oracles):
            t = measure.index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (name, docs[d])
        queries = ["".join(rng.choice(list(alphabet + "Z"), size=int(rng.integers(1, 12)))) for _ in range(12)]
        queries = [q for q in queries if q.replace(" ", "")]
        for norm in (True, False):
            measure.normalized = norm
            table = measure.relevance_table(queries)
            for k, q in enumerate(queries):
                for d, o in enumerate(oracles):
                    assert table[k, d] == o.score(q, normalized=norm), (docs[d], q, norm)


def test_medium_docs_vs_oracle(hip, oracle):
    """8 word-stream docs of 64 KiB in text mode (3-word strings): bit-exact tables and scores
    against the oracle (fast walk, itself pinned to the faithful walk in the CPU tier)."""
    from east import relevance, utils
    rng = np.random.default_rng(20243)
    texts = [word_stream(rng, 64 << 10) for _ in range(8)]
    measure = relevance.ASTRelevanceMeasure()
    measure.set_text_collection(texts)
    collections = [utils.text_to_strings_collection(t) for t in texts]
    oracles = [oracle.OracleEASA(sc) for sc in collections]
    for d, o in enumerate(oracles):
        t = measure.index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
    kps = []
    for i in range(200):
        if i % 2 == 0:
            toks = texts[i % 8].decode().split()
            st = int(rng.integers(0, len(toks) - 3))
            kps.append(" ".join(toks[st:st + int(rng.integers(1, 4))]))
        else:
            kps.append(word_stream(rng, int(rng.integers(4, 24))).decode().strip())
    kps = [k for k in kps if k.replace(" ", "")]
    for norm in (True, False):
        measure.normalized = norm
        table = measure.relevance_table([utils.prepare_text(k) for k in kps])
        for k, kp in enumerate(kps):
            for d, o in enumerate(oracles):
                assert table[k, d] == o.score(utils.prepare_text(kp), normalized=norm, fast=True)


def test_score_invariant_to_sharding(hip):
    """Shard-emulation (SURVEY.md section 4 tier 5): the K x D table does not depend on how the
    documents are split into device shards or on document order."""
    from east import relevance, utils
    rng = np.random.default_rng(7)
    texts = [word_stream(rng, 8 << 10) for _ in range(12)]
    kps = [utils.prepare_text(word_stream(rng, 12).decode()) for _ in range(40)]
    full = relevance.ASTRelevanceMeasure()
    full.set_text_collection(texts)
    want = full.relevance_table(kps)
    for shards in (2, 3, 4):
        cols = []
        for r in range(shards):
            part = texts[r::shards]
            m = relevance.ASTRelevanceMeasure()
            m.set_text_collection(part)
            cols.append((list(range(len(texts)))[r::shards], m.relevance_table(kps)))
        got = np.empty_like(want)
        for idx, block in cols:
            got[:, idx] = block
        assert np.array_equal(got, want)


def test_wide_text_alphabet_vs_oracle(hip, oracle):
    """~2500 distinct text code points: level-0 keys need the 64-bit compressed-terminator path."""
    from east import relevance
    rng = np.random.default_rng(5)
    docs = []
    for _ in range(3):
        docs.append(["".join(chr(int(c)) for c in rng.integers(2, 0x0A00, size=int(rng.integers(1, 40))))
                     for _ in range(int(rng.integers(50, 200)))])
    measure = relevance.ASTRelevanceMeasure()
    measure.set_strings_collections(docs)
    assert measure.index.info()["sigma_text"] > 1024
    for d, sc in enumerate(docs):
        o = oracle.OracleEASA(sc)
        t = measure.index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        queries = [sc[i][:12] for i in range(0, len(sc), 17) if sc[i]]
        table = measure.relevance_table(queries)
        for k, q in enumerate(queries):
            assert table[k, d] == o.score(q, fast=True)


def test_many_strings_terminator_order(hip, oracle):
    """Many short and duplicate strings: suffixes that differ only in their terminator must come
    out in terminator (= position) order -- the stable level-0 sort with shared terminator code."""
    from east.asts import base
    rng = np.random.default_rng(9)
    strings = ["".join(rng.choice(list("AB"), size=int(rng.integers(0, 4)))) for _ in range(3000)]
    ast = base.AST.get_ast(strings)
    o = oracle.OracleEASA(strings)
    for name in TABLES:
        assert np.array_equal(getattr(ast, name), getattr(o, name)), name
    for q in ["A", "AB", "ABA", "BBB", "ABAB"]:
        assert ast.score(q) == o.score(q) and ast.score(q, normalized=False) == o.score(q, normalized=False)


def test_16mib_document_vs_oracle(hip, oracle):
    """One 16 MiB word-stream document in text mode (15 M symbols, 0.75 M strings): SA, LCP and
    annotation table bit-exact against the oracle; 500 keyphrases bit-equal."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 2)
    _, sym, m = synthetic.word_stream_document(rng, 16 << 20, want_text=False)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([m]))
    t = index.tables(0, names=("suftab", "lcptab", "anntab"))
    o = oracle.OracleEASA(symbols=sym, n_strings=m)
    for name in ("suftab", "lcptab", "anntab"):
        assert np.array_equal(t[name], getattr(o, name)), name
    qs, qo = synthetic.keyphrases(rng, sym, 500)
    for norm in (True, False):
        table = index.score_table(qs, qo, norm)
        for k in range(500):
            assert table[k, 0] == o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True)


def test_64mib_document_vs_oracle(hip, oracle, request):
    """BASELINE configs[1] -- the headline configuration -- bit-exact at its real size: the 64 MiB word-stream document in
    text mode (61.1 M symbols, 2.98 M strings), all six tables array_equal to the oracle (easa.py:16-24) and the bench's
    1 000 keyphrases bit-equal in both modes (easa.py:26-36, 91-139).  The shipping path only: the oracle build alone
    is 15 s of one core."""
    _only_paths(request, "window_sort")
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 2)                  # bench.py's document and keyphrases
    _, sym, m = synthetic.word_stream_document(rng, 64 << 20, want_text=False)
    qs, qo = synthetic.keyphrases(rng, sym, 1000)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([m]))
    info = index.info()
    assert info["n_total"] == sym.size and info["window_sorted"] == 1 and info["fused_finish"] == 1
    o = oracle.OracleEASA(symbols=sym, n_strings=m)
    for name in TABLES:                                      # one at a time: 61 M int64 entries each
        got = index.tables(0, names=(name,))[name]
        assert np.array_equal(got, getattr(o, name)), name
        del got
    for norm in (True, False):
        table = index.score_table(qs, qo, norm)
        want = np.array([o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True) for k in range(1000)])
        assert np.array_equal(table[:, 0], want), norm
        for k in range(0, 1000, 100):                        # ... and the reference's own walk over the sibling chains
            assert table[k, 0] == o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=False), (k, norm)


@pytest.mark.parametrize("n_docs", [1, 8])
@pytest.mark.parametrize("n", [1000, 10000, 100000])
def test_reference_worst_case_collection_vs_oracle(hip, oracle, request, suffix_sort_path, n, n_docs):
    """The input of the reference's own runtime harness (analysis/runtime.py:19-31 on analysis/utils.py:5-9): m = 100
    identical strings of n - 4 letters -- every suffix in a tie group of 100 that only the terminators tell apart, common
    prefixes as long as the string (far beyond the direct-comparison cap at n = 10^5: the blocked-Kasai finish) -- as one
    document and as 8 documents of that shape.  All six tables array_equal to the oracle, scores bit-equal."""
    if n == 100000:
        _only_paths(request, "window_sort", "dc3_only", "window_sort_seg")
    from east import hip_backend, synthetic
    rng = np.random.default_rng(4100 + n + n_docs)
    docs = [synthetic.worst_case_collection(rng, 100, n) for _ in range(n_docs)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs], dtype=np.int32))
    if suffix_sort_path == "window_sort" and n * n_docs <= 10000:
        # (100 K .. 1 M symbols tied in groups of 100: the domain fits the chip, one persistent launch runs every round --
        # csrc/persist_rounds.h -- instead of ~15 launches per round)
        assert index.info()["persist_rounds"] >= 5, index.info()
    qs, qo = synthetic.keyphrases(rng, sym, 60)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    sampled = range(n_docs) if n < 100000 else sorted({0, n_docs - 1})       # (11 s of oracle per document at 10^5)
    for d in sampled:
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        assert int(o.lcptab.max()) == n - 4
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d, n)
        for norm in (True, False):
            for k in range(60):
                assert tables[norm][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True), (d, k, norm)
        for k in range(0, 60, 6):
            assert tables[True][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=False), (d, k)


@pytest.mark.parametrize("max_wgs", [3, 25, 0])
@pytest.mark.parametrize("case", ["identical_strings", "copies_in_two_documents", "binary_text"])
def test_persistent_rounds_large_form_on_small_domains(hip, oracle, request, case, max_wgs):
    """The large form of the persistent rounds (csrc/persist_rounds.h: refine_persist2_kernel -- a workgroup walks several
    tiles per round, the tiles' state in global memory, ranges that move from round to round) is what a 10 M-symbol
    domain takes; east_hip_debug_set_persist(1, n) runs it on small repetitive collections with 3 / 25 / all workgroups,
    i.e. with dozens of tiles, a few, one per workgroup: the hand-off of a tile's tail to its right neighbour (found
    unsorted at tile boundaries while the barrier had no release / acquire), groups of 2 .. 100 equal suffixes, two
    documents.  All six tables array_equal to the oracle."""
    _only_paths(request, "window_sort", "window_sort_unfused")
    from east import hip_backend, synthetic
    from east.asts import utils as ast_utils
    lib = hip.load()
    rng = np.random.default_rng(31 + len(case))
    if case == "identical_strings":
        parts = [synthetic.worst_case_collection(rng, 100, 1500)[0]]
        ms = [100]
    elif case == "copies_in_two_documents":
        blob = "".join(rng.choice(list("AB"), size=20000))
        docs = [[blob, blob, "C" + blob], [blob[::-1], blob[::-1]]]
        parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
        ms = [3, 2]
    else:
        text = "".join(rng.choice(list("AB"), size=150000))
        parts = [ast_utils.strings_to_symbols([text[:90000], text[30000:]])]
        ms = [2]
    sym = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    assert lib.east_hip_debug_set_persist(1, max_wgs) == 0
    try:
        index = hip_backend.HipIndex()
        index.build(sym, off, np.array(ms, dtype=np.int32))
        info = index.info()
        assert info["persist_rounds"] >= 3, info
        for d in range(len(parts)):
            o = oracle.OracleEASA(symbols=parts[d], n_strings=ms[d])
            t = index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (name, d, case, max_wgs, info)
    finally:
        assert lib.east_hip_debug_set_persist(0, 0) == 0


def test_sixteen_copies_of_a_passage_in_one_string(hip, oracle, request):
    """`get_ast([one string])` on a 1 MiB passage written 16 times in a row (16.8 M symbols, no terminator in between):
    common prefixes of up to 15 MiB, tie groups nested 16 deep.  SA, LCP and annotation array_equal to the oracle."""
    _only_paths(request, "window_sort", "dc3_only")
    from east import hip_backend, synthetic
    rng = np.random.default_rng(1616)
    sym, m = synthetic.repeated_passage_document(rng, 1 << 20, 16)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([m]))
    o = oracle.OracleEASA(symbols=sym, n_strings=m)
    assert int(o.lcptab.max()) == 15 << 20
    t = index.tables(0)
    for name in TABLES:
        assert np.array_equal(t[name], getattr(o, name)), name
    qs, qo = synthetic.keyphrases(rng, sym, 100)
    table = index.score_table(qs, qo, True)
    for k in range(100):
        assert table[k, 0] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=True), k


def _assert_scores(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError("%s: %r differs at %s: %r, want %r" % (what, got.shape, tuple(bad), got[tuple(bad)],
                                                                    want[tuple(bad)]))


def _check_index(oracle, index, sym, off, ms, names=TABLES, left=True, scores=None, group=1 << 25):
    """Every document of a build checked in full against the definitions of its tables (oracle.check_tables, linear time:
    the suffix array by the rank-pair condition, LCP by Kasai from it, anntab, child tables and the lcp-interval lefts
    from LCP), the documents read back and checked in runs of about `group` symbols.  `scores`: (q_symbols, q_offsets,
    {normalized: score table, or (table, per-suffix results) as score_table(want_suffix=True) gives them}[, rows]) --
    the given rows (default: all) of every document equal to the batched interval walk (easa_score_fast), bit for bit."""
    off = np.asarray(off, np.int64)
    ms = np.asarray(ms, np.int64)
    if scores is not None:
        qs, qo, got = scores[:3]
        rows = np.arange(qo.size - 1) if len(scores) < 4 else np.asarray(scores[3])
        sub = [qs[qo[k]:qo[k + 1]] for k in rows]
        sub_qs, sub_qo = np.concatenate(sub), np.concatenate([[0], np.cumsum([q.size for q in sub])])
    d0 = 0
    while d0 < ms.size:
        d1 = d0 + 1
        while d1 < ms.size and off[d1 + 1] - off[d0] <= group:
            d1 += 1
        t = {}
        for name in names:                                       # (one table at a time: int32 read-back, int64 copy)
            t[name] = np.concatenate([index.tables(d, names=(name,))[name] for d in range(d0, d1)])
        if left:
            t["left"] = np.concatenate([index.lcp_interval_lefts(d) for d in range(d0, d1)])
        s, loc = sym[off[d0]:off[d1]], off[d0:d1 + 1] - off[d0]
        try:
            oracle.check_tables(s, loc, ms[d0:d1], t)
        except oracle.TableMismatch as e:
            raise oracle.TableMismatch(e.doc + d0, e.table, e.rank)
        if scores is not None:
            for norm, g in got.items():
                table, suf = g if isinstance(g, tuple) else (g, None)
                want = oracle.score_table_fast(s, loc, ms[d0:d1], t["suftab"], sub_qs, sub_qo, norm,
                                               want_suffix=suf is not None)
                if suf is not None:
                    want, want_suf = want
                    _assert_scores(suf[d0:d1], want_suf, "per-suffix scores of documents %d.. (%s)" % (d0, norm))
                _assert_scores(table[rows, d0:d1], want, "scores of documents %d.. (%s)" % (d0, norm))
        del t
        d0 = d1


def test_64mib_document_properties(hip, oracle, request, suffix_sort_path):
    """BASELINE configs[1] at full size (64 MiB, text mode): all six tables and the lcp-interval lefts checked in full
    against their definitions, the 1 000 keyphrases bit-equal to the interval walk, normalized and -d."""
    if "_seg" in suffix_sort_path:
        pytest.skip("one document: nothing to segment (the same build as the path without _seg)")
    _three_paths(request, "window_sort_unfused", "window_sort_ht", "window_sort_ht_unfused")
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 2)
    _, sym, m = synthetic.word_stream_document(rng, 64 << 20, want_text=False)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([m]))
    qs, qo = synthetic.keyphrases(rng, sym, 1000)
    table = index.score_table(qs, qo, True)
    _check_index(oracle, index, sym, [0, sym.size], [m], scores=(qs, qo, {True: table, False: index.score_table(qs, qo, False)}))
    assert table.shape == (1000, 1) and (table >= 0).all() and (table <= 1).all()
    assert (table[0::2] > 0).all()                               # keyphrases copied from the text match
    # idempotence: rebuilding and rescoring gives the same bits
    index.build(sym, np.array([0, sym.size]), np.array([m]))
    assert np.array_equal(index.score_table(qs, qo, True), table)


def test_256_documents_batched_equals_individual(hip):
    """BASELINE configs[2] shape (many 1 MiB documents in one batched build), reduced to 24
    documents: every per-document table equals a build of that document alone."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 3)
    docs = [synthetic.word_stream_document(rng, 1 << 20, want_text=False)[1:] for _ in range(24)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    ms = np.array([d[1] for d in docs])
    batch = hip_backend.HipIndex()
    batch.build(sym, off, ms)
    qs, qo = synthetic.keyphrases(rng, sym, 300)
    table = batch.score_table(qs, qo, True)
    single = hip_backend.HipIndex()
    for d in (0, 7, 23):
        single.build(docs[d][0], np.array([0, docs[d][0].size]), np.array([docs[d][1]]))
        tb, ts = batch.tables(d), single.tables(0)
        for name in TABLES:
            assert np.array_equal(tb[name], ts[name]), (name, d)
        assert np.array_equal(single.score_table(qs, qo, True)[:, 0], table[:, d])


def test_config2_256_documents_10000_keyphrases_vs_oracle(hip, oracle, request, suffix_sort_path):
    """BASELINE configs[2] at its full size: 256 word-stream documents of 1 MiB (text mode) and
    10 000 keyphrases in ONE batched build + ONE score call.  Every document: all six tables and the lcp-interval
    lefts checked in full against their definitions, every tenth keyphrase bit-equal to the interval walk; 8 sampled
    documents: all six tables array_equal to the oracle and all 10 000 scores bit-equal, normalized and denormalized
    (applications.py:43-52)."""
    # (by its size this shard takes the segmented sort on every window-sort path: the `_seg` paths would repeat the others --
    # one of them runs with the document number in the keys instead, the other two are skipped at this size)
    if suffix_sort_path in ("window_sort_seg_unfused", "window_sort_seg_ht"):
        pytest.skip("the same builds as window_sort_unfused / window_sort_ht at this size")
    _three_paths(request, "window_sort_unfused", "window_sort_ht", "window_sort_ht_unfused", "window_sort_seg")
    if suffix_sort_path == "window_sort_seg":
        assert hip.load().east_hip_debug_set_segmented_sort(0) == 0      # (the autouse fixture restores the default)
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 3)
    docs = [synthetic.word_stream_document(rng, 1 << 20, want_text=False)[1:] for _ in range(256)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    ms = np.array([d[1] for d in docs], dtype=np.int32)
    index = hip_backend.HipIndex()
    index.build(sym, off, ms)
    assert index.info()["n_docs"] == 256 and index.info()["n_total"] == sym.size
    qs, qo = synthetic.keyphrases(rng, sym, 10000)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    assert tables[True].shape == (10000, 256)
    _check_index(oracle, index, sym, off, ms, scores=(qs, qo, tables, np.arange(0, 10000, 10)))
    sampled = [0, 1, 37, 100, 128, 199, 254, 255]
    for d in sampled:
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for norm in (True, False):
            want = np.array([o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True) for k in range(10000)])
            assert np.array_equal(tables[norm][:, d], want), (d, norm)
        if d == 37:     # ... and the reference's own walk over the sibling chains (easa.py:91-139, not the interval walk) on 200 of them
            for k in range(0, 10000, 50):
                assert tables[True][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=False), (d, k)
    # every keyphrase copied from a document scores > 0 there (keyphrases() takes the even ones from the corpus)
    assert (tables[True].max(axis=1)[0::2] > 0).all()


class _Synonimizer(object):
    def __init__(self, mapping):
        self.mapping = mapping

    def get_synonyms(self):
        return self.mapping


def test_traversals_vs_reference_fixture(hip):
    """AST.traverse() (base.py:28-34 -> easa.py:38-85): the visits in pre- and post-order, leaves and
    the nested children lists included, as recorded from the reference."""
    from east import consts
    from east.asts import base
    for case in load_golden("traversal_synonyms.json")["traversals"]:
        ast = base.AST.get_ast(case["strings"])
        pre, post = [], []
        ast.traverse(pre.append, consts.TraversalOrder.DEPTH_FIRST_PRE_ORDER)
        ast.traverse(post.append, consts.TraversalOrder.DEPTH_FIRST_POST_ORDER)
        assert [[v[0], v[1], v[2], ord(v[3]) if v[3] else -1] for v in pre] == case["pre_order"], case["strings"]
        assert type(pre[0]) is list and all(type(v) is tuple for v in pre[1:])     # easa.py:45, 363-376
        assert [[v[0], v[1], v[2], [c[:3] for c in v[3]]] for v in post] == case["post_order"], case["strings"]
        assert post[-1] == case["root_nested"]
        ast.traverse(pre.append)                                                    # default order: pre-order
        assert len(pre) == 2 * len(case["pre_order"])
        with pytest.raises(NotImplementedError):
            ast.traverse(post.append, consts.TraversalOrder.BREADTH_FIRST)


def test_traversals_of_the_documents_of_a_measure(hip):
    """measure.asts[d] (relevance.py:41-47) offers the same traverse() as a stand-alone AST: all fixture
    collections as the documents of ONE batched build, built from strings and from raw texts."""
    from east import consts, relevance
    cases = load_golden("traversal_synonyms.json")["traversals"]
    measure = relevance.ASTRelevanceMeasure()
    measure.set_strings_collections([c["strings"] for c in cases])
    for d, case in enumerate(cases):
        pre, post = [], []
        measure.asts[d].traverse(pre.append)
        measure.asts[d].traverse(post.append, consts.TraversalOrder.DEPTH_FIRST_POST_ORDER)
        assert [[v[0], v[1], v[2], ord(v[3]) if v[3] else -1] for v in pre] == case["pre_order"], case["strings"]
        assert post[-1] == case["root_nested"]
    measure.set_text_collection([b"xabxac hi", b"abcd efg ops xyzq test"])
    post = []
    measure.asts[0].traverse(post.append, consts.TraversalOrder.DEPTH_FIRST_POST_ORDER)
    pre = []
    measure.asts[0].traverse(pre.append)
    assert post[-1][:3] == [0, 0, len([v for v in pre if v[1] == v[2]]) - 1]
    assert "".join(v[3] for v in pre if v[1] == v[2] and ord(v[3] or " ") < 0x0A00) != ""


def test_traversal_of_a_large_document_vs_lcp_scan(hip, oracle):
    """64 KiB word-stream document: the post-order visits equal a plain stack scan over the oracle's
    LCP table (Kasai et al. 2001), the pre-order visits cover every rank exactly once as a leaf."""
    from east import utils
    from east.asts import base
    rng = np.random.default_rng(31)
    strings = utils.text_to_strings_collection(word_stream(rng, 64 << 10))
    ast = base.AST.get_ast(strings)
    lcp = oracle.OracleEASA(strings).lcptab
    want, stack = [], [(0, 0)]
    for r in range(1, len(lcp)):
        lb = r - 1
        while lcp[r] < stack[-1][0]:
            l, lb = stack.pop()
            want.append((l, lb, r - 1))
        if lcp[r] > stack[-1][0]:
            stack.append((int(lcp[r]), lb))
    want.append((0, 0, len(lcp) - 1))
    post, pre = [], []
    ast.traverse_depth_first_post_order(lambda v: post.append((v[0], v[1], v[2])))
    assert post == want
    ast.traverse_depth_first_pre_order(pre.append)
    assert sorted(v[1] for v in pre if v[1] == v[2]) == list(range(len(lcp)))
    assert sorted((v[0], v[1], v[2]) for v in pre if v[1] != v[2]) == sorted(want)


def test_synonym_expanded_scores_vs_reference_fixture(hip):
    """easa.py:27-34 on the AST surface and on the measure / table path (relevance.py:51-53,
    applications.py:43-52): extra queries + a segmented max on the device; `normalized` is ignored
    under a synonimizer, as in the reference."""
    from east import applications, relevance, utils
    from east.asts import base
    g = load_golden("traversal_synonyms.json")
    for case in g["synonym_scores"]:
        ast = base.AST.get_ast(case["strings"])
        syn = _Synonimizer(case["synonyms"])
        for norm in (True, False):
            got = ast.score(case["query"], normalized=norm, synonimizer=syn)
            assert got == case["score"] and abs(got - case["score"]) <= TOL, (case["strings"], case["query"])
    for case in g["synonym_tables"]:
        texts = {k: v.encode("utf-8") for k, v in case["texts"].items()}
        syn = _Synonimizer(case["synonyms"])
        measure = relevance.ASTRelevanceMeasure("easa", case["normalized"])
        table = applications.keyphrases_table(case["keyphrases"], texts, measure, syn)
        _table_equal(table, case["table"])
        names = list(texts)
        for kp in case["keyphrases"]:                      # the per-pair surface and the per-document AST views
            for j, name in enumerate(names):
                assert measure.relevance(utils.prepare_text(kp), j, synonimizer=syn) == case["table"][kp][name]
                assert measure.asts[j].score(utils.prepare_text(kp), synonimizer=syn) == case["table"][kp][name]
        total, suffixes = measure.asts[0].score("QUICK FOX", normalized=case["normalized"], return_suffix_scores=True)
        assert total == measure.relevance("QUICK FOX", 0) and set(suffixes) == {"QUICKFOX"[i:] for i in range(8)}
        with pytest.raises(KeyError):
            measure.relevance("UNKNOWN WORD", 0, synonimizer=syn)


def test_keyphrases_graph_fixture(hip):
    """applications.keyphrases_graph + graph2gml / graph2edges on the HSE corpus (17 keyphrases)."""
    from east import applications, formatting, relevance
    g = load_golden("hse_graph.json")
    texts = {k: v.encode("utf-8") for k, v in load_golden(g["texts_from"])["texts"].items()}
    for case in g["cases"]:
        graph = applications.keyphrases_graph(g["keyphrases"], texts, case["referral_confidence"],
                                              case["relevance_threshold"], case["support_threshold"],
                                              relevance.ASTRelevanceMeasure("easa", True))
        assert graph == case["graph"]
        assert formatting.graph2gml(graph) == case["gml"]
        if case["edges"] is not None:
            assert formatting.graph2edges(graph) == case["edges"]


def test_cli_table_and_graph(hip, tmp_path, capsys):
    """`east keyphrases table|graph` end to end (README.rst:27-63): directory mode, single-file mode,
    -d, -f csv / xml / gml."""
    from east import main
    g = load_golden("hse_config1.json")
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, text in g["texts"].items():
        (tdir / (name + ".txt")).write_bytes(text.encode("utf-8"))
    (tdir / "ignored.dat").write_text("not a text")
    kp = tmp_path / "kp.txt"
    kp.write_bytes(("\n".join(g["keyphrases"]) + "\n\n").encode("utf-8"))     # trailing empty lines are skipped
    assert main.main(["keyphrases", "table", str(kp), str(tdir)]) == 0
    assert capsys.readouterr().out == g["xml_normalized"] + "\n"
    assert main.main(["-f", "csv", "-a", "ast_linear", "keyphrases", "table", str(kp), str(tdir)]) == 0
    assert capsys.readouterr().out == g["csv_normalized"] + "\n"
    s = load_golden("sample_table.json")
    one = tmp_path / "test.txt"
    one.write_bytes("\n".join(s["texts"][k] for k in sorted(s["texts"], key=int)).encode("utf-8"))
    kp2 = tmp_path / "kp2.txt"
    kp2.write_text("\n".join(s["keyphrases"]))
    assert main.main(["-d", "keyphrases", "table", str(kp2), str(one)]) == 0
    assert capsys.readouterr().out == s["xml_denormalized"] + "\n"
    gg = load_golden("hse_graph.json")
    kp3 = tmp_path / "kp3.txt"
    kp3.write_bytes("\n".join(gg["keyphrases"]).encode("utf-8"))
    case = gg["cases"][1]
    assert main.main(["-f", "gml", "-c", str(case["referral_confidence"]), "-r", str(case["relevance_threshold"]),
                      "-p", str(case["support_threshold"]), "keyphrases", "graph", str(kp3), str(tdir)]) == 0
    assert capsys.readouterr().out == case["gml"] + "\n"


def test_natural_language_like_16mib_vs_oracle(hip, oracle):
    """BASELINE config 5 stand-in (Zipf word stream: repeated strings, LCP up to a whole string,
    deeper DC3 recursion, tie groups too large for the in-place resolve): 16 documents of 1 MiB,
    tables bit-exact and normalized + denormalized scores bit-equal against the oracle."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20245)
    vocab = synthetic.zipf_vocabulary(rng)
    docs = [synthetic.zipf_document(rng, 1 << 20, vocab) for _ in range(16)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    assert index.info()["refine_rounds"] > 0         # the tied names were refined by further windows
    qs, qo = synthetic.keyphrases(rng, sym, 200)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    for d in (0, 5, 15):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for norm in (True, False):
            for k in range(200):
                assert tables[norm][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True)
    assert float(tables[False].max()) > 1.0          # denormalized scores exceed 1 on deep matches


@pytest.mark.parametrize("seed", range(6))
def test_small_vocabulary_text_tie_refinement_vs_oracle(hip, oracle, seed):
    """Tiny vocabularies (8..200 words) make most names tie at DC3 level 0: the refinement rounds,
    the direct ordering of what is left and the recursion on refined names all get exercised.
    Suffix array + all tables bit-exact against the oracle."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(900 + seed)
    vocab = synthetic.zipf_vocabulary(rng, size=int(rng.choice([8, 30, 200])), exponent=1.0)
    docs = [synthetic.zipf_document(rng, int(rng.integers(20000, 300000)), vocab) for _ in range(3)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    for d in range(3):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d, index.info())


@pytest.mark.parametrize("lds_rounds", [1, 3, 2, 0])
@pytest.mark.parametrize("seed", range(4))
def test_refinement_rounds_in_lds_and_by_the_global_sort(hip, oracle, suffix_sort_path, seed, lds_rounds):
    """The rounds order tie groups that fit a workgroup's LDS there (csrc/lds_group_sort.h) and leave longer ones to
    the global radix sort: word text over small vocabularies gives both kinds in one domain -- groups of a few
    dozen members next to groups of tens of thousands --, single documents and several, with the in-LDS path on
    (1, the default: the in-LDS round also classifies the next domain, and a domain that fits the chip is finished by one
    persistent launch; 3: the same launch by launch; 2: with the stand-alone classification pass) and off.  All six tables
    bit-exact against the oracle, the LCP entries the rounds write included."""
    from east import hip_backend, synthetic
    lib = hip.load()
    rng = np.random.default_rng(7700 + seed)
    vocab = synthetic.zipf_vocabulary(rng, size=int(rng.choice([12, 60, 400, 3000])), exponent=1.0)
    n_docs = int(rng.choice([1, 2, 5]))
    docs = [synthetic.zipf_document(rng, int(rng.integers(100000, 700000)), vocab) for _ in range(n_docs)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    assert lib.east_hip_debug_set_lds_rounds(lds_rounds) == 0
    try:
        index = hip_backend.HipIndex()
        index.build(sym, off, np.array([d[1] for d in docs]))
        info = index.info()
        if suffix_sort_path == "window_sort":
            assert info["window_sorted"] == 1 and info["refine_rounds"] >= 1, info
            assert (info["lds_sorted"] > 0) == bool(lds_rounds), info
            assert lds_rounds == 1 or info["persist_rounds"] == 0, info       # (the persistent launch: the default only)
        if suffix_sort_path.startswith("window_sort_ht"):
            assert info["window_sorted"] == 1 and info["ht_keys"] >= 1, info      # variable-length keys really ran
            assert info["fused_finish"] == int(suffix_sort_path == "window_sort_ht"), info
        if "_seg" in suffix_sort_path:
            assert info["window_sorted"] == 1 and info["seg_sort"] == int(n_docs > 1), info   # the segmented sort really ran
        for d in range(n_docs):
            o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
            t = index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (name, d, info)
    finally:
        assert lib.east_hip_debug_set_lds_rounds(1) == 0


def test_segmented_sort_of_unequal_documents(hip, oracle, suffix_sort_path):
    """Documents of very different lengths in one shard -- two of more than 64 histogram groups (2 M suffixes: their
    spine is the column-parallel kernel), one of a few groups, one of less than a tile, one of a few symbols -- through
    the segmented first-level sort where the path or the sizes ask for it (csrc/radix_sort.h: RsSeg).  All six tables of
    every document bit-exact against the oracle."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(8642)
    vocab = synthetic.zipf_vocabulary(rng, size=2000, exponent=1.0)
    docs = [synthetic.word_stream_document(rng, 2_600_000, want_text=False)[1:], synthetic.zipf_document(rng, 40_000, vocab),
            synthetic.word_stream_document(rng, 300_000, want_text=False)[1:], synthetic.zipf_document(rng, 900, vocab),
            synthetic.zipf_document(rng, 2_300_000, vocab), synthetic.word_stream_document(rng, 12, want_text=False)[1:]]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    for _ in range(2):                                   # (the second build is the speculative one)
        index.build(sym, off, np.array([d[1] for d in docs]))
        info = index.info()
        if suffix_sort_path in ("window_sort", "window_sort_seg", "window_sort_seg_unfused"):
            assert info["window_sorted"] == 1 and info["seg_sort"] == 1, info     # (by size, too: 6 documents, 160 groups)
        for d in range(len(docs)):
            o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
            t = index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (name, d, info)


@pytest.mark.parametrize("document_number_in_keys", [False, True])
def test_first_build_plans_the_window_from_its_own_text(hip, oracle, suffix_sort_path, document_number_in_keys):
    """The first build on a fresh handle takes the window width and the fused finish from a sample of its own text
    (csrc/alphabet.h: sample_prefix_kernel) -- no build has to go before: natural-language-like text over a large
    alphabet (most suffixes tied behind the three symbols that fit a 32-bit key) sorts 64-bit first-level keys at once,
    a random word stream 32-bit keys with the last digit ordered in LDS; a second build on the handle (queued without
    waiting, no sample) does as the first.  The tables are the oracle's either way."""
    from east import hip_backend, synthetic
    if document_number_in_keys:                          # (the plan without the segmented sort; the autouse fixture restores the default)
        assert hip.load().east_hip_debug_set_segmented_sort(0) == 0
    rng = np.random.default_rng(4711)
    vocab = synthetic.zipf_vocabulary(rng, size=40, exponent=1.0)
    docs = [synthetic.zipf_document(rng, 400000, vocab) for _ in range(2)]
    sym = np.concatenate([d[0] for d in docs])
    # (more than 63 distinct symbols: 7 bits each, 3 symbols in a 32-bit key next to the document number)
    extra = np.arange(0x100, 0x100 + 70, dtype=np.uint32)
    text_pos = np.flatnonzero(sym < 0x0A00)
    sym[text_pos[rng.integers(0, text_pos.size, size=2000)]] = extra[rng.integers(0, extra.size, size=2000)]
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    m = np.array([d[1] for d in docs])
    index = hip_backend.HipIndex()
    index.build(sym, off, m)
    first = index.info()
    index.build(sym, off, m)
    second = index.info()
    if suffix_sort_path == "window_sort":
        assert first["window_sorted"] == 1 and second["window_sorted"] == 1
        if first["seg_sort"]:
            # two large documents sorted each inside its own range: all 32 key bits are text, and this text (a few symbols
            # make up most of it) gets variable-length code words into them -- both builds
            assert not document_number_in_keys and second["seg_sort"] == 1
            assert first["ht_keys"] == 1 and second["ht_keys"] == 1, (first, second)
        else:
            assert first["radix_passes_u32"] == 0 and second["radix_passes_u32"] == 0, (first, second)   # 64-bit first-level keys at once
    for d in range(2):
        o = oracle.OracleEASA(symbols=sym[off[d]:off[d + 1]], n_strings=int(m[d]))
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d, second)
    # a random word stream on a fresh handle: the narrow window, and (unless switched off) the fused finish
    docs = [synthetic.word_stream_document(rng, 300000, want_text=False)[1:] for _ in range(2)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    m = np.array([d[1] for d in docs])
    index = hip_backend.HipIndex()
    for _ in range(2):
        index.build(sym, off, m)
        info = index.info()
        if suffix_sort_path == "window_sort":
            assert info["radix_passes_u64"] == 0 and info["refine_rounds"] == 0, info
            assert info["fused_finish"] == int(_CURRENT["knob"] == 1), info
    for d in range(2):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


def test_plan_follows_the_text_on_one_handle(hip, oracle, suffix_sort_path):
    """A handle whose kind of text changes: the plan a speculative build takes over from the build before (wide window,
    fused finish) is dropped when that build's own counts say it was made for other text -- a random word stream after
    natural-language-like text fuses the end of its sort again after one build, not never.  Tables bit-exact throughout."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(909)
    vocab = synthetic.zipf_vocabulary(rng, size=300, exponent=1.0)

    def collection(kind):
        if kind == "words":
            docs = [synthetic.word_stream_document(rng, 300000, want_text=False)[1:] for _ in range(2)]
        else:
            docs = [synthetic.zipf_document(rng, 400000, vocab) for _ in range(2)]
        return (docs, np.concatenate([d[0] for d in docs]), np.concatenate([[0], np.cumsum([d[0].size for d in docs])]),
                np.array([d[1] for d in docs]))

    index = hip_backend.HipIndex()
    fused = []
    for kind in ("words", "zipf", "words", "words", "words"):
        docs, sym, off, m = collection(kind)
        index.build(sym, off, m)
        info = index.info()
        fused.append(info["fused_finish"])
        for d in range(2):
            o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
            t = index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (kind, name, d, info)
    if suffix_sort_path == "window_sort" and _CURRENT["knob"] == 1:
        assert fused[0] == 1 and fused[-1] == 1, fused        # back to the fused finish once the text is a word stream again


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_build_from_resident_symbols_at_any_alignment(hip, oracle, shift):
    """east_hip_build_device on a symbol array that starts 0..3 words into a device buffer (a view of
    a larger tensor is only 4-byte aligned): the 16-byte fast paths must not be taken blindly."""
    import torch
    from east import hip_backend, synthetic
    rng = np.random.default_rng(31 + shift)
    sym, m = synthetic.word_stream_document(rng, 50001 + shift, want_text=False)[1:]
    buf = torch.zeros(sym.size + 8, dtype=torch.int32, device="cuda:0")
    buf[shift:shift + sym.size] = torch.from_numpy(sym.astype(np.int32)).to(buf.device)
    view = buf[shift:shift + sym.size]
    assert view.data_ptr() % 16 == (4 * shift) % 16
    index = hip_backend.HipIndex()
    index.build_device(view.data_ptr(), sym.size, np.array([0, sym.size]), np.array([m]))
    o = oracle.OracleEASA(symbols=sym, n_strings=m)
    t = index.tables(0)
    for name in TABLES:
        assert np.array_equal(t[name], getattr(o, name)), name


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049, 3073, 65535, 65536, 65537, 66560, 70001])
def test_sizes_around_the_stretches_of_the_placement_pass(hip, oracle, n):
    """The fused finish works on stretches of 1 024 ranks with a halo to either side; the separate placement pass on
    stretches of 1 024 as well: symbol counts right at, just below and just above multiples of the stretch, on both
    sides of the 65 536-symbol border between the small-input limits and the ordinary ones, over a small alphabet (many
    ties, buckets that run across stretch borders) -- all six tables against the oracle."""
    from east import hip_backend
    rng = np.random.default_rng(n)
    for sigma, mean_len in ((3, 9), (20, 5)):
        # strings of random letters until n symbols are used up exactly (terminators included)
        parts, used, i = [], 0, 0
        while used < n:
            ln = int(min(max(1, rng.geometric(1.0 / mean_len)), n - used - 1)) if n - used > 1 else 0
            parts.append(rng.integers(65, 65 + sigma, size=ln, dtype=np.uint32))
            parts.append(np.array([0x0A00 + i], dtype=np.uint32))
            used += ln + 1
            i += 1
        sym = np.concatenate(parts)
        assert sym.size == n
        index = hip_backend.HipIndex()
        index.build(sym, np.array([0, n]), np.array([i]))
        o = oracle.OracleEASA(symbols=sym, n_strings=i)
        t = index.tables(0)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, n, sigma, index.info())


@pytest.mark.parametrize("seed", range(3))
def test_fused_finish_on_skewed_text(hip, oracle, seed):
    """The fused finish forced (knob 6) on text it is not planned for: natural-language-like documents with planted
    repeats, whose top-part buckets hold hundreds of suffixes -- they are handed to the refinement rounds as tie groups at the
    depth of the top part, the k-gram marks are found incomplete and the score side builds its own tables.  Tables and
    scores are the oracle's."""
    from east import hip_backend, synthetic
    assert hip.load().east_hip_debug_set_window_sort(6) == 0          # (the autouse fixture restores the default)
    rng = np.random.default_rng(8800 + seed)
    vocab = synthetic.zipf_vocabulary(rng, size=int(rng.choice([30, 400])), exponent=1.0)
    docs = [synthetic.zipf_document(rng, int(rng.integers(120000, 400000)), vocab) for _ in range(1 + seed)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    ms = np.array([d[1] for d in docs])
    index = hip_backend.HipIndex()
    index.build(sym, off, ms)
    info = index.info()
    assert info["fused_finish"] == 1 and info["window_sorted"] == 1 and info["refine_rounds"] >= 1, info
    queries = []
    for d in range(len(docs)):
        text = docs[d][0]
        for _ in range(6):
            a = int(rng.integers(0, text.size - 40))
            q = text[a:a + int(rng.integers(3, 30))]
            q = q[q < 0x0A00]
            if q.size:
                queries.append(q)
    qs = np.concatenate(queries)
    qo = np.concatenate([[0], np.cumsum([q.size for q in queries])])
    for normalized in (True, False):
        table = index.score_table(qs, qo, normalized)
        for d in range(len(docs)):
            o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
            if normalized:
                t = index.tables(d)
                for name in TABLES:
                    assert np.array_equal(t[name], getattr(o, name)), (name, d, info)
            for k, q in enumerate(queries):
                assert table[k, d] == o.score_symbols(q, normalized, fast=True), (k, d, normalized)


@pytest.mark.parametrize("knob", [3, 5])
@pytest.mark.parametrize("seed", range(4))
def test_wide_window_keys_on_small_inputs(hip, oracle, seed, knob):
    """Inputs of several hundred million symbols sort 64-bit window keys (separate key and element
    arrays, other kernel instantiations); forced here on small texts with few and with many ties, one
    and several documents, so that placement, refinement rounds and LCP-from-keys run on 64-bit keys."""
    from east import hip_backend, synthetic
    assert hip.load().east_hip_debug_set_window_sort(knob) == 0       # (the autouse fixture restores the default; 5: no fused finish)
    rng = np.random.default_rng(4100 + seed)
    if seed % 2 == 0:
        vocab = synthetic.zipf_vocabulary(rng, size=int(rng.choice([12, 300])), exponent=1.0)
        docs = [synthetic.zipf_document(rng, int(rng.integers(30000, 200000)), vocab) for _ in range(1 + seed)]
    else:
        docs = [synthetic.word_stream_document(rng, int(rng.integers(30000, 200000)), want_text=False)[1:]
                for _ in range(seed)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    assert index.info()["radix_elements_u64"] > 0
    for d in range(len(docs)):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


@pytest.mark.parametrize("case", ["one_document", "three_documents"])
def test_long_repeats_in_large_groups(hip, oracle, case):
    """Twenty copies of a 400-symbol string: tie groups larger than the direct ordering takes, with
    common prefixes far longer than a symbol window.  All-suffix mode: the rounds switch to prefix
    doubling and finish; DC3's sample sort works them off by symbol windows (or recurses on the refined names)."""
    from east import hip_backend
    from east.asts import utils as ast_utils
    rng = np.random.default_rng(8)
    blob = "".join(rng.choice(list("ABCDEFG"), size=400))
    filler = lambda k: "".join(rng.choice(list("ABCDEFG"), size=k))
    # (more than 65 536 sample suffixes: smaller inputs skip the rounds and order groups of up to 128 directly)
    doc = [blob + filler(int(rng.integers(1, 30))) for _ in range(20)] + [filler(120000)]
    docs = [doc] if case == "one_document" else [doc, [filler(3000), blob * 3], doc[:7]]
    parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
    index = hip_backend.HipIndex()
    index.build(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]),
                np.array([len(sc) for sc in docs]))
    info = index.info()
    assert info["refine_rounds"] > 0, info
    for d, sc in enumerate(docs):
        o = oracle.OracleEASA(sc)
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


# word-wise re-spellings of a-z in accented Latin, Greek and Cyrillic letters (all below the terminator base U+0A00)
_RESPELL = [str.maketrans("abcdefghijklmnopqrstuvwxyz", t) for t in
            ("\u00e1\u0180\u00e7\u0111\u00e9\u0192\u011f\u0125\u00ed\u0135\u0137\u0142m\u00f1\u00f3\u01a5q\u0155\u015f\u0163\u00fav\u0175x\u00fd\u017e",
             "\u03b1\u03b2\u03c8\u03b4\u03b5\u03c6\u03b3\u03b7\u03b9\u03be\u03ba\u03bb\u03bc\u03bd\u03bf\u03c0\u03b8\u03c1\u03c3\u03c4\u03c5\u03c9\u03c2\u03c7\u03c5\u03b6",
             "\u0430\u0431\u0446\u0434\u0435\u0444\u0433\u0445\u0438\u0439\u043a\u043b\u043c\u043d\u043e\u043f\u044f\u0440\u0441\u0442\u0443\u0436\u0432\u044c\u044b\u0437")]


def _prose_stand_in(n_bytes, seed=31):
    """Natural-language text of about n_bytes (UTF-8) for the real-prose cases, made from what the repository holds: the
    order-3 character model of east/synthetic.py (English letter statistics, digits, punctuation, capitals), one word in
    eight respelt in accented Latin, Greek or Cyrillic letters (a mixed alphabet of about a hundred symbols, as in
    documentation written in many languages), and passages of a few KB that recur throughout (boilerplate repeated
    across files).  The same bytes on every machine."""
    from east import synthetic
    rng = np.random.default_rng(seed)
    words = b"".join(synthetic.prose_like_texts(rng, 8, n_bytes // 8)).decode("ascii").split(" ")
    pick = rng.random(len(words))
    for k, table in enumerate(_RESPELL):
        for i in np.flatnonzero((pick >= k / 24.0) & (pick < (k + 1) / 24.0)):
            words[i] = words[i].translate(table)
    text = " ".join(words)
    passages = [text[int(s):int(s) + int(rng.integers(4096, 16384))] for s in rng.integers(0, len(text) // 2, size=8)]
    parts, pos = [], 0
    for cut in np.sort(rng.integers(0, len(text), size=48)):
        parts += [text[pos:int(cut)], passages[int(rng.integers(0, len(passages)))]]
        pos = int(cut)
    parts.append(text[pos:])
    return "\n".join(parts).encode("utf-8")[:n_bytes]


def test_real_prose_from_the_image(hip, oracle):
    """BASELINE config 5 on text with the traits of real natural language (_prose_stand_in: mixed alphabet of ~100
    symbols, most suffixes tied after the first window, boilerplate repeated across files).  Device text preparation
    + build of 0.5 MiB documents; tables of two documents bit-exact and the scores of 40 keyphrases bit-equal against
    the oracle."""
    from east import hip_backend, synthetic
    raw = _prose_stand_in(3 << 20)
    step = 1 << 19
    texts = [raw[i:i + step] for i in range(0, len(raw), step)]
    hip_backend.unicode_tables()
    index = hip_backend.HipIndex()
    index.build_texts(texts)
    info = index.info()
    assert info["sigma_text"] > 40 and info["refine_rounds"] > 0, info
    sym, off, ms = index.prepared()
    rng = np.random.default_rng(5)
    qs, qo = synthetic.keyphrases(rng, sym[off[0]:off[1]], 40)
    table = index.score_table(qs, qo, True)
    for d in (0, len(texts) - 1):
        o = oracle.OracleEASA(symbols=sym[off[d]:off[d + 1]], n_strings=int(ms[d]))
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for k in range(40):
            assert table[k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=True), (k, d)


@pytest.mark.parametrize("sigma", [33, 64, 130, 254])
def test_byte_stream_alphabet_sizes_vs_oracle(hip, oracle, sigma):
    """The byte stream serves text alphabets of up to 254 symbols: 6-, 7- and 8-bit window fields, no spare
    key bits at 8 bits per symbol, the terminator class as code 255 at sigma = 254.  Random and
    repetitive strings over `sigma` code points; tables bit-exact, scores bit-equal."""
    from east import hip_backend
    from east.asts import utils as ast_utils
    rng = np.random.default_rng(1000 + sigma)
    alphabet = [chr(0x0100 + i) for i in range(sigma)]
    docs = []
    for d in range(3):
        strings = ["".join(rng.choice(alphabet, size=int(rng.integers(1, 40)))) for _ in range(int(rng.integers(5, 400)))]
        strings += [strings[0]] * 12 + [strings[-1] + strings[0]]          # repeats: large tie groups
        docs.append(strings)
    docs[0] = ["".join(alphabet)] + docs[0]                                 # every symbol occurs
    parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
    index = hip_backend.HipIndex()
    index.build(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]),
                np.array([len(sc) for sc in docs]))
    assert index.info()["sigma_text"] == sigma
    queries = [docs[0][1][:5], docs[1][0], alphabet[3] + alphabet[7], docs[2][-1][2:]]
    qs, qo = hip_backend.pack_queries([q for q in queries if q])
    table = index.score_table(qs, qo, True)
    for d, sc in enumerate(docs):
        o = oracle.OracleEASA(sc)
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for k, q in enumerate([q for q in queries if q]):
            assert table[k, d] == o.score(q, fast=True), (d, k)


@pytest.mark.parametrize("case", ["two_documents_alike", "passage_repeated_in_one_document", "three_copies"])
def test_duplicated_passages_stay_on_the_window_sort(hip, oracle, case):
    """Duplicates -- a document that occurs twice, a long passage that occurs twice or three times --
    leave pairs / triples of suffixes that agree for thousands of symbols: too long to compare
    directly, too few to be a large group.  Such groups are marked and handed to the prefix-doubling
    rounds instead of giving the whole input up to DC3."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(91)
    a = synthetic.direct_document(rng, 70000)[0][:-1]
    b = synthetic.direct_document(rng, 50000)[0][:-1]
    c = synthetic.direct_document(rng, 90000)[0][:-1]
    term = lambda k: np.array([0x0A00 + k], dtype=np.uint32)
    if case == "two_documents_alike":
        docs = [np.concatenate([a, term(0)]), np.concatenate([b, term(0)]), np.concatenate([a, term(0)])]
    elif case == "passage_repeated_in_one_document":
        docs = [np.concatenate([c[:30000], a[:20000], c[30000:], a[:20000], b[:100], term(0)])]
    else:
        docs = [np.concatenate([a[:9000], b, a[:9000], c, a[:9000], term(0)])]
    sym = np.concatenate(docs)
    off = np.concatenate([[0], np.cumsum([d.size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.ones(len(docs), dtype=np.int32))
    info = index.info()
    if info["dc3_levels"] == 0:
        # (two documents alike: with the document number in the key their suffixes never meet -- no rounds at all)
        assert info["window_sorted"] == 1 and (info["refine_rounds"] > 0 or case == "two_documents_alike"), info
    for d in range(len(docs)):
        o = oracle.OracleEASA(symbols=docs[d], n_strings=1)
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


def test_recycled_handles_behave_like_new_ones(hip):
    """hip_backend keeps the handles of small indexes in a pool (create + destroy cost more than a small
    build).  A recycled handle must have forgotten index, keyphrases and prepared texts."""
    from east import exceptions, hip_backend
    from east.asts import utils as ast_utils
    a = hip_backend.HipIndex()
    sym = ast_utils.strings_to_symbols(["XABXAC", "BABXAC"])
    a.build(sym, np.array([0, sym.size]), np.array([2]))
    q = ast_utils.query_to_symbols("ABX")
    first = a.score_table(q, np.array([0, q.size]), True)[0, 0]
    a.set_keyphrases(q, np.array([0, q.size]))
    a.close()
    a.close()                                            # idempotent
    assert hip_backend._handle_pool[a.device], "a small handle should have been pooled"
    b = hip_backend.HipIndex()
    assert not hip_backend._handle_pool[b.device] or len(hip_backend._handle_pool[b.device]) < hip_backend.POOL_HANDLES
    with pytest.raises(exceptions.HipBackendError):      # nothing built yet on the recycled handle
        b.score_table(q, np.array([0, q.size]), True)
    with pytest.raises(exceptions.HipBackendError):
        b.tables(0)
    b.build(sym, np.array([0, sym.size]), np.array([2]))
    with pytest.raises(exceptions.HipBackendError):      # the keyphrases of the previous owner are gone
        out = np.zeros((1, 1))
        b.score_resident(True, out.ctypes.data)
    assert b.score_table(q, np.array([0, q.size]), True)[0, 0] == first
    with pytest.raises(exceptions.HipBackendError):      # a closed index refuses work
        a.build(sym, np.array([0, sym.size]), np.array([2]))


@pytest.mark.parametrize("wide_keys", [False, True])
@pytest.mark.parametrize("corpus", ["word_stream", "small_vocabulary", "real_prose"])
def test_resident_build_fits_the_planned_arena(hip, corpus, wide_keys):
    """east_hip_build_device has no staging area behind the planned arena: the sizing run must cover the
    real run exactly, also with 64-bit window keys, refinement rounds, prefix doubling and several
    documents (a transient of the rounds was once priced below a buffer allocated after it)."""
    import torch
    from east import hip_backend, synthetic
    rng = np.random.default_rng(17)
    if corpus == "word_stream":
        docs = [synthetic.word_stream_document(rng, 1 << 21, want_text=False)[1:] for _ in range(2)]
    elif corpus == "small_vocabulary":
        vocab = synthetic.zipf_vocabulary(rng, size=300, exponent=1.0)
        docs = [synthetic.zipf_document(rng, 1 << 20, vocab) for _ in range(3)]
    else:
        raw = _prose_stand_in(3 << 20)
        prep = hip_backend.HipIndex()
        prep.build_texts([raw[: len(raw) // 2], raw[len(raw) // 2:]])
        sym, off, ms = prep.prepared()
        docs = [(sym[off[d]:off[d + 1]], int(ms[d])) for d in range(2)]
    if wide_keys:
        assert hip.load().east_hip_debug_set_window_sort(3) == 0      # (the autouse fixture restores the default)
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    d_sym = torch.from_numpy(sym.astype(np.int32)).to("cuda:0")
    index = hip_backend.HipIndex()
    index.build_device(d_sym.data_ptr(), sym.size, off, np.array([d[1] for d in docs]))
    info = index.info()
    plan = hip.load().east_hip_plan_arena_bytes(sym.size, len(docs))
    assert info["arena_high_water"] <= plan and info["arena_bytes"] >= info["arena_high_water"], info
    t = index.tables(0, names=("suftab",))["suftab"]
    assert int(t.sum()) == docs[0][0].size * (docs[0][0].size - 1) // 2       # a permutation of the document's positions


def test_config5_zipf_100_documents_full_size(hip, oracle, request, suffix_sort_path):
    """BASELINE config 5 stand-in at its full size (enwik8 is not available offline): 100 natural-language-like
    documents of 1 MiB (Zipf vocabulary, 94 M symbols, tie-refinement rounds), one batched build.  Every document:
    all six tables and the lcp-interval lefts checked in full against their definitions, the 400 scores bit-equal to
    the interval walk, normalized and -d; 6 sampled documents: tables array_equal to the oracle, scores bit-equal to its
    walks (the oracle itself is pinned to ast_linear on the zipf_docs fixture)."""
    # (by its size this shard takes the segmented sort on every window-sort path: the `_seg` paths would repeat the others --
    # one of them runs with the document number in the keys instead, the other two are skipped at this size)
    if suffix_sort_path in ("window_sort_seg_unfused", "window_sort_seg_ht"):
        pytest.skip("the same builds as window_sort_unfused / window_sort_ht at this size")
    _three_paths(request, "window_sort_unfused", "window_sort_ht", "window_sort_ht_unfused", "window_sort_seg")
    if suffix_sort_path == "window_sort_seg":
        assert hip.load().east_hip_debug_set_segmented_sort(0) == 0      # (the autouse fixture restores the default)
    from east import hip_backend, synthetic
    rng = np.random.default_rng(20240 + 5)
    vocab = synthetic.zipf_vocabulary(np.random.default_rng(20245))
    docs = [synthetic.zipf_document(rng, 1 << 20, vocab) for _ in range(100)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs], dtype=np.int32))
    qs, qo = synthetic.keyphrases(rng, sym, 400)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    _check_index(oracle, index, sym, off, [d[1] for d in docs], scores=(qs, qo, tables))
    for d in (0, 17, 42, 63, 98, 99):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for norm in (True, False):
            want = np.array([o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True) for k in range(400)])
            assert np.array_equal(tables[norm][:, d], want) and np.abs(tables[norm][:, d] - want).max() <= TOL, (d, norm)
        if d == 42:     # ... and the reference's own walk over the sibling chains (easa.py:91-139) on half of them, normalized and -d
            for norm in (True, False):
                for k in range(0, 400, 2):
                    assert tables[norm][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=False), (d, k, norm)


def test_config5_prose_like_100_documents_full_size(hip, oracle, request):
    """BASELINE config 5, the second stand-in at full size: 100 documents of 1 MiB of prose-like text (the order-3
    character model of east/synthetic.py: English letter statistics, frequent words and word pairs -- the text class
    whose build goes through variable-length keys and prefix-doubling rounds) from raw bytes through the device text
    preparation; four sampled documents: the prepared symbols equal the host chain's, all six tables array_equal to the
    oracle, 300 keyphrases bit-equal in both modes (the oracle is pinned to ast_linear on prose_like_docs.json)."""
    _only_paths(request, "window_sort", "window_sort_ht_unfused", "dc3_only", "window_sort_seg")
    from east import hip_backend, synthetic, utils
    from east.asts import utils as ast_utils
    texts = synthetic.prose_like_texts(np.random.default_rng(20240 + 5), 100, 1 << 20)
    index = hip_backend.HipIndex()
    index.build_texts(texts)
    sym, off, ms = index.prepared()
    assert index.info()["n_docs"] == 100 and off[-1] == sym.size
    rng = np.random.default_rng(9)
    qs, qo = synthetic.keyphrases(rng, sym, 300)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    assert (tables[True].max(axis=1)[0::2] > 0).all()
    for d in (0, 41, 77, 99):
        want = ast_utils.strings_to_symbols(utils.text_to_strings_collection(texts[d]))
        assert np.array_equal(sym[off[d]:off[d + 1]], want), d
        o = oracle.OracleEASA(symbols=want, n_strings=int(ms[d]))
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for norm in (True, False):
            got = tables[norm][:, d]
            ref = np.array([o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True) for k in range(300)])
            assert np.array_equal(got, ref), (d, norm)
        for k in range(0, 300, 15):
            assert tables[True][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=False), (d, k)


def test_speculative_builds_on_one_handle(hip, oracle):
    """Builds after the first on a handle are queued without waiting for the device (alphabet size, "no large
    tie groups" taken from the build before) and checked by one read-back at the end: a right guess and
    every kind of wrong guess must give the same tables as the oracle."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(77)
    vocab = synthetic.zipf_vocabulary(rng, size=200, exponent=1.0)
    inputs = []
    inputs.append(synthetic.word_stream_document(rng, 300000, want_text=False)[1:])        # first build: no guess
    inputs.append(synthetic.word_stream_document(rng, 300000, want_text=False)[1:])        # right guess
    inputs.append(synthetic.zipf_document(rng, 300000, vocab))                             # wrong: tie groups need rounds
    inputs.append(synthetic.word_stream_document(rng, 200000, want_text=False)[1:])        # (after rounds: no guess)
    sym5 = rng.integers(65, 70, size=150001, dtype=np.uint32)                              # wrong: 5-letter alphabet
    sym5[-1] = 0x0A00
    inputs.append((sym5, 1))
    inputs.append(synthetic.word_stream_document(rng, 100000, want_text=False)[1:])
    rep = np.tile(np.array([65, 66, 67], dtype=np.uint32), 40000)                          # wrong: long repeats
    inputs.append((np.concatenate([rep, [0x0A00]]).astype(np.uint32), 1))
    index = hip_backend.HipIndex()
    for i, (sym, m) in enumerate(inputs):
        index.build(sym, np.array([0, sym.size]), np.array([m]))
        o = oracle.OracleEASA(symbols=sym, n_strings=m)
        t = index.tables(0)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (i, name)
    # the same sequence with the read-backs in place gives the same build facts
    lib = hip.load()
    assert lib.east_hip_debug_set_speculation(0) == 0
    try:
        sym, m = inputs[1]
        index.build(sym, np.array([0, sym.size]), np.array([m]))
        assert np.array_equal(index.tables(0)["suftab"], oracle.OracleEASA(symbols=sym, n_strings=m).suftab)
    finally:
        assert lib.east_hip_debug_set_speculation(1) == 0


def test_lean_build_without_refinement_rounds(hip, oracle):
    """When the buffers of the tie-refinement rounds do not fit the device, the build runs without
    them: heavy ties go straight to the DC3 recursion.  Forced here on a small-vocabulary text."""
    from east import hip_backend, synthetic
    assert hip.load().east_hip_debug_set_window_sort(2) == 0          # (the autouse fixture restores the default)
    rng = np.random.default_rng(77)
    vocab = synthetic.zipf_vocabulary(rng, size=40, exponent=1.0)
    docs = [synthetic.zipf_document(rng, 200000, vocab) for _ in range(2)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    info = index.info()
    assert info["refine_rounds"] == 0 and info["window_sorted"] == 0 and info["dc3_levels"] > 1
    for d in range(2):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


@pytest.mark.parametrize("case", ["one_symbol", "period3", "two_copies", "many_copies_multidoc"])
def test_repetitive_inputs_lcp_beyond_the_direct_cap(hip, oracle, case):
    """Common prefixes far beyond LCP_DIRECT_CAP (16384): the capped ranks are finished by the
    Kasai-style pass; DC3 recurses to the bottom.  Tables bit-exact against the oracle."""
    from east import hip_backend
    from east.asts import utils as ast_utils
    rng = np.random.default_rng(4)
    if case == "one_symbol":
        docs = [["A" * 60000]]
    elif case == "period3":
        docs = [["ABC" * 25000 + "X"]]
    elif case == "two_copies":
        blob = "".join(rng.choice(list("ABCD"), size=40000))
        docs = [[blob + "Q" + blob]]
    else:
        blob = "".join(rng.choice(list("AB"), size=20000))
        docs = [[blob, blob, "C" + blob], [blob[::-1], blob[::-1]]]
    parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
    index = hip_backend.HipIndex()
    index.build(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]),
                np.array([len(sc) for sc in docs]))
    for d, sc in enumerate(docs):
        o = oracle.OracleEASA(sc)
        assert int(o.lcptab.max()) > 16384
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, case, d)
    q = docs[0][0][:40]
    qs, qo = hip_backend.pack_queries([q])
    assert index.score_table(qs, qo, True)[0, 0] == oracle.OracleEASA(docs[0]).score(q)
    sym = np.concatenate(parts)
    qs, qo = _repeat_keyphrases(parts[0][parts[0] < 0x0A00])
    tables = {norm: index.score_table(qs, qo, norm, want_suffix=True) for norm in (True, False)}
    _check_index(oracle, index, sym, np.concatenate([[0], np.cumsum([p.size for p in parts])]), [len(sc) for sc in docs],
                 scores=(qs, qo, tables))


def _long_repeat_body(case, n, rng):
    if case in ("one_symbol", "one_letter"):
        return np.full(n, 65, np.uint32)
    if case == "period3":
        return np.resize(np.array([65, 66, 67], np.uint32), n)
    if case == "fibonacci":
        a, b = np.array([65], np.uint32), np.array([65, 66], np.uint32)
        while b.size < n:
            a, b = b, np.concatenate([b, a])
        return b[:n]
    return np.tile(rng.integers(65, 91, size=n // 16, dtype=np.uint32), 16)


def _repeat_keyphrases(body):
    """About 50 keyphrases for a text of long repeats: windows of the text of 1, 2, 3, 64 and 512 symbols (runs of the
    repeat), the same windows broken on their last symbol and in the middle, an absent symbol alone and after a match,
    and a window of 300 symbols -- longer than a workgroup (the reduction-kernel fallback of csrc/score.h)."""
    alphabet = np.unique(body)

    def other(c):                                               # another symbol of the text (one letter: an absent one)
        return alphabet[(np.searchsorted(alphabet, c) + 1) % alphabet.size] if alphabet.size > 1 else np.uint32(66)
    qs = []
    for length in (1, 2, 3, 64, 512):
        for start in (0, 1, 2, body.size // 2 + 1):
            w = body[start:start + length]
            qs.append(w)
            if length > 1:
                qs.append(np.concatenate([w[:-1], [other(w[-1])]]))
            if length > 2:
                qs.append(np.concatenate([w[:length // 2], [other(w[length // 2])], w[length // 2 + 1:]]))
    qs += [np.array([0x05D0]), np.concatenate([body[:5], [0x05D0]]), body[7:307]]
    qs = [np.asarray(q, np.uint32) for q in qs]
    return np.concatenate(qs), np.concatenate([[0], np.cumsum([q.size for q in qs])]).astype(np.int64)


@pytest.mark.parametrize("case", ["one_symbol", "period3", "fibonacci", "sixteen_copies"])
def test_long_repeats_at_four_million_symbols(hip, oracle, request, case):
    """Repetitive inputs at a size where a quadratic step shows (a blocked Kasai walk took 0.16 s here and 0.8 s at 16 M;
    the finishing pass now goes by the irreducible-LCP lemma, csrc/tables.h): 4 Mi symbols of one letter, of a period of
    three, a Fibonacci string, 16 copies of a passage -- suffix array and LCP table array_equal to the oracle's DC3 + Kasai
    (the reference's annotation pass, and with it the full oracle, is quadratic on such trees: minutes at 1 M), all six
    tables and the lcp-interval lefts checked in full against their definitions, ~50 keyphrases of runs and broken runs
    bit-equal to the interval walk with their per-suffix results, normalized and -d; and the build stays within a bound."""
    _only_paths(request, "window_sort", "dc3_only")
    import time
    from east import hip_backend
    n = 1 << 22
    rng = np.random.default_rng(7)
    body = _long_repeat_body(case, n, rng)
    sym = np.concatenate([body, [0x0A00]]).astype(np.uint32)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([1]))
    t0 = time.perf_counter()
    index.build(sym, np.array([0, sym.size]), np.array([1]))
    assert time.perf_counter() - t0 < 0.5                     # (60 ms or less on an MI355X; 0.16-0.2 s with the quadratic step)
    o = oracle.OracleEASA(symbols=sym, n_strings=1, tables=False)
    t = index.tables(0, names=("suftab", "lcptab", "anntab"))
    assert np.array_equal(t["suftab"], o.suftab) and np.array_equal(t["lcptab"], o.lcptab)
    assert int(t["anntab"][0]) == sym.size - 1
    del t, o
    qs, qo = _repeat_keyphrases(body)
    tables = {norm: index.score_table(qs, qo, norm, want_suffix=True) for norm in (True, False)}
    _check_index(oracle, index, sym, [0, sym.size], [1], scores=(qs, qo, tables))


@pytest.mark.parametrize("case", ["one_letter", "period3", "fibonacci"])
def test_long_repeats_at_sixteen_mi_symbols(hip, oracle, request, case):
    """The 16 Mi inputs of tools/long_repeat_profile.py, whose doubling rounds go launch by launch (fewer group-number
    bits, short first attempts, no direct comparisons once long repeats are known: DESIGN 5.6), each as one string: the
    suffix array by the rank-pair condition (no DC3 oracle at this size), LCP by Kasai, the other tables and the
    lcp-interval lefts from it, all in full; the keyphrases of runs and broken runs bit-equal to the interval walk."""
    _only_paths(request, "window_sort", "dc3_only")
    from east import hip_backend
    body = _long_repeat_body(case, 16 << 20, None)
    sym = np.concatenate([body, [0x0A00]]).astype(np.uint32)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, sym.size]), np.array([1]))
    qs, qo = _repeat_keyphrases(body)
    tables = {norm: index.score_table(qs, qo, norm, want_suffix=True) for norm in (True, False)}
    _check_index(oracle, index, sym, [0, sym.size], [1], scores=(qs, qo, tables))


def test_long_repeats_in_one_batched_build(hip, oracle, suffix_sort_path):
    """Long repeats next to each other and next to ordinary text in ONE build, so that the segmented first-level sort
    (the `_seg` paths) and domains of mixed documents meet them: 2 Mi of one letter, a 2 Mi Fibonacci string, a period
    of three cut into eight strings at cuts off the period, the reference's worst case (100 identical strings of 10^4),
    1 Mi of word stream.  Every table of every document and the lcp-interval lefts checked in full against their
    definitions; keyphrases of runs and of the word stream bit-equal to the interval walk, with per-suffix results."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(5150)
    period = np.resize(np.array([65, 66, 67], np.uint32), 1 << 20)
    cuts = np.sort(rng.choice(np.arange(1, period.size), size=7, replace=False))
    docs = [(np.concatenate([_long_repeat_body("one_letter", 2 << 20, None), [0x0A00]]).astype(np.uint32), 1),
            (np.concatenate([_long_repeat_body("fibonacci", 2 << 20, None), [0x0A00]]).astype(np.uint32), 1),
            (np.concatenate([np.concatenate([p, [0x0A00 + i]]) for i, p in enumerate(np.split(period, cuts))]).astype(np.uint32), 8),
            synthetic.worst_case_collection(rng, 100, 10 ** 4),
            synthetic.word_stream_document(rng, 1 << 20, want_text=False)[1:]]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    ms = np.array([d[1] for d in docs], dtype=np.int32)
    index = hip_backend.HipIndex()
    index.build(sym, off, ms)
    assert index.info()["n_docs"] == 5
    qa, oa = _repeat_keyphrases(docs[1][0][:-1])
    qb, ob = synthetic.keyphrases(rng, docs[4][0], 20)
    qs, qo = np.concatenate([qa, qb]), np.concatenate([oa, ob[1:] + oa[-1]])
    tables = {norm: index.score_table(qs, qo, norm, want_suffix=True) for norm in (True, False)}
    assert (tables[True][0][:, 0] > 0).any() and (tables[True][0][:, 4] > 0).any()
    _check_index(oracle, index, sym, off, ms, scores=(qs, qo, tables))


def test_host_symbols_go_up_as_16_bit_words(hip, oracle, request):
    """east_hip_build from host symbols of the reference encoding (4 Mi symbols or more): from a handle's second call on --
    the first one leaves the pinning of the ring to a background thread -- the symbols are narrowed to 16 bits by host
    threads, go up through the pinned ring and are widened on the device (upload.h: upload_symbols_narrow); text
    symbols right below U+0A00 and terminators far above it included.  Tables and scores as with the plain copy and as
    the oracle's."""
    _only_paths(request, "window_sort", "dc3_only", "window_sort_seg")
    import time
    from east import hip_backend, synthetic
    rng = np.random.default_rng(16)
    docs = [synthetic.word_stream_document(rng, int(sz), want_text=False)[1:] for sz in (3 << 20, 2 << 20, 700000)]
    docs[1][0][docs[1][0] == 65] = 0x09FF                     # a text symbol right below the terminator base
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    ms = np.array([d[1] for d in docs], dtype=np.int32)
    plain = hip_backend.HipIndex()
    os.environ["EAST_HIP_NO_SYMBOL_NARROW"] = "1"              # (the plain 4-byte copy, whatever ring a recycled handle brings)
    try:
        plain.build(sym, off, ms)
    finally:
        del os.environ["EAST_HIP_NO_SYMBOL_NARROW"]
    assert plain.info()["narrow_upload"] == 0
    want = {d: plain.tables(d) for d in range(3)}
    qs, qo = synthetic.keyphrases(rng, sym, 100)
    table = plain.score_table(qs, qo, True)
    # (a handle reserved for builds of this size has its ring pinned in the background from its creation on)
    index = hip_backend.HipIndex(reserve_symbols=int(sym.size))           # (a handle of its own: none out of the pool)
    for _ in range(200):                                       # the ring is pinned in the background: a few milliseconds
        index.build(sym, off, ms)
        if index.info()["narrow_upload"]:
            break
        time.sleep(0.01)
    assert index.info()["narrow_upload"] == 1
    for d in range(3):
        got = index.tables(d)
        for name in TABLES:
            assert np.array_equal(got[name], want[d][name]), (name, d)
    assert np.array_equal(index.score_table(qs, qo, True), table)
    o = oracle.OracleEASA(symbols=docs[1][0], n_strings=docs[1][1])
    for name in TABLES:
        assert np.array_equal(want[1][name], getattr(o, name)), name
    index.build(sym[: off[1]], off[:2], ms[:1])                # smaller than the threshold: the plain copy again
    assert index.info()["narrow_upload"] == 0


def test_host_symbols_go_up_as_bytes_when_the_text_fits_them(hip, oracle, request):
    """Text whose code points all lie below 0xFF -- the word streams of every BASELINE config -- goes up as BYTES (a
    quarter of the ABI's four bytes per symbol; upload.h: upload_symbols_narrow<uint8_t>, build_info[25] == 2): same
    tables and scores as the plain copy and as the oracle's.  A text symbol a byte cannot hold, met half-way through the
    upload (far behind the 64 Ki symbols the call looks at first), starts it over with 16-bit words -- for that call, with
    the right tables, and for the handle's later calls at once."""
    _only_paths(request, "window_sort", "dc3_only", "window_sort_seg")
    import time
    from east import hip_backend, synthetic
    rng = np.random.default_rng(17)
    docs = [synthetic.word_stream_document(rng, int(sz), want_text=False)[1:] for sz in (3 << 20, 2 << 20, 900000)]
    docs[2][0][docs[2][0] == 66] = 0xFE                         # the largest text symbol a byte holds
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])]).astype(np.int64)
    ms = np.array([d[1] for d in docs], dtype=np.int32)
    plain = hip_backend.HipIndex()
    os.environ["EAST_HIP_NO_SYMBOL_NARROW"] = "1"              # (the plain 4-byte copy, whatever ring a recycled handle brings)
    try:
        plain.build(sym, off, ms)
    finally:
        del os.environ["EAST_HIP_NO_SYMBOL_NARROW"]
    assert plain.info()["narrow_upload"] == 0
    want = {d: plain.tables(d) for d in range(3)}
    qs, qo = synthetic.keyphrases(rng, sym, 100)
    table = plain.score_table(qs, qo, True)
    index = hip_backend.HipIndex(reserve_symbols=int(sym.size))
    for _ in range(200):                                       # the ring is pinned in the background: a few milliseconds
        index.build(sym, off, ms)
        if index.info()["narrow_upload"]:
            break
        time.sleep(0.01)
    assert index.info()["narrow_upload"] == 2
    for d in range(3):
        got = index.tables(d)
        for name in TABLES:
            assert np.array_equal(got[name], want[d][name]), (name, d)
    assert np.array_equal(index.score_table(qs, qo, True), table)
    o = oracle.OracleEASA(symbols=docs[2][0], n_strings=docs[2][1])
    for name in TABLES:
        assert np.array_equal(want[2][name], getattr(o, name)), name
    # a symbol that does not fit, 4 M symbols into the stream
    sym2 = sym.copy()
    hit = np.flatnonzero(sym2[off[1]:off[2]] == 67) + off[1]
    sym2[hit] = 0x0416
    index.build(sym2, off, ms)
    assert index.info()["narrow_upload"] == 1
    o = oracle.OracleEASA(symbols=sym2[off[1]:off[2]], n_strings=int(ms[1]))
    got = index.tables(1)
    for name in TABLES:
        assert np.array_equal(got[name], getattr(o, name)), name
    index.build(sym, off, ms)                                  # the handle remembers: 16-bit words at once
    assert index.info()["narrow_upload"] == 1
    got = index.tables(0)
    for name in TABLES:
        assert np.array_equal(got[name], want[0][name]), name


def test_c_abi_rejects_inconsistent_input(hip):
    """n_strings that does not match the terminators, or a document without a final terminator,
    is an EAST_HIP_ERR_DOMAIN error (not silent garbage, not an out-of-bounds comparison)."""
    from east import exceptions, hip_backend
    sym = np.array([65, 66, 0x0A00, 67, 0x0A01], dtype=np.uint32)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, 5]), np.array([2]))                        # fine
    with pytest.raises(exceptions.HipBackendError, match="n_strings"):
        index.build(sym, np.array([0, 5]), np.array([1]))
    with pytest.raises(exceptions.HipBackendError, match="terminator"):
        index.build(sym[:4], np.array([0, 4]), np.array([1]))
    with pytest.raises(exceptions.HipBackendError, match="n_strings"):
        index.build(sym, np.array([0, 3, 5]), np.array([1, 2]))
    with pytest.raises(exceptions.HipBackendError):
        index.score_table(np.array([65], np.uint32), np.array([0, 1]))       # no valid index after a failed build


def _host_prepared(texts):
    from east import utils
    from east.asts import utils as ast_utils
    colls = [utils.text_to_strings_collection(t) for t in texts]
    parts = [ast_utils.strings_to_symbols(sc) for sc in colls]
    if any(ast_utils.is_tagged(p) for p in parts):            # kept text at or above U+0A00 anywhere: the tagged encoding
        parts = [ast_utils.tag_terminators(p) for p in parts]
    return (np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]),
            np.array([len(sc) for sc in colls]))


def _check_device_prep(hip, texts):
    index = hip.HipIndex()
    index.build_texts(texts)
    sym, off, m = index.prepared()
    want_sym, want_off, want_m = _host_prepared(texts)
    assert off.tolist() == want_off.tolist() and m.tolist() == want_m.tolist()
    assert np.array_equal(sym, want_sym)
    return index


@pytest.fixture(params=[-1, 0, 23, 600])
def text_stream(request, hip):
    """How the raw text reaches the device (east_hip_debug_set_text_stream): the default (chunks from 8 MiB on), in one
    piece, and in chunks of about 23 / 600 bytes -- every fixture then crosses cuts inside tokens' strings of three,
    inside documents and between them, with the counts carried from chunk to chunk on the device."""
    lib = hip.load()
    assert lib.east_hip_debug_set_text_stream(request.param) == 0
    yield request.param
    assert lib.east_hip_debug_set_text_stream(-1) == 0


def test_device_text_preparation_fixtures(hip, text_stream):
    """east_hip_build_texts == prepare_text + tokenize + text_to_strings_collection + make_unique_endings
    on the reference-derived vectors and the HSE corpus."""
    g = load_golden("utils_vectors.json")
    texts = [v["text_utf8"].encode("utf-8") for v in g["text_to_strings_collection"]]
    _check_device_prep(hip, texts)
    for t in texts:                                           # also one document at a time
        _check_device_prep(hip, [t])
    h = load_golden("hse_config1.json")
    _check_device_prep(hip, [t.encode("utf-8") for t in h["texts"].values()])
    _check_device_prep(hip, ["str input: no decoding, just upper", "ß stays ß, ŉ stays ŉ"])


def test_device_text_preparation_fuzz(hip, text_stream):
    """Random mixtures of ASCII, Latin-1, Greek, Cyrillic, Arabic-Indic digits, superscripts, fractions,
    apostrophes, underscores, non-word characters beyond U+0A00 (emoji, dashes, BOM) and malformed
    UTF-8 (stray continuations, truncated and overlong sequences, surrogates, > U+10FFFF)."""
    import random
    rng = random.Random(20240)
    chars = list("abcXYZ'_ 019,.-\n\t") + ["ß", "é", "Ж", "ж", "λ", "Σ", "ς", "٣", "²", "½", "ŉ", "ǅ", "ſ", "ı",
                                            "\U0001F600", "—", "’", "﻿", " ", "İ", "ͅ"]
    junk = [b"\x80", b"\xbf", b"\xc0", b"\xc1\x81", b"\xc2", b"\xe0\x80", b"\xe0\xa0", b"\xe4\xb8", b"\xed\xa0\x80",
            b"\xf0\x90\x80", b"\xf4\x90\x80\x80", b"\xf5", b"\xff", b"\xe2\x82", b"\xf0\x9f\x98"]
    # word characters at or above U+0A00 (every third round: the symbols then come in the tagged encoding)
    high = ["\u4e2d", "\u6587", "\u0e01", "\u0e02", "\u1ec7", "\u10e5", "\u2c6f", "\ud55c", "\U00010428", "\u0e53", "\u2177", "\u1fb3"]
    for it in range(180):
        texts = []
        pool = chars + high if it % 3 == 2 else chars
        for _ in range(rng.randint(1, 6)):
            parts = []
            for _ in range(rng.randint(0, 40)):
                if rng.random() < 0.12:
                    parts.append(rng.choice(junk))
                else:
                    parts.append("".join(rng.choice(pool) for _ in range(rng.randint(1, 6))).encode("utf-8"))
            texts.append(b"".join(parts))
        _check_device_prep(hip, texts)


@pytest.mark.parametrize("chunk", [-1, 0, 1 << 20, 3333333])
def test_device_text_preparation_large(hip, chunk):
    """16 MiB + three small documents, in one piece, in the default chunks and in chunks of 1 MiB / 3.3 MB; then the same
    words with non-ASCII characters sprinkled in (the chunks then take the general UTF-8 path) against the host chain."""
    from east import synthetic, utils
    from east.asts import utils as ast_utils
    lib = hip.load()
    rng = np.random.default_rng(3)
    text, sym, m = synthetic.word_stream_document(rng, 16 << 20)
    assert lib.east_hip_debug_set_text_stream(chunk) == 0
    try:
        index = hip.HipIndex()
        index.build_texts([text, text[: 1 << 20], b"", b"12 345 ab"])
        got, off, ms = index.prepared()
        assert ms[0] == m and np.array_equal(got[: off[1]], sym)
        assert got[off[2]:off[3]].tolist() == [32, 0x0A00] and got[off[3]:].tolist() == [32, 0x0A00]
        # four documents of 300 KB with accented letters, Greek and stray bytes at random places
        docs = []
        for d in range(4):
            raw = bytearray(text[d * 300000:(d + 1) * 300000])
            for pos in rng.integers(0, len(raw) - 4, size=400):
                ins = [b"\xc3\xa9", b"\xce\xbb", b"\xff", b"\xe2\x80\x94", b"\xc3"][int(rng.integers(0, 5))]
                raw[pos:pos + len(ins)] = ins
            docs.append(bytes(raw))
        index.build_texts(docs)
        got, off, ms = index.prepared()
        for d, raw in enumerate(docs):
            want = ast_utils.strings_to_symbols(utils.text_to_strings_collection(raw))
            assert np.array_equal(got[off[d]:off[d + 1]], want), d
    finally:
        assert lib.east_hip_debug_set_text_stream(-1) == 0


@pytest.mark.parametrize("slot", [64, 1000, 100000, 0])
def test_device_text_preparation_through_the_pinned_ring(hip, monkeypatch, request, slot):
    """Separate texts (east_hip_build_texts_v) of a streamed preparation go up through a ring of pinned host memory, filled
    by a few host threads and sent slot by slot (textfront.h: tp_fill_stream): forced on, with slots of 64 bytes to 4 MiB
    -- slots that end inside texts, at separators, inside chunks and at their ends, many times round the ring -- the
    prepared symbols equal the host chain's.  Fixtures, a fuzz, 40 documents of 300 KB, and the default path's choice."""
    import random
    from east import synthetic
    _only_paths(request, "window_sort", "dc3_only")           # (the upload does not depend on the sort path)
    lib = hip.load()
    monkeypatch.setattr(hip, "JOIN_FREE_MIN_BYTES", 0)        # (small collections through the separate-texts entry point too)
    assert lib.east_hip_debug_set_text_ring(1, slot) == 0
    try:
        g = load_golden("utils_vectors.json")
        texts = [v["text_utf8"].encode("utf-8") for v in g["text_to_strings_collection"]]
        h = load_golden("hse_config1.json")
        hse = [t.encode("utf-8") for t in h["texts"].values()]
        rng = random.Random(77)
        words = ["alpha", "be", "Gamma9", "12", "дом", "éclair", "x_y'z", "0042", "Ωmega", "it's"]
        fuzz = [[(" ".join(rng.choice(words) for _ in range(rng.randint(0, 60)))).encode("utf-8") for _ in range(rng.randint(1, 9))]
                for _ in range(25)]
        for chunk in (23, 600, 5000):
            assert lib.east_hip_debug_set_text_stream(chunk) == 0
            _check_device_prep(hip, texts)
            _check_device_prep(hip, hse)
            _check_device_prep(hip, [b"", b"a b", b"", b"only one tokenhere"])
            for collection in fuzz:
                _check_device_prep(hip, collection)
        assert lib.east_hip_debug_set_text_stream(-1) == 0
        if slot >= 100000 or slot == 0:                        # 12 MiB: the default chunks, the ring by its own choice as well
            nrng = np.random.default_rng(5)
            docs = [synthetic.word_stream_document(nrng, 300000)[0] for _ in range(40)]
            docs[7] = docs[7][:100] + "é λ — ".encode("utf-8") + docs[7][100:]
            _check_device_prep(hip, docs)
            assert lib.east_hip_debug_set_text_ring(-1, slot) == 0
            _check_device_prep(hip, docs)
    finally:
        assert lib.east_hip_debug_set_text_stream(-1) == 0
        assert lib.east_hip_debug_set_text_ring(-1, 0) == 0


def test_host_and_device_text_preparation_give_the_same_table(hip, monkeypatch):
    from east import applications, relevance
    g = load_golden("zipf_docs.json")
    texts = {k: v.encode("utf-8") for k, v in g["texts"].items()}
    tables = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("EAST_HIP_TEXT_PREP", mode)
        tables[mode] = applications.keyphrases_table(g["keyphrases"], texts, relevance.ASTRelevanceMeasure())
    assert tables["host"] == tables["device"] == g["normalized"]


def test_bucketed_rank_scatter_path(hip, oracle):
    """Inputs whose rank array exceeds the Infinity Cache take a bucketed scatter; force that
    path on small inputs (multi-document, single document, deep recursion) and compare with the oracle."""
    from east import relevance
    lib = hip.load()
    assert lib.east_hip_debug_set_rank_bucket_bytes(0) == 0
    try:
        rng = np.random.default_rng(12)
        docs = _random_collections(rng, 5, "ABCD", max_strings=40, max_len=30)
        docs.append(["AB" * 3000 + "C"])
        measure = relevance.ASTRelevanceMeasure()
        measure.set_strings_collections(docs)
        for d, sc in enumerate(docs):
            o = oracle.OracleEASA(sc)
            t = measure.index.tables(d)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (name, d)
        text = word_stream(rng, 1 << 20)
        measure.set_text_collection([text])
        from east import utils
        o = oracle.OracleEASA(utils.text_to_strings_collection(text))
        t = measure.index.tables(0, names=("suftab", "lcptab", "anntab"))
        for name in ("suftab", "lcptab", "anntab"):
            assert np.array_equal(t[name], getattr(o, name)), name
    finally:
        assert lib.east_hip_debug_set_rank_bucket_bytes(192 << 20) == 0


def test_many_small_documents(hip, oracle):
    """Single-file mode of the CLI (one text per line): 20 000 tiny documents in one batched build,
    including empty lines (-> [" "]) and lines without any kept token."""
    from east import relevance, utils
    rng = np.random.default_rng(21)
    lines = []
    for i in range(20000):
        kind = i % 11
        if kind == 0:
            lines.append(b"")
        elif kind == 1:
            lines.append(b"a bb 123 4567")
        else:
            lines.append(word_stream(rng, int(rng.integers(8, 120))))
    measure = relevance.ASTRelevanceMeasure()
    measure.set_text_collection(lines)
    kps = [utils.prepare_text(word_stream(rng, 10).decode()) for _ in range(20)] + ["A", "BB 12"]
    kps = [k for k in kps if k.replace(" ", "")]
    table = measure.relevance_table(kps)
    assert table.shape == (len(kps), len(lines))
    for d in list(range(0, 40)) + list(range(19960, 20000)) + rng.integers(0, 20000, size=60).tolist():
        o = oracle.OracleEASA(utils.text_to_strings_collection(lines[d]))
        t = measure.index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d)
        for k, kp in enumerate(kps):
            assert table[k, d] == o.score(kp, fast=True), (d, kp)


def _check_renamed(hip, oracle, docs, queries, alphabet=None):
    """docs: strings collections of one shard.  Tables and scores of every document against the oracle on the
    renamed alphabet (conftest.Renamed); returns the index."""
    from conftest import Renamed
    from east.asts import utils as ast_utils
    parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
    if any(ast_utils.is_tagged(p) for p in parts):
        parts = [ast_utils.tag_terminators(p) for p in parts]
    index = hip.HipIndex()
    index.build(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]),
                np.array([len(sc) for sc in docs]))
    stripped = [q.replace(" ", "") for q in queries]
    qs, qo = hip.pack_queries(stripped)
    tables = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    for d, sc in enumerate(docs):
        r = Renamed(sc, alphabet)
        o = oracle.OracleEASA(symbols=r.symbols, n_strings=r.n_strings)
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d, sc)
        for k, q in enumerate(queries):
            for norm in (True, False):
                assert tables[norm][k, d] == o.score_symbols(r.query(q), norm), (d, q, norm)
    return index


def test_text_above_the_terminator_base_fixture(hip, oracle, tmp_path, capsys):
    """high_text.json (generated from the reference): text at or above U+0A00 -- Thai, CJK, Hangul, Georgian,
    precomposed Vietnamese, a supplementary-plane letter.  The scores are those of ast_naive, the method as defined
    (the reference's easa and ast_linear break there, see the fixture); the tables those of easa.py on the
    order-preserving renaming of the text alphabet below U+0A00 (the oracle)."""
    from east import applications, main as east_main, relevance
    from east.asts import base
    g = load_golden("high_text.json")
    for case in g["cases"]:
        ast = base.AST.get_ast(case["strings"])
        assert ast.string == "".join(s + chr(0x0A00 + i) for i, s in enumerate(case["strings"]))
        for q in case["queries"]:
            qq = q["query"].replace(" ", "")
            for mode, norm in (("normalized", True), ("denormalized", False)):
                total, suffixes = ast.score(q["query"], normalized=norm, return_suffix_scores=True)
                assert abs(total - q[mode]) <= 1e-12, (case["strings"], q["query"], mode)
                assert all(abs(suffixes[qq[i:]] - q["suffix_" + mode][i]) <= 1e-12 for i in range(len(qq)))
        _check_renamed(hip, oracle, [case["strings"]], [q["query"] for q in case["queries"]])
    t = g["table"]
    texts = {k: v.encode("utf-8") for k, v in t["texts"].items()}
    for prep in ("device", "host"):
        os.environ["EAST_HIP_TEXT_PREP"] = prep
        try:
            for mode, norm in (("normalized", True), ("denormalized", False)):
                table = applications.keyphrases_table(t["keyphrases"], texts, relevance.ASTRelevanceMeasure(normalized=norm))
                for kp in t["keyphrases"]:
                    for name in texts:
                        assert abs(table[kp][name] - t[mode][kp][name]) <= 1e-12, (prep, mode, kp, name)
        finally:
            os.environ.pop("EAST_HIP_TEXT_PREP", None)
    # the CLI on the same collection
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, raw in texts.items():
        (tdir / (name + ".txt")).write_bytes(raw)
    (tmp_path / "kp.txt").write_text("\n".join(t["keyphrases"]) + "\n", encoding="utf-8")
    assert east_main.main(["-f", "csv", "keyphrases", "table", str(tmp_path / "kp.txt"), str(tdir)]) == 0
    assert "0.472" in capsys.readouterr().out


@pytest.mark.parametrize("seed", range(6))
def test_text_above_the_terminator_base_random_shards(hip, oracle, seed):
    """Shards mixing documents with and without text above U+0A00, narrow alphabets (the byte path and the window
    sort) and wide ones (more than 254 distinct text symbols: dense u32 codes, DC3), code points next to the
    terminator base and on the supplementary planes; queries with symbols absent from the text."""
    rng = np.random.default_rng(4200 + seed)
    pools = [list("ABC") + [chr(c) for c in (0x0A00, 0x0A01, 0x0A02, 0x0E01, 0x4E2D)],
             [chr(c) for c in range(0x4E00, 0x4E00 + 300)] + list("xy"),
             [chr(c) for c in (0x09FF, 0x0A00, 0x10FFFF, 0x10400, 0xFFFD, 0x41)],
             list("ABCDEFG"),
             [chr(c) for c in range(0x0400, 0x0400 + 200)] + [chr(c) for c in range(0xAC00, 0xAC00 + 100)]]
    pool_of_doc = [pools[int(rng.integers(len(pools)))] for _ in range(int(rng.integers(1, 7)))]
    if seed == 0:
        pool_of_doc = [pools[3], pools[0], pools[3]]          # (only some documents hold high text)
    docs = []
    for pool in pool_of_doc:
        m = int(rng.integers(1, 8))
        docs.append(["".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(0, 60)))) for _ in range(m)])
        if sum(len(s) for s in docs[-1]) == 0:
            docs[-1][0] = pool[0]
    every = sorted(set(ord(c) for sc in docs for s in sc for c in s))
    queries = []
    for _ in range(24):
        sc = docs[int(rng.integers(len(docs)))]
        s = sc[int(rng.integers(len(sc)))] or "A"
        a = int(rng.integers(len(s)))
        q = s[a:a + int(rng.integers(1, 9))]
        if rng.random() < 0.3:
            q = q + chr(int(rng.choice([0x0A00, 0x4E01, 0x42, 0x10FFFE])))
        queries.append(q)
    # one alphabet for the whole shard: the device numbers the text symbols of all documents together
    index = _check_renamed(hip, oracle, docs, queries, alphabet=every)
    assert index.info()["sigma_text"] == len(every)


@pytest.mark.parametrize("seed", range(3))
def test_text_above_the_terminator_base_with_refinement_rounds(hip, oracle, seed):
    """Word text over a small vocabulary whose letters lie above U+0A00: the tagged stream becomes a byte stream,
    takes the window sort and its refinement rounds (the arena is sized for that, not only for the widest alphabet a
    tagged stream could bring), and gives the tables of the same text spelled below U+0A00."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(8800 + seed)
    vocab = synthetic.zipf_vocabulary(rng, size=int(rng.choice([10, 50, 300])), exponent=1.0)
    docs = [synthetic.zipf_document(rng, int(rng.integers(150000, 600000)), vocab) for _ in range(int(rng.integers(1, 5)))]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    used = np.unique(sym[sym < 0x0A00])
    target = np.sort(rng.choice(0x110000 - 0x0A00, size=used.size, replace=False).astype(np.uint32) + 0x0A00)
    lifted = np.where(sym >= 0x0A00, (sym - 0x0A00) | np.uint32(0x80000000),
                      target[np.searchsorted(used, np.minimum(sym, used[-1]))]).astype(np.uint32)
    index = hip_backend.HipIndex()
    index.build(lifted, off, np.array([d[1] for d in docs]))
    for d in range(len(docs)):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        t = index.tables(d)
        for name in TABLES:
            assert np.array_equal(t[name], getattr(o, name)), (name, d, index.info())


def test_tagged_encoding_c_abi(hip, oracle):
    """The tagged encoding without any high text gives what the reference encoding gives; a symbol that is neither a
    tagged terminator nor a code point is refused; the encoding is a property of the handle until reset."""
    from east import exceptions
    from east.asts import utils as ast_utils
    docs = [["XABXAC", "BABXAC"], ["HELLO", "", "HELP"]]
    parts = [ast_utils.strings_to_symbols(sc) for sc in docs]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    m = np.array([len(sc) for sc in docs])
    plain, tagged = hip.HipIndex(), hip.HipIndex()
    plain.build(np.concatenate(parts), off, m)
    tagged.build(np.concatenate([ast_utils.tag_terminators(p) for p in parts]), off, m)
    for d in range(2):
        a, b = plain.tables(d), tagged.tables(d)
        for name in TABLES:
            assert np.array_equal(a[name], b[name])
    qs, qo = hip.pack_queries(["ABX", "HEL", "Q"])
    assert np.array_equal(plain.score_table(qs, qo, True), tagged.score_table(qs, qo, True))
    bad = np.concatenate([ast_utils.tag_terminators(p) for p in parts])
    bad[1] = 0x110000
    with pytest.raises(exceptions.HipBackendError, match="neither a tagged terminator nor a code point"):
        tagged.build(bad, off, m)
    bad[1] = 0x4E2D
    bad[-1] = 0x0A02                                              # the reference's terminator in a tagged stream: text
    with pytest.raises(exceptions.HipBackendError, match="terminator"):
        _build_tagged(hip, tagged, bad, off, m)


def _build_tagged(hip, index, symbols, off, m):
    """east_hip_build with the tagged encoding set by hand (HipIndex.build tells it from the last symbol)."""
    import ctypes
    lib = hip.load()
    assert lib.east_hip_set_symbol_encoding(index._h, 1) == 0
    symbols = np.ascontiguousarray(symbols, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    m = np.ascontiguousarray(m, dtype=np.int32)
    hip._check(lib.east_hip_build(index._h, symbols.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), symbols.size,
                                  off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m.size))


def test_score_in_stretches_of_documents(hip, oracle):
    """The per-suffix scratch of a score call is bounded: with a small bound the table and the per-suffix results
    come out a stretch of documents at a time, identical to the one-piece result."""
    from east import hip_backend, synthetic
    rng = np.random.default_rng(61)
    docs = [synthetic.word_stream_document(rng, int(rng.integers(200, 3000)), want_text=False)[1:] for _ in range(137)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    qs, qo = synthetic.keyphrases(rng, sym, 40)
    want, want_suf = index.score_table(qs, qo, True, want_suffix=True)
    lib = hip.load()
    assert lib.east_hip_debug_set_score_scratch(int(qo[-1]) * 8 * 10) == 0          # ten documents at a time
    try:
        got, got_suf = index.score_table(qs, qo, True, want_suffix=True)
        assert np.array_equal(got, want) and np.array_equal(got_suf, want_suf)
        index.set_keyphrases(qs, qo)
        index.score_resident(True)
        assert np.array_equal(index.score_table(qs, qo, False), index.score_table(qs, qo, False))
    finally:
        assert lib.east_hip_debug_set_score_scratch(0) == 0
    o = oracle.OracleEASA(symbols=docs[77][0], n_strings=docs[77][1])
    for k in range(40):
        assert want[k, 77] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=True)


def test_score_walk_grid_is_bounded(hip, oracle):
    """Many short documents x many keyphrases with the per-keyphrase sums inside the walk kernel: a launch takes at most
    a bounded number of workgroups (east_hip_debug_set_score_grid; by default 2^22, far below HIP's limit per grid
    dimension), so the table comes out a stretch of documents at a time -- identical to the one-launch table, bit-equal
    to the oracle.  Stretches of 8 or more documents are multiples of 8 (XCD-aware order), smaller ones are not."""
    from east import hip_backend, synthetic
    lib = hip.load()
    rng = np.random.default_rng(424242)
    docs = [synthetic.word_stream_document(rng, int(rng.integers(60, 400)), want_text=False)[1:] for _ in range(1500)]
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    index = hip_backend.HipIndex()
    index.build(sym, off, np.array([d[1] for d in docs]))
    qs, qo = synthetic.keyphrases(rng, sym, 700)
    want = {norm: index.score_table(qs, qo, norm) for norm in (True, False)}
    n_blk = -(-int(qo[-1]) // 256)                            # at least this many workgroups per document
    try:
        for grid in (n_blk * 100, n_blk * 9, n_blk * 3, 1):    # 96-document stretches, 8, 3 (or fewer), one document at a time
            assert lib.east_hip_debug_set_score_grid(grid) == 0
            for norm in (True, False):
                assert np.array_equal(index.score_table(qs, qo, norm), want[norm]), (grid, norm)
            index.set_keyphrases(qs, qo)
            index.score_resident(True)
    finally:
        assert lib.east_hip_debug_set_score_grid(0) == 0
    for d in (0, 7, 8, 95, 96, 97, 1499):
        o = oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1])
        for k in range(0, 700, 7):
            assert want[True][k, d] == o.score_symbols(qs[qo[k]:qo[k + 1]], True, fast=True), (d, k)


@pytest.mark.parametrize("mode", [1, 0, 2, 3, 4, 5])
def test_score_path_variants(hip, oracle, mode):
    """The score walk's two choices (east_hip_debug_set_score_path): k-gram tables in the pair layout (last level
    unfilled, 8-byte entries with the suffix position; the level above in a table of its own) or as one filled table,
    and the per-keyphrase sums inside the walk kernel or by the reduction kernel -- every combination bit-equal to the
    oracle, normalized and -d, the per-suffix results included; documents of very different sizes (tables of 1 to 4
    levels), natural-language-like text (mostly empty last-level tables), a keyphrase longer than a workgroup (the sums
    fall back to the reduction kernel), absent symbols, and scoring a stretch of documents at a time."""
    from east import hip_backend, synthetic
    lib = hip.load()
    rng = np.random.default_rng(8800)
    vocab = synthetic.zipf_vocabulary(np.random.default_rng(5), size=800, exponent=1.0)
    docs = []
    for i in range(21):
        size = int(rng.choice([300, 5000, 70000, 400000]))
        if i % 3 == 2:
            docs.append(synthetic.zipf_document(rng, size, vocab))
        else:
            docs.append(synthetic.word_stream_document(rng, size, want_text=False)[1:])
    sym = np.concatenate([d[0] for d in docs])
    off = np.concatenate([[0], np.cumsum([d[0].size for d in docs])])
    ms = np.array([d[1] for d in docs])
    qs, qo = synthetic.keyphrases(rng, sym, 300)
    parts = [qs[qo[k]:qo[k + 1]] for k in range(300)]
    parts[7] = np.concatenate([parts[7], np.array([ord("9")], dtype=np.uint32), parts[8]])      # a symbol absent from the corpus
    long_kp = sym[1000:1400][sym[1000:1400] < 0x0A00]
    assert lib.east_hip_debug_set_score_path(mode) == 0
    try:
        index = hip_backend.HipIndex()
        index.build(sym, off, ms)
        oracles = {d: oracle.OracleEASA(symbols=docs[d][0], n_strings=docs[d][1]) for d in (0, 2, 5, 11, 20)}
        for with_long in (False, True):
            ps = parts + [long_kp] if with_long else parts
            q = np.concatenate(ps)
            o = np.concatenate([[0], np.cumsum([p.size for p in ps])]).astype(np.int64)
            for norm in (True, False):
                table, suf = index.score_table(q, o, norm, want_suffix=True)
                plain = index.score_table(q, o, norm)
                assert np.array_equal(table, plain)
                index.set_keyphrases(q, o)
                index.score_resident(norm)
                for d, orc in oracles.items():
                    for k in range(0, len(ps), 1 if d == 5 else 7):
                        want, want_suf = orc.score_symbols(ps[k], norm, fast=True, want_suffix=True)
                        assert table[k, d] == want, (mode, d, k, norm)
                        assert np.array_equal(suf[d, o[k]:o[k + 1]], want_suf), (mode, d, k, norm)
        assert lib.east_hip_debug_set_score_scratch(int(qo[-1]) * 8 * 4) == 0       # four documents at a time
        t2, s2 = index.score_table(q, o, True, want_suffix=True)
        t1, s1 = index.score_table(q, o, False, want_suffix=True)
        assert np.array_equal(t1, table) and np.array_equal(s1, suf)
        assert np.array_equal(t2, index.score_table(q, o, True))
    finally:
        assert lib.east_hip_debug_set_score_scratch(0) == 0
        assert lib.east_hip_debug_set_score_path(1) == 0


def test_half_gib_symbols(hip, oracle, request, record_property, suffix_sort_path):
    """Maximum-size leg: one document of 2^29 symbols (a quarter of the 2^31 index range; 20 GB arena), checked in full
    in linear time: the suffix array by the rank-pair condition, LCP by Kasai, the annotation table; on window_sort also
    the three child tables (computed on the device at their first read) and the lcp-interval lefts; 100 scores bit-equal
    to the interval walk, normalized and -d.  Host memory: the tables are read one or two at a time, the checkers' scratch is
    int32 (peak RSS recorded as the test's `peak_rss_gib` property)."""
    if "_seg" in suffix_sort_path:
        pytest.skip("one document: nothing to segment (the same build as the path without _seg)")
    _three_paths(request, "window_sort_unfused", "window_sort_ht", "window_sort_ht_unfused")
    import resource
    from east import hip_backend, synthetic
    n = 1 << 29
    rng = np.random.default_rng(29)
    sym, m = synthetic.direct_document(rng, n)
    index = hip_backend.HipIndex()
    index.build(sym, np.array([0, n]), np.array([m]))
    info = index.info()
    assert info["n_total"] == n and (info["dc3_levels"] >= 1 or info["window_sorted"] == 1)
    t = {}
    for name in ("suftab", "lcptab", "anntab"):                 # (one at a time: int32 read-back, int64 copy)
        t[name] = index.tables(0, names=(name,))[name]
    oracle.check_tables(sym, [0, n], [m], t)
    del t["anntab"]
    qs, qo = synthetic.keyphrases(rng, sym[: 1 << 20], 100)
    for norm in (True, False):
        table = index.score_table(qs, qo, norm)
        _assert_scores(table, oracle.score_table_fast(sym, [0, n], [m], t["suftab"], qs, qo, norm), "scores (%s)" % norm)
        assert (table[0::2] > 0).all()
    del t["suftab"]
    if _raw_path(request) == "window_sort":                     # (two at a time on the checked lcp table; two passes run at once)
        oracle.check_tables(sym, [0, n], [m], {name: index.tables(0, names=(name,))[name]
                                               for name in ("childtab_up", "childtab_down")}, verified_lcptab=t["lcptab"])
        oracle.check_tables(sym, [0, n], [m], {"childtab_next_l_index": index.tables(0, names=("childtab_next_l_index",))[
            "childtab_next_l_index"], "left": index.lcp_interval_lefts(0)}, verified_lcptab=t["lcptab"])
    record_property("peak_rss_gib", resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20)
