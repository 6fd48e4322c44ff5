# -*- coding: utf-8 -*-
"""gpu tier: the BM25 score call of the cosine term index (csrc/bm25.h; include/east_hip.h, "BM25") against the exact model
of tests/bm25_exact.py: every score within (t + 24) * 2^-53 relative of the exact value (t = its contributing units), the
zeros exactly +0.0, the same bytes from any strip size and from a second call; the cache of the weights, the cosine scores
beside it untouched, and the consumers of the table it leaves.  The collections are those whose attainability
tests/test_bm25_host.py checks on the host path."""
import ctypes

import numpy as np
import pytest

import bm25_exact as bx
import cosine_exact as cx
from cosine_exact import ToyStemmer

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
INF = float("inf")
i32p, i64p, dblp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)


def _flat(id_lists):
    offsets = np.zeros(len(id_lists) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in id_lists], out=offsets[1:])
    return np.array([i for q in id_lists for i in q], dtype=np.int32), offsets


def _built(hip, texts, stopwords=()):
    index = hip.HipCosineIndex()
    index.build_texts(texts, sorted(cx.prepared_stopwords(stopwords)))
    return index


def _check_ids(index, model, id_lists, k1=bx.K1, b=bx.B, stems=False, what="bm25"):
    got = index.bm25_table(*_flat(id_lists), k1=k1, b=b)
    exact, terms = bx.Bm25(model, k1, b, stems).scores_from_ids(id_lists)
    bx.check(got, exact, terms, what)
    return got


def _raw_call(lib, index, id_lists, k1, b, out=None):
    ids, offsets = _flat(id_lists)
    return lib.east_hip_bm25_score_table(index._h, ids.ctypes.data_as(i32p), offsets.ctypes.data_as(i64p), ids.size, len(id_lists),
                                         ctypes.c_double(k1), ctypes.c_double(b), None if out is None else out.ctypes.data_as(dblp))


# ---- weights ------------------------------------------------------------------------------------------------------------------
def test_worked_case(hip):
    index = _built(hip, bx.WORKED_TEXTS)
    model = cx.build_model(bx.WORKED_TEXTS)
    queries = list(bx.WORKED)
    got = _check_ids(index, model, model.query_ids(queries), what="worked case")
    assert got[0, 1] == 0.0 and got[2, 0] == 0.0 and abs(got[3, 0] - 1.9731760785101862) < 1e-14
    info = index.bm25_info()
    assert info["N"] == 5 and info["avgdl"] == 2.5 and (info["k1"], info["b"]) == (1.2, 0.75) and info["weights_computed"] == 1


@pytest.mark.parametrize("k1,b", bx.PARAMETERS)
def test_every_posting_of_small_collections(hip, k1, b):
    """Single-unit queries for every unit: every posting's weight.  df = D, df = 1, a count of 1 000, n_d = 0, D = 1."""
    for texts, stop in (bx.small_collection(), bx.small_collection_full_df(), (["alpha beta alpha"], ())):
        model = cx.build_model(texts, stop)
        index = _built(hip, texts, stop)
        assert index.terms() == model.terms
        ids = [[u] for u in range(len(model.terms))] + [[0, 1, 0], [1, 1, 1, 0]]
        got = _check_ids(index, model, ids, k1, b, what="D %d k1 %g b %g" % (len(texts), k1, b))
        assert int((got > 0).sum()) >= model.postings
        info = index.bm25_info()
        assert info["N"] == bx.total(model) and info["avgdl"] == bx.avgdl(model)


# ---- parameters -------------------------------------------------------------------------------------------------------------------
def test_refused_parameters_leave_the_previous_table(hip):
    from test_gpu_top import agree, expected, orders
    lib = hip.load()
    texts, stop = bx.small_collection()
    index = _built(hip, texts, stop)
    ids = [[u] for u in range(index.n_terms)]
    table = index.bm25_table(*_flat(ids))
    for k1, b in ((-0.5, 0.75), (INF, 0.75), (float("nan"), 0.75), (1.2, -0.1), (1.2, 1.0000001), (1.2, float("nan"))):
        assert _raw_call(lib, index, ids, k1, b) == ERR_INVALID
        assert b"k1" in lib.east_hip_last_error()
        agree(index.top(1, 3), expected(table, 1, orders(table, 1, -INF), 3), (k1, b))
    assert _raw_call(lib, index, [[index.n_terms]], 1.2, 0.75) == ERR_INVALID       # (a bad id: refused as cosine refuses it)
    agree(index.top(0, 2), expected(table, 0, orders(table, 0, -INF), 2))
    assert index.bm25_info()["weights_computed"] == 1


# ---- queries ------------------------------------------------------------------------------------------------------------------------
def test_queries(hip):
    from test_gpu_top import agree, expected, orders
    lib = hip.load()
    texts, stop = bx.small_collection()
    model = cx.build_model(texts, stop)
    index = _built(hip, texts, stop)
    alpha, beta, every = (model.term_id[w] for w in ("ALPHA", "BETA", "EVERY"))
    ids = [[beta, beta, alpha], [alpha, beta, alpha, alpha], [-1, -1], [every], [], [alpha], [-1, alpha, -1], [beta, beta, alpha]]
    got = _check_ids(index, model, ids, what="queries")
    assert got[2].tobytes() == np.zeros(len(texts)).tobytes() and got[4].tobytes() == got[2].tobytes()      # +0.0, byte for byte
    assert got[0].tobytes() == got[7].tobytes() and got[5].tobytes() == got[6].tobytes()
    assert got[0, 0] > got[5, 0] > 0.0
    assert index.bm25_table(np.zeros(0, np.int32), np.zeros(1, np.int64)).shape == (0, len(texts))           # K = 0
    # out = NULL, then the ranking from source COSINE
    assert _raw_call(lib, index, ids, 1.2, 0.75) == OK
    for axis in (0, 1):
        agree(index.top(axis, 4), expected(got, axis, orders(got, axis, -INF), 4))
    assert index.bm25_table(*_flat(ids)).tobytes() == got.tobytes()


# ---- strips -------------------------------------------------------------------------------------------------------------------------
def _strip_queries(model, D):
    words = ["EVERY", "SECOND", "ODD", "ONLY0", "ONLY%d" % (D - 1), "ONLY63", "ONLY64", "GROUP0", "GROUP9", "GROUP%d" % ((D - 1) // 7)]
    single = [[model.term_id.get(w, -1)] for w in words]
    mixed = [[model.term_id.get(w, -1) for w in q.split()] for q in
             ("EVERY ONLY%d EVERY" % (D - 1), "GROUP9 ODD SECOND SECOND", "ONLY63 ONLY64 GROUP%d" % ((D - 1) // 7), "NOPE EVERY")]
    return single + mixed


@pytest.mark.parametrize("D", [1, 63, 64, 65, 257, 600])
def test_strips(hip, D):
    """Strip boundaries inside the collection (the knob at 64) and none (the default): the same bytes, both held to the
    model.  A unit whose postings lie only in the last strip (ONLY<D - 1>), lists that end at a strip's last document (ONLY63,
    ODD at D = 64) and that start at a strip's first (ONLY64, GROUP<...>).  D = 600: a workgroup per item, above 512
    documents, and with 2 000 keyphrases x 10 strips its grid loop beyond 16 384 workgroups."""
    lib = hip.load()
    texts = cx.one_line_documents(D)
    model = cx.build_model(texts)
    index = _built(hip, texts)
    ids = _strip_queries(model, D)
    if D == 600:
        ids = ids + [[u % len(model.terms)] for u in range(2000)]
    default = _check_ids(index, model, ids, what="D %d" % D)
    try:
        for strip in (64, 7, 1 << 20):
            assert lib.east_hip_debug_set_bm25_strip(strip) == OK
            assert index.bm25_table(*_flat(ids)).tobytes() == default.tobytes(), strip
    finally:
        assert lib.east_hip_debug_set_bm25_strip(0) == OK
    assert index.bm25_table(*_flat(ids)).tobytes() == default.tobytes()


@pytest.mark.parametrize("K", [1, 70000])
def test_many_keyphrases_of_one_unit(hip, K):
    """K = 70 000 at D = 3: four wavefronts a workgroup, the grid loop beyond 16 384 workgroups."""
    texts = cx.three_documents()
    model = cx.build_model(texts)
    index = _built(hip, texts)
    ids = [[k % len(model.terms)] for k in range(K)]
    got = _check_ids(index, model, ids, what="K %d" % K)
    V = len(model.terms)
    if K > V:
        assert got[V:2 * V].tobytes() == got[:V].tobytes() and got[K - 1].tobytes() == got[(K - 1) % V].tobytes()


# ---- stems ----------------------------------------------------------------------------------------------------------------------------
def test_stems_and_class_maps(hip):
    from east import relevance
    texts = ["testing the tests of a test", "tests and foxes", "fox testing", "", "foxes foxes tested"]
    stop = ["the", "and"]
    queries = ["TESTS FOX", "TESTING TESTING FOXES", "THE", "NOPE TEST", "TESTED"]
    model = cx.build_model(texts, stop, ToyStemmer())
    m = relevance.BM25RelevanceMeasure("stems", stopwords=stop, stemmer=ToyStemmer())
    m.set_text_collection(texts)
    exact, terms = bx.Bm25(model, stems=True).scores(queries)
    bx.check(m.relevance_table(queries), exact, terms, "stems")
    index = m.index
    assert index.info()["classes"] == model.n_classes
    # an arbitrary class map, then back to the terms
    V = len(model.terms)
    term_class = [(t * 5) % 3 for t in range(V)]
    order = {}
    term_class = [order.setdefault(c, len(order)) for c in term_class]          # (classes numbered by their smallest term)
    other = model.with_classes(term_class, len(order))
    index.set_classes(term_class, len(order))
    _check_ids(index, other, [[c] for c in range(len(order))] + [[0, 1, 0, -1]], stems=True, what="class map")
    index.set_classes([], 0)
    assert index.info()["classes"] == 0
    _check_ids(index, model, [[t] for t in range(V)], what="back to the terms")


# ---- cache ------------------------------------------------------------------------------------------------------------------------------
def test_weights_cache(hip):
    texts, stop = bx.small_collection()
    model = cx.build_model(texts, stop)
    index = _built(hip, texts, stop)
    ids = _flat([[u] for u in range(len(model.terms))] + [[0, 1, 1]])
    info = index.bm25_info()
    assert info["weights_computed"] == 0 and np.isnan(info["k1"]) and np.isnan(info["b"])
    assert info["N"] == bx.total(model) and info["avgdl"] == bx.avgdl(model)
    first = index.bm25_table(*ids, k1=1.2, b=0.75)
    assert index.bm25_info()["weights_computed"] == 1
    assert index.bm25_table(*ids, k1=1.2, b=0.75).tobytes() == first.tobytes()
    assert index.bm25_info()["weights_computed"] == 1                             # the same parameters: + 0
    other = index.bm25_table(*ids, k1=2.0, b=0.75)
    info = index.bm25_info()
    assert info["weights_computed"] == 2 and (info["k1"], info["b"]) == (2.0, 0.75) and other.tobytes() != first.tobytes()
    assert index.bm25_table(*ids, k1=1.2, b=0.5).tobytes() != first.tobytes() and index.bm25_info()["weights_computed"] == 3
    assert index.bm25_table(*ids, k1=1.2, b=0.75).tobytes() == first.tobytes()    # the first parameters again: + 1, the same bytes
    assert index.bm25_info()["weights_computed"] == 4
    V = len(model.terms)
    index.set_classes(list(range(V)), V)                                           # (the identity: the same scores, new weights)
    assert np.isnan(index.bm25_info()["k1"])
    assert index.bm25_table(*ids, k1=1.2, b=0.75).tobytes() == first.tobytes() and index.bm25_info()["weights_computed"] == 5
    index.set_classes([], 0)
    index.bm25_table(*ids, k1=1.2, b=0.75)
    assert index.bm25_info()["weights_computed"] == 6
    # a rebuild with other texts: the count starts over, N and avgdl are the new collection's
    texts2 = cx.three_documents()
    model2 = cx.build_model(texts2)
    index.build_texts(texts2)
    info = index.bm25_info()
    assert info["weights_computed"] == 0 and np.isnan(info["k1"]) and info["N"] == bx.total(model2) and info["avgdl"] == bx.avgdl(model2)
    _check_ids(index, model2, [[u] for u in range(len(model2.terms))], what="rebuilt")
    assert index.bm25_info()["weights_computed"] == 1


# ---- beside cosine --------------------------------------------------------------------------------------------------------------------------
def test_beside_the_cosine_scores(hip):
    lib = hip.load()
    texts, stop = bx.small_collection()
    model = cx.build_model(texts, stop)
    ids = _flat([[u] for u in range(len(model.terms))] + [[0, 1, 1], [2, 0]])
    index = _built(hip, texts, stop)
    tfidf, tf = index.score_table(*ids, tfidf=True), index.score_table(*ids, tfidf=False)
    bm = index.bm25_table(*ids)
    assert index.info()["score_us"] >= 0
    assert index.score_table(*ids, tfidf=True).tobytes() == tfidf.tobytes() and index.score_table(*ids, tfidf=False).tobytes() == tf.tobytes()
    assert index.bm25_table(*ids).tobytes() == bm.tobytes() and index.bm25_info()["weights_computed"] == 1
    fresh = _built(hip, texts, stop)                                                # the order reversed on a fresh index
    assert fresh.bm25_table(*ids).tobytes() == bm.tobytes()
    assert fresh.score_table(*ids, tfidf=True).tobytes() == tfidf.tobytes() and fresh.score_table(*ids, tfidf=False).tobytes() == tf.tobytes()
    assert fresh.bm25_table(*ids).tobytes() == bm.tobytes()
    # NOT_BUILT before any build and after east_hip_reset
    handle = hip.HipIndex()
    empty = hip.HipCosineIndex(index=handle)
    buf = np.zeros(5)
    for _ in range(2):
        assert lib.east_hip_bm25_info(handle._h, buf.ctypes.data_as(dblp), 5) == ERR_NOT_BUILT
        assert b"no cosine index has been built" in lib.east_hip_last_error()
        assert _raw_call(lib, empty, [[0]], 1.2, 0.75) == ERR_NOT_BUILT
        assert b"no cosine index has been built" in lib.east_hip_last_error()
        empty.build_texts(texts)
        assert lib.east_hip_bm25_info(handle._h, buf.ctypes.data_as(dblp), 5) == OK
        lib.east_hip_reset(handle._h)


# ---- consumers --------------------------------------------------------------------------------------------------------------------------------
def test_consumers_of_the_table(hip):
    import similar_exact
    from east import applications
    from test_gpu_top import agree, expected, orders
    texts = cx.one_line_documents(20)
    model = cx.build_model(texts)
    index = _built(hip, texts)
    words = ["EVERY", "SECOND", "ODD", "GROUP0", "GROUP1", "GROUP2", "ONLY3", "ONLY4"]
    ids = [[model.term_id[w]] for w in words] + [[model.term_id["GROUP0"], model.term_id["ODD"]]]
    kps = [w.lower() for w in words] + ["group0 odd"]
    table = index.bm25_table(*_flat(ids))
    for axis, n, threshold in ((0, 3, -INF), (1, 5, 0.5), (1, 64, -INF)):
        agree(index.top(axis, n, threshold), expected(table, axis, orders(table, axis, threshold), n), (axis, n))
    rows = np.arange(len(kps), dtype=np.int32)
    names = ["t%d" % d for d in range(len(texts))]
    want = applications._graph_from_array(kps, applications.ScoreTable(kps, names, table), 0.5, 0.3, 2)
    assert applications.KeyphraseGraph.from_device(kps, index.graph(rows, 0.3, 2, 0.5), 0.5, 0.3, 2) == want
    for axis, P in ((1, table), (0, np.ascontiguousarray(table.T))):
        M, L = P.shape
        assert index.similarity(axis) == (M, L)
        S, _ = index.similarity_matrix()
        want_S = similar_exact.exact(P)[0]
        assert float(np.nanmax(np.abs(S - want_S))) <= similar_exact.bound(L)
        ranked = index.similar(axis, 3)
        assert ranked.count.tolist() == [min(3, M - 1)] * M
        # the clusters of that matrix: the device's merges are the host's on the same bytes
        index.similarity(axis)
        index.clusters_build(hip.GRAPH_SOURCE_SIMILARITY)
        got = index.clusters_merges()
        host = applications._single_linkage(S)
        assert got[0].tolist() == host[0].tolist() and got[1].tolist() == host[1].tolist() and got[2].tobytes() == host[2].tobytes()


def test_measure_through_the_applications(hip):
    """relevance_top / graph / similar / clusters of the measure: the inherited code over the BM25 table."""
    from east import applications, relevance
    texts = {"t%d" % d: t for d, t in enumerate(cx.one_line_documents(12))}
    kps = ["every", "second", "odd", "group0", "group1", "only3 only4"]
    m = relevance.BM25RelevanceMeasure("words", stopwords=[])
    table = applications.keyphrases_table(kps, texts, m)
    top = applications.keyphrases_top(kps, texts, 2, "text", None, m)
    for name in texts:
        best = sorted(kps, key=lambda kp: -table[kp][name])[:2]
        assert [kp for kp, _ in top[name]] == best and top[name][0][1] == table[best[0]][name]
    assert applications.keyphrases_similar(kps, texts, 2, "keyphrase", None, m)
    assert applications.keyphrases_graph(kps, texts, 0.6, 0.3, 1, m) is not None
    found = applications.keyphrases_clusters(kps, texts, "text", None, 3, m)
    assert len(found.clusters) == 3
    assert m.index.bm25_info()["weights_computed"] == 1
    with pytest.raises(ValueError):
        m.relevance_clusters()


# ---- breadth ------------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_rounds(hip):
    from east import relevance
    above, worst = 0, 0.0
    for r in cx.fuzz_rounds()[:50]:
        stems = r["space"] == "stems"
        model = cx.build_model(r["texts"], r["stopwords"], ToyStemmer() if stems else None)
        m = relevance.BM25RelevanceMeasure(r["space"], stopwords=list(r["stopwords"]), stemmer=ToyStemmer() if stems else None)
        m.set_text_collection(r["texts"])
        exact, terms = bx.Bm25(model, stems=stems).scores(r["queries"])
        share, n, zeros_ok = bx.share_of_bound(m.relevance_table(r["queries"]), exact, terms)
        assert zeros_ok and share <= 1.0, share
        above += n
        worst = max(worst, share)
    print("bm25 fuzz: %d scores above zero, largest error %.3f of the bound (t + %d) * 2^-53" % (above, worst, bx.BOUND_EXTRA))
    assert above >= 150                                                            # (not a vacuous fuzz)


@pytest.mark.parametrize("stems", [False, True])
def test_zipf_collection(hip, stems):
    from east import relevance
    texts, queries, _ = cx.zipf_collection()
    model = cx.zipf_model(False)
    queries = queries[:1000]
    m = relevance.BM25RelevanceMeasure("stems" if stems else "words", stopwords=[], stemmer=ToyStemmer())
    m.set_text_collection(texts)
    exact, terms = bx.Bm25(model, stems=stems).scores(queries)
    bx.check(m.relevance_table(queries), exact, terms, "zipf stems" if stems else "zipf words")
