# -*- coding: utf-8 -*-
"""gpu tier: the cosine term index on the device (csrc/cosine.h) against the exact host model of tests/cosine_exact.py --
the integer structures (terms, counts of east_hip_cosine_info, look-ups) and every score of every document, to 1e-12
absolute, the same zeros, and the relative bound of DESIGN.md 9 ("How it is tested").  The collections are those whose
attainability test_cosine_exact_host.py checks on the host."""
import numpy as np
import pytest

import cosine_exact as cx
from cosine_exact import ToyStemmer, check_scores

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("built", "n_docs", "kept_tokens", "words", "terms", "classes", "postings")
JOINED = 1 << 60                                 # hip_backend.JOIN_FREE_*_BYTES that no collection reaches


def _measure(space, weighting, stopwords=()):
    from east import relevance
    return relevance.CosineRelevanceMeasure(space, weighting, stopwords=list(stopwords),
                                            stemmer=ToyStemmer() if space == "stems" else None)


def _info(index):
    info = index.info()
    return {name: info[name] for name in INFO_FIELDS}


def check_index(measure_or_index, model, texts, stems=False):
    """The terms, the counts and the look-ups of a built index against the model."""
    from east import hip_backend
    index = measure_or_index if isinstance(measure_or_index, hip_backend.HipCosineIndex) else measure_or_index.index
    assert index.terms() == model.terms
    assert _info(index) == model.info(stems)
    present, absent = cx.lookup_probes(model, texts)
    assert index.lookup(present).tolist() == [model.term_id[t] for t in present]
    got = index.lookup(absent).tolist()
    assert got == [-1] * len(absent), [w[:40] for w, g in zip(absent, got) if g != -1][:5]


def check_measure(measure, model, texts, queries):
    """check_index + every score of the measure's table against the model."""
    stems = measure.vector_space == "stems"
    check_index(measure, model, texts, stems)
    table = measure.relevance_table(queries)
    assert table.shape == (len(queries), len(texts))
    q_len = [len(q) for q in model.query_ids(queries, stems)]
    check_scores(table, model.scores(queries, measure.vector_space, measure.term_weighting), model.postings_per_doc(stems), q_len)
    return table


def _run(texts, queries, space, weighting, stopwords=()):
    m = _measure(space, weighting, stopwords)
    m.set_text_collection(texts)
    model = cx.build_model(texts, stopwords, ToyStemmer() if space == "stems" else None, fast=sum(len(t) for t in texts) > 1 << 18)
    return m, model, check_measure(m, model, texts, queries)


def _flat(id_lists):
    offsets = np.zeros(len(id_lists) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in id_lists], out=offsets[1:])
    return np.array([i for q in id_lists for i in q], dtype=np.int32), offsets


def check_id_scores(index, model, ids, offsets, tfidf, stems=False):
    table = index.score_table(ids, offsets, tfidf)
    exact = model.scores_from_ids(cx.split_ids(ids, offsets), tfidf, stems)
    check_scores(table, exact, model.postings_per_doc(stems), np.diff(offsets))
    return table


# ---- a. Unicode and malformed input, fuzzed ------------------------------------------------------------------------------
def test_fuzz_of_unicode_and_malformed_input(hip):
    rounds = cx.fuzz_rounds()
    assert len(rounds) >= 150
    positive = 0
    for r in rounds:
        _, _, table = _run(r["texts"], r["queries"], r["space"], r["weighting"], r["stopwords"])
        positive += int((table > 0).sum())
    assert positive >= 500                                               # (not a vacuous fuzz: scores above zero in number)


# ---- b. both entry points -----------------------------------------------------------------------------------------------
def _through(hip, monkeypatch, joined, texts, queries, space, weighting, stopwords):
    monkeypatch.setattr(hip, "JOIN_FREE_MIN_BYTES", JOINED if joined else 0)
    monkeypatch.setattr(hip, "JOIN_FREE_RING_BYTES", JOINED if joined else 0)
    assert hip._join_free(hip._raw_texts(texts)) == (not joined)
    m = _measure(space, weighting, stopwords)
    m.set_text_collection(texts)
    return m.index.terms(), _info(m.index), m.relevance_table(queries).tobytes()


def test_both_entry_points_give_the_same_index(hip, monkeypatch):
    cases = [(r["texts"], r["queries"], r["space"], r["weighting"], r["stopwords"]) for r in cx.fuzz_rounds()]
    texts, queries = cx.two_mib_collection()
    assert sum(len(t) for t in texts) >= 2 << 20
    cases += [(texts, queries, "words", "tf-idf", ()), (texts, queries, "stems", "tf", queries[0].split())]
    for case in cases:
        separate = _through(hip, monkeypatch, False, *case)
        joined = _through(hip, monkeypatch, True, *case)
        assert separate == joined


# ---- c. piece boundaries ---------------------------------------------------------------------------------------------------
def test_piece_boundaries_and_forced_collisions(hip):
    texts, families, near = cx.piece_collection()
    queries = cx.piece_queries(families, near)
    members = [w for fam in families for w in fam]
    model = cx.build_model(texts)
    lib = hip.load()

    def run():
        m = _measure("words", "tf-idf")
        m.set_text_collection(texts)
        table = check_measure(m, model, texts, queries)
        assert m.index.lookup(members).tolist() == [model.term_id[w] for w in members]
        assert m.index.lookup(near).tolist() == [-1] * len(near)
        return m.index.terms(), _info(m.index), table.tobytes(), m.index.info()["hash_attempts"]

    plain = run()
    assert plain[3] == 1
    for bits in (1, 2, 8):
        assert lib.east_hip_debug_set_term_hash_bits(bits) == 0
        try:
            forced = run()
        finally:
            assert lib.east_hip_debug_set_term_hash_bits(0) == 0
        assert forced[3] == 2, bits
        assert forced[:3] == plain[:3], bits


def test_collisions_that_differ_in_length_only(hip):
    """Under a truncated hash the colliding tokens of prefix_chain() are prefixes of their first occurrence: only the
    comparison of the lengths tells them apart."""
    texts, chain = cx.prefix_chain()
    queries = chain[:8] + [chain[10] + " " + chain[200], chain[303] + " " + chain[303] + "A"]
    model = cx.build_model(texts)
    lib = hip.load()
    results = []
    for bits in (0, 1, 2, 8):
        assert lib.east_hip_debug_set_term_hash_bits(bits) == 0
        try:
            m = _measure("words", "tf-idf")
            m.set_text_collection(texts)
            table = check_measure(m, model, texts, queries)
            assert m.index.lookup(chain).tolist() == list(range(len(chain)))
            assert m.index.info()["hash_attempts"] == (2 if bits else 1), bits
            results.append((m.index.terms(), _info(m.index), table.tobytes()))
        finally:
            assert lib.east_hip_debug_set_term_hash_bits(0) == 0
    assert all(r == results[0] for r in results)


# ---- d. stopword lists -------------------------------------------------------------------------------------------------------
def test_stopword_list_of_every_kind(hip):
    stop, texts, queries, (long_in, long_out) = cx.stopword_case()
    for space, weighting in cx.MODES:
        m, model, table = _run(texts, queries, space, weighting, stop)
        assert m.index.lookup([long_in, long_out, "THE", "ЖУК", "STRASSE", "STRAßE"]).tolist() == [-1] * 6
        assert model.n_d[1] == 0 and not table[:, 1].any()                  # the document of stopwords only: norm 1, zeros
        assert (table[:, 0] > 0).any() and (table[:, 2] > 0).any()
        # every kept word a stopword
        m, model, table = _run(cx.all_stop_texts(), queries, space, weighting, stop)
        info = m.index.info()
        assert info["kept_tokens"] > 0 and info["terms"] == 0 and info["postings"] == 0 and not table.any()
        assert m.index.lookup(sorted(model.stop) + ["CAT"]).tolist() == [-1] * (len(model.stop) + 1)


# ---- e. degenerate collections ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cx.degenerate_collections()))
def test_degenerate_collections(hip, name):
    texts = cx.degenerate_collections()[name]
    for space, weighting in cx.MODES:
        m, model, table = _run(texts, cx.DEGENERATE_QUERIES, space, weighting)
        stems = space == "stems"
        units = model.space(stems)[2]
        if name in ("all empty", "short tokens only", "one empty text alone"):
            assert units == 0 and model.kept_tokens == 0 and not table.any()
        # straight to the index: empty queries, queries of -1 only, normal ones
        id_lists = [[], [-1, -1, -1], [], list(range(units)), [-1] + [0] * min(units, 1), []]
        ids, offsets = _flat(id_lists)
        direct = check_id_scores(m.index, model, ids, offsets, weighting == "tf-idf", stems)
        assert not direct[[0, 1, 2, 5]].any()
        if name == "two identical":
            assert np.array_equal(table[:, 0], table[:, 1]) and table[1, 0] > 0


# ---- f. score kernel shapes --------------------------------------------------------------------------------------------------
def _three_document_index(hip):
    texts = cx.three_documents()
    index = hip.HipCosineIndex()
    index.build_texts(texts)
    model = cx.build_model(texts)
    check_index(index, model, texts)
    return index, model


@pytest.mark.parametrize("K", [1, 65_535, 65_536, 65_537, 150_000])
def test_number_of_queries(hip, K):
    index, model = _three_document_index(hip)
    ids, offsets = cx.id_queries(150_000, len(model.terms), seed=21)
    ids, offsets = ids[:offsets[K]], offsets[:K + 1]
    for tfidf in (True, False):
        table = check_id_scores(index, model, ids, offsets, tfidf)
        assert table.shape == (K, 3) and (table[-1] > 0).any() == bool((ids[offsets[K - 1]:] >= 0).any())
    index.close()


def test_long_query_and_its_permutation(hip):
    index, model = _three_document_index(hip)
    rng = np.random.default_rng(23)
    one = rng.integers(-1, len(model.terms), size=1000).astype(np.int32)
    other = rng.permutation(one)
    assert (one == -1).sum() > 10 and not np.array_equal(one, other)
    ids, offsets = _flat([one.tolist(), other.tolist(), one[:1].tolist()])
    for tfidf in (True, False):
        table = check_id_scores(index, model, ids, offsets, tfidf)       # both rows against the same exact scores
        assert np.array_equal(table[0] == 0.0, table[1] == 0.0) and (table[0] > 0).all()
    index.close()


@pytest.mark.parametrize("D", [255, 256, 257, 70_000])
def test_number_of_documents_and_long_posting_lists(hip, D):
    texts = cx.one_line_documents(D)
    queries = ["EVERY", "SECOND EVERY", "ONLY5 ODD", "GROUP3 ONLY%d" % (D - 1), "EVERY EVERY NOPE GROUP0"]
    for space, weighting in (("words", "tf-idf"), ("stems", "tf")):
        m, model, table = _run(texts, queries, space, weighting)
        assert model.df[model.term_id["EVERY"]] == D and (table[0] > 0).all()
        assert np.array_equal(table[2] > 0, (np.arange(D) % 2 == 1) | (np.arange(D) == 5))
        assert (table[3] > 0).sum() == 8                                     # the 7 documents of a group and the last one


def test_documents_on_both_sides_of_the_norm_slices(hip):
    texts = cx.slice_documents()
    for space, weighting in cx.MODES:
        m, model, table = _run(texts, cx.SLICE_QUERIES, space, weighting)
        assert tuple(model.postings_per_doc()) == cx.SLICE_POSTINGS
        assert not table[:, 0].any() and (table[0, 1:] > 0).all()


# ---- g. the full mode matrix where lists are long ----------------------------------------------------------------------------
@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("space", ["words", "stems"])
def test_mode_matrix_on_the_zipf_collection(hip, space, stop):
    texts, queries, top = cx.zipf_collection()
    model = cx.zipf_model(stop)
    for weighting in ("tf", "tf-idf"):
        m = _measure(space, weighting, top if stop else ())
        m.set_text_collection(texts)
        table = check_measure(m, model, texts, queries)
        assert (table > 0).mean() > 0.1
        if space == "stems":
            assert m.index.info()["classes"] == model.n_classes < len(model.terms)


# ---- h. classes through the C ABI ----------------------------------------------------------------------------------------------
def test_classes_through_the_c_abi(hip):
    texts, _, _ = cx.zipf_collection()
    model = cx.zipf_model(False)
    V = len(model.terms)
    index = hip.HipCosineIndex()
    index.build_texts(texts)
    term_ids, term_off = cx.id_queries(3000, V, seed=31)
    before = [index.score_table(term_ids, term_off, tfidf).tobytes() for tfidf in (False, True)]

    # the identity: the classes are the terms
    index.set_classes(np.arange(V), V)
    same = model.with_classes(range(V), V)
    assert _info(index) == same.info(True) and same.cls_postings == model.postings
    for tfidf in (False, True):
        assert check_id_scores(index, same, term_ids, term_off, tfidf, True).tobytes() == before[int(tfidf)]

    # every term in one class: one posting per document, its count n_d
    index.set_classes(np.zeros(V, dtype=np.int32), 1)
    one = model.with_classes([0] * V, 1)
    assert _info(index) == one.info(True) and one.cls_postings == sum(1 for n in model.n_d if n)
    assert [c.get(0, 0) for c in one.cls_counts] == model.n_d
    table = check_id_scores(index, one, np.zeros(1, dtype=np.int32), np.array([0, 1]), False, True)
    assert np.array_equal(table[0], np.array([1.0 if n else 0.0 for n in model.n_d]))

    # a random many-to-one map, the classes renumbered by their smallest term id
    rng = np.random.default_rng(32)
    number = {}
    term_class = [number.setdefault(c, len(number)) for c in rng.integers(0, V // 3, size=V).tolist()]
    merged = model.with_classes(term_class, len(number))
    index.set_classes(term_class, len(number))
    assert _info(index) == merged.info(True) and merged.cls_postings < model.postings
    assert max(max(c.values()) for c in merged.cls_counts) > max(max(c.values()) for c in model.counts)
    ids, offsets = _flat([[c] for c in range(len(number))])                # count / n_d / norm: the merged counts show
    for tfidf in (False, True):
        check_id_scores(index, merged, ids, offsets, tfidf, True)

    # back to the terms
    index.set_classes([], 0)
    assert _info(index) == model.info(False)
    assert [index.score_table(term_ids, term_off, tfidf).tobytes() for tfidf in (False, True)] == before
    index.close()


# ---- i. cached state ------------------------------------------------------------------------------------------------------------
def test_weightings_alternate_on_one_index(hip):
    texts, queries = cx.two_mib_collection()
    model = cx.build_model(texts, (), ToyStemmer(), fast=True)
    index = hip.HipCosineIndex()
    index.build_texts(texts)
    for stems in (False, True):
        if stems:
            index.set_classes(model.term_class, model.n_classes)
        ids, offsets = _flat(model.query_ids(queries, stems))
        rows = [check_id_scores(index, model, ids, offsets, tfidf, stems).tobytes() for tfidf in (False, True, False, True)]
        assert rows[0] == rows[2] and rows[1] == rows[3] and rows[0] != rows[1]
    index.close()


def _fresh(texts, queries, space, weighting, stopwords=()):
    m = _measure(space, weighting, stopwords)
    m.set_text_collection(texts)
    return m.index.terms(), _info(m.index), m.relevance_table(queries).tobytes()


def test_rebuilds_on_one_measure(hip):
    """Large, small, large again, and the same across east_hip_reset: every result is a fresh measure's."""
    big, big_queries, _ = cx.zipf_collection()
    small = next(r for r in cx.fuzz_rounds() if len(r["texts"]) > 2 and not r["stopwords"] and sum(len(t) for t in r["texts"]) > 300)
    for space, weighting in (("words", "tf-idf"), ("stems", "tf")):
        want_big = _fresh(big, big_queries, space, weighting)
        want_small = _fresh(small["texts"], small["queries"], space, weighting)
        assert want_big[1]["terms"] > want_small[1]["terms"] > 0
        m = _measure(space, weighting)
        for texts, queries, want in ((big, big_queries, want_big), (small["texts"], small["queries"], want_small),
                                     (big, big_queries, want_big)):
            m.set_text_collection(texts)
            assert (m.index.terms(), _info(m.index), m.relevance_table(queries).tobytes()) == want
        assert hip.load().east_hip_reset(m.index._h) == 0
        assert m.index.info()["built"] == 0
        for texts, queries, want in ((small["texts"], small["queries"], want_small), (big, big_queries, want_big)):
            m.set_text_collection(texts)
            assert (m.index.terms(), _info(m.index), m.relevance_table(queries).tobytes()) == want


def test_easa_build_between_cosine_builds_on_a_shared_handle(hip):
    from east import exceptions, utils
    big, big_queries, _ = cx.zipf_collection()
    model = cx.zipf_model(False)
    ids, offsets = _flat(model.query_ids(big_queries))
    idx = hip.HipIndex()
    cos = hip.HipCosineIndex(index=idx)
    cos.build_texts(big)
    table = check_id_scores(cos, model, ids, offsets, True)
    a_texts = [b"The quick brown fox jumps", b"XABXAC suffix arrays of the texts"]
    idx.build_texts(a_texts)
    qs, qo = hip.pack_queries([utils.prepare_text(k) for k in ("quick fox", "ABC", "suffix")])
    easa = idx.score_table(qs, qo)
    assert easa.any()
    assert cos.score_table(ids, offsets, True).tobytes() == table.tobytes()       # the EASA build left the cosine index alone
    small = ["alpha beta gamma", "beta gamma delta delta"]
    cos.build_texts(small)
    small_model = cx.build_model(small)
    check_index(cos, small_model, small)
    check_id_scores(cos, small_model, *_flat(small_model.query_ids(["BETA DELTA NOPE"])), True)
    assert np.array_equal(idx.score_table(qs, qo), easa)
    assert hip.load().east_hip_reset(idx._h) == 0                                 # releases the large build scratch
    assert cos.info()["built"] == 0
    with pytest.raises(exceptions.HipBackendError):
        cos.score_table(ids, offsets, True)
    cos.build_texts(big)
    check_index(cos, model, big)
    assert cos.score_table(ids, offsets, True).tobytes() == table.tobytes()
    idx.build_texts(a_texts)
    assert np.array_equal(idx.score_table(qs, qo), easa)
    assert cos.score_table(ids, offsets, True).tobytes() == table.tobytes()
    idx.close()


# ---- k. counts on both sides of a tile of the prefix sums ------------------------------------------------------------------------
@pytest.mark.parametrize("n", cx.SCAN_TILE_SIZES)
def test_counts_on_both_sides_of_a_scan_tile(hip, n):
    """Every count of a build is the last word of a prefix sum over one element more than it has inputs: tokens, kept
    tokens, words, terms, postings (and, under stems, the classes' postings) at n, n + 1 and n + 2 around one and two
    tiles of 4096, in one document and dealt over three."""
    for name, (texts, stop) in cx.scan_tile_collections(n).items():
        for space, weighting in (("words", "tf-idf"), ("stems", "tf")):
            m, model, table = _run(texts, cx.scan_tile_queries(n), space, weighting, stop)
            extra = 1 if stop else 0
            assert _info(m.index)["kept_tokens"] == _info(m.index)["words"] == n + extra, name
            assert _info(m.index)["terms"] == _info(m.index)["postings"] == n, name
            assert (table[:3] > 0).any(axis=1).all() and (table[3:] > 0).any(axis=1).all(), name
            assert m.index.lookup(["THE", "AB"]).tolist() == [-1, -1]
