# -*- coding: utf-8 -*-
"""CPU tier: the exact model of tests/cosine_exact.py against the fixture recorded from the reference, the plain-double
restatement of test_cosine_host.py against the exact model on every collection the gpu tier uses (the check that 1e-12 is
attainable by a correct double-precision implementation with a margin of 10), the model's two paths against each other,
and what the generators claim to cover."""
import numpy as np

import cosine_exact as cx
from conftest import load_golden
from test_cosine_host import ToyStemmer, assert_scores, case_texts, restate

MARGIN_TOL = 1e-13


def _close(got, exact, tol=MARGIN_TOL):
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    assert got.shape == exact.shape
    if got.size:
        assert np.abs(got - exact).max() <= tol, np.abs(got - exact).max()
        assert np.array_equal(got == 0.0, exact == 0.0)


def _restate_against_exact(texts, queries, stopwords=(), modes=cx.MODES, fast=False):
    """restate() within 1e-13 of the exact model, in the given (space, weighting) modes."""
    from east import utils
    model = cx.build_model(texts, stopwords, ToyStemmer(), fast=fast)
    prepared = [utils.prepare_text(q) for q in queries]
    for space, weighting in modes:
        _close(restate(texts, queries, space, weighting, stopwords, ToyStemmer()), model.scores(prepared, space, weighting))
    return model


def test_toy_stemmer_is_the_fixtures():
    for word, stem in load_golden("cosine.json")["toy_stems"].items():
        assert cx.ToyStemmer().stem(word) == stem == ToyStemmer().stem(word)


def test_exact_model_reproduces_the_recorded_modes():
    from east import utils
    g = load_golden("cosine.json")
    n = 0
    for case in g["cases"]:
        texts = case_texts(g, case)
        prepared = [utils.prepare_text(q) for q in case["queries"]]
        for mode in case["modes"]:
            stop = g["stopwords"] if mode["stopwords"] else ()
            model = cx.build_model(texts, stop, cx.ToyStemmer() if mode["space"] == "stems" else None)
            got = model.scores(prepared, mode["space"], mode["weighting"])
            assert_scores(got.tolist(), mode["scores"], 1e-12)
            _close(restate(texts, case["queries"], mode["space"], mode["weighting"], stop, ToyStemmer()), got)
            n += 1
    assert n == 15


def test_restatement_margin_on_the_fuzz_rounds():
    for r in cx.fuzz_rounds():
        _restate_against_exact(r["texts"], r["queries"], r["stopwords"], [(r["space"], r["weighting"])])


def test_restatement_margin_on_the_small_collections():
    texts, families, near = cx.piece_collection()
    _restate_against_exact(texts, cx.piece_queries(families, near), modes=[("words", "tf"), ("words", "tf-idf")])
    texts, chain = cx.prefix_chain()
    _restate_against_exact(texts, chain[:8] + [chain[10] + " " + chain[200], chain[303] + " " + chain[303] + "A"],
                           modes=[("words", "tf-idf")])
    stop, texts, queries, _ = cx.stopword_case()
    _restate_against_exact(texts, queries, stop)
    _restate_against_exact(cx.all_stop_texts(), queries, stop)
    for texts in cx.degenerate_collections().values():
        _restate_against_exact(texts, cx.DEGENERATE_QUERIES)
    _restate_against_exact(cx.slice_documents(), cx.SLICE_QUERIES)
    texts, queries = cx.two_mib_collection()
    _restate_against_exact(texts, queries, fast=True)


def _word_queries(model, ids, offsets, n):
    """The first n id queries as words (-1 = an absent word)."""
    return [" ".join(model.terms[i] if i >= 0 else "ABSENTWORD" for i in q) for q in cx.split_ids(ids, offsets)[:n]]


def test_restatement_margin_on_the_score_shapes():
    texts = cx.three_documents()
    model = cx.build_model(texts)
    ids, offsets = cx.id_queries(150_000, len(model.terms), seed=21)
    queries = _word_queries(model, ids, offsets, 3000)
    queries.append(" ".join(_word_queries(model, *cx.id_queries(1000, len(model.terms), seed=23, q_max=1), n=1000)))
    _restate_against_exact(texts, queries)
    for D in (255, 256, 257, 70_000):
        texts = cx.one_line_documents(D)
        queries = ["EVERY", "SECOND EVERY", "ONLY5 ODD", "GROUP3 ONLY%d" % (D - 1), "EVERY EVERY NOPE GROUP0"]
        _restate_against_exact(texts, queries, modes=[("words", "tf-idf"), ("stems", "tf")], fast=True)


def test_restatement_margin_on_the_zipf_collection():
    """All 64 documents and all 2 000 queries; with and without the stopwords, both spaces and both weightings."""
    texts, queries, top = cx.zipf_collection()
    for stop, modes in (((), [("words", "tf-idf"), ("stems", "tf")]), (top, [("stems", "tf-idf"), ("words", "tf")])):
        model = cx.zipf_model(bool(stop))
        for space, weighting in modes:
            _close(restate(texts, queries, space, weighting, stop, ToyStemmer()), model.scores(queries, space, weighting))


def test_fast_path_is_the_slow_path():
    cases = [(r["texts"], r["stopwords"]) for r in cx.fuzz_rounds()[:40]]
    stop, texts, _, _ = cx.stopword_case()
    cases += [(texts, stop), (cx.all_stop_texts(), stop), (cx.slice_documents(), ["W00001"]), (cx.piece_collection()[0], ())]
    cases += [(t, ()) for t in cx.degenerate_collections().values()]
    cases.append((cx.two_mib_collection()[0][:4], ["the"]))
    for texts, stopwords in cases:
        slow = cx.build_model(texts, stopwords, cx.ToyStemmer())
        fast = cx.build_model(texts, stopwords, cx.ToyStemmer(), fast=True)
        assert slow.structures() == fast.structures()
        assert slow.stem_class == fast.stem_class


def _byte_widths(token):
    return set(len(c.encode("utf-8")) for c in token)


def test_generators_cover_what_the_gpu_tests_claim():
    # the fuzz: tokens of exactly 2 and exactly 3 code points of 1-, 2-, 3- and 4-byte sequences; empty texts; junk
    seen, empty, modes, stopped = set(), 0, set(), 0
    for r in cx.fuzz_rounds():
        assert 1 <= len(r["texts"]) <= 6
        empty += sum(1 for t in r["texts"] if not t)
        modes.add((r["space"], r["weighting"], bool(r["stopwords"])))
        for text in r["texts"]:
            for tok in cx.all_tokens(text):
                if len(tok) in (2, 3) and len(_byte_widths(tok)) == 1:
                    seen.add((len(tok), _byte_widths(tok).pop()))
    assert seen == set((n, w) for n in (2, 3) for w in (1, 2, 3, 4))
    assert len(cx.fuzz_rounds()) >= 150 and empty >= 20 and len(modes) == 8
    assert any(b"\xed\xa0\x80" in t for r in cx.fuzz_rounds() for t in r["texts"])
    tokens = set(tok for r in cx.fuzz_rounds() for t in r["texts"] for tok in cx.all_tokens(t))
    assert {"FOX", "ΣΑΣ", "ßßß", "ǄǄǄ", "İİİ", "'''", "123", "٣٤٥", "DON'T"} <= tokens

    # the pieces: every length, and the family of every long one
    texts, families, near = cx.piece_collection()
    model = cx.build_model(texts)
    lengths = set(len(t) for t in model.terms)
    assert {3, 2047, 2048, 2049, 4096, 4097, 4095, 6145, 6146, 6144} <= lengths
    assert len(families) == 2 * len(cx.PIECE_LENGTHS)
    for fam in families:
        assert all(w in model.term_id for w in fam)
        if len(fam[0]) >= 2047:
            n = len(fam[0])
            diffs = set(next(i for i in range(n) if w[i] != fam[0][i]) for w in fam[1:] if len(w) == n)
            assert diffs == set(p for p in (0, 2046, 2047, n - 1) if p < n)          # a first, a middle, a last piece
            assert fam[0][:-1] in fam and sum(1 for w in fam if len(w) == n + 1 and w[:n] == fam[0]) == 1
    assert not any(w in model.term_id for w in near)
    assert max(model.df) == 5 and min(model.df) == 1 and max(max(c.values()) for c in model.counts) > 1

    # the chain of prefixes: more tokens than 8 hash bits have values, each a proper prefix of every earlier one
    texts, chain = cx.prefix_chain()
    model = cx.build_model(texts)
    assert model.terms == chain and len(chain) > 256 and model.kept_tokens == len(chain) + 2
    assert all(len(b) < len(a) and a.startswith(b) for a, b in zip(chain, chain[1:]))
    assert {2047, 2048, 2049, 4095, 4096, 4097, 3} <= set(len(w) for w in chain)

    # the stopword list and its two extremes
    stop, texts, queries, (long_in, long_out) = cx.stopword_case()
    assert "" in stop and len(stop) != len(set(stop)) and any(len(w) == 2 for w in stop) and len(long_in) == 4097
    model = cx.build_model(texts, stop)
    assert long_in in model.stop and long_in not in model.term_id and long_out in model.stop
    assert any(long_in in cx.all_tokens(t) for t in texts) and not any(long_out in cx.all_tokens(t) for t in texts)
    assert model.n_d[1] == 0 and len([t for t in cx.all_tokens(texts[1]) if len(t) >= 3]) > 0      # only stopwords
    assert model.n_d[0] > 0 and long_in[:-1] in model.term_id
    empty = cx.build_model(cx.all_stop_texts(), stop)
    assert empty.kept_tokens > 0 and empty.terms == [] and empty.postings == 0

    # the norm's slices; a term in every document and one of df 1; counts above 1
    model = cx.build_model(cx.slice_documents())
    assert tuple(model.postings_per_doc()) == cx.SLICE_POSTINGS == (0, 1, 63, 64, 65, 127, 128, 129, 4097)
    assert max(max(c.values()) for c in model.counts if c) > 1
    for D in (255, 257):
        model = cx.build_model(cx.one_line_documents(D), fast=True)
        assert model.df[model.term_id["EVERY"]] == D and model.df[model.term_id["SECOND"]] == (D + 1) // 2
        assert model.df[model.term_id["ONLY7"]] == 1

    # the counts around the tiles of the prefix sums: the five counts at n, or one apart from each other
    assert cx.SCAN_TILE_SIZES == (4095, 4096, 4097, 8192, 8193)
    for n in cx.SCAN_TILE_SIZES:
        cases = cx.scan_tile_collections(n)
        for name, (texts, stop) in cases.items():
            model = cx.build_model(texts, stop, cx.ToyStemmer(), fast=True)
            counts = (sum(len(cx.all_tokens(t)) for t in texts), model.kept_tokens, model.words, len(model.terms), model.postings)
            assert counts == ((n + 2, n + 1, n + 1, n, n) if stop else (n, n, n, n, n)), (n, name)
            assert min(len(t) for t in model.terms) >= 3 and model.cls_postings == model.n_classes == n
            assert sum(model.n_d) == n and all(q and all(len(i) > 0 for i in model.query_ids([q])) for q in cx.scan_tile_queries(n))
        assert [len(t) for t, _ in cases.values()] == [1, 1, 3] and [bool(s) for _, s in cases.values()] == [False, True, False]
        assert [d for d in cx.build_model(*cases["three documents"]).n_d] == [len(range(i, n, 3)) for i in range(3)]

    # the Zipf collection: long lists, classes of several members in one document, non-ASCII terms
    texts, queries, top = cx.zipf_collection()
    assert len(texts) == 64 and len(queries) == 2000 and len(top) == 50
    assert min(len(t) for t in texts) <= 1 << 10 and max(len(t) for t in texts) == 1 << 20
    model = cx.zipf_model(False)
    assert max(model.df) == 64 and min(model.df) == 1 and max(model.postings_per_doc()) > 4097
    assert model.n_classes < len(model.terms) and model.cls_postings < model.postings
    assert any(ord(t[0]) > 0x0390 for t in model.terms)
    stopped = cx.zipf_model(True)
    assert len(stopped.terms) == len(model.terms) - 50 and stopped.kept_tokens == model.kept_tokens
    ids = stopped.query_ids(queries)
    assert any(q == [] for q in ids) and any(-1 in q for q in ids) and any(len(q) == 4 for q in ids)
