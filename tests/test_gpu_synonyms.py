# -*- coding: utf-8 -*-
"""gpu tier: synonym extraction on the device (csrc/synonyms.h through include/east_hip.h) against the exact host model of
tests/synonyms_exact.py and the reference's recorded results (tests/golden/synonyms.json).  Which features a row holds and
which pairs share a feature are compared with ==; I and the similarities to 1e-12 (synonyms_exact.ABS_TOL).  The worst
deviations are printed in front of the assertions (run with -s to see them).

The pair kernel takes tiles of SRC = 16 sources x TGT = 256 targets and stages CHUNK (128, here a few dozen through
east_hip_debug_set_synonyms_chunk) entries of a source row at a time: the generated shapes sit on both sides of each."""
import collections
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import synonyms_exact
from conftest import load_golden
from test_synonyms_host import case_similarities, case_triples

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("synonyms.json")["cases"]
TOL = synonyms_exact.ABS_TOL
SRC, TGT, CHUNK = 16, 256, 24
NOT_BUILT, INVALID = "(code -6)", "(code -2)"


@pytest.fixture()
def small_chunk(hip):
    lib = hip.load()
    lib.east_hip_debug_set_synonyms_chunk(CHUNK)
    yield CHUNK
    lib.east_hip_debug_set_synonyms_chunk(0)


class Built(object):
    """A HipSynonyms built from string triples, with the model of the same triples."""

    def __init__(self, hip, triples, index=None, dev=None):
        from east.synonyms import synonyms
        self.model = synonyms_exact.Model(triples)
        self.words, self.relations, w1, rel, w2, inverse = synonyms.intern_triples(triples)
        assert self.words == self.model.words and self.relations == self.model.relations
        self.id = {w: i for i, w in enumerate(self.words)}
        self.dev = dev if dev is not None else hip.HipSynonyms(index=index)
        self.dev.build(w1, rel, w2, inverse, len(self.words))
        self.n_raw = len(triples)

    def close(self):
        self.dev.close()

    def check_rows(self):
        """The CSR rows equal the model's: the same features in the same order, I to 1e-12, the row sums to 1e-12 relative
        (n terms, each partial sum rounded once: n * 2^-53 relative, n a few hundred)."""
        m = self.model
        offsets, relation, word, value, row_sum = self.dev.rows()
        info = self.dev.info()
        assert info["raw_triples"] == self.n_raw and info["distinct_triples"] == len(m.f)
        assert info["words"] == len(self.words) and info["relations"] == len(self.relations)
        assert info["features"] == sum(len(r) for r in m.rows.values()) == offsets[-1]
        assert info["longest_row"] == max(len(r) for r in m.rows.values())
        worst = 0.0
        for i, w in enumerate(self.words):
            b, e = int(offsets[i]), int(offsets[i + 1])
            assert [(self.relations[relation[p]], self.words[word[p]]) for p in range(b, e)] == [k for k, _ in m.rows[w]], w
            for p, (_, v) in zip(range(b, e), m.rows[w]):
                worst = max(worst, abs(value[p] - float(v)))
            assert abs(row_sum[i] - float(m.row_sum[w])) <= 1e-12 * max(1.0, float(m.row_sum[w])), w
        print("worst |I - model| over %d features: %.3e" % (info["features"], worst))
        assert worst <= TOL
        return worst

    def check_pairs(self, candidates, threshold):
        """The pair list at `threshold` equals the model's: the same pairs in the same order, similarities to 1e-12.  The
        model's own margin is asserted first: no similarity within 1e-9 of the threshold (a seed's business, not a
        tolerance of the comparison)."""
        want = self.model.pairs(candidates, 0.0)
        assert all(abs(s - threshold) > 1e-9 for _, _, s in want), "the generated case has a similarity at the threshold"
        want = [(a, b, s) for a, b, s in want if s > threshold]
        a, b, sim = self.dev.pairs([self.id[w] for w in candidates], threshold)
        got = [(self.words[x], self.words[y]) for x, y in zip(a.tolist(), b.tolist())]
        assert got == [(x, y) for x, y, _ in want]
        worst = max([abs(s - t[2]) for s, t in zip(sim.tolist(), want)] or [0.0])
        print("threshold %.2f: %d pairs of %d candidates, worst |similarity - model| %.3e" % (threshold, len(want), len(candidates), worst))
        assert worst <= TOL
        return a, b, sim


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_fixture_case(hip, case):
    built = Built(hip, case_triples(case))
    try:
        assert built.words == case["words"]
        built.check_rows()
        # every I > 0 of the reference
        offsets, relation, word, value, _ = built.dev.rows()
        got = sorted([built.words[i], built.relations[relation[p]], built.words[word[p]], float(value[p])]
                     for i in range(len(built.words)) for p in range(int(offsets[i]), int(offsets[i + 1])))
        assert [g[:3] for g in got] == [w[:3] for w in case["I"]]
        assert max([abs(g[3] - w[3]) for g, w in zip(got, case["I"])] or [0.0]) <= TOL
        # every candidate pair's similarity: against the reference and against the model
        cand, recorded = case["candidates"], case_similarities(case)
        pa = [built.id[a] for a, _, _ in recorded]
        pb = [built.id[b] for _, b, _ in recorded]
        sims = built.dev.similarity(pa, pb)
        worst_ref = max([abs(s - w[2]) for s, w in zip(sims.tolist(), recorded)] or [0.0])
        worst_model = max([abs(s - built.model.similarity(a, b)) for s, (a, b, _) in zip(sims.tolist(), recorded)] or [0.0])
        print("%s: worst |similarity - reference| %.3e, - model %.3e over %d pairs" % (case["name"], worst_ref, worst_model, len(pa)))
        assert worst_ref <= TOL and worst_model <= TOL
        assert (built.dev.similarity(pb, pa) == sims).all()                     # symmetric, bit for bit
        # the synonym lists at 0.3, and at 0.0 exactly the pairs that share a feature
        a, b, sim = built.check_pairs(cand, 0.3)
        lists = collections.defaultdict(list)
        for x, y in zip(a.tolist(), b.tolist()):
            lists[built.words[x]].append(built.words[y])
            lists[built.words[y]].append(built.words[x])
        assert {w: sorted(v) for w, v in lists.items()} == case["synonyms_0.3"]
        a, b, sim = built.dev.pairs([built.id[w] for w in cand], 0.0)
        got0 = [(built.words[x], built.words[y]) for x, y in zip(a.tolist(), b.tolist())]
        assert got0 == built.model.sharing_pairs(cand)
        assert sorted(got0) == sorted((x, y) for x, y, s in recorded if s > 0.0)
        assert (sim > 0.0).all()
    finally:
        built.close()


def test_extractor_against_the_fixture(hip):
    """The Python class end to end: get_synonyms (with and without the measure, kept per arguments), similarity, T, I."""
    from east import synonyms
    for case in GOLDEN:
        ex = synonyms.SynonymExtractor.from_texts([case["text"]] + [""] * (case["number_of_texts"] - 1), case_triples(case))
        got = ex.get_synonyms()
        assert isinstance(got, collections.defaultdict) and got["no such word"] == []
        assert {w: v for w, v in got.items() if v} == case["synonyms_0.3"], case["name"]      # (in code-point order: sorted)
        assert ex.get_synonyms() is got and ex.get_synonyms(0.3, False) is got
        assert {w: sorted(v) for w, v in ex.get_synonyms(0.0).items() if v} == case["synonyms_0.0"]
        measured = ex.get_synonyms(return_similarity_measure=True)
        assert {w: [x for x, _ in v] for w, v in measured.items() if v} == case["synonyms_0.3"]
        want = {(a, b): s for a, b, s in case_similarities(case)}
        for w, lst in measured.items():
            for other, s in lst:
                assert abs(s - want[tuple(sorted((w, other)))]) <= TOL and s == ex.similarity(w, other)
        w, r, w2, v = case["I"][len(case["I"]) // 2]
        assert abs(ex.I(w, r, w2) - v) <= TOL and ex.I(w, r, "no such word") == 0.0
        assert ex.T(w) == set((i[1], i[2]) for i in case["I"] if i[0] == w)
        assert ex.similarity(w, "no such word") == 0.0
        ex.close()


@pytest.mark.parametrize("C", [1, 2, SRC - 1, SRC, SRC + 1, 2 * SRC + 1, TGT - 1, TGT, TGT + 1, 2 * TGT + 1])
def test_candidate_counts_around_the_tiles(hip, C):
    """C candidates on both sides of the source tile (16) and the target tile (256): seeded Zipf triples."""
    triples = synonyms_exact.zipf_triples(seed=100 + C, n_words=C + C // 4 + 12, n_relations=5, n_triples=min(4000, 60 + 8 * C))
    built = Built(hip, triples)
    try:
        assert len(built.words) >= C
        if C <= 2 * SRC + 1:                                            # few candidates: the words with the longest rows
            by_length = sorted(range(len(built.words)), key=lambda i: (-len(built.model.rows[built.words[i]]), i))
            cand = [built.words[i] for i in sorted(by_length[:C])]
        else:
            rng = np.random.default_rng(C)
            cand = [built.words[i] for i in sorted(rng.choice(len(built.words), size=C, replace=False).tolist())]
        assert C < 2 or len(built.model.sharing_pairs(cand)) > 0
        built.check_pairs(cand, 0.12)
        a, b, _ = built.dev.pairs([built.id[w] for w in cand], 0.0)
        assert [(built.words[x], built.words[y]) for x, y in zip(a.tolist(), b.tolist())] == built.model.sharing_pairs(cand)
    finally:
        built.close()


@pytest.mark.parametrize("D", synonyms_exact.SCAN_TILE_DISTINCT)
def test_distinct_triples_around_a_tile_of_the_scan(hip, D):
    """D distinct triples out of M = 2 N sorted keys (4094, 4096, 4096, 4098), both on both sides of the 4096 elements a
    workgroup of the prefix sums takes: the numbers of the distinct triples and of their groups are prefix sums over the
    M keys' run heads, the slots of the kept features one over the D triples.  Ids against the array model: info and the
    features with ==, I and the row sums to 1e-12."""
    w1, rel, w2, inverse, W = case = synonyms_exact.distinct_count_case(D)
    model = synonyms_exact.array_model(*case)
    assert model.key.size == D and 2 * w1.size == D + D % 2 and abs(2 * w1.size - 4096) <= 2
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        assert dev.info() == model.info()
        offsets, relation, word, value, row_sum = dev.rows()
        assert np.array_equal(offsets, model.offsets())
        assert np.array_equal(relation, model.relation) and np.array_equal(word, model.word)
        want_I, want_sum = model.I.astype(np.float64), model.sums().astype(np.float64)
        assert want_I.size > 0 and np.abs(value - want_I).max() <= TOL
        assert (np.abs(row_sum - want_sum) <= 1e-12 * np.maximum(1.0, want_sum)).all()
    finally:
        dev.close()


def _row_length_case():
    """Rows of 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 3 entries, a few others, and a hub whose row is longer
    than all the others together; plus the feature words' own short rows."""
    lengths = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 5, 7, 3, 12, 30, 2, 4 * CHUNK, 9, 17, CHUNK + 2, 40, 6]
    hub = sum(lengths) + 3 * CHUNK + 5
    lengths.append(hub)
    triples = synonyms_exact.row_length_triples(lengths, seed=4)
    triples.append((synonyms_exact.word_name(0), "solo", "S00"))       # a word with q == 1 and nothing else: an empty row
    return lengths, hub, triples


def test_row_lengths_around_the_chunk(hip, small_chunk):
    lengths, hub, triples = _row_length_case()
    built = Built(hip, triples)
    try:
        got_lengths = [len(built.model.rows[synonyms_exact.word_name(i)]) for i in range(len(lengths))]
        assert got_lengths == lengths                                   # what the case is for
        built.check_rows()
        cand = [synonyms_exact.word_name(i) for i in range(len(lengths))]
        cand = cand[::-1] + [w for w in built.words if w.startswith("P")]        # (not in id order: the hub first)
        assert len(built.model.rows[cand[0]]) == hub > sum(len(built.model.rows[w]) for w in cand[1:])
        assert any(built.model.shared(cand[0], w) for w in cand[1:]), "the hub shares nothing"
        results = {}
        for chunk in (small_chunk, 7, 0):                               # 0: the default chunk, every row in one piece but the hub's
            hip.load().east_hip_debug_set_synonyms_chunk(chunk)
            results[chunk] = built.check_pairs(cand, 0.05)
            a, b, _ = built.dev.pairs([built.id[w] for w in cand], 0.0)
            assert [(built.words[x], built.words[y]) for x, y in zip(a.tolist(), b.tolist())] == built.model.sharing_pairs(cand)
        for chunk in (7, 0):                                            # the pairs do not depend on the chunk: the same bytes
            for x, y in zip(results[small_chunk], results[chunk]):
                assert x.tobytes() == y.tobytes()
        # every pair of these words through the look-up, too
        pa = [built.id[a] for i, a in enumerate(cand) for _ in cand[i + 1:]]
        pb = [built.id[b] for i, _ in enumerate(cand) for b in cand[i + 1:]]
        sims = built.dev.similarity(pa, pb)
        worst = max(abs(s - built.model.similarity(built.words[x], built.words[y])) for s, x, y in zip(sims.tolist(), pa, pb))
        print("look-ups: worst |similarity - model| %.3e over %d pairs" % (worst, len(pa)))
        assert worst <= TOL
    finally:
        built.close()


def test_subset_of_the_words_three_thresholds_and_a_smaller_second_build(hip, small_chunk):
    triples = synonyms_exact.zipf_triples(seed=77, n_words=300, n_relations=6, n_triples=3000)
    built = Built(hip, triples)
    try:
        built.check_rows()
        cand = built.words[3::7] + built.words[2:40:7]                  # a strict subset, ids neither contiguous nor ascending
        assert len(set(cand)) == len(cand) < len(built.words)
        counts = []
        for threshold in (0.25, 0.08, 0.5):                             # the same build, three thresholds in a row
            a, _, _ = built.check_pairs(cand, threshold)
            counts.append(a.size)
        assert counts[1] > counts[0] > counts[2]
        # a second, smaller build on the same handle
        second = Built(hip, synonyms_exact.zipf_triples(seed=78, n_words=40, n_relations=3, n_triples=200), dev=built.dev)
        second.check_rows()
        second.check_pairs(second.words, 0.1)
        with pytest.raises(hip.exceptions.HipBackendError) as e:           # ids of the first build are out of range now
            second.dev.pairs([len(second.words)], 0.1)
        assert INVALID in str(e.value)
    finally:
        built.close()


def test_two_runs_give_the_same_bytes(hip):
    triples = synonyms_exact.zipf_triples(seed=5, n_words=600, n_relations=8, n_triples=4000)
    runs = []
    for _ in range(2):
        built = Built(hip, triples)
        try:
            ids = np.arange(len(built.words), dtype=np.int32)
            runs.append([x.tobytes() for x in built.dev.rows()] + [x.tobytes() for x in built.dev.pairs(ids, 0.1)])
            again = [x.tobytes() for x in built.dev.pairs(ids, 0.1)]
            assert again == runs[-1][5:]
        finally:
            built.close()
    assert len(runs[0][5]) > 0
    assert runs[0] == runs[1]


def test_arguments_and_states(hip):
    idx = hip.HipIndex()
    dev = hip.HipSynonyms(index=idx)
    E = hip.exceptions.HipBackendError
    try:
        for call in (dev.info, dev.rows, lambda: dev.similarity([0], [0]), lambda: dev.pairs([0, 1], 0.3)):
            with pytest.raises(E) as e:
                call()
            assert NOT_BUILT in str(e.value)
        one = np.zeros(1, dtype=np.int32)
        for w1, rel, w2, inverse, n_words in ((one, one, one + 1, one, 1), (one, one + 1, one, one, 1), (one - 1, one, one, one, 1),
                                              (one, one, one, np.array([1, 1], np.int32), 1), (one, one, one, one, (1 << 26) + 1),
                                              (one[:0], one[:0], one[:0], one, 1)):
            with pytest.raises(E) as e:
                dev.build(w1, rel, w2, inverse, n_words)
            assert INVALID in str(e.value)
        with pytest.raises(E) as e:
            dev.build(one, one, one, np.zeros((1 << 12) + 1, np.int32), 1)
        assert INVALID in str(e.value)
        built = Built(hip, synonyms_exact.zipf_triples(seed=9, n_words=30, n_relations=3, n_triples=150), dev=dev)
        W = len(built.words)
        with pytest.raises(E) as e:                                     # fetch before any pairs call
            hip._check(hip.load().east_hip_synonyms_fetch(idx._h, None, None, None))
        assert NOT_BUILT in str(e.value)
        for cand, threshold in (([0, W], 0.3), ([-1, 0], 0.3), ([1, 2, 1], 0.3), ([0, 1], -0.1), ([0, 1], float("nan"))):
            with pytest.raises(E) as e:
                dev.pairs(cand, threshold)
            assert INVALID in str(e.value)
        for a, b in (([0], [W]), ([-1], [0])):
            with pytest.raises(E) as e:
                dev.similarity(a, b)
            assert INVALID in str(e.value)
        assert dev.pairs([], 0.3, fetch=False) == 0 and dev.pairs([3], 0.3, fetch=False) == 0
        assert dev.similarity([], []).size == 0
        assert [x.size for x in dev.pairs([3], 0.0)] == [0, 0, 0]
        assert dev.pairs(list(range(W)), float("inf"), fetch=False) == 0
        assert dev.last_ms >= 0.0
    finally:
        dev.close()
        idx.close()


def test_the_handle_keeps_its_other_indexes(hip):
    """A synonyms build between an EASA build and its score call changes no score; the reset call withdraws the synonyms."""
    texts = [b"the quick brown fox jumps over the lazy dog", b"suffix trees and suffix arrays index every substring", b"xabxac"]
    q_symbols, q_offsets = hip.pack_queries(["QUICK FOX", "SUFFIX ARRAY", "ABC"])
    idx = hip.HipIndex()
    try:
        idx.build_texts(texts)
        want = idx.score_table(q_symbols, q_offsets)
        idx.build_texts(texts)
        built = Built(hip, synonyms_exact.zipf_triples(seed=3, n_words=80, n_relations=4, n_triples=600), index=idx)
        pairs = built.dev.pairs(np.arange(len(built.words), dtype=np.int32), 0.1)
        assert (idx.score_table(q_symbols, q_offsets) == want).all()
        idx.build_texts(texts)                                          # ... and an EASA build leaves the synonyms alone
        again = built.dev.pairs(np.arange(len(built.words), dtype=np.int32), 0.1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(pairs, again)) and pairs[0].size > 0
        built.check_rows()
        assert hip.load().east_hip_reset(idx._h) == 0
        for call in (built.dev.info, built.dev.rows, lambda: built.dev.pairs([0, 1], 0.3), lambda: built.dev.similarity([0], [1])):
            with pytest.raises(hip.exceptions.HipBackendError) as e:
                call()
            assert NOT_BUILT in str(e.value)
    finally:
        idx.close()


class _Recorded(object):
    """A plain synonimizer that returns a recorded mapping (tests/test_gpu_parity.py pins this path)."""

    def __init__(self, mapping):
        self.mapping = collections.defaultdict(list, {w: list(v) for w, v in mapping.items()})

    def get_synonyms(self):
        return self.mapping


@pytest.mark.parametrize("name", ["length_filter", "non_ascii", "tomita_xml"])
def test_keyphrases_table_with_an_extractor(hip, name):
    from east import applications, relevance, synonyms
    case = next(c for c in GOLDEN if c["name"] == name)
    words = case["candidates"]
    texts = {"t%d" % i: " ".join(words[i::3] + words[:2]).lower().encode("utf-8") for i in range(3)}
    texts["all"] = case["text"].encode("utf-8")
    with_synonyms = [w for w in words if w in case["synonyms_0.3"]]
    assert with_synonyms
    keyphrases = [with_synonyms[0].lower(), " ".join(with_synonyms[:2]).lower(), words[-1].lower() + " " + with_synonyms[-1].lower()]
    ex = synonyms.SynonymExtractor.from_texts([case["text"]], case_triples(case))
    try:
        got = applications.keyphrases_table(keyphrases, texts, relevance.ASTRelevanceMeasure(), ex)
        want = applications.keyphrases_table(keyphrases, texts, relevance.ASTRelevanceMeasure(), _Recorded(case["synonyms_0.3"]))
        plain = applications.keyphrases_table(keyphrases, texts, relevance.ASTRelevanceMeasure())
        assert got == want
        assert got != plain                                             # the synonyms do change a score
    finally:
        ex.close()


def test_cli_with_triples(hip, tmp_path):
    """`east -y -t <triples>` end to end: the table equals the one the library call gives."""
    from east import applications, formatting, main, relevance, synonyms
    case = next(c for c in GOLDEN if c["name"] == "length_filter")
    d = tmp_path / "texts"
    d.mkdir()
    words = case["candidates"]
    (d / "a.txt").write_text(case["text"], encoding="utf-8")
    (d / "b.txt").write_text(" ".join(words[::2]).lower(), encoding="utf-8")
    (tmp_path / "kp.txt").write_text("cow pull\nhorse\n", encoding="utf-8")
    (tmp_path / "triples.tsv").write_text("".join("%s\t%s\t%s\n" % tuple(t) for t in case["triples"]), encoding="utf-8")
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main.main(["-y", "-t", str(tmp_path / "triples.tsv"), "-f", "csv", "keyphrases", "table", str(tmp_path / "kp.txt"), str(d)])
    assert rc == 0
    ex = synonyms.SynonymExtractor(str(d), triples=str(tmp_path / "triples.tsv"))
    assert ex.number_of_texts == 2
    texts = {"a": (d / "a.txt").read_bytes(), "b": (d / "b.txt").read_bytes()}
    table = applications.keyphrases_table(["cow pull", "horse"], texts, relevance.ASTRelevanceMeasure(), ex)
    assert out.getvalue() == formatting.format_table(table, "csv") + "\n"
    plain = applications.keyphrases_table(["cow pull", "horse"], texts, relevance.ASTRelevanceMeasure())
    assert table != plain
    ex.close()
