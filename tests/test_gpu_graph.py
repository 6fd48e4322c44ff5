"""gpu tier: the keyphrase graph built on the device (csrc/graph.h through include/east_hip.h) against the host code of
east/applications.py fed with the same table -- the reference-shaped loops of keyphrases_graph on a plain dict table for
small K, _graph_from_array (which tests/test_host_logic.py pins to those loops) above that.  Nodes, supports and every
edge's source, target and confidence are compared with ==; nothing is sampled."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

LOOPS_MAX_K = 65                    # up to here the yardstick is the loops, above it _graph_from_array


class _ArrayMeasure(object):
    """A batched measure without `relevance_graph` that returns a given K x D array: keyphrases_graph stays on the host."""

    def __init__(self, scores):
        self.scores = scores

    def set_text_collection(self, texts, language=None):
        pass

    def relevance_table(self, prepared):
        return self.scores


def _listed(K):
    """K keyphrases in list order, one of them listed twice when there is room; -> (list, unique, rows)."""
    kps = ["kp%d" % i for i in range(K)]
    if K >= 4:
        kps[3] = kps[1]
    uniq = list(dict.fromkeys(kps))
    row_of = {kp: i for i, kp in enumerate(uniq)}
    return kps, uniq, np.array([row_of[kp] for kp in kps], dtype=np.int32)


def _host_graph(monkeypatch, kps, uniq, scores, rc, rt, st):
    """The yardstick: the host path of keyphrases_graph on this table."""
    from east import applications
    D = scores.shape[1]
    texts = {"t%d" % i: b"x" for i in range(D)}
    if len(kps) <= LOOPS_MAX_K:
        monkeypatch.setattr(applications, "ARRAY_TABLE_MIN_SCORES", 1 << 62)        # a plain dict table: the loops
        graph = applications.keyphrases_graph(kps, texts, rc, rt, st, _ArrayMeasure(scores))
        monkeypatch.undo()
        return graph
    table = applications.ScoreTable(uniq, list(texts), scores)
    return applications._graph_from_array(kps, table, rc, rt, st)


def _device_graph(index, kps, rows, scores, rc, rt, st):
    from east import applications
    found = index.graph_from_table(scores, rows, rt, st, rc)
    return found, applications.KeyphraseGraph.from_device(kps, found, rc, rt, st)


def _check(monkeypatch, index, kps, uniq, rows, scores, rc, rt, st):
    want = _host_graph(monkeypatch, kps, uniq, scores, rc, rt, st)
    found, graph = _device_graph(index, kps, rows, scores, rc, rt, st)
    with np.errstate(invalid="ignore"):
        support = (scores[rows] >= rt).sum(axis=1)
    assert found.support.tolist() == support.tolist()
    got = graph.to_dict()
    assert got["nodes"] == want["nodes"]
    assert len(got["edges"]) == len(want["edges"])
    assert got["edges"] == want["edges"]
    assert got == want and graph == want
    return want


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1000])
def test_host_table_entry_point_on_random_tables(hip, monkeypatch, K):
    """K x D random tables of several densities through east_hip_graph_build_host: every word count around the 64-column
    words and the 64-row tiles, support thresholds 0, 1, 3 and D + 1 (no nodes), a keyphrase that occurs nowhere, one
    listed twice, a row that is a subset of another (confidence 1.0 one way)."""
    index = hip.HipIndex()
    rng = np.random.default_rng(1000 + K)
    kps, uniq, rows = _listed(K)
    edges_seen = 0
    for D in (1, 63, 64, 65, 256, 1000, 4097):
        for density, rc in ((0.05, 0.2), (0.4, 0.6), (0.9, 0.95)):
            scores = np.where(rng.random((len(uniq), D)) < density, 0.3 + 0.7 * rng.random((len(uniq), D)),
                              0.2 * rng.random((len(uniq), D)))
            scores[0] = 0.1                                    # a keyphrase that occurs nowhere
            if len(uniq) >= 8:
                scores[6] = np.where(rng.random(D) < 0.5, scores[5], 0.0)      # 6's texts are a subset of 5's
            for st in (0, 1, 3, D + 1):
                want = _check(monkeypatch, index, kps, uniq, rows, scores, rc, 0.25, st)
                edges_seen += len(want["edges"])
                if st == D + 1:
                    assert want["nodes"] == [] and want["edges"] == []
    assert K < 63 or edges_seen > 0
    index.close()


def _rows_with(D, occurrences):
    """A table whose row i occurs (score 0.5) exactly in the given columns, 0.0 elsewhere."""
    scores = np.zeros((len(occurrences), D))
    for i, cols in enumerate(occurrences):
        scores[i, list(cols)] = 0.5
    return scores


def test_equality_at_the_thresholds(hip, monkeypatch):
    index = hip.HipIndex()
    # scores exactly at the relevance threshold occur; NaN never does; -0.0 >= 0.0 does
    rt = 0.1 + 0.2
    scores = np.array([[rt, np.nextafter(rt, 0.0), np.nan, rt], [rt, rt, np.nan, np.nextafter(rt, 1.0)],
                       [np.nan, np.nan, np.nan, np.nan]])
    kps, uniq, rows = ["a", "b", "c"], ["a", "b", "c"], np.arange(3, dtype=np.int32)
    want = _check(monkeypatch, index, kps, uniq, rows, scores, 0.6, rt, 0)
    assert [n["support"] for n in want["nodes"]] == [2, 3, 0]
    scores = np.array([[-0.0, 0.0, np.nan, -1e-300], [0.0, -0.0, -0.0, np.nan]])
    want = _check(monkeypatch, index, ["a", "b"], ["a", "b"], np.arange(2, dtype=np.int32), scores, 0.6, 0.0, 1)
    assert [n["support"] for n in want["nodes"]] == [2, 3] and [(e["source"], e["target"]) for e in want["edges"]] == [(0, 1), (1, 0)]

    # the decision is the division Python makes
    D = 256
    for sup, shared, rc, edge in ((5, 3, 0.6, True), (10, 3, 0.1 + 0.2, False), (100, 55, 0.55, True), (180, 99, 0.55, True),
                                  (200, 110, 0.55, True), (220, 121, 0.55, True)):
        assert (shared / sup >= rc) is edge
        if sup >= 100:
            assert not shared >= rc * sup                   # a cross-multiplied test says no edge here
        # source: the first `sup` texts; target: `shared` of them and every text behind them
        scores = _rows_with(D, [range(sup), list(range(shared)) + list(range(sup, D))])
        want = _check(monkeypatch, index, ["a", "b"], ["a", "b"], np.arange(2, dtype=np.int32), scores, rc, 0.25, 1)
        assert [n["support"] for n in want["nodes"]] == [sup, shared + D - sup]
        forward = [e for e in want["edges"] if (e["source"], e["target"]) == (0, 1)]
        assert len(forward) == (1 if edge else 0)
        if edge:
            assert forward[0]["confidence"] == shared / sup

    # referral_confidence 0.0: every ordered pair of distinct nodes, sources without support included (support threshold 0)
    kps, uniq, rows = _listed(70)
    rng = np.random.default_rng(3)
    scores = np.where(rng.random((len(uniq), 130)) < 0.2, 0.5, 0.0)
    scores[0] = 0.0
    scores[10] = 0.0
    want = _check(monkeypatch, index, kps, uniq, rows, scores, 0.0, 0.25, 0)
    assert [(e["source"], e["target"]) for e in want["edges"]] == [(a, b) for a in range(70) for b in range(70) if a != b]
    want = _check(monkeypatch, index, kps, uniq, rows, scores, 0.0, 0.25, 1)
    assert len(want["nodes"]) == 68 and len(want["edges"]) == 68 * 67
    want = _check(monkeypatch, index, kps, uniq, rows, scores, -0.0, 0.25, 0)
    assert len(want["edges"]) == 70 * 69
    # referral_confidence 1.0: subset relations only
    scores[20] = np.where(rng.random(130) < 0.5, scores[21], 0.0)
    scores[22] = scores[23]
    want = _check(monkeypatch, index, kps, uniq, rows, scores, 1.0, 0.25, 1)
    hits = scores[rows] >= 0.25
    subset = [(a, b) for a in range(70) for b in range(70)
              if a != b and hits[a].sum() >= 1 and hits[b].sum() >= 1 and not (hits[a] & ~hits[b]).any()]
    assert [(e["source"], e["target"]) for e in want["edges"]] == subset and len(subset) >= 4
    assert all(e["confidence"] == 1.0 for e in want["edges"])
    # a NaN confidence threshold gives no edge, as `confidence >= nan` in Python
    want = _check(monkeypatch, index, kps, uniq, rows, scores, float("nan"), 0.25, 1)
    assert want["edges"] == [] and len(want["nodes"]) > 0
    index.close()


def test_large_output_in_order(hip):
    """3 000 nodes at referral_confidence 0.0: 8 997 000 edges, compared as arrays with np.nonzero of the expected matrix
    in row-major order (the reference's order), the shared counts with the integer products."""
    K, D = 3000, 96
    rng = np.random.default_rng(8)
    scores = np.where(rng.random((K, D)) < 0.3, 0.5, 0.0)
    index = hip.HipIndex()
    found = index.graph_from_table(scores, np.arange(K, dtype=np.int32), 0.25, 0, 0.0)
    hits = (scores >= 0.25)
    support = hits.sum(axis=1)
    assert found.support.tolist() == support.tolist() and found.kept.tolist() == list(range(K))
    src, dst = np.nonzero(~np.eye(K, dtype=bool))
    assert src.size == 8997000 == found.edge_source.size == found.edge_target.size == found.edge_shared.size
    assert np.array_equal(found.edge_source, src) and np.array_equal(found.edge_target, dst)
    shared = (hits.astype(np.float32) @ hits.astype(np.float32).T).astype(np.int32)        # (counts up to D: exact in float32)
    assert np.array_equal(found.edge_shared, shared[src, dst])
    # ... and a threshold in between: the same against the expected matrix of that threshold
    found = index.graph_from_table(scores, np.arange(K, dtype=np.int32), 0.25, 1, 0.4)
    kept = np.flatnonzero(support >= 1)
    conf = shared[np.ix_(kept, kept)].astype(np.float64) / np.maximum(support[kept], 1).astype(np.float64)[:, None]
    want = conf >= 0.4
    np.fill_diagonal(want, False)
    src, dst = np.nonzero(want)
    assert 10 ** 4 < src.size < 8 * 10 ** 6
    assert np.array_equal(found.kept, kept)
    assert np.array_equal(found.edge_source, kept[src]) and np.array_equal(found.edge_target, kept[dst])
    assert np.array_equal(found.edge_shared, shared[kept[src], kept[dst]])
    index.close()


def test_configs2_shape_against_the_array_code(hip):
    """BASELINE configs[2]'s shape, 10 000 x 256, a table with topic structure: the whole graph against _graph_from_array."""
    from east import applications, synthetic
    K, D = 10000, 256
    scores = synthetic.topic_score_table(np.random.default_rng(7), K, D)
    kps = ["kp%d" % i for i in range(K)]
    kps[77] = kps[5]
    uniq = list(dict.fromkeys(kps))
    row_of = {kp: i for i, kp in enumerate(uniq)}
    rows = np.array([row_of[kp] for kp in kps], dtype=np.int32)
    table = applications.ScoreTable(uniq, ["t%d" % i for i in range(D)], scores[:len(uniq)])
    want = applications._graph_from_array(kps, table, 0.6, 0.25, 1)
    assert 10 ** 5 < len(want["edges"]) < 10 ** 7
    index = hip.HipIndex()
    found, graph = _device_graph(index, kps, rows, scores[:len(uniq)], 0.6, 0.25, 1)
    assert graph.node_ids.tolist() == [n["id"] for n in want["nodes"]]
    assert graph.support[graph.node_ids].tolist() == [n["support"] for n in want["nodes"]]
    assert graph.edge_source.tolist() == [e["source"] for e in want["edges"]]
    assert graph.edge_target.tolist() == [e["target"] for e in want["edges"]]
    assert graph.edge_confidence.tolist() == [e["confidence"] for e in want["edges"]]
    assert graph == want
    # two runs of the same build give the same arrays
    again = index.graph_from_table(scores[:len(uniq)], rows, 0.25, 1, 0.6)
    for name in hip.GraphArrays.__slots__:
        assert np.array_equal(getattr(found, name), getattr(again, name)), name
    assert 0.0 < index.last_graph_ms < 1000.0
    index.close()


def _both_paths(monkeypatch, kps, texts, rc, rt, st, make_measure):
    from east import applications
    monkeypatch.delenv("EAST_HIP_GRAPH", raising=False)
    device = applications.keyphrases_graph(kps, texts, rc, rt, st, make_measure())
    arrays = applications.keyphrases_graph_arrays(kps, texts, rc, rt, st, make_measure())
    monkeypatch.setenv("EAST_HIP_GRAPH", "host")
    host = applications.keyphrases_graph(kps, texts, rc, rt, st, make_measure())
    monkeypatch.delenv("EAST_HIP_GRAPH")
    assert type(device) is dict and type(host) is dict
    assert isinstance(arrays, applications.KeyphraseGraph) and arrays == device
    return device, host, arrays


def test_resident_ast_table_on_the_hse_fixture(hip, monkeypatch):
    from east import formatting, relevance
    g = load_golden("hse_graph.json")
    texts = {k: v.encode("utf-8") for k, v in load_golden(g["texts_from"])["texts"].items()}
    calls = []
    real = relevance.ASTRelevanceMeasure.relevance_graph

    def counting(self, *a):
        calls.append(1)
        return real(self, *a)

    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "relevance_graph", counting)
    for case in g["cases"]:
        device, host, arrays = _both_paths(monkeypatch, g["keyphrases"], texts, case["referral_confidence"],
                                           case["relevance_threshold"], case["support_threshold"],
                                           lambda: relevance.ASTRelevanceMeasure("easa", True))
        assert device == case["graph"] and host == case["graph"]
        assert formatting.graph2gml(arrays) == case["gml"] and formatting.graph2gml(device) == case["gml"]
        if case["edges"] is not None:
            assert formatting.graph2edges(arrays) == case["edges"]
    assert len(calls) == 2 * len(g["cases"])                 # the default path went through the device, the host path did not


def _cosine_measure(space, weighting):
    from east import relevance
    return relevance.CosineRelevanceMeasure(space, weighting, stopwords=[])


def test_resident_cosine_table_on_the_cosine_fixture(hip, monkeypatch):
    g = load_golden("cosine.json")["cli"]
    hse = load_golden("hse_config1.json")["texts"]
    texts = {name: hse[name].encode("utf-8") for name in sorted(hse)}
    device, host, _ = _both_paths(monkeypatch, g["keyphrases"], texts, 0.6, 0.25, 1, lambda: _cosine_measure("words", "tf-idf"))
    assert device == host
    for graph in (device, host):
        assert graph["nodes"] == g["graph"]["nodes"]
        assert [(e["source"], e["target"]) for e in graph["edges"]] == [(e["source"], e["target"]) for e in g["graph"]["edges"]]
        assert [e["confidence"] for e in graph["edges"]] == [e["confidence"] for e in g["graph"]["edges"]]


def _synthetic_collection():
    """A few dozen prose-like documents and a few hundred keyphrases: one or two consecutive words of a document each,
    some listed twice."""
    from east import synthetic
    rng = np.random.default_rng(77)
    docs = synthetic.prose_like_texts(rng, 36, 2500)
    texts = {"doc%02d" % i: d for i, d in enumerate(docs)}
    kps = []
    for i in range(300):
        words = [w for w in docs[int(rng.integers(0, len(docs)))].decode("ascii").split() if w.isalpha() and len(w) >= 4]
        a = int(rng.integers(0, len(words) - 1))
        kps.append(" ".join(words[a:a + 1 + int(rng.integers(0, 2))]))
    kps[50] = kps[7]
    kps[51] = kps[7]
    return kps, texts


def test_resident_tables_on_a_synthetic_collection(hip, monkeypatch):
    from east import relevance
    kps, texts = _synthetic_collection()
    seen = 0
    for normalized, rt in ((True, 0.2), (False, 0.2)):
        device, host, _ = _both_paths(monkeypatch, kps, texts, 0.5, rt, 2, lambda: relevance.ASTRelevanceMeasure("easa", normalized))
        assert device == host and len(device["nodes"]) > 0
        seen += len(device["edges"])
    for weighting in ("tf", "tf-idf"):
        device, host, _ = _both_paths(monkeypatch, kps, texts, 0.5, 0.05, 1, lambda: _cosine_measure("words", weighting))
        assert device == host and len(device["nodes"]) > 10
        seen += len(device["edges"])
    assert seen > 100


def test_cli_graph_in_both_formats(hip, tmp_path, monkeypatch):
    from east import main
    monkeypatch.delenv("EAST_HIP_GRAPH", raising=False)
    g = load_golden("hse_graph.json")
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, text in load_golden(g["texts_from"])["texts"].items():
        (tdir / (name + ".txt")).write_bytes(text.encode("utf-8"))
    kp = tmp_path / "kp.txt"
    kp.write_bytes("\n".join(g["keyphrases"]).encode("utf-8"))
    for case in g["cases"]:
        for fmt in ("gml", "edges"):
            if case[fmt] is None:
                continue
            for mode in ("device", "host"):
                monkeypatch.setenv("EAST_HIP_GRAPH", mode)
                buf = io.StringIO()
                with redirect_stdout(buf):
                    assert main.main(["-f", fmt, "-c", str(case["referral_confidence"]), "-r", str(case["relevance_threshold"]),
                                      "-p", str(case["support_threshold"]), "keyphrases", "graph", str(kp), str(tdir)]) == 0
                assert buf.getvalue() == case[fmt] + "\n", (fmt, mode)


def test_lifetime_of_the_graph_buffers(hip, monkeypatch):
    import ctypes
    from east import applications, exceptions, relevance
    lib = hip.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    monkeypatch.delenv("EAST_HIP_GRAPH", raising=False)

    # a graph call before any score call is an error, not a crash -- on a new handle, after a build, after new keyphrases
    index = hip.HipIndex()
    rows = np.zeros(1, dtype=np.int32)
    with pytest.raises(exceptions.HipBackendError):
        index.graph(rows, 0.25, 1, 0.6)
    support = np.zeros(1, dtype=np.int32)
    assert lib.east_hip_graph_fetch(index._h, support.ctypes.data_as(i32p), None, None, None, None) != 0
    assert index.last_graph_ms == -1.0
    index.build_texts([b"alpha beta gamma delta", b"beta gamma epsilon"])
    with pytest.raises(exceptions.HipBackendError):
        index.graph(rows, 0.25, 1, 0.6)
    cosine = hip.HipCosineIndex(index=index)
    with pytest.raises(exceptions.HipBackendError):
        cosine.graph(rows, 0.25, 1, 0.6)
    cosine.build_texts([b"alpha beta gamma delta", b"beta gamma epsilon"])
    with pytest.raises(exceptions.HipBackendError):
        cosine.graph(rows, 0.25, 1, 0.6)
    qs, qo = hip.pack_queries(["BETA", "GAMMA", "ALPHA"])
    table = index.score_table(qs, qo, True)
    with pytest.raises(exceptions.HipBackendError):           # a row outside the table
        index.graph(np.array([0, 3], dtype=np.int32), 0.25, 1, 0.6)
    with pytest.raises(exceptions.HipBackendError):           # an unknown source
        hip._graph_build(lib, index._h, 7, None, rows, 0.25, 1, 0.6)

    # an AST graph and a cosine graph on a shared handle do not disturb each other
    all_rows = np.arange(3, dtype=np.int32)
    cos_table = cosine.score_table(cosine.lookup(["BETA", "GAMMA", "ALPHA"]), np.arange(4, dtype=np.int64), True)
    ast_1 = index.graph(all_rows, 0.2, 1, 0.5)
    cos_1 = cosine.graph(all_rows, 0.2, 1, 0.5)
    ast_2 = index.graph(all_rows, 0.2, 1, 0.5)
    cos_2 = cosine.graph(all_rows, 0.2, 1, 0.5)
    kps = ["beta", "gamma", "alpha"]
    for one, two, scores in ((ast_1, ast_2, table), (cos_1, cos_2, cos_table)):
        for name in hip.GraphArrays.__slots__:
            assert np.array_equal(getattr(one, name), getattr(two, name)), name
        want = applications._graph_from_array(kps, applications.ScoreTable(kps, ["a", "b"], scores), 0.5, 0.2, 1)
        assert applications.KeyphraseGraph.from_device(kps, one, 0.5, 0.2, 1) == want
    assert ast_1.support.tolist() == (table >= 0.2).sum(axis=1).tolist() and ast_1.support[:2].tolist() == [2, 2]
    assert (0, 1) in zip(ast_1.edge_source.tolist(), ast_1.edge_target.tolist())
    index.set_keyphrases(qs, qo)                               # new keyphrases: the table of the old ones is withdrawn
    with pytest.raises(exceptions.HipBackendError):
        index.graph(all_rows, 0.2, 1, 0.5)
    index.score_resident(True)
    ast_3 = index.graph(all_rows, 0.2, 1, 0.5)
    assert all(np.array_equal(getattr(ast_1, name), getattr(ast_3, name)) for name in hip.GraphArrays.__slots__)

    # after east_hip_reset the graph is gone
    assert lib.east_hip_graph_fetch(index._h, None, None, None, None, None) == 0
    assert lib.east_hip_reset(index._h) == 0
    assert lib.east_hip_graph_fetch(index._h, None, None, None, None, None) != 0
    assert index.last_graph_ms == -1.0
    with pytest.raises(exceptions.HipBackendError):
        index.graph(all_rows, 0.2, 1, 0.5)
    found = index.graph_from_table(table, all_rows, 0.2, 1, 0.5)      # ... and the handle builds the next one
    assert all(np.array_equal(getattr(ast_1, name), getattr(found, name)) for name in hip.GraphArrays.__slots__)
    cosine.close()
    index.close()

    # build the graph, rebuild the index with another collection, build the graph again: one measure, two collections
    g = load_golden("hse_graph.json")
    hse = {k: v.encode("utf-8") for k, v in load_golden(g["texts_from"])["texts"].items()}
    kps2, synthetic_texts = _synthetic_collection()
    case = g["cases"][1]
    measure = relevance.ASTRelevanceMeasure("easa", True)
    args = (case["referral_confidence"], case["relevance_threshold"], case["support_threshold"])
    assert applications.keyphrases_graph(g["keyphrases"], hse, *args, similarity_measure=measure) == case["graph"]
    second = applications.keyphrases_graph(kps2[:80], synthetic_texts, 0.5, 0.2, 2, measure)
    assert applications.keyphrases_graph(g["keyphrases"], hse, *args, similarity_measure=measure) == case["graph"]
    monkeypatch.setenv("EAST_HIP_GRAPH", "host")
    assert applications.keyphrases_graph(kps2[:80], synthetic_texts, 0.5, 0.2, 2, measure) == second
    assert len(second["nodes"]) > 0
