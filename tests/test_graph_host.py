"""CPU tier: the keyphrase graph as arrays (applications.KeyphraseGraph), the formatters' array path and the choice between
the device path and the host path of keyphrases_graph -- no device."""
import numpy as np
import pytest

from conftest import load_golden


def _graph(keyphrases, support, node_ids, edges, thresholds=(0.6, 0.25, 1)):
    from east import applications
    src = np.array([e[0] for e in edges], dtype=np.int32)
    dst = np.array([e[1] for e in edges], dtype=np.int32)
    conf = np.array([e[2] for e in edges], dtype=np.float64)
    return applications.KeyphraseGraph(keyphrases, np.array(support, dtype=np.int32), np.array(node_ids, dtype=np.int32),
                                       src, dst, conf, *thresholds)


# (keyphrases, support per position, node positions, edges): filtered nodes, sources without edges, a label listed twice
# whose two positions are sources, and no edges at all
HAND_MADE = [
    (["a", "b", "c", "d"], [2, 0, 3, 1], [0, 2, 3], [(0, 2, 1.0), (0, 3, 0.5), (3, 0, 1.0), (3, 2, 1.0)]),
    (["x", "y", "x", "z"], [4, 4, 4, 2], [0, 1, 2, 3], [(0, 2, 1.0), (1, 3, 0.75), (2, 0, 1.0), (2, 1, 0.6)]),
    (["only"], [1], [0], []),
    (["p", "q"], [0, 0], [], []),
]


def test_keyphrase_graph_is_the_dict_of_the_reference():
    from east import applications
    for kps, support, nodes, edges in HAND_MADE:
        g = _graph(kps, support, nodes, edges)
        want = {"nodes": [{"id": p, "label": kps[p], "support": support[p]} for p in nodes],
                "edges": [{"source": s, "target": t, "confidence": c} for s, t, c in edges],
                "referral_confidence": 0.6, "relevance_threshold": 0.25, "support_threshold": 1}
        d = g.to_dict()
        assert type(d) is dict and d == want
        assert all(type(n["id"]) is int and type(n["support"]) is int for n in d["nodes"])
        assert all(type(e["source"]) is int and type(e["target"]) is int and type(e["confidence"]) is float for e in d["edges"])
        assert g == want and want == g and not (g != want)
        assert g == _graph(kps, support, nodes, edges)
        other = dict(want, support_threshold=2)
        assert g != other and not (g == other)
        assert (g == 3) is False
        back = applications.KeyphraseGraph.from_dict(kps, want)
        assert back == want and back.to_dict() == want
        assert back.support[nodes].tolist() == [support[p] for p in nodes]


def test_formatters_give_the_bytes_of_the_dict_form():
    from east import formatting
    for kps, support, nodes, edges in HAND_MADE:
        for thresholds in ((0.6, 0.25, 1), (0.3, 0.1, 2.0)):
            g = _graph(kps, support, nodes, edges, thresholds)
            assert formatting.graph2gml(g) == formatting.graph2gml(g.to_dict())
            assert formatting.graph2edges(g) == formatting.graph2edges(g.to_dict())
            assert formatting.format_graph(g, "gml") == formatting.format_graph(g.to_dict(), "gml")
            assert formatting.format_graph(g, "edges") == formatting.format_graph(g.to_dict(), "edges")
    assert formatting.graph2edges(_graph(*HAND_MADE[1])) == "x -> x, x, y\ny -> z\n"
    with pytest.raises(Exception):
        formatting.format_graph(_graph(*HAND_MADE[0]), "dot")


def test_formatters_against_the_recorded_strings():
    from east import applications, formatting
    g = load_golden("hse_graph.json")
    for case in g["cases"]:
        graph = applications.KeyphraseGraph.from_dict(g["keyphrases"], case["graph"])
        assert graph == case["graph"]
        assert formatting.graph2gml(graph) == case["gml"]
        if case["edges"] is not None:
            assert formatting.graph2edges(graph) == case["edges"]


class _ArrayMeasure(object):
    def __init__(self, scores):
        self.scores = scores

    def set_text_collection(self, texts, language=None):
        pass

    def relevance_table(self, prepared):
        return self.scores


class _RefusingGraphMeasure(_ArrayMeasure):
    def relevance_graph(self, *args):
        raise AssertionError("the device path must not be taken")


class _NoneGraphMeasure(_ArrayMeasure):
    relevance_graph = None


def test_host_path_is_kept_where_the_device_path_does_not_apply(monkeypatch):
    """Without `relevance_graph` (or with None for it), with EAST_HIP_GRAPH=host, with a synonimizer: keyphrases_table is
    called as before and the result is the plain dict; keyphrases_graph_arrays wraps that dict."""
    from east import applications, parallel, relevance
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_graph is None
    assert parallel.DistributedASTRelevanceMeasure.relevance_graph is None
    assert callable(relevance.ASTRelevanceMeasure.relevance_graph) and callable(relevance.CosineRelevanceMeasure.relevance_graph)
    rng = np.random.default_rng(11)
    kps = ["kp%d" % i for i in range(9)]
    scores = rng.random((9, 6)) * 0.5
    texts = {"t%d" % i: b"x" for i in range(6)}
    plain = {k: {t: float(scores[i, j]) for j, t in enumerate(texts)} for i, k in enumerate(kps)}
    want = applications.keyphrases_graph(kps, texts, 0.4, 0.25, 1, _ArrayMeasure(scores))
    assert type(want) is dict and want["edges"]
    calls = []

    def recording(*a, **k):
        calls.append(a)
        return plain

    monkeypatch.setattr(applications, "keyphrases_table", recording)
    for measure, env, syn in ((_ArrayMeasure(scores), None, None), (_NoneGraphMeasure(scores), None, None),
                              (_RefusingGraphMeasure(scores), "host", None), (_RefusingGraphMeasure(scores), None, {"a": ["b"]})):
        if env is None:
            monkeypatch.delenv("EAST_HIP_GRAPH", raising=False)
        else:
            monkeypatch.setenv("EAST_HIP_GRAPH", env)
        del calls[:]
        got = applications.keyphrases_graph(kps, texts, 0.4, 0.25, 1, measure, syn)
        assert type(got) is dict and got == want and len(calls) == 1
        arrays = applications.keyphrases_graph_arrays(kps, texts, 0.4, 0.25, 1, measure, syn)
        assert isinstance(arrays, applications.KeyphraseGraph) and arrays == want and len(calls) == 2


def test_device_path_is_taken_when_the_measure_offers_it(monkeypatch):
    """A measure with `relevance_graph`: keyphrases_table is not called, the keyphrases are prepared and deduplicated as
    keyphrases_table does it, and the arrays that come back become the dict / the KeyphraseGraph."""
    from east import applications, hip_backend, utils
    monkeypatch.delenv("EAST_HIP_GRAPH", raising=False)
    seen = {}

    class Measure(object):
        def set_text_collection(self, texts, language=None):
            seen["texts"] = list(texts)

        def relevance_table(self, prepared):
            raise AssertionError("the table must not be fetched")

        def relevance_graph(self, prepared, rows, referral_confidence, relevance_threshold, support_threshold):
            seen["prepared"], seen["rows"] = list(prepared), rows.tolist()
            seen["thresholds"] = (referral_confidence, relevance_threshold, support_threshold)
            i32 = lambda *v: np.array(v, dtype=np.int32)
            return hip_backend.GraphArrays(i32(3, 0, 3), i32(0, 2), i32(0, 2), i32(2, 0), i32(3, 2))

    monkeypatch.setattr(applications, "keyphrases_table", lambda *a, **k: pytest.fail("host path taken"))
    kps = ["one two", "never", "one two"]
    texts = {"a": b"A", "b": b"B", "c": b"C"}
    got = applications.keyphrases_graph(kps, texts, 0.6, 0.25, 1, Measure())
    assert seen["prepared"] == [utils.prepare_text("one two"), utils.prepare_text("never")] and seen["rows"] == [0, 1, 0]
    assert seen["texts"] == [b"A", b"B", b"C"] and seen["thresholds"] == (0.6, 0.25, 1)
    assert type(got) is dict
    assert got == {"nodes": [{"id": 0, "label": "one two", "support": 3}, {"id": 2, "label": "one two", "support": 3}],
                   "edges": [{"source": 0, "target": 2, "confidence": 1.0}, {"source": 2, "target": 0, "confidence": 2.0 / 3}],
                   "referral_confidence": 0.6, "relevance_threshold": 0.25, "support_threshold": 1}
    arrays = applications.keyphrases_graph_arrays(kps, texts, 0.6, 0.25, 1, Measure())
    assert isinstance(arrays, applications.KeyphraseGraph) and arrays == got and arrays.support.tolist() == [3, 0, 3]
    with pytest.raises(KeyError):                           # an empty keyphrase: as table[""] on the host path
        applications.keyphrases_graph(["one", ""], texts, 0.6, 0.25, 1, Measure())


def test_topic_table_gives_a_graph_worth_comparing():
    """The generator of the configs[2]-shaped gpu case and of tools/graph_bench.py: between 10^5 and 10^7 edges at
    10 000 x 256, counted here with exact integer products."""
    from east import synthetic
    scores = synthetic.topic_score_table(np.random.default_rng(7), 10000, 256)
    hits = (scores >= 0.25).astype(np.float32)
    support = hits.sum(axis=1).astype(np.float64)
    edges = 0
    for b in range(0, 10000, 2500):
        conf = (hits[b:b + 2500] @ hits.T).astype(np.float64) / np.maximum(support[b:b + 2500, None], 1.0)
        found = conf >= 0.6
        edges += int(found.sum()) - int(found[np.arange(found.shape[0]), np.arange(b, b + found.shape[0])].sum())
    assert 10 ** 5 < edges < 10 ** 7, edges
