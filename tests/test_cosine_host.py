"""CPU tier: the cosine relevance measure's contract (reference relevance.py:56-168, utils.py:31-46) restated in plain
Python and checked against the fixture recorded from the reference (tests/golden/cosine.json, tools/gen_cosine_golden.py),
and the refusals of `east -s cosine` -- none of which builds anything or needs a GPU."""
import io
import math
from collections import Counter
from contextlib import redirect_stdout

import pytest

from conftest import load_golden


class ToyStemmer(object):
    """The fixture's toy stemmer (tools/gen_cosine_golden.py): lower case, then a final ING or S stripped."""

    def stem(self, token):
        t = token.lower()
        for suffix in ("ing", "s"):
            if t.endswith(suffix) and len(t) > len(suffix) + 1:
                return t[:-len(suffix)]
        return t


def case_texts(golden, case):
    if "texts" in case:
        return case["texts"]
    texts = load_golden(case["texts_from"])["texts"]
    return [texts[name] for name in case["text_names"]]


def restate(texts, queries, space, weighting, stopwords=(), stemmer=None):
    """K x D scores of the contract: tokens [\\w']+ of the prepared text with >= 3 code points that are not stopwords
    (upper-cased), stemmed in the stems space; tf = count / max(n_d, 1), times 1 + ln(D / df) under tf-idf; the query's
    entries count / max(its tokens, 1) over the collection's terms; dot / (|w_d| |q|), the norm of a zero vector 1."""
    from east import utils
    stop = frozenset(utils.prepare_text(w) for w in stopwords)

    def terms(text):
        tokens = [t for t in utils.tokenize(utils.prepare_text(text)) if len(t) >= 3 and t not in stop]
        return [stemmer.stem(t) for t in tokens] if space == "stems" else tokens

    docs = [terms(t) for t in texts]
    order = {}
    for doc in docs:
        for t in doc:
            order.setdefault(t, len(order))
    df = Counter(t for doc in docs for t in set(doc))
    weights, norms = [], []
    for doc in docs:
        counts = Counter(doc)
        w = {}
        for t in sorted(counts, key=order.get):
            tf = counts[t] * 1.0 / max(len(doc), 1)
            w[t] = tf * (1.0 + math.log(len(docs) * 1.0 / df[t])) if weighting == "tf-idf" else tf
        s = 0.0
        for v in w.values():
            s += v * v
        weights.append(w)
        norms.append(math.sqrt(s) if w else 1.0)
    out = []
    for query in queries:
        qt = terms(query)
        counts = Counter(qt)
        q = {}
        for t in qt:
            if t in order and t not in q:
                q[t] = counts[t] * 1.0 / max(len(qt), 1)
        qn = math.sqrt(sum(v * v for v in q.values())) if q else 1.0
        row = []
        for w, norm in zip(weights, norms):
            dot = 0.0
            for t, v in q.items():
                dot += w.get(t, 0.0) * v
            row.append(dot / (norm * qn))
        out.append(row)
    return out


def assert_scores(got, want, tol=1e-12):
    assert len(got) == len(want)
    for g_row, w_row in zip(got, want):
        assert len(g_row) == len(w_row)
        for g, w in zip(g_row, w_row):
            assert abs(g - w) <= tol, (g, w)
            assert (g == 0.0) == (w == 0.0), (g, w)


def test_restatement_matches_the_reference_fixture():
    g = load_golden("cosine.json")
    stemmer = ToyStemmer()
    for word, stem in g["toy_stems"].items():
        assert stemmer.stem(word) == stem
    n = 0
    for case in g["cases"]:
        texts = case_texts(g, case)
        for mode in case["modes"]:
            got = restate(texts, case["queries"], mode["space"], mode["weighting"],
                          g["stopwords"] if mode["stopwords"] else (), stemmer)
            assert_scores(got, mode["scores"])
            n += 1
    assert n == 15
    # what the fixture pins: DON'T and 123 are terms, empty texts / queries score 0.0, one text means idf = 1
    synthetic = g["cases"][1]
    words_tfidf = synthetic["modes"][1]["scores"]
    assert synthetic["queries"][2] == "don't 123" and words_tfidf[2][1] > 0.0
    assert synthetic["texts"][8] == "" and all(row[8] == 0.0 for row in words_tfidf)
    assert synthetic["queries"][13] == "a" and all(x == 0.0 for x in words_tfidf[13])


def test_cli_table_xml_of_the_fixture_is_the_formatted_table():
    from east import formatting
    g = load_golden("cosine.json")["cli"]
    assert formatting.table2xml(g["table"]) == g["xml"]
    texts = load_golden("hse_config1.json")["texts"]
    names = sorted(texts)
    want = restate([texts[n] for n in names], g["keyphrases"], "words", "tf-idf")
    assert_scores([[g["table"][kp][n] for n in names] for kp in g["keyphrases"]], want)


def _cli(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def _nltk_importable():
    try:
        import nltk  # noqa: F401
        return True
    except ImportError:
        return False


@pytest.fixture
def no_device_work(monkeypatch):
    """Every way to the device fails the test."""
    from east import hip_backend

    def refuse(*args, **kwargs):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(hip_backend.HipIndex, "__init__", refuse)
    monkeypatch.setattr(hip_backend.HipCosineIndex, "__init__", refuse)
    monkeypatch.setattr(hip_backend, "load", refuse)


def test_cli_cosine_refusals(tmp_path, monkeypatch, no_device_work):
    kp = tmp_path / "k.txt"
    kp.write_text("quick fox\n")
    tx = tmp_path / "t.txt"
    tx.write_text("the quick brown fox\n")
    args = ["keyphrases", "table", str(kp), str(tx)]
    rc, out = _cli(["-s", "cosine", "-v", "lemmata"] + args)
    assert rc == 1 and "lemmata" in out and len(out.strip().splitlines()) == 1
    rc, out = _cli(["-s", "cosine", "-v", "words", "-w", "bogus"] + args)
    assert rc == 1 and "bogus" in out and len(out.strip().splitlines()) == 1
    rc, out = _cli(["-s", "cosine", "-v", "bogus"] + args)
    assert rc == 1 and "bogus" in out
    rc, out = _cli(["-s", "cosine", "-v", "words", "-g", "2"] + args)
    assert rc == 1 and "one device" in out
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    rc, out = _cli(["-s", "cosine", "-v", "words"] + args)
    assert rc == 1 and "one device" in out
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    if not _nltk_importable():
        rc, out = _cli(["-s", "cosine"] + args)            # the default -v stems
        assert rc == 1 and "stemmer" in out.lower() and "-v words" in out
    rc, out = _cli(["-s", "nonsense"] + args)
    assert rc == 1 and "'cosine'" in out


def test_measure_arguments_without_device_work(no_device_work):
    from east import consts, exceptions, relevance
    with pytest.raises(exceptions.LemmataUnavailableException):
        relevance.CosineRelevanceMeasure(consts.VectorSpace.LEMMATA)
    with pytest.raises(exceptions.NoSuchVectorSpace):
        relevance.CosineRelevanceMeasure("letters", stemmer=ToyStemmer())
    with pytest.raises(exceptions.NoSuchTermWeighting):
        relevance.CosineRelevanceMeasure("words", "bm25")
    m = relevance.CosineRelevanceMeasure("stems", "tf", stemmer=ToyStemmer(), stopwords=["the", "don't"])
    assert m.stopwords == frozenset(["THE", "DON'T"]) and m.stopwords_source == "given"
    assert m._query_terms("TESTING THE TESTS A 123") == ["test", "test", "123"]
    if not _nltk_importable():
        with pytest.raises(exceptions.StemmerUnavailableException) as e:
            relevance.CosineRelevanceMeasure()
        assert isinstance(e.value, exceptions.EastException) and "-v words" in str(e.value)
        m = relevance.CosineRelevanceMeasure("words")
        assert m.stopwords == frozenset() and m.stopwords_source == "none"


def test_cosine_binding_matches_the_header():
    """Every cosine entry point of include/east_hip.h has its ctypes signature (the one-to-one check of the whole header
    is test_host_logic's)."""
    from east import hip_backend
    names = [n for n in hip_backend.SIGNATURES if "cosine" in n or "term_hash" in n]
    assert sorted(names) == sorted(["east_hip_cosine_build_texts", "east_hip_cosine_build_texts_v", "east_hip_cosine_info",
                                    "east_hip_cosine_get_terms", "east_hip_cosine_set_classes", "east_hip_cosine_lookup",
                                    "east_hip_cosine_score_table", "east_hip_debug_set_term_hash_bits"])
    assert len(hip_backend.COSINE_INFO_FIELDS) == 10
