# -*- coding: utf-8 -*-
"""CPU tier: the exact BM25 model (tests/bm25_exact.py) pinned to the worked case of include/east_hip.h's contract, the
host path of relevance.BM25RelevanceMeasure (EAST_HIP_BM25=host) held to the bound of the GPU tier on every collection
tests/test_gpu_bm25.py uses -- the attainability check of that tier --, the command line through the host path and every
refusal of `east -s bm25`.  Nothing here builds anything on a device.

Largest share of the bound (t + 24) * 2^-53 the host path reached here: 0.20, on the Zipf collection (every check prints
its own)."""
import io
import math
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import bm25_exact
import cosine_exact
from test_cosine_host import no_device_work  # noqa: F401  (the fixture)


@pytest.fixture
def host(monkeypatch, no_device_work):  # noqa: F811
    monkeypatch.setenv("EAST_HIP_BM25", "host")


def _cli(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def _prepared(queries):
    from east import utils
    return [utils.prepare_text(q) for q in queries]


# ---- the model --------------------------------------------------------------------------------------------------------------
def test_model_is_pinned_to_the_worked_case():
    model = cosine_exact.build_model(bm25_exact.WORKED_TEXTS)
    assert model.n_d == [3, 2] and bm25_exact.total(model) == 5 and bm25_exact.avgdl(model) == 2.5
    bm = bm25_exact.Bm25(model)
    got, terms = bm.scores(list(bm25_exact.WORKED))
    for row, t, want in zip(got, terms, bm25_exact.WORKED.values()):
        for g, n, w in zip(row, t, want):
            if w is None:
                continue
            if w == 0.0:
                assert g == 0.0 and not math.copysign(1.0, g) < 0 and n == 0
            else:
                assert abs(g - w) <= 1e-15 * w, (g, w)
    assert got[0][0] == pytest.approx(math.log(2.0) * 4.4 / 3.38, rel=1e-15)
    assert terms[3].tolist() == [2, 1]


def test_model_facts():
    texts, stop = bm25_exact.small_collection_full_df()
    model = cosine_exact.build_model(texts, stop)
    D = model.n_docs
    every = model.term_id["EVERY"]
    assert model.df[every] == D and model.counts[1][model.term_id["THOUSAND"]] == 1000
    # k1 = 0: the sum of qtf * idf
    ids = [[every, model.term_id["ALPHA"], every], [model.term_id["BETA"]]]
    got, _ = bm25_exact.Bm25(model, 0.0, 0.75).scores_from_ids(ids)
    for k, q in enumerate(ids):
        for d in range(D):
            want = sum(bm25_exact.idf(D, model.df[u]) * q.count(u) for u in dict.fromkeys(q) if u in model.counts[d])
            assert got[k, d] == float(want)
    # b = 0 does not depend on n_d: the same counts in documents of other lengths
    longer = cosine_exact.build_model([t + " padding words here" * (i + 1) for i, t in enumerate(texts)], stop)
    a, _ = bm25_exact.Bm25(model, 2.0, 0.0).scores_from_ids(ids)
    b, _ = bm25_exact.Bm25(longer, 2.0, 0.0).scores_from_ids(ids)
    assert longer.n_d != model.n_d and np.array_equal(a, b)
    c, _ = bm25_exact.Bm25(longer, 2.0, 0.5).scores_from_ids(ids)
    assert not np.array_equal(a, c)
    # idf strictly decreases in df and is > 0 at df = D
    for n_docs in (1, 2, 7, 1 << 20):
        values = [bm25_exact.idf(n_docs, df) for df in sorted(set([1, 2, 3, n_docs // 2 + 1, n_docs - 1, n_docs])) if 1 <= df <= n_docs]
        assert all(x > y for x, y in zip(values, values[1:])) and values[-1] > 0
    assert float(bm25_exact.idf(1 << 20, 1 << 20)) == pytest.approx(math.log1p(0.5 / ((1 << 20) + 0.5)), rel=1e-15)


# ---- the host path against the model ------------------------------------------------------------------------------------------
def _host_scores(texts, stopwords, space, queries, k1, b, stemmer=None):
    from east import relevance
    m = relevance.BM25RelevanceMeasure(space, k1, b, stopwords=stopwords, stemmer=stemmer)
    assert m.on_host and m.relevance_graph is None and m.relevance_top is None and m.relevance_similar is None
    assert m.relevance_clusters is None and m.index is None
    m.set_text_collection(texts)
    return m.relevance_table(_prepared(queries))


def _all_queries(model):
    return list(model.terms) + ["NOPE"]


def test_host_path_worked_case_and_weights_of_every_posting(host):
    model = cosine_exact.build_model(bm25_exact.WORKED_TEXTS)
    queries = list(bm25_exact.WORKED)
    exact, terms = bm25_exact.Bm25(model).scores(queries)
    bm25_exact.check(_host_scores(bm25_exact.WORKED_TEXTS, (), "words", queries, 1.2, 0.75), exact, terms, "worked case")
    shares = []
    for texts, stop in (bm25_exact.small_collection(), bm25_exact.small_collection_full_df(), (["alpha beta alpha"], ())):
        model = cosine_exact.build_model(texts, stop)
        queries = _all_queries(model) + ["BETA BETA ALPHA", "ALPHA ALPHA ALPHA EVERY", ""]
        for k1, b in bm25_exact.PARAMETERS:
            exact, terms = bm25_exact.Bm25(model, k1, b).scores(queries)
            shares.append(bm25_exact.check(_host_scores(texts, stop, "words", queries, k1, b), exact, terms, "k1 %g b %g" % (k1, b)))
    assert max(shares) > 0.0


@pytest.mark.parametrize("D", [1, 63, 64, 65, 257])
def test_host_path_one_line_documents(host, D):
    texts = cosine_exact.one_line_documents(D)
    model = cosine_exact.build_model(texts)
    queries = ["EVERY", "SECOND ODD", "GROUP0 EVERY EVERY", "ONLY%d" % (D - 1), "GROUP%d ONLY0 SECOND SECOND SECOND" % ((D - 1) // 7), "NOPE"]
    exact, terms = bm25_exact.Bm25(model).scores(queries)
    bm25_exact.check(_host_scores(texts, (), "words", queries, 1.2, 0.75), exact, terms)


def test_host_path_stems(host):
    texts = ["testing the tests of a test", "tests and foxes", "fox testing", ""]
    model = cosine_exact.build_model(texts, ["the", "and"], cosine_exact.ToyStemmer())
    queries = ["TESTS FOX", "TESTING TESTING FOXES", "THE", "NOPE TEST"]
    exact, terms = bm25_exact.Bm25(model, stems=True).scores(queries)
    assert (terms.max(axis=1) == [2, 2, 0, 1]).all()
    bm25_exact.check(_host_scores(texts, ["the", "and"], "stems", queries, 1.2, 0.75, cosine_exact.ToyStemmer()), exact, terms, "stems")


def test_host_path_fuzz_rounds(host):
    above, worst = 0, 0.0
    for r in cosine_exact.fuzz_rounds()[:50]:
        stems = r["space"] == "stems"
        model = cosine_exact.build_model(r["texts"], r["stopwords"], cosine_exact.ToyStemmer() if stems else None)
        queries = _prepared(r["queries"])
        exact, terms = bm25_exact.Bm25(model, stems=stems).scores(queries)
        got = _host_scores(r["texts"], r["stopwords"], r["space"], r["queries"], 1.2, 0.75, cosine_exact.ToyStemmer())
        share, n, zeros_ok = bm25_exact.share_of_bound(got, exact, terms)
        assert zeros_ok and share <= 1.0, share
        above += n
        worst = max(worst, share)
    print("fuzz: %d scores above zero, largest error %.3f of the bound" % (above, worst))
    assert above >= 150


@pytest.mark.parametrize("stems", [False, True])
def test_host_path_zipf_collection(host, stems):
    texts, queries, _ = cosine_exact.zipf_collection()
    model = cosine_exact.zipf_model(False)
    queries = queries[:300]
    exact, terms = bm25_exact.Bm25(model, stems=stems).scores(queries)
    got = _host_scores(texts, (), "stems" if stems else "words", queries, 1.2, 0.75, cosine_exact.ToyStemmer())
    bm25_exact.check(got, exact, terms, "zipf")


# ---- the command line through the host path -------------------------------------------------------------------------------------
@pytest.fixture
def files(tmp_path):
    kp = tmp_path / "k.txt"
    kp.write_text("quick fox\nlazy dog\nriver bank\nfox\n")
    tx = tmp_path / "t.txt"
    tx.write_text("the quick brown fox jumps over the lazy dog\nthe river bank and the fox\nlazy river dog dog\nquick quick bank\n")
    return str(kp), str(tx)


def test_cli_commands_print_through_the_host_path(host, files):
    from east import applications, formatting, relevance
    kp, tx = files
    rc, out = _cli(["-s", "bm25", "-v", "words", "-f", "csv", "keyphrases", "table", kp, tx])
    assert rc == 0
    keyphrases = open(kp).read().splitlines()
    texts = {str(i): line for i, line in enumerate(open(tx, "rb").read().splitlines())}
    table = applications.keyphrases_table(keyphrases, texts, relevance.BM25RelevanceMeasure("words"))
    assert out == formatting.format_table(table, "csv") + "\n"
    assert table["fox"]["0"] > 0.0 and table["fox"]["2"] == 0.0
    rc, other = _cli(["-s", "bm25", "-v", "words", "-z", "0,0.5", "-f", "csv", "keyphrases", "table", kp, tx])
    assert rc == 0 and other != out
    for command, extra in (("top", ["-n", "2"]), ("graph", ["-r", "0.1"]), ("similar", ["-n", "2"]), ("clusters", ["-k", "2"])):
        rc, out = _cli(["-s", "bm25", "-v", "words"] + extra + ["keyphrases", command, kp, tx])
        assert rc == 0 and out.strip(), command


def test_cli_refusals(tmp_path, monkeypatch, no_device_work):  # noqa: F811
    def refuse_reading(path):
        raise AssertionError("a file was read")
    from east import main
    monkeypatch.setattr(main, "_read", refuse_reading)
    args = ["keyphrases", "table", "k.txt", "t.txt"]

    def one_line(argv, *words):
        rc, out = _cli(argv)
        assert rc == 1 and len(out.strip().splitlines()) == 1, out
        for w in words:
            assert w in out, (w, out)
    one_line(["-s", "bm25", "-w", "tf"] + args, "-w", "'bm25'")
    one_line(["-z", "1.2,0.75"] + args, "-z", "-s bm25")
    one_line(["-s", "cosine", "-z", "1.2,0.75"] + args, "-z", "-s bm25")
    for bad in ("1.2", "1.2,0.75,3", "a,b", ",", "-1,0.5", "inf,0.5", "nan,0.5", "1,-0.1", "1,1.5", "1,nan", ""):
        one_line(["-s", "bm25", "-z", bad] + args, "Invalid BM25 parameters", "'%s'" % bad)
    one_line(["-s", "bm25", "-v", "lemmata"] + args, "lemmata", "'bm25'")
    one_line(["-s", "bm25", "-v", "words", "-g", "2"] + args, "'bm25' runs on one device", "-g 2")
    one_line(["-s", "bm25", "-v", "words", "-g", "two"] + args, "Invalid number of GPUs")
    for sub in ("top", "similar", "graph", "clusters"):
        one_line(["-s", "bm25", "-v", "words", "-g", "2", "keyphrases", sub, "k.txt", "t.txt"], "'bm25' runs on one device")
    monkeypatch.setenv("EAST_HIP_FORCE_DIST", "1")
    one_line(["-s", "bm25", "-v", "words"] + args, "'bm25' runs on one device", "collective path")
    monkeypatch.delenv("EAST_HIP_FORCE_DIST")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    one_line(["-s", "BM25", "-v", "words"] + args, "'bm25' runs on one device", "WORLD_SIZE=2")
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    for command in (["texts", "similar"], ["texts", "related"], ["texts", "clusters"], ["keyphrases", "extract"]):
        one_line(["-s", "bm25"] + command + ["t.txt"], "'bm25'", " ".join(command))


def test_unknown_measure_line_names_the_three(files, no_device_work):  # noqa: F811
    kp, tx = files
    for argv in (["-s", "nonsense", "keyphrases", "table", kp, tx], ["-s", "nonsense", "-k", "2", "keyphrases", "clusters", kp, tx]):
        rc, out = _cli(argv)
        assert rc == 1 and "(use 'ast', 'cosine' or 'bm25')" in out and "'cosine'" in out


def test_missing_nltk_is_cosines_behaviour(no_device_work):  # noqa: F811
    from east import exceptions, relevance
    try:
        import nltk  # noqa: F401
        return
    except ImportError:
        pass
    with pytest.raises(exceptions.StemmerUnavailableException):
        relevance.BM25RelevanceMeasure()
    rc, out = _cli(["-s", "bm25", "keyphrases", "table", __file__, __file__])
    assert rc == 1 and "stemmer" in out.lower() and "-v words" in out
    assert relevance.BM25RelevanceMeasure("words").stopwords_source == "none"


# ---- everything else ------------------------------------------------------------------------------------------------------------
def test_constructor_and_applications_refuse_without_device_work(no_device_work):  # noqa: F811
    from east import applications, consts, exceptions, relevance
    for k1, b in ((-1, 0.5), (float("inf"), 0.5), (float("nan"), 0.5), (1, -0.1), (1, 1.1), (1, float("nan")), ("x", 0.5), (None, 0.5)):
        with pytest.raises(ValueError):
            relevance.BM25RelevanceMeasure("words", k1, b)
    with pytest.raises(exceptions.LemmataUnavailableException):
        relevance.BM25RelevanceMeasure(consts.VectorSpace.LEMMATA)
    with pytest.raises(exceptions.NoSuchVectorSpace):
        relevance.BM25RelevanceMeasure("letters", stemmer=cosine_exact.ToyStemmer())
    with pytest.raises(exceptions.NoSuchTermWeighting):
        relevance.CosineRelevanceMeasure("words", "bm25")          # BM25 is a measure, not a -w value
    assert consts.RelevanceMeasure.BM25 == "bm25" and "bm25" not in consts.TermWeighting
    m = relevance.BM25RelevanceMeasure("words")
    assert isinstance(m, relevance.CosineRelevanceMeasure) and (m.k1, m.b) == (1.2, 0.75) and not m.on_host
    m = relevance.BM25RelevanceMeasure("words", 0, 1)
    assert (m.k1, m.b) == (0.0, 1.0)
    for call in (lambda: m.relevance_texts_similar(3), m.text_similarity_matrix, m.extract_phrases, m.relevance_clusters):
        with pytest.raises(ValueError) as e:
            call()
        assert "cosine" in str(e.value).lower() and len(str(e.value).splitlines()) == 1
    texts = {"a": "alpha beta", "b": "beta gamma"}
    for call in (lambda: applications.texts_similar(texts, 1, None, m), lambda: applications.texts_clusters(texts, None, 1, m)):
        with pytest.raises(ValueError) as e:
            call()
        assert "cosine" in str(e.value).lower() and "BM25RelevanceMeasure" in str(e.value)


def test_binding_matches_the_header_and_options():
    import ctypes
    import os
    from east import hip_backend, main
    names = sorted(n for n in hip_backend.SIGNATURES if "bm25" in n)
    assert names == ["east_hip_bm25_info", "east_hip_bm25_score_table", "east_hip_debug_set_bm25_strip"]
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "east_hip.h")) as f:
        header = f.read()
    assert "\n * BM25 (" in header
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "const int32_t *": hip_backend._c_i32p, "const int64_t *": hip_backend._c_i64p,
                "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "double *": hip_backend._c_dblp}
    for name in names:
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, name
        types = []
        for arg in decl.group(1).replace("\n", " ").split(","):
            kind = re.sub(r"\w+$", "", arg.strip()).strip()
            types.append(ctype_of[kind])
        res, args = hip_backend.SIGNATURES[name]
        assert res is ctypes.c_int and args == types, name
    assert len(hip_backend.BM25_INFO_FIELDS) == 5
    assert "z:" in main._OPTIONS and "-s bm25" in main.__doc__
