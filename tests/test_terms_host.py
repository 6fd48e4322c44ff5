"""CPU tier of the characteristic terms (include/east_hip.h, "Characteristic terms"): the model of tests/terms_exact.py on
a case worked by hand, the host path of east.applications against the model to the contract's bound on every generated
collection, the twice-the-bound rule for the names, the CLI through EAST_HIP_TERMS=host and the binding against the
header."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import cosine_exact
import terms_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["AAA AAA AAA BBB BBB BBB BBB", "AAA AAA AAA AAA CCC CCC CCC", "DDD DDD DDD EEE EEE EEE EEE"]


def _measure(stop=(), stems=False, tfidf=True):
    from east import relevance
    return relevance.CosineRelevanceMeasure("stems" if stems else "words", "tf-idf" if tfidf else "tf", stopwords=stop,
                                            stemmer=cosine_exact.ToyStemmer() if stems else None)


def _host_vectors(name, tfidf, group, G):
    from east import applications, relevance
    texts, stop, stems = model.collections()[name]
    measure = _measure(stop, stems, tfidf)
    doc_units, number, _ = relevance.host_doc_units(texts, measure, "english")
    group = list(range(len(texts))) if group is None else group
    return applications._terms_vectors(doc_units, len(number), tfidf, group, G), list(number)


# ---- the model on a case worked by hand -------------------------------------------------------------------------------------
def test_model_three_texts_by_hand():
    """tf: the texts' vectors are (3, 4) / 5 over (A, B), (4, 3) / 5 over (A, C) and (3, 4) / 5 over (D, E); texts 0 and 1
    are one group: A (3/5 + 4/5) / 2, B (4/5) / 2, C (3/5) / 2."""
    m = cosine_exact.build_model(HAND)
    assert m.terms == ["AAA", "BBB", "CCC", "DDD", "EEE"]
    ex = model.exact(m, False, [0, 0, 1], 2)
    assert ex.members.tolist() == [2, 1] and ex.offsets.tolist() == [0, 3, 5]
    assert ex.unit.tolist() == [0, 1, 2, 3, 4] and ex.texts.tolist() == [2, 1, 1, 1, 1]
    assert ex.value.tolist() == [0.7, 0.4, 0.3, 0.6, 0.8]
    assert ex.bound.tolist() == [2 + 0.5 + 48, 1 + 0.5 + 48, 1 + 0.5 + 48, 1 + 0.5 + 48, 1 + 0.5 + 48] and ex.df.tolist() == [2, 1, 1, 1, 1]
    count, unit, value, texts, df = model.ranked(ex.offsets, ex.unit, ex.value, ex.texts, ex.df, 1, 2)
    assert count.tolist() == [2, 2] and unit.tolist() == [[0, 1], [4, 3]] and value.tolist() == [[0.7, 0.4], [0.8, 0.6]]
    assert texts.tolist() == [[2, 1], [1, 1]] and df.tolist() == [[2, 1], [1, 1]]
    count, unit, value, _, _ = model.ranked(ex.offsets, ex.unit, ex.value, ex.texts, ex.df, 2, 2)
    assert count.tolist() == [1, 0] and unit.tolist() == [[0, -1], [-1, -1]] and np.isnan(value[1]).all()
    # tf-idf per text: idf(A) = 1 + ln(3 / 2), idf(B) = 1 + ln 3; text 0 is (3 idf_A, 4 idf_B) / its length
    ex = model.exact(m, True)
    a, b = 3 * (1 + np.log(1.5)), 4 * (1 + np.log(3.0))
    assert ex.value[:2] == pytest.approx([a / np.hypot(a, b), b / np.hypot(a, b)], rel=1e-15)


def test_rank_orders_by_value_then_unit_and_filters_by_texts():
    unit, value, texts = np.array([5, 2, 9, 1]), np.array([0.5, 0.25, 0.5, 0.125]), np.array([1, 3, 2, 2])
    assert model.rank(unit, value, texts, 1, 10) == [0, 2, 1, 3]
    assert model.rank(unit, value, texts, 2, 2) == [2, 1] and model.rank(unit, value, texts, 4, 2) == []


# ---- the host path against the model -------------------------------------------------------------------------------------
def _cases():
    for name, (texts, _, _) in model.collections().items():
        if name.startswith("runs"):
            yield name, "run", model.run_group(len(texts) - 1)
        elif name in ("segments", "ties", "long text"):
            yield name, "per text", (None, len(texts))
            if name == "long text":
                yield name, "one group", ([0] * len(texts), 1)
        else:
            yield name, "per text", (None, len(texts))
            for label, grouping in model.groupings(len(texts)).items():
                yield name, label, grouping


@pytest.mark.parametrize("name,label,grouping", list(_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_host_path_within_the_bound_of_the_model(name, label, grouping):
    group, G = grouping
    stems = model.collections()[name][2]
    for tfidf in (False, True):
        ex = model.exact(model.model_of(name), tfidf, group, G, stems)
        (members, offsets, unit, value, texts, df), names = _host_vectors(name, tfidf, group, G)
        assert np.array_equal(members, ex.members) and np.array_equal(df, ex.df)
        share = model.check_vectors(offsets, unit, value, texts, ex)
        print("%s, %s, %s: host path at %.3g of the bound" % (name, label, "tf-idf" if tfidf else "tf", share))
        if not stems:
            assert names == model.model_of(name).terms


def test_host_path_names_the_models_terms_where_the_rule_decides():
    """On the `spread` collection: per text, in four groups and in one, at most 5 % of all list positions are left undecided
    by the twice-the-bound rule (from the model alone), and the host path names the model's term at every decided one."""
    from east import applications
    texts = model.spread_texts()
    m = model.model_of("spread")
    positions = undecided = 0
    for tfidf in (False, True):
        for group, G in ((None, len(texts)), model.groupings(len(texts))["four equal"], ([0] * len(texts), 1)):
            ex = model.exact(m, tfidf, group, G)
            (_, offsets, unit, value, tx, _), _ = _host_vectors("spread", tfidf, group, G)
            for g, (want, flags) in enumerate(model.decided(ex, 1, 10)):
                a, e = int(offsets[g]), int(offsets[g + 1])
                got = a + applications._terms_ranked(unit[a:e], value[a:e], tx[a:e], 1, 10)
                assert len(got) == len(want)
                for r, ok in enumerate(flags):
                    positions += 1
                    undecided += not ok
                    if ok:
                        assert unit[got[r]] == ex.unit[want[r]], (tfidf, g, r)
    print("%d of %d list positions undecided" % (undecided, positions))
    assert positions > 500 and undecided <= 0.05 * positions


def test_texts_terms_on_the_host(monkeypatch):
    from east import applications
    monkeypatch.setenv("EAST_HIP_TERMS", "host")
    monkeypatch.setenv("EAST_HIP_CLUSTERS", "host")                 # (texts_clusters itself, for the comparison)
    texts = {"t%d" % d: text for d, text in enumerate(HAND)}
    found = applications.texts_terms(texts, 2, 1, _measure(tfidf=False))
    assert [g.names for g in found] == [["t0"], ["t1"], ["t2"]]
    assert [[t.text for t in g.terms] for g in found] == [["BBB", "AAA"], ["AAA", "CCC"], ["EEE", "DDD"]]
    assert found[0].terms[0] == applications.Term("BBB", pytest.approx(0.8, rel=1e-15), 1, 1)
    assert found[0].terms[1] == applications.Term("AAA", pytest.approx(0.6, rel=1e-15), 1, 2)
    # two clusters: texts 0 and 1 share AAA, text 2 stands alone -- the groups texts_clusters finds with the same arguments
    for linkage in applications.LINKAGES:
        found = applications.texts_terms(texts, 3, 1, _measure(tfidf=False), k=2, linkage=linkage)
        clusters = applications.texts_clusters(texts, None, 2, _measure(tfidf=False), linkage=linkage).clusters
        assert [g.names for g in found] == clusters == [["t0", "t1"], ["t2"]]
        assert [(t.text, t.texts, t.df) for t in found[0].terms] == [("AAA", 2, 2), ("BBB", 1, 1), ("CCC", 1, 1)]
        assert [t.value for t in found[0].terms] == pytest.approx([0.7, 0.4, 0.3], rel=1e-15)
    assert [t.text for t in applications.texts_terms(texts, 3, 2, _measure(tfidf=False), k=2)[0].terms] == ["AAA"]
    assert applications.texts_terms(texts, 3, 2, _measure(tfidf=False), k=2)[1].terms == []
    assert applications.texts_terms({}, 3, similarity_measure=_measure()) == []


def test_texts_terms_refuses_other_measures_and_bad_arguments():
    from east import applications, relevance

    class Other(object):
        pass

    with pytest.raises(ValueError, match="CosineRelevanceMeasure"):
        applications.texts_terms({"a": "x"}, similarity_measure=Other())
    bm25 = relevance.BM25RelevanceMeasure("words", stopwords=())
    with pytest.raises(ValueError, match="BM25"):
        applications.texts_terms({"a": "x"}, similarity_measure=bm25)
    for method in (lambda: bm25.relevance_terms(3), bm25.unit_names):
        with pytest.raises(ValueError, match="cosine measure's"):
            method()
    for bad in (dict(n=0), dict(n=1025), dict(n=1.5), dict(min_texts=0), dict(threshold=0.5, k=2), dict(k=0), dict(linkage="ward")):
        with pytest.raises(ValueError):
            applications.texts_terms({"a": "x"}, similarity_measure=_measure(), **bad)


def test_unit_names_inverts_the_stem_classes():
    m = _measure(stems=True)
    m._stem_class = {"RUN": 0, "TEST": 1, "FOX": 2}
    assert m.unit_names() == ["RUN", "TEST", "FOX"]


def test_format_terms():
    from east import applications, formatting
    result = [applications.TermGroup(["a", "b"], [applications.Term("FOX", 0.25, 2, 3), applications.Term('SAY "X"', 0.125, 1, 1)]),
              applications.TermGroup(["c"], [])]
    assert formatting.format_terms(result, "csv") == '"a|b","FOX",0.250,2,3\n"a|b","SAY \'X\'",0.125,1,1\n'
    assert formatting.format_terms(result, "xml") == (
        '<terms groups="2">\n  <group id="1" size="2">\n    <member name="a"/>\n    <member name="b"/>\n'
        '    <term rank="1" texts="2" df="3" value="0.250">FOX</term>\n    <term rank="2" texts="1" df="1" value="0.125">SAY "X"</term>\n'
        '  </group>\n  <group id="2" size="1">\n    <member name="c"/>\n  </group>\n</terms>\n')
    with pytest.raises(Exception, match="Unknown terms format"):
        formatting.format_terms(result, "txt")


# ---- the command line ---------------------------------------------------------------------------------------------------------
def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def test_cli_on_the_host_path(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("EAST_HIP_TERMS", "host")
    for d, text in enumerate(HAND):
        (tmp_path / ("t%d.txt" % d)).write_text(text)
    t = str(tmp_path)
    rc, out = _east(["-v", "words", "-w", "tf", "-n", "2", "-f", "csv", "texts", "terms", t])
    assert rc == 0 and out == ('"t0","BBB",0.800,1,1\n"t0","AAA",0.600,1,2\n"t1","AAA",0.800,1,2\n"t1","CCC",0.600,1,1\n'
                               '"t2","EEE",0.800,1,1\n"t2","DDD",0.600,1,1\n\n')
    for flags in (["-k", "2"], ["-k", "2", "-j", "average"], ["-r", "0.4", "-j", "complete"]):
        rc, out = _east(["-v", "words", "-w", "tf", "-n", "2"] + flags + ["-f", "csv", "texts", "terms", t])
        assert rc == 0 and out == '"t0|t1","AAA",0.700,2,2\n"t0|t1","BBB",0.400,1,1\n"t2","EEE",0.800,1,1\n"t2","DDD",0.600,1,1\n\n', flags
    rc, out = _east(["-v", "words", "-w", "tf", "-k", "2", "-u", "2", "texts", "terms", t])
    assert rc == 0 and out.count("<term ") == 1 and '<group id="1" size="2">' in out and 'texts="2" df="2" value="0.700">AAA</term>' in out


def test_cli_refuses_before_any_work(tmp_path, monkeypatch):
    from east import main, relevance
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    touched = []
    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr(main, "launch_ranks", lambda *a: touched.append("ranks") or 0)
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    t = str(tmp_path)
    refused = [(["-s", "ast"], "-s ast"), (["-s", "bm25"], "bm25"), (["-s", "other"], "-s other"), (["-v", "lemmata"], "-v lemmata"),
               (["-y"], "-y"), (["-o", "directed"], "-o directed"), (["-b", "text"], "-b text"), (["-c", "0.5"], "-c 0.5"),
               (["-p", "2"], "-p 2"), (["-r", "0.5", "-k", "2"], "one of the two"), (["-j", "average"], "-j average"),
               (["-j", "ward", "-k", "2"], "'ward'"), (["-n", "0"], "'0'"), (["-n", "1025"], "'1025'"), (["-n", "x"], "'x'"),
               (["-u", "0"], "'0'"), (["-u", "x"], "'x'"), (["-r", "x"], "'x'"), (["-r", "nan"], "'nan'"), (["-k", "0"], "'0'"),
               (["-k", "x"], "'x'"), (["-g", "2"], "-g 2"), (["-g", "x"], "'x'"), (["-f", "txt"], "'txt'")]
    for flags, said in refused:
        rc, out = _east(flags + ["texts", "terms", t])
        assert rc == 1 and out.count("\n") == 1 and said in out, (flags, out)
    rc, out = _east(["texts", "terms"])
    assert rc == 1 and "texts terms" in out
    rc, out = _east(["texts", "term", t])
    assert rc == 1 and out.count("\n") == 1 and "'terms'" in out
    monkeypatch.setenv("EAST_HIP_FORCE_DIST", "1")
    rc, out = _east(["texts", "terms", t])
    assert rc == 1 and out.count("\n") == 1 and "collective path" in out
    monkeypatch.delenv("EAST_HIP_FORCE_DIST")
    monkeypatch.setenv("WORLD_SIZE", "2")
    rc, out = _east(["texts", "terms", t])
    assert rc == 1 and out.count("\n") == 1 and "WORLD_SIZE=2" in out
    monkeypatch.setenv("RANK", "1")                                # (only rank 0 says it)
    assert _east(["-n", "0", "texts", "terms", t]) == (1, "")
    assert touched == []
    assert "texts terms" in main.__doc__


# ---- the binding against the header -------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        src = f.read()
    assert "Characteristic terms" in src
    names = ["east_hip_terms_build", "east_hip_terms_fetch", "east_hip_terms_fetch_vectors", "east_hip_last_terms_ms",
             "east_hip_debug_set_terms_select"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp,
                "int32_t *": hip_backend._c_i32p, "int32_t": ctypes.c_int32, "int": ctypes.c_int}
    for name in names:
        m = re.search(r"\b(int|double)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = hip_backend.SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "double": ctypes.c_double}[m.group(1)]
        declared = []
        for a in m.group(2).split(","):
            kind = re.match(r"^(.*?)\w+$", " ".join(a.split())).group(1).replace("const ", "").strip()
            declared.append(ctype_of[kind])
        assert declared == list(args), name
    assert len(hip_backend.TERMS_INFO_FIELDS) == 10
