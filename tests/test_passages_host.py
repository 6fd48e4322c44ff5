"""CPU tier of the shared passages (include/east_hip.h, "Shared passages"): the model of tests/passages_exact.py pinned to
cases worked by hand, the host path of east.applications held to the model with == on every generated collection, w = 1 .. 8;
the distinct shingles at the shared starts against the overlap's intersections; the command line through
EAST_HIP_PASSAGES=host (both formats, every refusal with no file opened) and the binding against the header.  Nothing here
has a tolerance."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import pytest

import cosine_exact
import overlap_exact
import passages_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _measure(stop=()):
    from east import relevance
    return relevance.CosineRelevanceMeasure("words", "tf", stopwords=stop)


def _triples(found):
    return list(zip(found["start"], found["words"], found["at"]))


# ---- the model by hand ----------------------------------------------------------------------------------------------------
def test_model_worked_case():
    found = model.exact(model.WORKED, (), [(0, 1), (1, 0)], 2)
    assert found["text_start"] == [0, 7, 12]
    assert found["pair_off"] == [0, 2, 3] and _triples(found) == [(1, 3, 8), (5, 2, 8), (8, 3, 1)]
    assert found["starts"] == [3, 2] and found["covered"] == [5, 3] and found["found"] == [2, 1]
    tokens = model.token_lists(model.WORKED)
    assert [" ".join(tokens[0][1:4]), " ".join(tokens[0][5:7])] == ["BCD CDE DEF", "BCD CDE"]


def test_model_a_stopword_splits_a_passage():
    texts = ("aaa bbb the ccc ddd", "aaa bbb ccc ddd the aaa bbb")
    found = model.exact(texts, model.STOP, [(0, 1), (1, 0)], 2)
    # AAA BBB | the | CCC DDD in text 0: BBB CCC is no shingle of text 0; in text 1 BBB CCC is not shared, so 3 passages there
    assert _triples(found)[:2] == [(0, 2, 5), (3, 2, 7)] and found["starts"][0] == 2 and found["covered"][0] == 4
    assert _triples(found)[2:] == [(5, 2, 0), (7, 2, 3), (10, 2, 0)]
    whole = model.exact(texts, (), [(1, 0)], 2)         # without the stopword the break is a word of its own
    assert _triples(whole) == [(5, 2, 0), (7, 2, 3), (10, 2, 0)]


def test_model_no_passage_crosses_a_text_boundary():
    texts = model.neighbours_texts()
    found = model.exact(texts, (), [(0, 3), (1, 3), (1, 2)], 1)
    # CCC ends text 0 at position 2, DDD starts text 1 at position 3; text 3 holds both, next to each other
    assert _triples(found) == [(0, 1, 9), (2, 1, 10), (3, 1, 11), (5, 1, 8), (3, 1, 7)]
    assert found["starts"] == [2, 2, 1] and found["covered"] == [2, 2, 1]
    assert model.exact(texts, (), [(0, 3)], 2)["starts"] == [0]


def test_model_one_word_300_times():
    texts = (" ".join(["aaa"] * 300), "aaa aaa")
    found = model.exact(texts, (), [(0, 1), (1, 0)], 2)
    assert _triples(found) == [(0, 300, 300), (300, 2, 0)] and found["starts"] == [299, 1] and found["covered"] == [300, 2]
    assert model.exact(texts, (), [(0, 1)], 2, 301)["found"] == [0]


def test_model_order_and_cut():
    texts = model.order_texts()
    found = model.exact(texts, (), [(0, 1)], 2)
    assert found["words"] == [5, 5, 3, 3, 3, 2] and found["start"] == [4, 17, 0, 10, 23, 14]
    cut = model.exact(texts, (), [(0, 1)], 2, 3, 4)
    assert cut["found"] == [5] and cut["start"] == [4, 17, 0, 10] and cut["starts"] == found["starts"] == [15]


# ---- the host path against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(model.generated()))
def test_host_path_against_the_model(name):
    from east import applications
    texts, stop = model.generated()[name]
    D = len(texts)
    pairs = model.some_pairs(D, 30) if D > 1 else []
    _, positions = applications._passage_tokens(texts, cosine_exact.prepared_stopwords(stop))
    assert positions == model.token_lists(texts, stop)
    for w in range(1, model.MAX_WORDS + 1):
        for min_words, per_pair in ((None, 0), (w + 1, 2)):
            want = model.exact(texts, stop, pairs, w, min_words, per_pair)
            base = want["text_start"]
            for i, (a, b) in enumerate(pairs):
                starts, covered, found, passages = applications._passages_of_pair(positions[a], positions[b], w, min_words or w, per_pair)
                assert (starts, covered, found) == (want["starts"][i], want["covered"][i], want["found"][i]), (name, w, a, b)
                assert [(j + base[a], n, at + base[b]) for j, n, at in passages] == _triples(want)[want["pair_off"][i]:want["pair_off"][i + 1]]


@pytest.mark.parametrize("name", sorted(model.generated()))
def test_distinct_shingles_at_the_shared_starts_are_the_overlap(name):
    texts, stop = model.generated()[name]
    tokens = model.token_lists(texts, stop)
    for w in (1, 2, 4):
        I = overlap_exact.exact(texts, stop, w)[3]
        for a, b in (model.some_pairs(len(texts), 30) if len(texts) > 1 else []):
            assert len(model.pair_exact(tokens, a, b, w)[4]) == I[a, b], (name, w, a, b)


def test_application_on_the_host(monkeypatch):
    from east import applications
    monkeypatch.setenv("EAST_HIP_PASSAGES", "host")
    texts = {"t%d" % d: text for d, text in enumerate(model.content_texts())}
    ranked = applications.texts_passages(texts, 2, 2, similarity_measure=_measure(model.STOP))
    assert list(ranked) == list(texts)
    monkeypatch.setenv("EAST_HIP_OVERLAP", "host")
    overlap = applications.texts_overlap(texts, 2, 2, similarity_measure=_measure(model.STOP))
    assert {t: [(p.other, p.value) for p in pairs] for t, pairs in ranked.items()} == overlap
    first = ranked["t0"][1]
    whole = model.content_texts()[0].upper()
    assert first == applications.PassagePair("t3", 0.6, 9, 10, 1, [applications.Passage(0, 10, 3, whole)])
    assert ranked["t4"][0].passages == [] and ranked["t4"][0].starts == 0
    named = applications.texts_passages(texts, words=3, per_pair=1, pairs=[("t3", "t0"), ("t0", "t3"), ("t3", "t0")],
                                        similarity_measure=_measure(model.STOP))
    assert list(named) == ["t3", "t0"] and named["t3"][0] == named["t3"][1]
    assert named["t3"][0] == applications.PassagePair("t0", None, 8, 10, 1, [applications.Passage(3, 10, 0, whole)])
    assert applications.texts_passages({}, 3) == {}
    # the positions are the text's own, whatever stands in front of it in the collection
    shifted = applications.texts_passages({"x": "one two three", "a": model.WORKED[0], "b": model.WORKED[1]}, words=2, pairs=[("a", "b")],
                                          similarity_measure=_measure())
    assert [tuple(p) for p in shifted["a"][0].passages] == [(1, 3, 1, "BCD CDE DEF"), (5, 2, 1, "BCD CDE")]


def test_arguments_are_refused():
    from east import applications, relevance
    texts = {"a": "xxx yyy", "b": "xxx yyy"}
    for bad in (dict(words=0), dict(words=9), dict(words=2.5), dict(words=True), dict(orientation="both"), dict(n=0), dict(n=1025),
                dict(overlap_threshold=float("nan")), dict(similarity_measure=object()), dict(min_words=3), dict(min_words=2.5),
                dict(per_pair=-1), dict(per_pair=True), dict(pairs=[("a", "a")]), dict(pairs=[("a", "c")]), dict(pairs=[("a",)])):
        with pytest.raises(ValueError):
            applications.texts_passages(texts, **bad)
    bm25 = relevance.BM25RelevanceMeasure.__new__(relevance.BM25RelevanceMeasure)
    with pytest.raises(ValueError, match="BM25"):
        applications.texts_passages(texts, similarity_measure=bm25)
    with pytest.raises(ValueError, match="cosine measure's"):
        bm25.shared_passages([(0, 1)])


# ---- the command line ---------------------------------------------------------------------------------------------------------
def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


CLI_TEXTS = (model.WORKED[0], model.WORKED[1], "xxx yyy zzz")


def test_cli_on_the_host_path(tmp_path, monkeypatch):
    from east import relevance
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("EAST_HIP_PASSAGES", "host")
    monkeypatch.setattr(relevance, "default_stopwords", lambda: frozenset())
    for d, text in enumerate(CLI_TEXTS):
        (tmp_path / ("t%d.txt" % d)).write_text(text)
    t = str(tmp_path)
    rc, out = _east(["-x", "2", "-f", "csv", "texts", "passages", t])
    assert rc == 0
    assert out == ('"t0","t1",0.286,1,3,1,"BCD CDE DEF"\n"t0","t1",0.286,5,2,1,"BCD CDE"\n'       # (2 / (5 + 4 - 2))
                   '"t1","t0",0.286,1,3,1,"BCD CDE DEF"\n\n')
    rc, out = _east(["-x", "2", "-m", "3", "-n", "1", "-o", "directed", "texts", "passages", t])
    assert rc == 0 and out.startswith("<passages>\n") and out.count("<passage ") == 2
    assert ('  <text name="t0">\n    <text name="t1" rank="1" value="0.400" starts="3" covered="5" found="1">\n'
            '      <passage start="1" words="3" at="1">BCD CDE DEF</passage>\n    </text>\n  </text>\n') in out
    assert '<text name="t2">\n    <text name="t0" rank="1" value="0.000" starts="0" covered="0" found="0">\n    </text>' in out
    rc, out = _east(["-x", "2", "-k", "1", "-r", "0.1", "-f", "csv", "texts", "passages", t])
    assert rc == 0 and out.count("\n") == 3 and '"BCD CDE"\n' not in out
    rc, out = _east(["-x", "2", "-k", "0", "-f", "csv", "texts", "passages", t])
    assert rc == 0 and out.count("\n") == 4


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
    refused = [(["-s", "cosine"], "-s cosine"), (["-s", "ast"], "-s ast"), (["-s", "bm25"], "bm25"), (["-w", "tf"], "-w tf"),
               (["-v", "words"], "-v words"), (["-y"], "-y"), (["-b", "text"], "-b text"), (["-c", "0.5"], "-c 0.5"), (["-p", "2"], "-p 2"),
               (["-u", "2"], "-u 2"), (["-z", "1.2,0.75"], "-z"), (["-j", "single"], "-j single"), (["-g", "2"], "-g 2"), (["-g", "x"], "'x'"),
               (["-x", "0"], "'0'"), (["-x", "9"], "'9'"), (["-x", "two"], "'two'"), (["-m", "3"], "'3'"), (["-x", "3", "-m", "2"], "'2'"),
               (["-m", "x"], "'x'"), (["-k", "-1"], "'-1'"), (["-k", "x"], "'x'"), (["-n", "0"], "'0'"), (["-n", "1025"], "'1025'"),
               (["-n", "x"], "'x'"), (["-r", "x"], "'x'"), (["-r", "nan"], "'nan'"), (["-o", "both"], "'both'"), (["-f", "txt"], "'txt'"),
               (["-f", "merges"], "'merges'")]
    for flags, said in refused:
        rc, out = _east(flags + ["texts", "passages", t])
        assert rc == 1 and out.count("\n") == 1 and said in out, (flags, out)
    rc, out = _east(["texts", "passages"])
    assert rc == 1 and "texts passages" in out
    rc, out = _east(["texts", "passage", t])
    assert rc == 1 and out.count("\n") == 1 and out.rstrip().endswith("'overlap', 'passages'.")
    monkeypatch.setenv("EAST_HIP_FORCE_DIST", "1")
    rc, out = _east(["texts", "passages", t])
    assert rc == 1 and out.count("\n") == 1 and "collective path" in out
    monkeypatch.delenv("EAST_HIP_FORCE_DIST")
    monkeypatch.setenv("WORLD_SIZE", "2")
    rc, out = _east(["texts", "passages", t])
    assert rc == 1 and out.count("\n") == 1 and "WORLD_SIZE=2" in out
    monkeypatch.setenv("RANK", "1")                                # (only rank 0 says it)
    assert _east(["-x", "0", "texts", "passages", t]) == (1, "")
    assert touched == []
    assert "texts passages" in main.__doc__


# ---- the binding against the header -------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        src = f.read()
    assert "Shared passages" in src
    names = ["east_hip_passages_build", "east_hip_passages_fetch", "east_hip_passages_phases", "east_hip_last_passages_ms",
             "east_hip_debug_set_passages_route"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp,
                "int32_t *": hip_backend._c_i32p, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
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
    assert len(hip_backend.PASSAGES_INFO_FIELDS) == 12
    assert set(hip_backend.PassageArrays.__slots__) >= {"pair_off", "starts", "covered", "found", "start", "words", "at", "text_start"}
    with open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "handle.h")) as f:
        enum = f.read()
    assert "SLOT_CLU, SLOT_PHR, N_CONSUMERS = SLOT_PHR + 4" in enum and "SLOT_OVL = SLOT_PHR + 2" in enum
    assert "SLOT_PAS = SLOT_PHR + 3" in enum
    with open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "east_hip.hip")) as f:
        assert '#include "passages.h"' in f.read()
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        assert "texts passages" in f.read()
