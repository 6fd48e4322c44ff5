# -*- coding: utf-8 -*-
"""CPU tier: phrase extraction (applications.keyphrases_extract) on the host path, the command line and the binding of the
new entry points -- no device.  The yardstick is tests/phrases_exact.py, the contract of include/east_hip.h ("Phrase
extraction") as a dict of word tuples; hand-written expectations pin that model first.  Everything is integers and text:
every comparison is ==."""
import ctypes
import io
import os
import re
from contextlib import redirect_stdout

import pytest

import cosine_exact
import phrases_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND_WRITTEN = [
    # (texts, stopwords, parameters, [(text, words, count, texts, first)])
    (model.HEADER_EXAMPLE, (), {}, model.HEADER_EXPECTED),
    # the period-1 text: overlapping occurrences all count, and every length has a count of its own
    (model.one_word(5), (), {}, [("AAA AAA AAA", 3, 3, 1, 0), ("AAA AAA", 2, 4, 1, 0), ("AAA", 1, 5, 1, 0)]),
    # EDGE NEXT lies across two text boundaries, twice: it is no phrase, so NEXT stays closed
    (["left middle edge", "next left middle edge", "next other"], (), {},
     [("LEFT MIDDLE EDGE", 3, 2, 2, 0), ("NEXT", 1, 2, 2, 3)]),
    # stopwords are breaks and count as positions: QUICK at 10 is followed by one
    (["the quick fox and quick fox the the quick fox", "quick the fox quick fox and"], ("the", "and"), {},
     [("QUICK FOX", 2, 4, 2, 1), ("QUICK", 1, 5, 2, 1), ("FOX", 1, 5, 2, 2)]),
]


@pytest.mark.parametrize("case", range(len(HAND_WRITTEN)))
def test_hand_written_expectations_pin_the_model(case):
    texts, stop, params, want = HAND_WRITTEN[case]
    got = model.PhraseModel(texts, stop).extract(**params)
    assert got.tuples() == want
    assert got.candidates == len(want)


def test_the_model_on_the_parameters():
    m = model.PhraseModel(model.HEADER_EXAMPLE)
    assert [t[0] for t in m.extract(max_words=1).tuples()] == ["ABC", "BCD", "CDE"]            # (n = max_words is closed)
    assert m.extract(max_words=1).count.tolist() == [4, 4, 3]
    assert [t[0] for t in m.extract(min_count=4).tuples()] == ["ABC BCD"]
    assert m.extract(min_count=4).levels == 3 and m.extract(min_count=5).levels == 1
    assert m.extract(min_count=4).domain.tolist()[:3] == [11, 7, 3] and m.extract(min_count=4).survivors.tolist()[:3] == [2, 1, 0]
    assert m.extract(n=2).strings == ["ABC BCD CDE", "BCD CDE ABC"] and m.extract(n=2).candidates == 4
    assert m.extract(min_texts=2).strings == [] and m.extract(min_words=3).strings == ["ABC BCD CDE", "BCD CDE ABC", "CDE ABC BCD"]
    e = m.extract()
    assert e.term_ids.tolist() == [0, 1, 2, 1, 2, 0, 2, 0, 1, 0, 1] and e.text_off.tolist() == [0, 11, 22, 33, 40]
    assert e.first_text.tolist() == [0, 0, 0, 0] and e.levels == 3


def _host(texts, stop=(), **params):
    from east import applications
    args = dict(n=0, max_words=3, min_words=1, min_count=2, min_texts=1)
    args.update(params)
    return applications._phrases_on_host(list(texts), cosine_exact.prepared_stopwords(stop), **args)


def _same_as_model(texts, stop, m, what, **params):
    rows, candidates = _host(texts, stop, **params)
    want = m.extract(**params)
    assert [r[:5] for r in rows] == want.tuples(), what
    assert [r[5] for r in rows] == want.first_text.tolist(), what
    assert [i for r in rows for i in r[6]] == want.term_ids.tolist(), what
    assert candidates == want.candidates, what


def test_host_path_is_the_model_on_the_small_collections():
    cases = {"header": (model.HEADER_EXAMPLE, ()), "period 2": (model.two_word_period(), ())}
    cases.update(("repeat %d" % k, (model.one_word(k), ())) for k in model.REPEATS)
    cases.update(model.boundary_collections())
    cases.update(model.break_collections())
    cases["ties"] = model.ties_collection()
    for name, (texts, stop) in cases.items():
        m = model.PhraseModel(texts, stop)
        for params in ({}, {"max_words": 8, "min_count": 1}, {"max_words": 2, "min_texts": 2}, {"min_words": 2, "n": 3}):
            _same_as_model(texts, stop, m, (name, params), **params)
    for it, rnd in enumerate(cosine_exact.fuzz_rounds()):
        m = model.PhraseModel(rnd["texts"], rnd["stopwords"], longest=5)
        _same_as_model(rnd["texts"], rnd["stopwords"], m, ("fuzz", it), max_words=4, min_count=1 + it % 2)


def test_host_path_is_the_model_on_the_parameter_sweep():
    texts, stop = model.zipf_collection()
    m = model.PhraseModel(texts, stop)
    assert 19000 <= m.kept_tokens <= 21000 and len(texts) == 16
    for max_words in (1, 3, 8):
        for min_count in (1, 2, 50):
            _same_as_model(texts, stop, m, (max_words, min_count), max_words=max_words, min_count=min_count)
    C = m.extract().candidates
    for n in (1, 5, C - 1, C, C + 1):
        _same_as_model(texts, stop, m, n, n=n)
    for min_words, min_texts in ((2, 2), (3, 16)):
        _same_as_model(texts, stop, m, (min_words, min_texts), min_words=min_words, min_texts=min_texts)
    assert m.extract(min_count=50, max_words=8).levels < 8                                   # (the early end)
    texts, stop = model.wide_collection()
    _same_as_model(texts, stop, model.PhraseModel(texts, stop, longest=3), "wide", max_words=2)


def test_ties_collection_has_what_it_promises():
    texts, stop = model.ties_collection()
    e = model.PhraseModel(texts, stop).extract()
    six = [t for t in e.tuples() if t[1] * t[2] == 6]
    assert len(six) == 36 and {t[1] for t in six} == {1, 2, 3}
    assert [(t[1], t[4]) for t in six] == sorted((t[1], t[4]) for t in six)                  # (words, then first)


# ---- keyphrases_extract and the command line ---------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from east import hip_backend
    monkeypatch.setattr(hip_backend, "load", lambda: pytest.fail("the host path touched the device library"))
    monkeypatch.setattr(hip_backend.HipCosineIndex, "__init__", lambda *a, **k: pytest.fail("the host path made an index"))


def test_keyphrases_extract_on_the_host(monkeypatch):
    from east import applications, relevance
    monkeypatch.setenv("EAST_HIP_EXTRACT", "host")
    _no_device(monkeypatch)
    measure = relevance.CosineRelevanceMeasure("words", stopwords=())
    got = applications.keyphrases_extract({"a": model.HEADER_EXAMPLE[0]}, similarity_measure=measure)
    assert got == [applications.Phrase(t, w, c, x, c * w) for t, w, c, x, _ in model.HEADER_EXPECTED]
    assert all(type(v) is int for p in got for v in p[1:]) and all(type(p.text) is str for p in got)
    assert applications.keyphrases_extract(model.HEADER_EXAMPLE, n=1, similarity_measure=measure) == got[:1]
    assert applications.keyphrases_extract([b"abc abc", "abc"], min_texts=2, similarity_measure=measure) == [
        applications.Phrase("ABC", 1, 3, 2, 3)]
    stopping = relevance.CosineRelevanceMeasure("words", stopwords=("bcd",))
    assert [p.text for p in applications.keyphrases_extract(model.HEADER_EXAMPLE, similarity_measure=stopping)] == ["CDE ABC", "ABC"]       # (ABC | CDE ABC | CDE ABC | CDE ABC |)
    for bad in (dict(n=-1), dict(max_words=0), dict(max_words=9), dict(min_words=0), dict(min_words=4), dict(min_count=0),
                dict(min_texts=0), dict(n=1.5)):
        with pytest.raises(ValueError) as e:
            applications.keyphrases_extract(model.HEADER_EXAMPLE, similarity_measure=measure, **bad)
        assert list(bad)[0] in str(e.value)
    with pytest.raises(ValueError):
        applications.keyphrases_extract(model.HEADER_EXAMPLE, similarity_measure=relevance.CosineRelevanceMeasure(
            "stems", stopwords=(), stemmer=cosine_exact.ToyStemmer()))
    with pytest.raises(ValueError):
        applications.keyphrases_extract(model.HEADER_EXAMPLE, similarity_measure=object())


def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def _clean(monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)


def test_cli_formats_and_the_keyphrase_file(tmp_path, monkeypatch):
    from east import applications, formatting, relevance
    _clean(monkeypatch)
    monkeypatch.setenv("EAST_HIP_EXTRACT", "host")
    _no_device(monkeypatch)
    monkeypatch.setattr(relevance, "default_stopwords", lambda: frozenset(["THE"]))
    (tmp_path / "a.txt").write_bytes(b"the quick fox, the quick fox; slow \"dog\"")
    (tmp_path / "b.txt").write_bytes(b"slow dog the quick fox")
    (tmp_path / "c.md").write_bytes(b"quick fox quick fox quick fox")
    tail = ["keyphrases", "extract", str(tmp_path)]
    want = [applications.Phrase("QUICK FOX", 2, 3, 2, 6), applications.Phrase("SLOW DOG", 2, 2, 2, 4)]
    rc, out = _east(tail)
    assert (rc, out) == (0, "QUICK FOX\nSLOW DOG\n")
    assert out == formatting.format_phrases(want, "txt") == formatting.format_phrases(want)
    # the txt output is a keyphrase file: read as `keyphrases table` reads one, it gives the same phrases
    (tmp_path / "kp.txt").write_text(out)
    from east import main
    assert main._read(str(tmp_path / "kp.txt")).decode("utf-8", errors="replace").splitlines() == [p.text for p in want]
    (tmp_path / "kp.txt").unlink()
    rc, out = _east(["-f", "csv"] + tail)
    assert (rc, out) == (0, '"QUICK FOX",2,3,2,6\n"SLOW DOG",2,2,2,4\n')
    rc, out = _east(["-f", "xml"] + tail)
    assert rc == 0 and out == ('<phrases count="2">\n  <phrase rank="1" words="2" count="3" texts="2" score="6">QUICK FOX</phrase>\n'
                               '  <phrase rank="2" words="2" count="2" texts="2" score="4">SLOW DOG</phrase>\n</phrases>\n')
    assert _east(["-n", "1"] + tail) == (0, "QUICK FOX\n")
    assert _east(["-x", "1", "-m", "3", "-v", "words", "-g", "1", "-l", "german"] + tail) == (0, "QUICK\nFOX\n")
    assert _east(["-u", "3"] + tail) == (0, "")
    assert _east(["-n", "0", "-m", "1", "-x", "8"] + tail)[1].splitlines()[0] == "QUICK FOX"
    with pytest.raises(Exception):
        formatting.format_phrases(want, "gml")


def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch):
    from east import main, relevance
    _clean(monkeypatch)
    touched = []
    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr(main, "launch_ranks", lambda *a: touched.append("ranks") or 0)
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    tail = ["keyphrases", "extract", str(tmp_path)]
    for bad, word in ((["-s", "cosine"], "-s cosine"), (["-s", "ast"], "-s ast"), (["-w", "tf"], "-w tf"), (["-v", "stems"], "-v stems"),
                      (["-v", "lemmata"], "-v lemmata"), (["-y"], "-y"), (["-y", "-t", "triples.txt"], "-y"), (["-o", "directed"], "-o directed"),
                      (["-b", "text"], "-b text"), (["-r", "0.5"], "-r 0.5"), (["-k", "3"], "-k 3"), (["-c", "0.6"], "-c 0.6"),
                      (["-p", "1"], "-p 1"), (["-g", "4"], "-g 4"), (["-g", "x"], "'x'"), (["-n", "-1"], "'-1'"), (["-n", "many"], "'many'"),
                      (["-x", "0"], "'0'"), (["-x", "9"], "'9'"), (["-x", "2.5"], "'2.5'"), (["-m", "0"], "'0'"), (["-m", "x"], "'x'"),
                      (["-u", "0"], "'0'"), (["-u", ""], "''"), (["-f", "gml"], "'gml'")):
        rc, out = _east(bad + tail)
        assert rc == 1 and out.count("\n") == 1 and word in out, (bad, out)
    monkeypatch.setenv("EAST_HIP_DEVICES", "2")
    rc, out = _east(tail)
    assert rc == 1 and out.count("\n") == 1 and "-g 2" in out
    monkeypatch.delenv("EAST_HIP_DEVICES")
    monkeypatch.setenv("WORLD_SIZE", "2")
    rc, out = _east(tail)
    assert rc == 1 and out.count("\n") == 1 and "WORLD_SIZE=2" in out
    monkeypatch.setenv("RANK", "1")                                           # (only rank 0 says it)
    assert _east(tail) == (1, "")
    monkeypatch.delenv("RANK")
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("EAST_HIP_FORCE_DIST", "1")
    rc, out = _east(tail)
    assert rc == 1 and out.count("\n") == 1 and "collective" in out
    monkeypatch.delenv("EAST_HIP_FORCE_DIST")
    rc, out = _east(["keyphrases", "extract"])                                # (dispatched before the four-argument check)
    assert rc == 1 and "keyphrases extract" in out
    assert touched == []
    monkeypatch.undo()
    assert "keyphrases extract" in main.__doc__ and all(c + ":" in main._OPTIONS for c in "xmu")
    rc, out = _east(["keyphrases"])
    assert rc == 1 and "extract" in out
    import inspect
    assert "'clusters', 'extract'." in inspect.getsource(main._run)         # (the line an unknown subcommand ends with)


# ---- the binding ---------------------------------------------------------------------------------------------------------------
NAMES = ["east_hip_phrases_build", "east_hip_phrases_fetch", "east_hip_phrases_levels", "east_hip_last_phrases_ms"]


def test_binding_against_the_header():
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Phrase extraction" in text and "abc bcd cde abc bcd cde abc bcd cde abc bcd" in text
    for line in ("ABC BCD CDE  (3 words, count 3, score 9, first 0)", "BCD CDE ABC  (3 words, count 3, score 9, first 1)",
                 "CDE ABC BCD  (3 words, count 3, score 9, first 2)", "ABC BCD      (2 words, count 4, score 8, first 0)"):
        assert line in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "uint32_t *": hip_backend._c_u32p,
                "int32_t *": hip_backend._c_i32p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in NAMES:
        m = re.search(r"\b(int|double)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = hip_backend.SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "double": ctypes.c_double}[m.group(1)]
        declared = [ctype_of[re.match(r"^(.*?)\w+$", " ".join(a.split())).group(1).strip()] for a in m.group(2).split(",")]
        assert declared == list(args), name
    for owner in (hip_backend.HipIndex, hip_backend.HipCosineIndex):
        assert callable(owner.phrases)
    assert not re.search(r"#define\s+EAST_HIP_GRAPH_SOURCE_\w+\s+[67]\b", src)      # (no new table source)
    handle = open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "handle.h")).read()
    assert re.search(r"SLOT_CLU,\s*SLOT_PHR,\s*N_CONSUMERS", handle)
    kernel = open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "phrases.h")).read()
    assert re.search(r"#define\s+PHR_MAX_WORDS\s+%d\b" % hip_backend.PHRASES_MAX_WORDS, kernel)
    assert "atomic" not in re.sub(r"//.*", "", kernel)


def test_null_handle_calls_are_invalid():
    from east import hip_backend
    if not os.path.exists(hip_backend.LIB_PATH):      # a fresh checkout: hipcc cross-compiles without a GPU
        import __graft_entry__
        __graft_entry__.build()
    lib = hip_backend.load()
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        invalid = -1 * abs(int(re.search(r"#define\s+EAST_HIP_ERR_INVALID\s+\(?(-?\d+)\)?", f.read()).group(1)))
    out = (ctypes.c_int64 * 8)()
    assert lib.east_hip_phrases_build(None, 1, 3, 2, 1, 0, out) == invalid
    assert lib.east_hip_phrases_fetch(None, None, None, None, None, None, None, None, None) == invalid
    assert lib.east_hip_phrases_levels(None, out, out) == invalid
    assert lib.east_hip_last_phrases_ms(None) == -1.0
