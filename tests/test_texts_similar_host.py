"""CPU tier: text-to-text cosine similarity (applications.texts_similar) on the host path, the command line's refusals and
the binding of the new entry points -- no device.  The yardstick is tests/texts_cosine_exact.py: the contract of
include/east_hip.h ("Text-to-text cosine similarity") at 50 digits for the values, the ranking's contract
(applications._top_select) for the selection, applied to the matrix the host path itself reported (its full lists).  Values
are compared to the bound (t_ab + ceil(p_a / 64) + ceil(p_b / 64) + 176) * 2^-52 * exact, names and order with ==."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import cosine_exact
import texts_cosine_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _sizes():
    from east import hip_backend
    return hip_backend.COSINE_TEXTS_CHUNK, hip_backend.COSINE_TEXTS_SEG


def _names():
    return sorted(model.collections(*_sizes()))


@pytest.mark.parametrize("tfidf", (False, True), ids=("tf", "tf-idf"))
def test_model_against_plain_doubles(tfidf):
    """The margin argument of DESIGN.md 9: plain doubles, the dot products in ascending unit order, stay within a tenth of the
    bound on every collection of the gpu tier -- a correct double-precision kernel then has a factor of 10 to spare."""
    chunk, seg = _sizes()
    assert chunk == 32 and seg % chunk == 0
    for name in _names():
        stems = model.collections(chunk, seg)[name][2]
        C, own = model.plain_doubles(model.model_of(name, chunk, seg), tfidf, stems)
        model.check(C, own, None, model.exact_of(name, chunk, seg, tfidf), tenth=True)


def test_collections_have_the_shapes_they_promise():
    chunk, seg = _sizes()
    for U in model.unit_edge_sizes(chunk, seg):
        m = model.model_of("units %d" % U, chunk, seg)
        assert len(m.terms) == U and m.n_docs == 65 and m.terms[0] == model.word(0) and m.terms[-1] == model.word(U - 1)
        ex = model.exact_of("units %d" % U, chunk, seg, True)
        assert ex.p[0] == U and ex.p[1] == 2 and ex.t[2, 3] == 1 and (U - 1) in m.counts[2] and (U - 1) in m.counts[3]
        if U > seg:
            assert list(m.counts[1]) == [seg - 1, seg]
    ex = model.exact_of("document shapes", chunk, seg, True)
    assert ex.p.tolist()[:3] == [0, 0, 1] and ex.p[9] == 0 and ex.t[5, 6] == 0 and ex.C[5, 6] == 0.0
    assert abs(ex.C[3, 4] - 1.0) <= model.ULP
    ex = model.exact_of("cursor skew", chunk, seg, False)
    assert ex.p[0] == 200 and (ex.p[1:] == 1).all() and ex.p.size == 65
    assert model.exact_of("long text", chunk, seg, False).p[0] == 20000
    m = model.model_of("stems", chunk, seg)
    assert m.n_classes < len(m.terms)


def _measure(space="words", weighting="tf-idf", stopwords=model.STOPWORDS):
    from east import relevance
    return relevance.CosineRelevanceMeasure(space, weighting, stopwords=stopwords, stemmer=cosine_exact.ToyStemmer())


def _matrix_of(full, names):
    where = {name: i for i, name in enumerate(names)}
    H = np.full((len(names), len(names)), NAN)
    for member, entries in full.items():
        for other, value in entries:
            H[where[member], where[other]] = value
    return H


def _named(lists, names):
    return {names[s]: [(names[i], v) for i, v in entries] for s, entries in enumerate(lists)}


def _same(got, want):
    assert got == want
    flat = lambda r: [repr(v) for entries in r.values() for _, v in entries]
    assert flat(got) == flat(want)
    assert all(type(m) is str and type(v) is float for entries in got.values() for m, v in entries)


def _no_device(monkeypatch):
    from east import hip_backend
    monkeypatch.setattr(hip_backend, "load", lambda: pytest.fail("the host path touched the device library"))
    monkeypatch.setattr(hip_backend.HipCosineIndex, "__init__", lambda *a, **k: pytest.fail("the host path made an index"))


@pytest.mark.parametrize("space", ("words", "stems"))
@pytest.mark.parametrize("weighting", ("tf", "tf-idf"))
def test_host_path_is_the_contract(monkeypatch, space, weighting):
    from east import applications
    monkeypatch.setenv("EAST_HIP_TEXTS_SIMILAR", "host")
    _no_device(monkeypatch)
    chunk, seg = _sizes()
    stems, tfidf = space == "stems", weighting == "tf-idf"
    for name in ("stems", "document shapes", "units %d" % (chunk + 1)):
        raw = model.collections(chunk, seg)[name][0]
        texts = {"t%03d" % i: t.encode() for i, t in enumerate(raw)}
        names, D = list(texts), len(raw)
        m = cosine_exact.build_model(list(raw), model.STOPWORDS, cosine_exact.ToyStemmer())
        ex = model.exact(m, tfidf, stems)
        full = applications.texts_similar(texts, 1024, None, _measure(space, weighting))
        assert list(full) == names and all(member not in [o for o, _ in entries] for member, entries in full.items())
        assert all(len(entries) == D - 1 for entries in full.values())           # (a text without a term is still a column)
        H = _matrix_of(full, names)
        matrix, own, postings = applications._texts_similar_on_host(texts, _measure(space, weighting), "english")
        assert np.array_equal(np.isnan(H), np.isnan(matrix)) and H[~np.isnan(H)].tobytes() == matrix[~np.isnan(matrix)].tobytes()
        model.check(matrix, own, postings, ex)
        if name != "document shapes":
            continue
        assert all(repr(v) == "0.0" for _, v in full["t000"]) and all(repr(v) == "0.0" for _, v in full["t001"])
        # two identical texts: a tie for everybody else, in the order of `texts`
        for member, entries in full.items():
            order = [o for o, _ in entries]
            if member not in ("t003", "t004"):
                assert H[names.index(member), 3] == H[names.index(member), 4]
                assert order.index("t003") + 1 == order.index("t004")
        finite = H[np.isfinite(H) & (H > 0.0)]
        present = float(np.sort(finite)[finite.size // 2])
        for n in (1, 2, D - 1, D + 3, 1024):                                      # (n above D - 1: the lists are shorter)
            for threshold in (None, -INF, present, np.nextafter(present, 2.0), np.nextafter(present, -2.0), 0.0, 2.0):
                got = applications.texts_similar(texts, n, threshold, _measure(space, weighting))
                _same(got, _named(applications._top_select(H, 1, n, -INF if threshold is None else threshold), names))
                assert all(len(entries) <= min(n, D - 1) for entries in got.values())
                if threshold == 2.0:
                    assert all(entries == [] for entries in got.values()) and len(got) == D


def test_column_blocks_of_the_host_path_do_not_show(monkeypatch):
    """The term axis goes through dense arrays of a fixed number of columns: a block of 7 units cuts every text, the values
    stay inside the bound."""
    from east import applications
    chunk, seg = _sizes()
    raw = model.collections(chunk, seg)["units %d" % (chunk + 1)][0]
    texts = {str(i): t for i, t in enumerate(raw)}
    ex = model.exact_of("units %d" % (chunk + 1), chunk, seg, True)
    monkeypatch.setattr(applications, "_TEXTS_SIMILAR_HOST_BLOCK", 7)
    model.check(*applications._texts_similar_on_host(texts, _measure(stopwords=()), "english"), ex)


class _RepeatedTitles(object):
    """A text collection whose titles repeat (a list of pairs behind the mapping's methods the applications use)."""

    def __init__(self, pairs):
        self.pairs = pairs

    def keys(self):
        return [k for k, _ in self.pairs]

    def values(self):
        return [v for _, v in self.pairs]


def test_small_collections_bad_arguments_and_where_the_host_path_is_taken(monkeypatch):
    from east import applications, hip_backend, parallel, relevance
    monkeypatch.delenv("EAST_HIP_TEXTS_SIMILAR", raising=False)
    assert relevance.ASTRelevanceMeasure.relevance_texts_similar is None
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_texts_similar is None
    assert getattr(parallel.DistributedASTRelevanceMeasure, "relevance_texts_similar", None) is None
    assert callable(relevance.CosineRelevanceMeasure.relevance_texts_similar)
    assert callable(relevance.CosineRelevanceMeasure.text_similarity_matrix)

    class Refusing(relevance.CosineRelevanceMeasure):
        def set_text_collection(self, texts, language=None):
            raise AssertionError("the device path must not be taken")

    refusing = Refusing("words", "tf", stopwords=())
    assert applications.texts_similar({}, 5, None, refusing) == {}
    texts = {"x": b"alpha beta gamma", "y": b"beta gamma delta delta", "z": b"epsilon"}
    with pytest.raises(AssertionError):
        applications.texts_similar(texts, 2, None, refusing)
    monkeypatch.setenv("EAST_HIP_TEXTS_SIMILAR", "host")
    _no_device(monkeypatch)
    assert applications.texts_similar({"only": b"one single text here"}, 5, None, refusing) == {"only": []}
    got = applications.texts_similar(texts, 2, None, refusing)
    assert [o for o, _ in got["x"]] == ["y", "z"] and got["x"][1][1] == 0.0 and got["z"] == [("x", 0.0), ("y", 0.0)]
    assert abs(got["x"][0][1] - 2.0 / (3.0 ** 0.5 * 6.0 ** 0.5)) < 1e-15 and got["x"][0][1] == got["y"][0][1]
    monkeypatch.delenv("EAST_HIP_TEXTS_SIMILAR")
    # repeated titles: the host path over all three texts; a repeated title keeps its last list, as a dict does
    repeated = _RepeatedTitles([("x", texts["x"]), ("y", texts["y"]), ("x", texts["z"])])
    got = applications.texts_similar(repeated, 2, None, refusing)
    assert list(got) == ["x", "y"] and got["x"] == [("x", 0.0), ("y", 0.0)] and [o for o, _ in got["y"]] == ["x", "x"]
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            applications.texts_similar(texts, bad, None, refusing)
    with pytest.raises(ValueError):
        applications.texts_similar(texts, 3, NAN, refusing)
    # a measure that is no cosine measure: ValueError, naming texts_related
    ast = relevance.ASTRelevanceMeasure.__new__(relevance.ASTRelevanceMeasure)
    with pytest.raises(ValueError, match="texts_related"):
        applications.texts_similar(texts, 3, None, ast)

    seen = {}

    class Device(relevance.CosineRelevanceMeasure):
        def set_text_collection(self, texts, language=None):
            seen["texts"] = list(texts)

        def relevance_texts_similar(self, n, threshold):
            seen["call"] = (n, threshold)
            return hip_backend.TopArrays(np.array([2, 0, 1], dtype=np.int32), np.array([[1, 2], [-1, -1], [0, -1]], dtype=np.int32),
                                         np.array([[0.75, 0.0], [0.0, 0.0], [0.5, 0.0]]))

    got = applications.texts_similar(texts, 2, None, Device("words", "tf", stopwords=()))
    assert seen["call"] == (2, -INF) and seen["texts"] == list(texts.values())
    _same(got, {"x": [("y", 0.75), ("z", 0.0)], "y": [], "z": [("x", 0.5)]})


def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch):
    """A bad -n or -r, -s ast, -v lemmata, -y, -o, -g N > 1, EAST_HIP_DEVICES > 1, a launcher, the forced collective path: one
    line and exit code 1, before a file is read or a measure is made."""
    from east import main, relevance
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    touched = []
    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr(main, "launch_ranks", lambda *a: touched.append("ranks") or 0)
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    tail = ["texts", "similar", str(tmp_path)]
    for bad, word in ((["-n", "0"], "0"), (["-n", "1025"], "1025"), (["-n", "2.5"], "2.5"), (["-r", "nan"], "nan"),
                      (["-r", "high"], "high"), (["-s", "ast"], "texts related"), (["-s", "AST"], "texts related"),
                      (["-s", "jaccard"], "jaccard"), (["-v", "lemmata"], "lemmata"), (["-y"], "-y"),
                      (["-y", "-t", "triples.txt"], "-y"), (["-o", "directed"], "-o directed"), (["-g", "4"], "-g 4"),
                      (["-g", "x"], "'x'")):
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
    rc, out = _east(["texts", "alike", str(tmp_path)])
    assert rc == 1 and "'related'" in out and "'similar'" in out
    rc, out = _east(["texts", "similar"])
    assert rc == 1 and "texts similar" in out
    assert touched == []
    monkeypatch.undo()
    assert "texts similar" in main.__doc__ and "texts related" in main.__doc__


def test_cli_prints_the_result_and_says_what_is_missing(tmp_path, monkeypatch, capsys):
    """The options reach texts_similar and its result is printed through format_similar; a missing stemmer is one line."""
    from east import applications, exceptions, formatting, main, relevance
    for name in ("WORLD_SIZE", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    made = []

    def init(self, *a, **k):
        made.append(a)
        self.stopwords_source = "none"

    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", init)
    (tmp_path / "t.txt").write_bytes(b"one\ntwo\n")
    seen = []
    result = {"0": [("1", 0.5)], "1": [("0", 0.5)]}

    def fake(texts, n, threshold, measure, language):
        seen.append((dict(texts), n, threshold, type(measure).__name__, language))
        return result

    monkeypatch.setattr(applications, "texts_similar", fake)
    tail = ["texts", "similar", str(tmp_path / "t.txt")]
    rc = main.main(tail)
    printed = capsys.readouterr()
    assert rc == 0 and printed.out == formatting.format_similar(result, "text", "xml") + "\n"
    assert "no stopwords are removed" in printed.err                          # (said on stderr, as _run_cosine says it)
    assert seen[-1] == ({"0": b"one", "1": b"two"}, 10, None, "CosineRelevanceMeasure", "english")
    assert made[-1] == ("stems", "tf-idf")
    rc = main.main(["-n", "3", "-r", "0.2", "-w", "tf", "-v", "words", "-s", "cosine", "-f", "csv", "-g", "1", "-l", "german"] + tail)
    assert rc == 0 and capsys.readouterr().out == formatting.format_similar(result, "text", "csv") + "\n"
    assert seen[-1][1:3] == (3, 0.2) and seen[-1][4] == "german" and made[-1] == ("words", "tf")
    rc, out = _east(["-f", "gml"] + tail)
    assert rc == 1 and out.count("\n") == 1

    def no_stemmer(self, *a, **k):
        raise exceptions.StemmerUnavailableException()

    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", no_stemmer)
    rc, out = _east(tail)
    assert rc == 1 and out.count("\n") == 1 and out.strip() == str(exceptions.StemmerUnavailableException())


def test_binding_against_the_header():
    """Every entry point of the text-to-text cosine is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Text-to-text cosine similarity" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS\s+5\b", src)
    assert hip_backend.GRAPH_SOURCE_COSINE_TEXTS == 5
    names = ["east_hip_text_similarity_build", "east_hip_text_similarity_fetch", "east_hip_last_text_similarity_ms",
             "east_hip_debug_set_text_similarity_batch"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp,
                "int32_t *": hip_backend._c_i32p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int}
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
    if not os.path.exists(hip_backend.LIB_PATH):      # a fresh checkout: hipcc cross-compiles without a GPU
        import __graft_entry__
        __graft_entry__.build()
    lib = hip_backend.load()
    for name in names:
        assert hasattr(lib, name), name
    invalid = -1 * abs(int(re.search(r"#define\s+EAST_HIP_ERR_INVALID\s+\(?(-?\d+)\)?", src).group(1)))
    assert lib.east_hip_last_text_similarity_ms(None) == -1.0
    assert lib.east_hip_text_similarity_fetch(None, None, None, None) == invalid
    assert lib.east_hip_text_similarity_build(None, 1, None) == invalid
    assert lib.east_hip_text_similarity_build(None, 7, None) == invalid
    assert lib.east_hip_debug_set_text_similarity_batch(1) == 0 and lib.east_hip_debug_set_text_similarity_batch(0) == 0
    for method in ("texts_build", "texts_matrix", "rank_texts", "texts_similar", "last_texts_ms"):
        assert callable(getattr(hip_backend.HipCosineIndex, method)), method
    src_kernel = open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "cosine_texts.h")).read()
    assert re.search(r"#define\s+COSTEXT_SEG\s+%du\b" % hip_backend.COSINE_TEXTS_SEG, src_kernel)
    assert hip_backend.COSINE_TEXTS_CHUNK == int(re.search(r"#define\s+SIM_CHUNK\s+(\d+)u", open(os.path.join(
        ROOT, "ast-text-analysis_amd", "csrc", "similarity.h")).read()).group(1))
