"""CPU tier: text-to-text relatedness (applications.texts_related) on the host path, format_related, the command line's
refusals and the binding of the new entry points -- no device.  The yardstick is tests/related_exact.py: the contract of
include/east_hip.h ("Text-to-text relatedness") in exact arithmetic for the values, the ranking's contract
(applications._top_select) for the selection, applied to the matrix the host path itself reported (its full lists).  Values
are compared to the bound (max(c_A, c_B) + 4) * 2^-53 * exact, names and order with ==."""
import io
import os
import random
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import related_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
ORIENTATIONS = (("directed", model.DIRECTED), ("symmetric", model.SYMMETRIC))


def stub_score(s, d):
    """A seeded score of the string s against document d: a double of [0, 1) with a full mantissa."""
    return random.Random("%s|%d" % (s, d)).random()


class _StubMeasure(object):
    """A batched measure without `relevance_related` (the host path): relevance_table returns the seeded table of the strings
    it is asked for, and remembers them."""

    def __init__(self):
        self.asked = []
        self.D = 0

    def set_text_collection(self, texts, language=None):
        self.D = len(list(texts))

    def relevance_table(self, prepared, synonimizer=None):
        assert prepared and all(s.replace(" ", "") for s in prepared)       # (an empty keyphrase divides by zero)
        self.asked.extend(prepared)
        return np.array([[stub_score(s, d) for d in range(self.D)] for s in prepared], dtype=np.float64).reshape(len(prepared), self.D)


class _RefusingMeasure(_StubMeasure):
    def relevance_related(self, *args):
        raise AssertionError("the device path must not be taken")


WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda omicron sigma upsilon omega "
         "wording found tree annotated suffix relatedness texts strings device").split()


def _prose(seed, n_words):
    rng = random.Random(seed)
    return " ".join(rng.choice(WORDS) for _ in range(n_words)).encode()


def _texts():
    return {"long": _prose(1, 40), "none": b"a 12 to 7 it", "short": b"wording found here", "twin": _prose(1, 40),
            "mid": _prose(2, 17), "other": _prose(3, 23)}


def _collections(texts):
    from east import utils
    return [utils.text_to_strings_collection(t) for t in texts.values()]


def _matrix_of(full, names):
    """The matrix the path under test ranked, from its full lists (n = 1024, no threshold): NaN where a pair is not listed."""
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


@pytest.mark.parametrize("orientation,code", ORIENTATIONS)
def test_host_path_is_the_contract(monkeypatch, orientation, code):
    from east import applications
    monkeypatch.delenv("EAST_HIP_RELATED", raising=False)
    texts = _texts()
    names = list(texts)
    D = len(names)
    collections = _collections(texts)
    assert collections[names.index("none")] == [" "]
    want = model.exact(collections, stub_score, code)
    assert want.scored[names.index("none")] == 0 and want.scored[names.index("short")] == 1
    measure = _StubMeasure()
    full = applications.texts_related(texts, 1024, orientation, None, measure)
    assert " " not in measure.asked and len(measure.asked) == int(want.scored.sum())
    assert list(full) == names and all(member not in [o for o, _ in entries] for member, entries in full.items())
    assert all(len(entries) == D - 1 for entries in full.values())          # (a text without a string is still a column)
    H = _matrix_of(full, names)
    own = np.array([float(want.f[a]) for a in range(D)])                     # (self is not part of the lists)
    model.check(H, own, want.scored, want)
    none = names.index("none")
    if code == model.DIRECTED:
        assert all(repr(v) == "0.0" for _, v in full["none"])                # the row of +0.0: no division by zero
        assert any(H[a, none] > 0.0 for a in range(D) if a != none)
    else:
        assert H.tobytes() == H.T.copy().tobytes()
        assert all(H[none, b] == H[b, none] and H[none, b] > 0.0 for b in range(D) if b != none)
    if code == model.DIRECTED:                                               # equal texts: equal rows (the stub's columns differ)
        a, b = names.index("long"), names.index("twin")
        others = [i for i in range(D) if i not in (a, b)]
        assert np.array_equal(H[a, others], H[b, others])
    finite = H[np.isfinite(H)]
    present = float(np.sort(finite)[finite.size // 2])
    for n in (1, 2, D - 1, D + 3, 1024):                                      # (n above D - 1: the lists are shorter)
        for threshold in (None, -INF, present, np.nextafter(present, 2.0), np.nextafter(present, -2.0), 0.0, 2.0):
            got = applications.texts_related(texts, n, orientation, threshold, _StubMeasure())
            _same(got, _named(applications._top_select(H, 1, n, -INF if threshold is None else threshold), names))
            assert all(len(entries) <= min(n, D - 1) for entries in got.values())
            if threshold == 2.0:
                assert all(entries == [] for entries in got.values()) and len(got) == D


def test_chunks_of_the_host_path_do_not_show(monkeypatch):
    """The strings go through relevance_table a chunk at a time: a chunk of 5 strings cuts every text, the values stay inside
    the bound and every string is asked for once."""
    from east import applications
    texts = _texts()
    want = model.exact(_collections(texts), stub_score, model.SYMMETRIC)
    monkeypatch.setattr(applications, "_RELATED_HOST_CHUNK", 5)
    measure = _StubMeasure()
    full = applications.texts_related(texts, 1024, "symmetric", None, measure)
    assert len(measure.asked) == int(want.scored.sum())
    model.check(_matrix_of(full, list(texts)), [float(f) for f in want.f], want.scored, want)


def test_small_collections_and_bad_arguments(monkeypatch):
    from east import applications
    monkeypatch.delenv("EAST_HIP_RELATED", raising=False)
    assert applications.texts_related({"only": b"one single text here"}, 5, "symmetric", None, _StubMeasure()) == {"only": []}
    assert applications.texts_related({}, 5, "symmetric", None, _RefusingMeasure()) == {}
    got = applications.texts_related({"x": b"", "y": b"12 34"}, 5, "directed", None, _StubMeasure())
    _same(got, {"x": [("y", 0.0)], "y": [("x", 0.0)]})                      # no string anywhere: +0.0 everywhere, nothing asked
    texts = _texts()
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            applications.texts_related(texts, bad, "symmetric", None, _StubMeasure())
    for bad in ("both", "", None, 1):
        with pytest.raises(ValueError):
            applications.texts_related(texts, 3, bad, None, _StubMeasure())
    with pytest.raises(ValueError):
        applications.texts_related(texts, 3, "directed", NAN, _StubMeasure())


class _RepeatedTitles(object):
    """A text collection whose titles repeat (a list of pairs behind the mapping's methods the applications use)."""

    def __init__(self, pairs):
        self.pairs = pairs

    def keys(self):
        return [k for k, _ in self.pairs]

    def values(self):
        return [v for _, v in self.pairs]


def test_where_the_host_path_is_taken(monkeypatch):
    """EAST_HIP_RELATED=host, repeated titles, a measure whose `relevance_related` is None: the host path; a measure that
    offers `relevance_related` is asked otherwise."""
    from east import applications, hip_backend, parallel, relevance
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_related is None
    assert parallel.DistributedASTRelevanceMeasure.relevance_related is None
    assert callable(relevance.ASTRelevanceMeasure.relevance_related) and callable(relevance.ASTRelevanceMeasure.relatedness_matrix)
    texts = {"x": _prose(4, 9), "y": _prose(5, 12), "z": _prose(6, 7)}

    class NoneRelated(_StubMeasure):
        relevance_related = None

    monkeypatch.delenv("EAST_HIP_RELATED", raising=False)
    want = applications.texts_related(texts, 2, "symmetric", 0.01, NoneRelated())
    assert list(want) == ["x", "y", "z"] and all(len(e) == 2 for e in want.values())
    monkeypatch.setenv("EAST_HIP_RELATED", "host")
    _same(applications.texts_related(texts, 2, "symmetric", 0.01, _RefusingMeasure()), want)
    monkeypatch.delenv("EAST_HIP_RELATED")
    with pytest.raises(AssertionError):
        applications.texts_related(texts, 2, "symmetric", 0.01, _RefusingMeasure())
    # repeated titles: the host path over all three texts; a repeated title keeps its last list, as a dict does
    repeated = _RepeatedTitles([("x", texts["x"]), ("y", texts["y"]), ("x", texts["z"])])
    got = applications.texts_related(repeated, 2, "directed", None, _RefusingMeasure())
    exact = model.exact(_collections(texts), stub_score, model.DIRECTED)
    assert list(got) == ["x", "y"]
    order = applications._top_select(exact.R, 1, 2, -INF)
    assert [o for o, _ in got["x"]] == [["x", "y", "x"][i] for i, _ in order[2]]
    assert [o for o, _ in got["y"]] == [["x", "y", "x"][i] for i, _ in order[1]]

    seen = {}

    class Measure(object):
        def set_text_collection(self, texts, language=None):
            seen["texts"] = list(texts)

        def relevance_table(self, prepared):
            raise AssertionError("the host path must not be taken")

        def relevance_related(self, orientation, n, threshold):
            seen["call"] = (orientation, n, threshold)
            return hip_backend.TopArrays(np.array([2, 0, 1], dtype=np.int32), np.array([[1, 2], [-1, -1], [0, -1]], dtype=np.int32),
                                         np.array([[0.75, 0.0], [0.0, 0.0], [0.5, 0.0]]))

    got = applications.texts_related(texts, 2, "symmetric", None, Measure())
    assert seen["call"] == (hip_backend.RELATED_SYMMETRIC, 2, -INF) and seen["texts"] == list(texts.values())
    _same(got, {"x": [("y", 0.75), ("z", 0.0)], "y": [], "z": [("x", 0.5)]})
    applications.texts_related(texts, 7, "directed", 0.1, Measure())
    assert seen["call"] == (hip_backend.RELATED_DIRECTED, 7, 0.1)


def test_format_related_on_a_hand_written_case():
    from east import formatting
    result = {"b": [('say "hi"', 0.5125), ("a", 0.25)], "a": [("b", 0.0)], "c": []}
    assert formatting.format_related(result, "xml") == (
        '<related>\n'
        '  <text name="a">\n'
        '    <text name="b" rank="1">0.000</text>\n'
        '  </text>\n'
        '  <text name="b">\n'
        '    <text name="say "hi"" rank="1">0.512</text>\n'
        '    <text name="a" rank="2">0.250</text>\n'
        '  </text>\n'
        '  <text name="c">\n'
        '  </text>\n'
        '</related>\n')
    assert formatting.format_related(result, "csv") == '"a","b",1,0.000\n"b","say \'hi\'",1,0.512\n"b","a",2,0.250\n'
    assert formatting.format_related(result, "csv") == formatting.format_similar(result, "text", "csv")
    assert formatting.format_related({}, "xml") == '<related>\n</related>\n'
    assert formatting.format_related({}, "csv") == ""
    with pytest.raises(Exception):
        formatting.format_related(result, "gml")


def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch):
    """A bad -n, -r or -o, -s cosine, -y, -g N > 1, a launcher, the forced collective path: one line and exit code 1, before a
    file is read or a measure is made."""
    from east import main, relevance
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    touched = []
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr(main, "launch_ranks", lambda *a: touched.append("ranks") or 0)
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    tail = ["texts", "related", str(tmp_path)]
    for bad, word in ((["-n", "0"], "0"), (["-n", "1025"], "1025"), (["-n", "2.5"], "2.5"), (["-r", "nan"], "nan"),
                      (["-r", "high"], "high"), (["-o", "both"], "both"), (["-s", "cosine"], "cosine"), (["-y"], "-y"),
                      (["-y", "-t", "triples.txt"], "-y"), (["-g", "4"], "-g 4"), (["-g", "x"], "'x'"),
                      (["-g", "4", "-o", "sideways"], "sideways")):
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
    assert rc == 1 and "'related'" in out
    rc, out = _east(["texts", "related"])
    assert rc == 1 and "texts related" in out
    rc, out = _east(["texts"])
    assert rc == 1 and "'related'" in out
    assert touched == []
    monkeypatch.undo()
    assert "texts related" in main.__doc__ and "o:" in main._OPTIONS
    rc, out = _east([])
    assert rc == 1 and "keyphrases, texts" in out
    rc, out = _east(["words", "related", str(tmp_path)])
    assert rc == 1 and "'texts'" in out


def test_cli_prints_the_result(tmp_path, monkeypatch):
    """The options reach texts_related and its result is printed in the format asked for."""
    from east import applications, formatting, main, relevance
    for name in ("WORLD_SIZE", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    made = []
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: made.append(a))
    (tmp_path / "t.txt").write_bytes(b"one\ntwo\n")
    seen = []
    result = {"0": [("1", 0.5)], "1": [("0", 0.5)]}

    def fake(texts, n, orientation, threshold, measure, language):
        seen.append((dict(texts), n, orientation, threshold, type(measure).__name__))
        return result

    monkeypatch.setattr(applications, "texts_related", fake)
    tail = ["texts", "related", str(tmp_path / "t.txt")]
    assert _east(tail) == (0, formatting.format_related(result, "xml") + "\n")
    assert seen[-1] == ({"0": b"one", "1": b"two"}, 10, "symmetric", None, "ASTRelevanceMeasure")
    assert made[-1][1] is True                                                # normalized
    assert _east(["-n", "3", "-o", "Directed", "-r", "0.2", "-d", "-f", "csv", "-g", "1"] + tail) == (0, formatting.format_related(result, "csv") + "\n")
    assert seen[-1][1:4] == (3, "directed", 0.2) and made[-1][1] is False
    rc, out = _east(["-f", "gml"] + tail)
    assert rc == 1 and out.count("\n") == 1
    folder = tmp_path / "dir"
    folder.mkdir()
    (folder / "b.txt").write_bytes(b"second")
    (folder / "a.txt").write_bytes(b"first")
    (folder / "notes.md").write_bytes(b"no text")
    assert _east(["texts", "related", str(folder)])[0] == 0
    assert seen[-1][0] == {"a": b"first", "b": b"second"} and list(seen[-1][0]) == ["a", "b"]


def test_binding_against_the_header():
    """Every relatedness entry point is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Text-to-text relatedness" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, value in (("EAST_HIP_RELATED_DIRECTED", 0), ("EAST_HIP_RELATED_SYMMETRIC", 1), ("EAST_HIP_GRAPH_SOURCE_RELATED", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src), name
    assert (hip_backend.RELATED_DIRECTED, hip_backend.RELATED_SYMMETRIC, hip_backend.GRAPH_SOURCE_RELATED) == (0, 1, 4)
    names = ["east_hip_related_build", "east_hip_related_fetch", "east_hip_last_related_ms", "east_hip_debug_set_related_chunk"]
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
    assert lib.east_hip_last_related_ms(None) == -1.0
    assert lib.east_hip_related_fetch(None, None, None, None) == invalid
    assert lib.east_hip_related_build(None, 1, 1, None) == invalid
    assert lib.east_hip_related_build(None, 1, 7, None) == invalid
    assert lib.east_hip_debug_set_related_chunk(256) == 0 and lib.east_hip_debug_set_related_chunk(0) == 0
    for method in ("related_build", "related_matrix", "related", "rank_related", "last_related_ms"):
        assert callable(getattr(hip_backend.HipIndex, method)), method
