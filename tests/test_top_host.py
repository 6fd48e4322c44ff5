"""CPU tier: ranked keyphrases (applications.keyphrases_top) on the host path, format_top, the command line's refusals and
the binding of the new entry points -- no device.  The yardstick is the contract of include/east_hip.h ("Ranked
keyphrases") written out here with Python's sorted; it never calls the project's own selection."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def contract(values, n, threshold):
    """One segment: [(member, score)] -- eligible iff score >= threshold (a NaN never is), score descending, member
    ascending among equal scores (-0.0 == 0.0), the first n."""
    v = [float(x) for x in values]
    order = sorted((i for i in range(len(v)) if v[i] >= threshold), key=lambda i: (-v[i], i))[:n]
    return [(i, v[i]) for i in order]


def same(got, want):
    """Equal entries, the sign of a zero included (0.0 == -0.0 in Python)."""
    assert got == want
    flat = lambda top: [repr(score) for entries in top.values() for _, score in entries]
    assert flat(got) == flat(want)
    assert all(type(m) is str and type(s) is float for entries in got.values() for m, s in entries)


class _ArrayMeasure(object):
    """A batched measure that returns a given K x D array and has no `relevance_top`: keyphrases_top stays on the host."""

    def __init__(self, scores):
        self.scores = scores

    def set_text_collection(self, texts, language=None):
        pass

    def relevance_table(self, prepared, synonimizer=None):
        return self.scores


class _RefusingTopMeasure(_ArrayMeasure):
    def relevance_top(self, *args):
        raise AssertionError("the device path must not be taken")


def _want(kps, titles, scores, n, by, threshold):
    if by == "text":
        return {t: [(kps[i], s) for i, s in contract(scores[:, d], n, threshold)] for d, t in enumerate(titles)}
    return {k: [(titles[i], s) for i, s in contract(scores[r], n, threshold)] for r, k in enumerate(kps)}


def _tables():
    rng = np.random.default_rng(5)
    ties = rng.choice([0.0, 0.25, 0.5], size=(23, 9))
    zeros = np.where(rng.random((11, 7)) < 0.5, -0.0, 0.0)
    zeros[3] = [0.5, -0.0, 0.0, -1.0, -0.0, 0.5, 0.0]
    nans = rng.random((13, 5))
    nans[rng.random((13, 5)) < 0.4] = NAN
    nans[4] = NAN
    nans[:, 2] = NAN
    return {"ties": ties, "zeros": zeros, "nans": nans, "random": rng.random((17, 6))}


@pytest.mark.parametrize("name", ["ties", "zeros", "nans", "random"])
def test_host_path_is_the_contract(monkeypatch, name):
    from east import applications
    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    scores = _tables()[name]
    K, D = scores.shape
    kps = ["kp%d" % i for i in range(K)]
    texts = {"t%d" % d: b"x" for d in range(D)}
    present = float(scores[np.isfinite(scores)].flat[3])
    for by in ("text", "keyphrase"):
        for n in (1, 2, 5, max(K, D) + 3, 1024):                    # (n > L: the lists are shorter)
            for threshold in (None, -INF, 0.0, 0.25, present, 2.0):  # a value that occurs; above everything
                got = applications.keyphrases_top(kps, texts, n, by, threshold, _ArrayMeasure(scores))
                same(got, _want(kps, list(texts), scores, n, by, -INF if threshold is None else threshold))
                if threshold == 2.0:
                    assert all(entries == [] for entries in got.values()) and len(got) == (D if by == "text" else K)
    with np.errstate(invalid="ignore"):
        full = applications.keyphrases_top(kps, texts, 1024, "text", None, _ArrayMeasure(scores))
    assert [len(full["t%d" % d]) for d in range(D)] == np.isfinite(scores).sum(axis=0).tolist()


def test_large_table_goes_through_the_array(monkeypatch):
    """From ARRAY_TABLE_MIN_SCORES scores on keyphrases_table gives a ScoreTable: the same answer."""
    from east import applications
    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    monkeypatch.setattr(applications, "ARRAY_TABLE_MIN_SCORES", 16)
    scores = _tables()["ties"]
    kps = ["kp%d" % i for i in range(scores.shape[0])]
    texts = {"t%d" % d: b"x" for d in range(scores.shape[1])}
    for by in ("text", "keyphrase"):
        same(applications.keyphrases_top(kps, texts, 4, by, 0.25, _ArrayMeasure(scores)), _want(kps, list(texts), scores, 4, by, 0.25))


def test_duplicate_and_empty_keyphrases(monkeypatch):
    from east import applications
    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    scores = np.array([[0.5, 0.1, 0.3], [0.5, 0.7, 0.3], [0.2, 0.7, NAN]])
    listed = ["b", "", "a", "b", "c", "", "a"]                      # kept: b, a, c -- the member index is the position among them
    texts = {"x": b"", "y": b"", "z": b""}
    for by in ("text", "keyphrase"):
        same(applications.keyphrases_top(listed, texts, 2, by, None, _ArrayMeasure(scores)), _want(["b", "a", "c"], list(texts), scores, 2, by, -INF))
    assert applications.keyphrases_top(listed, texts, 1, "text", None, _ArrayMeasure(scores)) == {"x": [("b", 0.5)], "y": [("a", 0.7)], "z": [("b", 0.3)]}
    # no keyphrase to score
    assert applications.keyphrases_top(["", ""], texts, 3, "text", None, _RefusingTopMeasure(scores)) == {"x": [], "y": [], "z": []}
    assert applications.keyphrases_top([], texts, 3, "keyphrase", None, _RefusingTopMeasure(scores)) == {}
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            applications.keyphrases_top(listed, texts, bad, "text", None, _ArrayMeasure(scores))
    with pytest.raises(ValueError):
        applications.keyphrases_top(listed, texts, 3, "rows", None, _ArrayMeasure(scores))
    with pytest.raises(ValueError):
        applications.keyphrases_top(listed, texts, 3, "text", NAN, _ArrayMeasure(scores))


class _RepeatedTitles(object):
    """A text collection whose titles repeat (a list of pairs behind the mapping's methods keyphrases_table uses)."""

    def __init__(self, pairs):
        self.pairs = pairs

    def keys(self):
        return [k for k, _ in self.pairs]

    def values(self):
        return [v for _, v in self.pairs]


def test_where_the_host_path_is_taken(monkeypatch):
    """EAST_HIP_TOP=host, a synonimizer, repeated titles, a measure whose `relevance_top` is None: keyphrases_table is
    called; a measure that offers `relevance_top` is asked otherwise, with the keyphrases as keyphrases_table takes them."""
    from east import applications, hip_backend, parallel, relevance, utils
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_top is None
    assert parallel.DistributedASTRelevanceMeasure.relevance_top is None
    assert callable(relevance.ASTRelevanceMeasure.relevance_top) and callable(relevance.CosineRelevanceMeasure.relevance_top)
    scores = np.array([[0.5, 0.1, 0.3], [0.5, 0.7, 0.3]])
    kps, texts = ["a", "b"], {"x": b"", "y": b"", "z": b""}
    want = _want(kps, list(texts), scores, 2, "text", 0.2)

    class NoneTop(_ArrayMeasure):
        relevance_top = None

    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    same(applications.keyphrases_top(kps, texts, 2, "text", 0.2, NoneTop(scores)), want)
    same(applications.keyphrases_top(kps, texts, 2, "text", 0.2, _RefusingTopMeasure(scores), {"a": ["b"]}), want)
    monkeypatch.setenv("EAST_HIP_TOP", "host")
    same(applications.keyphrases_top(kps, texts, 2, "text", 0.2, _RefusingTopMeasure(scores)), want)
    monkeypatch.delenv("EAST_HIP_TOP")
    with pytest.raises(AssertionError):
        applications.keyphrases_top(kps, texts, 2, "text", 0.2, _RefusingTopMeasure(scores))
    # repeated titles: the host path; a repeated title keeps its last column, as in keyphrases_table's dict
    repeated = _RepeatedTitles([("x", b""), ("y", b""), ("x", b"")])
    got = applications.keyphrases_top(kps, repeated, 2, "text", None, _RefusingTopMeasure(scores))
    same(got, {"x": [(kps[i], s) for i, s in contract(scores[:, 2], 2, -INF)], "y": [(kps[i], s) for i, s in contract(scores[:, 1], 2, -INF)]})

    seen = {}

    class Measure(object):
        def set_text_collection(self, texts, language=None):
            seen["texts"] = list(texts)

        def relevance_table(self, prepared):
            raise AssertionError("the table must not be fetched")

        def relevance_top(self, prepared, axis, n, threshold):
            seen["call"] = (list(prepared), axis, n, threshold)
            return hip_backend.TopArrays(np.array([2, 0, 1], dtype=np.int32), np.array([[1, 0], [-1, -1], [0, -1]], dtype=np.int32),
                                         np.array([[0.75, -0.0], [0.0, 0.0], [0.5, 0.0]]))

    monkeypatch.setattr(applications, "keyphrases_table", lambda *a, **k: pytest.fail("host path taken"))
    got = applications.keyphrases_top(["one two", "", "never", "one two"], texts, 2, "text", None, Measure())
    assert seen["call"] == ([utils.prepare_text("one two"), utils.prepare_text("never")], 0, 2, -INF)
    assert seen["texts"] == [b"", b"", b""]
    same(got, {"x": [("never", 0.75), ("one two", -0.0)], "y": [], "z": [("one two", 0.5)]})
    got = applications.keyphrases_top(["p", "q", "r"], {"x": b"", "y": b""}, 2, "keyphrase", 0.1, Measure())
    assert seen["call"][1:] == (1, 2, 0.1)
    same(got, {"p": [("y", 0.75), ("x", -0.0)], "q": [], "r": [("x", 0.5)]})


def test_format_top_on_a_hand_written_case():
    from east import formatting
    by_text = {"b": [('say "hi"', 0.5125), ("kp", 0.25)], "a": [("kp", -0.0)], "c": []}
    assert formatting.format_top(by_text, "text", "xml") == (
        '<top by="text">\n'
        '  <text name="a">\n'
        '    <keyphrase value="kp" rank="1">-0.000</keyphrase>\n'
        '  </text>\n'
        '  <text name="b">\n'
        '    <keyphrase value="say "hi"" rank="1">0.512</keyphrase>\n'
        '    <keyphrase value="kp" rank="2">0.250</keyphrase>\n'
        '  </text>\n'
        '  <text name="c">\n'
        '  </text>\n'
        '</top>\n')
    assert formatting.format_top(by_text, "text", "csv") == '"a","kp",1,-0.000\n"b","say \'hi\'",1,0.512\n"b","kp",2,0.250\n'
    by_keyphrase = {"kp2": [("t1", 1.0), ("t0", 0.9996)], "kp1": [("t0", 0.1)]}
    assert formatting.format_top(by_keyphrase, "keyphrase", "xml") == (
        '<top by="keyphrase">\n'
        '  <keyphrase value="kp1">\n'
        '    <text name="t0" rank="1">0.100</text>\n'
        '  </keyphrase>\n'
        '  <keyphrase value="kp2">\n'
        '    <text name="t1" rank="1">1.000</text>\n'
        '    <text name="t0" rank="2">1.000</text>\n'
        '  </keyphrase>\n'
        '</top>\n')
    assert formatting.format_top(by_keyphrase, "keyphrase", "csv") == '"kp1","t0",1,0.100\n"kp2","t1",1,1.000\n"kp2","t0",2,1.000\n'
    assert formatting.format_top({}, "keyphrase", "xml") == '<top by="keyphrase">\n</top>\n'
    assert formatting.format_top({}, "keyphrase", "csv") == ""
    with pytest.raises(Exception):
        formatting.format_top(by_text, "text", "gml")
    with pytest.raises(Exception):
        formatting.format_top(by_text, "rows", "xml")


def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch):
    """-n 0, -n 1025, -n x, -b rows: one line and exit code 1, before a file is read or a measure is made."""
    from east import main, relevance
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EAST_HIP_DEVICES", raising=False)
    touched = []
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    tail = ["keyphrases", "top", str(tmp_path / "kp.txt"), str(tmp_path)]
    for bad in (["-n", "0"], ["-n", "1025"], ["-n", "x"], ["-n", "-3"], ["-n", "2.5"], ["-b", "rows"], ["-r", "high"],
                ["-g", "4", "-n", "0"]):
        rc, out = _east(bad + tail)
        assert rc == 1 and out.count("\n") == 1 and bad[-1] in out, (bad, out)
    assert touched == []
    assert "keyphrases top" in main.__doc__ and "n:" in main._OPTIONS and "b:" in main._OPTIONS
    rc, out = _east([])
    assert rc == 1 and "table/graph/top" in out
    (tmp_path / "kp.txt").write_bytes(b"alpha\n")
    (tmp_path / "t.txt").write_bytes(b"alpha beta\n")
    monkeypatch.undo()
    rc, out = _east(["keyphrases", "rank", str(tmp_path / "kp.txt"), str(tmp_path / "t.txt")])
    assert rc == 1 and "'top'" in out


def test_cli_prints_the_host_path(tmp_path, monkeypatch):
    """The options reach keyphrases_top and its result is printed in the format asked for."""
    from east import applications, formatting, main, relevance
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EAST_HIP_DEVICES", raising=False)
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: None)
    (tmp_path / "kp.txt").write_bytes(b"alpha\nbeta\n")
    (tmp_path / "t.txt").write_bytes(b"one\ntwo\n")
    seen = []
    top = {"0": [("alpha", 0.5)], "1": [("beta", 0.25), ("alpha", 0.125)]}

    def fake(keyphrases, texts, n, by, threshold, measure, synonimizer, language):
        seen.append((list(keyphrases), list(texts), n, by, threshold, synonimizer))
        return top

    monkeypatch.setattr(applications, "keyphrases_top", fake)
    tail = ["keyphrases", "top", str(tmp_path / "kp.txt"), str(tmp_path / "t.txt")]
    assert _east(tail) == (0, formatting.format_top(top, "text", "xml") + "\n")
    assert seen[-1] == (["alpha", "beta"], ["0", "1"], 10, "text", None, None)
    assert _east(["-n", "3", "-b", "keyphrase", "-r", "0.2", "-f", "csv"] + tail) == (0, formatting.format_top(top, "keyphrase", "csv") + "\n")
    assert seen[-1][2:5] == (3, "keyphrase", 0.2)
    rc, out = _east(["-f", "gml"] + tail)
    assert rc == 1 and out.count("\n") == 1


def test_binding_against_the_header():
    """Every ranking entry point is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Ranked keyphrases" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+EAST_HIP_TOP_BY_TEXT\s+0\b", src) and re.search(r"#define\s+EAST_HIP_TOP_BY_KEYPHRASE\s+1\b", src)
    assert (hip_backend.TOP_BY_TEXT, hip_backend.TOP_BY_KEYPHRASE) == (0, 1)
    names = ["east_hip_top_build_resident", "east_hip_top_build_host", "east_hip_top_fetch", "east_hip_last_top_ms",
             "east_hip_debug_set_top_tile"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int32_t *": hip_backend._c_i32p,
                "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp, "int64_t": ctypes.c_int64,
                "int32_t": ctypes.c_int32, "double": ctypes.c_double, "int": ctypes.c_int}
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
    assert lib.east_hip_debug_set_top_tile(7) == 0 and lib.east_hip_debug_set_top_tile(0) == 0
    assert lib.east_hip_last_top_ms(None) == -1.0
    assert lib.east_hip_top_fetch(None, None, None, None) != 0
    assert lib.east_hip_top_build_resident(None, 0, 0, 10, 0.0, None) != 0
