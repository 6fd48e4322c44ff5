"""CPU tier: similar texts and keyphrases (applications.keyphrases_similar) on the host path, format_similar, the command
line's refusals and the binding of the new entry points -- no device.  The yardstick is tests/similar_exact.py: the
contract of include/east_hip.h ("Similar texts and keyphrases") in extended precision for the values, the ranking's
contract (np.lexsort) for the selection, applied to the matrix the host path itself reported (its full lists).  Values are
compared to the bound (2 L + 16) * 2^-53, names and order with ==."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import similar_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


class _ArrayMeasure(object):
    """A batched measure that returns a given K x D array and has no `relevance_similar`: the host path."""

    def __init__(self, scores):
        self.scores = scores

    def set_text_collection(self, texts, language=None):
        pass

    def relevance_table(self, prepared, synonimizer=None):
        return self.scores


class _RefusingMeasure(_ArrayMeasure):
    def relevance_similar(self, *args):
        raise AssertionError("the device path must not be taken")


def _tables():
    rng = np.random.default_rng(7)
    hand = np.array([[0.5, 0.0, 0.5, -0.5, 0.25, 1e-3],        # columns 0 and 2 are equal, 3 is their opposite, 1 is a zero profile
                     [0.25, -0.0, 0.25, -0.25, 0.5, 0.75],
                     [0.125, 0.0, 0.125, -0.125, 0.0, 0.3],
                     [1.0, 0.0, 1.0, -1.0, 0.7, 0.1]])
    rows = np.ascontiguousarray(hand.T)                       # the same profiles as rows
    nans = rng.random((9, 7))
    nans[3, 4] = NAN                                          # keyphrase 3 and text 4 have no number
    random = rng.random((12, 8))
    random[rng.random((12, 8)) < 0.1] = 0.0
    return {"hand": hand, "rows": rows, "nans": nans, "random": random}


def _matrix_of(full, names):
    """The matrix the path under test ranked, from its full lists ({member: [(other, similarity)]}, n = 1024, no
    threshold): NaN where a pair is not listed."""
    where = {name: i for i, name in enumerate(names)}
    H = np.full((len(names), len(names)), NAN)
    for member, entries in full.items():
        for other, value in entries:
            H[where[member], where[other]] = value
    return H


def _named(selection, names):
    count, index, score = selection
    return {names[s]: [(names[i], float(v)) for i, v in zip(index[s, :count[s]].tolist(), score[s, :count[s]].tolist())]
            for s in range(len(names))}


def _same(got, want):
    assert got == want
    flat = lambda r: [repr(v) for entries in r.values() for _, v in entries]
    assert flat(got) == flat(want)
    assert all(type(m) is str and type(v) is float for entries in got.values() for m, v in entries)


@pytest.mark.parametrize("name", ["hand", "rows", "nans", "random"])
def test_host_path_is_the_contract(monkeypatch, name):
    from east import applications
    monkeypatch.delenv("EAST_HIP_SIMILAR", raising=False)
    scores = _tables()[name]
    K, D = scores.shape
    kps = ["kp%d" % i for i in range(K)]
    texts = {"t%d" % d: b"x" for d in range(D)}
    for axis, by, names in ((0, "text", list(texts)), (1, "keyphrase", kps)):
        M, L = (D, K) if axis == 0 else (K, D)
        full = applications.keyphrases_similar(kps, texts, 1024, by, None, _ArrayMeasure(scores))
        assert list(full) == names and all(member not in [o for o, _ in entries] for member, entries in full.items())
        H = _matrix_of(full, names)
        want, _ = model.exact(model.profiles_of(scores, axis))
        assert np.array_equal(np.isnan(H), np.isnan(want))
        assert np.nanmax(np.abs(H - want), initial=0.0) <= model.bound(L)
        assert H.tobytes() == H.T.copy().tobytes()
        finite = H[np.isfinite(H)]
        present = float(finite[finite.size // 2])
        for n in (1, 2, M - 1, M + 3, 1024):                   # (n above M - 1: the lists are shorter)
            for threshold in (None, -INF, present, np.nextafter(present, 2.0), np.nextafter(present, -2.0), 0.0, 2.0):
                got = applications.keyphrases_similar(kps, texts, n, by, threshold, _ArrayMeasure(scores))
                _same(got, _named(model.select(H, n, -INF if threshold is None else threshold), names))
                assert all(len(entries) <= min(n, M - 1) for entries in got.values())
                if threshold == 2.0:
                    assert all(entries == [] for entries in got.values()) and len(got) == M


def test_hand_made_profiles():
    """Equal profiles: 1 to the bound (not clamped); opposite ones: -1 to the bound; a zero profile: +0.0 with everyone;
    a NaN score: its member lists nobody and nobody lists it."""
    from east import applications
    t = _tables()
    kps = ["kp%d" % i for i in range(4)]
    texts = {"t%d" % d: b"x" for d in range(6)}
    got = applications.keyphrases_similar(kps, texts, 10, "text", None, _ArrayMeasure(t["hand"]))
    by_name = {member: dict(entries) for member, entries in got.items()}
    assert abs(by_name["t0"]["t2"] - 1.0) <= model.bound(4) and by_name["t0"]["t2"] == by_name["t2"]["t0"]
    assert abs(by_name["t0"]["t3"] + 1.0) <= model.bound(4) and abs(by_name["t3"]["t2"] + 1.0) <= model.bound(4)
    assert all(repr(v) == "0.0" for v in by_name["t1"].values()) and len(by_name["t1"]) == 5
    assert all(repr(by_name[m]["t1"]) == "0.0" for m in by_name if m != "t1")
    assert [o for o, _ in got["t0"]][0] == "t2" and [o for o, _ in got["t0"]][-1] == "t3"
    kps9 = ["kp%d" % i for i in range(9)]
    texts7 = {"t%d" % d: b"x" for d in range(7)}
    got = applications.keyphrases_similar(kps9, texts7, 10, "keyphrase", None, _ArrayMeasure(t["nans"]))
    assert got["kp3"] == [] and all("kp3" not in [o for o, _ in e] for e in got.values())
    assert all(len(e) == 7 for m, e in got.items() if m != "kp3")
    got = applications.keyphrases_similar(kps9, texts7, 10, "text", None, _ArrayMeasure(t["nans"]))
    assert got["t4"] == [] and all(len(e) == 5 for m, e in got.items() if m != "t4")


def test_duplicate_and_empty_keyphrases_and_bad_arguments(monkeypatch):
    from east import applications
    monkeypatch.delenv("EAST_HIP_SIMILAR", raising=False)
    scores = np.array([[0.5, 0.1, 0.3], [0.5, 0.7, 0.3], [0.2, 0.7, 0.9]])
    listed = ["b", "", "a", "b", "c", "", "a"]                 # kept: b, a, c -- a member's index is its position among them
    texts = {"x": b"", "y": b"", "z": b""}
    for by, names in (("text", list(texts)), ("keyphrase", ["b", "a", "c"])):
        full = applications.keyphrases_similar(listed, texts, 1024, by, None, _ArrayMeasure(scores))
        assert list(full) == names
        H = _matrix_of(full, names)
        want, _ = model.exact(model.profiles_of(scores, 0 if by == "text" else 1))
        assert np.nanmax(np.abs(H - want)) <= model.bound(3)
        _same(applications.keyphrases_similar(listed, texts, 1, by, None, _ArrayMeasure(scores)), _named(model.select(H, 1, -INF), names))
    assert applications.keyphrases_similar(["", ""], texts, 3, "text", None, _RefusingMeasure(scores)) == {"x": [], "y": [], "z": []}
    assert applications.keyphrases_similar([], texts, 3, "keyphrase", None, _RefusingMeasure(scores)) == {}
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            applications.keyphrases_similar(listed, texts, bad, "text", None, _ArrayMeasure(scores))
    with pytest.raises(ValueError):
        applications.keyphrases_similar(listed, texts, 3, "rows", None, _ArrayMeasure(scores))
    with pytest.raises(ValueError):
        applications.keyphrases_similar(listed, texts, 3, "text", NAN, _ArrayMeasure(scores))


class _RepeatedTitles(object):
    """A text collection whose titles repeat (a list of pairs behind the mapping's methods keyphrases_table uses)."""

    def __init__(self, pairs):
        self.pairs = pairs

    def keys(self):
        return [k for k, _ in self.pairs]

    def values(self):
        return [v for _, v in self.pairs]


def test_where_the_host_path_is_taken(monkeypatch):
    """EAST_HIP_SIMILAR=host, a synonimizer, repeated titles, a measure whose `relevance_similar` is None: keyphrases_table
    is called; a measure that offers `relevance_similar` is asked otherwise, with the keyphrases as keyphrases_table takes
    them."""
    from east import applications, hip_backend, parallel, relevance, utils
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_similar is None
    assert parallel.DistributedASTRelevanceMeasure.relevance_similar is None
    assert callable(relevance.ASTRelevanceMeasure.relevance_similar) and callable(relevance.CosineRelevanceMeasure.relevance_similar)
    scores = np.array([[0.5, 0.1, 0.3], [0.5, 0.7, 0.3]])
    kps, texts = ["a", "b"], {"x": b"", "y": b"", "z": b""}

    class NoneSimilar(_ArrayMeasure):
        relevance_similar = None

    monkeypatch.delenv("EAST_HIP_SIMILAR", raising=False)
    want = applications.keyphrases_similar(kps, texts, 2, "text", 0.2, NoneSimilar(scores))
    assert list(want) == ["x", "y", "z"] and all(len(e) == 2 for e in want.values())
    _same(applications.keyphrases_similar(kps, texts, 2, "text", 0.2, _RefusingMeasure(scores), {"a": ["b"]}), want)
    monkeypatch.setenv("EAST_HIP_SIMILAR", "host")
    _same(applications.keyphrases_similar(kps, texts, 2, "text", 0.2, _RefusingMeasure(scores)), want)
    monkeypatch.delenv("EAST_HIP_SIMILAR")
    with pytest.raises(AssertionError):
        applications.keyphrases_similar(kps, texts, 2, "text", 0.2, _RefusingMeasure(scores))
    # repeated titles: the host path over all three columns; a repeated title keeps its last list, as a dict does
    repeated = _RepeatedTitles([("x", b""), ("y", b""), ("x", b"")])
    got = applications.keyphrases_similar(kps, repeated, 2, "text", None, _RefusingMeasure(scores))
    H, _ = model.exact(model.profiles_of(scores, 0))
    assert list(got) == ["x", "y"]
    assert [o for o, _ in got["x"]] == [["x", "y", "x"][i] for i in model.select(H, 2, -INF)[1][2]]
    assert [o for o, _ in got["y"]] == [["x", "y", "x"][i] for i in model.select(H, 2, -INF)[1][1]]
    assert all(abs(v - H[2, i]) <= model.bound(2) for (_, v), i in zip(got["x"], model.select(H, 2, -INF)[1][2]))

    seen = {}

    class Measure(object):
        def set_text_collection(self, texts, language=None):
            seen["texts"] = list(texts)

        def relevance_table(self, prepared):
            raise AssertionError("the table must not be fetched")

        def relevance_similar(self, prepared, axis, n, threshold):
            seen["call"] = (list(prepared), axis, n, threshold)
            return hip_backend.TopArrays(np.array([2, 0, 1], dtype=np.int32), np.array([[1, 2], [-1, -1], [0, -1]], dtype=np.int32),
                                         np.array([[0.75, -0.0], [0.0, 0.0], [0.5, 0.0]]))

    monkeypatch.setattr(applications, "keyphrases_table", lambda *a, **k: pytest.fail("host path taken"))
    got = applications.keyphrases_similar(["one two", "", "never", "one two"], texts, 2, "text", None, Measure())
    assert seen["call"] == ([utils.prepare_text("one two"), utils.prepare_text("never")], 0, 2, -INF)
    assert seen["texts"] == [b"", b"", b""]
    _same(got, {"x": [("y", 0.75), ("z", -0.0)], "y": [], "z": [("x", 0.5)]})
    got = applications.keyphrases_similar(["p", "q", "r"], {"x": b"", "y": b""}, 2, "keyphrase", 0.1, Measure())
    assert seen["call"][1:] == (1, 2, 0.1)
    _same(got, {"p": [("q", 0.75), ("r", -0.0)], "q": [], "r": [("p", 0.5)]})


def test_the_fraction_model_agrees_with_the_wide_one():
    """The yardstick's fallback (for machines whose long double is a double) is the same function where both exist."""
    if not model.WIDE:
        pytest.skip("np.longdouble is no wider than a double here: there is nothing to compare the Fraction model with")
    rng = np.random.default_rng(11)
    P = rng.random((9, 13)) - 0.3
    P[4] = 0.0
    P[6] = -P[2]
    wide, q_wide = model.exact_wide(P)
    frac, q_frac = model.exact_fraction(P)
    assert np.array_equal(np.isnan(wide), np.isnan(frac)) and np.isnan(np.diag(wide)).all()
    assert np.nanmax(np.abs(wide - frac)) <= 2.0 ** -52 and np.array_equal(q_wide, q_frac)
    assert not wide[4, [0, 1, 2, 3, 5]].any() and abs(wide[2, 6] + 1.0) <= 2.0 ** -52


def test_format_similar_on_a_hand_written_case():
    from east import formatting
    by_text = {"b": [('say "hi"', 0.5125), ("a", 0.25)], "a": [("b", -0.0)], "c": []}
    assert formatting.format_similar(by_text, "text", "xml") == (
        '<similar by="text">\n'
        '  <text name="a">\n'
        '    <text name="b" rank="1">-0.000</text>\n'
        '  </text>\n'
        '  <text name="b">\n'
        '    <text name="say "hi"" rank="1">0.512</text>\n'
        '    <text name="a" rank="2">0.250</text>\n'
        '  </text>\n'
        '  <text name="c">\n'
        '  </text>\n'
        '</similar>\n')
    assert formatting.format_similar(by_text, "text", "csv") == '"a","b",1,-0.000\n"b","say \'hi\'",1,0.512\n"b","a",2,0.250\n'
    by_keyphrase = {"kp2": [("kp1", 1.0), ("kp0", 0.9996)], "kp1": [("kp2", -1.0)]}
    assert formatting.format_similar(by_keyphrase, "keyphrase", "xml") == (
        '<similar by="keyphrase">\n'
        '  <keyphrase value="kp1">\n'
        '    <keyphrase value="kp2" rank="1">-1.000</keyphrase>\n'
        '  </keyphrase>\n'
        '  <keyphrase value="kp2">\n'
        '    <keyphrase value="kp1" rank="1">1.000</keyphrase>\n'
        '    <keyphrase value="kp0" rank="2">1.000</keyphrase>\n'
        '  </keyphrase>\n'
        '</similar>\n')
    assert formatting.format_similar(by_keyphrase, "keyphrase", "csv") == '"kp1","kp2",1,-1.000\n"kp2","kp1",1,1.000\n"kp2","kp0",2,1.000\n'
    assert formatting.format_similar({}, "keyphrase", "xml") == '<similar by="keyphrase">\n</similar>\n'
    assert formatting.format_similar({}, "text", "csv") == ""
    with pytest.raises(Exception):
        formatting.format_similar(by_text, "text", "gml")
    with pytest.raises(Exception):
        formatting.format_similar(by_text, "rows", "xml")


def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch):
    """-n 0, -n 1025, -b x, -r nan: one line and exit code 1, before a file is read or a measure is made."""
    from east import main, relevance
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EAST_HIP_DEVICES", raising=False)
    touched = []
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    tail = ["keyphrases", "similar", str(tmp_path / "kp.txt"), str(tmp_path)]
    for bad in (["-n", "0"], ["-n", "1025"], ["-b", "x"], ["-r", "nan"], ["-n", "2.5"], ["-g", "4", "-n", "0"],
                ["-s", "cosine", "-b", "x"]):
        rc, out = _east(bad + tail)
        assert rc == 1 and out.count("\n") == 1 and bad[-1] in out, (bad, out)
    assert touched == []
    monkeypatch.undo()
    assert "keyphrases similar" in main.__doc__
    rc, out = _east([])
    assert rc == 1 and "table/graph/top/similar" in out
    (tmp_path / "kp.txt").write_bytes(b"alpha\n")
    (tmp_path / "t.txt").write_bytes(b"alpha beta\n")
    rc, out = _east(["keyphrases", "alike", str(tmp_path / "kp.txt"), str(tmp_path / "t.txt")])
    assert rc == 1 and "'similar'" in out


def test_cli_prints_the_result(tmp_path, monkeypatch):
    """The options reach keyphrases_similar and its result is printed in the format asked for."""
    from east import applications, formatting, main, relevance
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EAST_HIP_DEVICES", raising=False)
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: None)
    (tmp_path / "kp.txt").write_bytes(b"alpha\nbeta\n")
    (tmp_path / "t.txt").write_bytes(b"one\ntwo\n")
    seen = []
    result = {"0": [("1", 0.5)], "1": [("0", 0.5)]}

    def fake(keyphrases, texts, n, by, threshold, measure, synonimizer, language):
        seen.append((list(keyphrases), list(texts), n, by, threshold, synonimizer))
        return result

    monkeypatch.setattr(applications, "keyphrases_similar", fake)
    tail = ["keyphrases", "similar", str(tmp_path / "kp.txt"), str(tmp_path / "t.txt")]
    assert _east(tail) == (0, formatting.format_similar(result, "text", "xml") + "\n")
    assert seen[-1] == (["alpha", "beta"], ["0", "1"], 10, "text", None, None)
    assert _east(["-n", "3", "-b", "keyphrase", "-r", "0.2", "-f", "csv"] + tail) == (0, formatting.format_similar(result, "keyphrase", "csv") + "\n")
    assert seen[-1][2:5] == (3, "keyphrase", 0.2)
    rc, out = _east(["-f", "gml"] + tail)
    assert rc == 1 and out.count("\n") == 1


def test_binding_against_the_header():
    """Every similarity entry point is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Similar texts and keyphrases" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+EAST_HIP_GRAPH_SOURCE_SIMILARITY\s+3\b", src)
    assert hip_backend.GRAPH_SOURCE_SIMILARITY == 3
    names = ["east_hip_similarity_build_resident", "east_hip_similarity_build_host", "east_hip_similarity_fetch",
             "east_hip_last_similarity_ms"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp,
                "int32_t": ctypes.c_int32}
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
    assert lib.east_hip_last_similarity_ms(None) == -1.0
    assert lib.east_hip_similarity_fetch(None, None, None) != 0
    assert lib.east_hip_similarity_build_resident(None, 0, 0, None) != 0
    for method in ("similarity", "similarity_from_table", "similarity_from_uploaded", "similarity_matrix", "similar", "last_similarity_ms"):
        assert hasattr(hip_backend.HipIndex, method), method
    for method in ("similarity", "similarity_matrix", "similar"):
        assert hasattr(hip_backend.HipCosineIndex, method), method
