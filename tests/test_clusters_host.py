"""CPU tier of the clusters (include/east_hip.h, "Clusters"): the model on hand-made cases, the host path of
applications.texts_clusters / keyphrases_clusters against it, the cuts, the formats, to_linkage, the CLI's refusals and
the binding against the header."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import clusters_exact as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _matrix(M, pairs):
    """NaN everywhere but the given {(a, b): w} (a < b), mirrored."""
    S = np.full((M, M), NAN)
    for (a, b), w in pairs.items():
        S[a, b] = S[b, a] = w
    return S


def _merges(S):
    a, b, w = model.merges(S)
    return list(zip(a.tolist(), b.tolist(), w.tolist()))


# ---- the model on hand-made cases ------------------------------------------------------------------------------------------
def test_model_all_equal_is_the_star_from_member_0():
    S = np.full((5, 5), 0.5)
    assert _merges(S) == [(0, 1, 0.5), (0, 2, 0.5), (0, 3, 0.5), (0, 4, 0.5)]                  # (the diagonal is never read)


def test_model_zeros_tie_and_keep_their_sign():
    S = _matrix(4, {(0, 1): -0.0, (0, 2): 0.0, (1, 2): 0.0, (1, 3): -0.0, (2, 3): 0.25})
    S[1, 0], S[2, 0] = 0.0, -0.0                                    # the mirror image of a zero may take the other sign
    a, b, w = model.merges(S)
    assert list(zip(a.tolist(), b.tolist())) == [(2, 3), (0, 1), (0, 2)]      # 0.25 first; the zeros by (a, b); (1, 2) closes a cycle
    assert np.signbit(w).tolist() == [False, True, False]           # the upper triangle's own bytes


def test_model_nan_row_and_blocks_joined_only_by_nan():
    S = np.full((5, 5), 1.0)
    S[2, :] = S[:, 2] = NAN
    S[0, 1] = S[1, 0] = 3.0
    assert _merges(S) == [(0, 1, 3.0), (0, 3, 1.0), (0, 4, 1.0)]    # member 2 is isolated: F = M - 2
    labels, clusters, applied = model.cut(5, *model.merges(S), k=1)
    assert (labels.tolist(), clusters, applied) == ([0, 0, 2, 0, 0], 2, 3)    # never fewer than M - F clusters
    blocks = _matrix(6, {(0, 1): 0.5, (1, 2): 0.75, (3, 4): 0.75, (4, 5): 0.5})
    assert _merges(blocks) == [(1, 2, 0.75), (3, 4, 0.75), (0, 1, 0.5), (4, 5, 0.5)]
    assert model.cut(6, *model.merges(blocks), threshold=-INF)[0].tolist() == [0, 0, 0, 3, 3, 3]


def test_model_infinities_are_ordinary_weights():
    S = _matrix(4, {(0, 1): -INF, (0, 2): INF, (1, 2): -INF, (2, 3): 0.0, (0, 3): -1.0, (1, 3): INF})
    assert _merges(S) == [(0, 2, INF), (1, 3, INF), (2, 3, 0.0)]
    S = _matrix(3, {(0, 1): -INF, (1, 2): -INF})
    assert _merges(S) == [(0, 1, -INF), (1, 2, -INF)]
    assert model.cut(3, *model.merges(S), threshold=-INF)[1:] == (1, 2)


def test_model_cuts_on_a_present_value_and_one_ulp_either_side():
    S = _matrix(5, {(0, 1): 0.9, (1, 2): 0.7, (2, 3): 0.7, (3, 4): 0.1, (0, 4): 0.05})
    a, b, w = model.merges(S)
    assert w.tolist() == [0.9, 0.7, 0.7, 0.1]
    assert model.cut(5, a, b, w, threshold=0.7)[0].tolist() == [0, 0, 0, 0, 4]
    assert model.cut(5, a, b, w, threshold=float(np.nextafter(0.7, 1.0)))[0].tolist() == [0, 0, 2, 3, 4]
    assert model.cut(5, a, b, w, threshold=float(np.nextafter(0.7, 0.0)))[0].tolist() == [0, 0, 0, 0, 4]
    assert model.cut(5, a, b, w, k=1)[1:] == (1, 4) and model.cut(5, a, b, w, k=5)[1:] == (5, 0)
    assert model.cut(5, a, b, w, k=9)[1:] == (5, 0)
    assert model.cut(5, a, b, w, k=3)[0].tolist() == [0, 0, 0, 3, 4]     # of the two merges at 0.7 the order takes (1, 2) first
    assert model.merges(np.zeros((0, 0)))[0].size == 0 and model.merges(np.full((1, 1), NAN))[0].size == 0


@pytest.mark.parametrize("name", ("distinct", "ties", "equal", "chain", "hierarchy", "nan", "inf"))
def test_host_kruskal_is_the_model(name):
    from east import applications
    for M in (0, 1, 2, 3, 17, 64, 65):
        S = model.family(name, M)
        got, want = applications._single_linkage(S), model.merges(S)
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), (name, M)


# ---- the host path of the applications ---------------------------------------------------------------------------------------
class StubAST(object):
    """An AST-like measure without a device: the score of a string in a text = the share of the string's letters the text
    holds, a plain function of the two."""

    def set_text_collection(self, texts, language=None):
        self.texts = [t.decode() if isinstance(t, bytes) else t for t in texts]

    def relevance_table(self, strings, synonimizer=None):
        return np.array([[sum(c in t.upper() for c in s.replace(" ", "")) / float(max(len(s.replace(" ", "")), 1)) for t in self.texts]
                         for s in strings], dtype=np.float64).reshape(len(strings), len(self.texts))


TEXTS = {"fox": "the quick brown fox jumps", "dog": "over the lazy dog", "tree": "suffix trees index every substring",
         "array": "suffix arrays index every suffix", "none": "zzz", "bank": "the river bank near the dog"}
KEYPHRASES = ["quick fox", "lazy dog", "suffix array", "river", "", "quick fox", "index"]


def _same_clustering(found, names, S, threshold=None, k=None):
    a, b, w = model.merges(S)
    assert found.names == names
    assert found.merge_a.tobytes() == a.tobytes() and found.merge_b.tobytes() == b.tobytes() and found.merge_w.tobytes() == w.tobytes()
    assert found.merges == [(names[x], names[y], z) for x, y, z in zip(a.tolist(), b.tolist(), w.tolist())]
    assert all(type(x) is str and type(y) is str and type(z) is float for x, y, z in found.merges)
    if threshold is None and k is None:
        assert found.labels is None and found.clusters is None
        return
    labels = model.cut(len(names), a, b, w, threshold=threshold, k=k)[0].tolist()
    assert found.labels == labels and all(type(x) is int for x in found.labels)
    assert found.clusters == [[names[v] for v in range(len(names)) if labels[v] == root] for root in sorted(set(labels))]


def test_texts_clusters_on_the_host_is_the_model(monkeypatch):
    from east import applications, hip_backend
    monkeypatch.delenv("EAST_HIP_CLUSTERS", raising=False)
    monkeypatch.setattr(hip_backend, "load", lambda: pytest.fail("the host path touched the device library"))
    names = list(TEXTS)
    S = applications._related_on_host(TEXTS, 1, StubAST(), "english")[0]
    assert S.shape == (6, 6) and np.isnan(S.diagonal()).all()
    _same_clustering(applications.texts_clusters(TEXTS, similarity_measure=StubAST()), names, S)
    present = float(model.merges(S)[2][2])
    for t in (present, float(np.nextafter(present, INF)), float(np.nextafter(present, -INF)), -INF, INF):
        _same_clustering(applications.texts_clusters(TEXTS, threshold=t, similarity_measure=StubAST()), names, S, threshold=t)
    for k in (1, 2, 6, 9):
        _same_clustering(applications.texts_clusters(TEXTS, k=k, similarity_measure=StubAST()), names, S, k=k)
    empty = applications.texts_clusters({}, k=2, similarity_measure=StubAST())
    assert (empty.names, empty.merges, empty.labels, empty.clusters) == ([], [], [], [])
    one = applications.texts_clusters({"only": "text"}, k=2, similarity_measure=StubAST())
    assert (one.merges, one.labels, one.clusters) == ([], [0], [["only"]])
    for bad in (dict(threshold=0.5, k=2), dict(threshold=NAN), dict(k=0), dict(k=2.5), dict(k=True)):
        with pytest.raises(ValueError):
            applications.texts_clusters(TEXTS, similarity_measure=StubAST(), **bad)


@pytest.mark.parametrize("by", ("text", "keyphrase"))
def test_keyphrases_clusters_on_the_host_is_the_model(monkeypatch, by):
    from east import applications, hip_backend
    monkeypatch.delenv("EAST_HIP_CLUSTERS", raising=False)
    monkeypatch.setattr(hip_backend, "load", lambda: pytest.fail("the host path touched the device library"))
    wanted = ["quick fox", "lazy dog", "suffix array", "river", "index"]
    names = list(TEXTS) if by == "text" else wanted
    stub = StubAST()
    table = applications.keyphrases_table(wanted, TEXTS, stub)
    scores = np.array([[table[kp][title] for title in TEXTS] for kp in wanted])
    S = applications._similarity_matrix(scores, ("text", "keyphrase").index(by))
    _same_clustering(applications.keyphrases_clusters(KEYPHRASES, TEXTS, by, similarity_measure=stub), names, S)
    _same_clustering(applications.keyphrases_clusters(KEYPHRASES, TEXTS, by, k=2, similarity_measure=stub), names, S, k=2)
    _same_clustering(applications.keyphrases_clusters(KEYPHRASES, TEXTS, by, threshold=0.9, similarity_measure=stub), names, S, threshold=0.9)
    assert applications.keyphrases_clusters(["", ""], TEXTS, by, k=1, similarity_measure=stub).clusters == []
    with pytest.raises(ValueError):
        applications.keyphrases_clusters(KEYPHRASES, TEXTS, "row", k=1, similarity_measure=stub)


def test_where_the_device_is_asked(monkeypatch):
    """The device route is taken when the measure has relevance_clusters, the titles are distinct and EAST_HIP_CLUSTERS is
    not host; the measures over several devices or ranks have none."""
    from east import applications, parallel, relevance
    assert callable(relevance.ASTRelevanceMeasure.relevance_clusters) and callable(relevance.CosineRelevanceMeasure.relevance_clusters)
    assert relevance.MultiDeviceASTRelevanceMeasure.relevance_clusters is None
    assert parallel.DistributedASTRelevanceMeasure.relevance_clusters is None
    asked = []

    class Index(object):
        def clusters_merges(self):
            return np.array([1, 0], dtype=np.int32), np.array([2, 1], dtype=np.int32), np.array([0.5, 0.25])

        def clusters_cut(self, threshold=None, k=None):
            asked.append(("cut", threshold, k))
            return np.array([0, 1, 1], dtype=np.int32), 2, 1

    class Device(StubAST):
        def relevance_clusters(self, prepared_keyphrases=None, axis=None):
            asked.append(("build", prepared_keyphrases, axis))
            return Index()

    texts = {"a": "one", "b": "two", "c": "three"}
    monkeypatch.delenv("EAST_HIP_CLUSTERS", raising=False)
    found = applications.texts_clusters(texts, k=2, similarity_measure=Device())
    assert asked == [("build", None, None), ("cut", None, 2)]
    assert found.merges == [("b", "c", 0.5), ("a", "b", 0.25)] and found.clusters == [["a"], ["b", "c"]]
    del asked[:]
    found = applications.keyphrases_clusters(["x y", "z", "w"], texts, "keyphrase", similarity_measure=Device())
    assert asked == [("build", ["X Y", "Z", "W"], 1)] and found.labels is None
    del asked[:]
    monkeypatch.setenv("EAST_HIP_CLUSTERS", "host")
    applications.texts_clusters(texts, k=2, similarity_measure=Device())
    applications.keyphrases_clusters(["x y", "z"], texts, "text", k=1, similarity_measure=Device(), synonimizer=None)
    monkeypatch.delenv("EAST_HIP_CLUSTERS")

    class Repeated(object):
        def keys(self):
            return ["a", "b", "a"]

        def values(self):
            return ["one", "two", "three"]

    assert applications.texts_clusters(Repeated(), k=1, similarity_measure=Device()).names == ["a", "b", "a"]
    applications.keyphrases_clusters(["x"], texts, "text", k=1, similarity_measure=Device(), synonimizer=object())
    assert asked == []


# ---- formats and to_linkage ----------------------------------------------------------------------------------------------------
def test_format_clusters():
    from east import applications, formatting
    found = applications.Clustering(["a", 'say "b"', "c", "d"], [2, 0], [3, 1], [0.75, 0.5], [0, 0, 2, 2])
    assert formatting.format_clusters(found, "xml") == (
        '<clusters count="2">\n  <cluster id="1" size="2">\n    <member name="a"/>\n    <member name="say "b""/>\n  </cluster>\n'
        '  <cluster id="2" size="2">\n    <member name="c"/>\n    <member name="d"/>\n  </cluster>\n</clusters>\n')
    assert formatting.format_clusters(found, "csv") == '"a",1,"a"\n"say \'b\'",1,"a"\n"c",2,"c"\n"d",2,"c"\n'
    assert formatting.format_clusters(found, "merges") == '"c","d",0.750\n"a","say \'b\'",0.500\n'
    uncut = applications.Clustering(["a", "b"], [0], [1], [0.25])
    assert formatting.format_clusters(uncut, "merges") == '"a","b",0.250\n'
    for fmt in ("xml", "csv", "gml"):
        with pytest.raises(Exception):
            formatting.format_clusters(uncut, fmt)


def test_to_linkage_is_scipys_single_linkage():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    distance = pytest.importorskip("scipy.spatial.distance")
    from east import applications
    for M in (2, 3, 17, 40):
        S = model.family("distinct", M)
        names = ["m%d" % v for v in range(M)]
        found = applications._clustering_of_matrix(names, S, None, None)
        Z = found.to_linkage()
        D = 1.0 - S
        np.fill_diagonal(D, 0.0)
        want = hierarchy.linkage(distance.squareform(D, checks=False), "single")
        assert Z.shape == want.shape == (M - 1, 4)
        assert np.array_equal(Z[:, [0, 1, 3]], want[:, [0, 1, 3]])
        assert np.array_equal(1.0 - Z[:, 2], want[:, 2])               # the similarity stands where SciPy's distance does
    with pytest.raises(ValueError):
        applications._clustering_of_matrix(["a", "b", "c"], _matrix(3, {(0, 1): 1.0}), None, None).to_linkage()


# ---- the command line --------------------------------------------------------------------------------------------------------
def _east(argv):
    from east import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(argv)
    return rc, buf.getvalue()


@pytest.mark.parametrize("command", ("texts", "keyphrases"))
def test_cli_refusals_come_before_any_work(tmp_path, monkeypatch, command):
    from east import main, relevance
    for name in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    touched = []
    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", lambda self, *a, **k: touched.append("measure"))
    monkeypatch.setattr(main, "_read", lambda path: touched.append(path) or b"")
    monkeypatch.setattr(main, "launch_ranks", lambda *a: touched.append("ranks") or 0)
    monkeypatch.setattr("builtins.open", lambda *a, **k: touched.append(a) or pytest.fail("a file was opened"))
    tail = [command, "clusters"] + ([str(tmp_path / "k.txt")] if command == "keyphrases" else []) + [str(tmp_path)]
    cut = ["-k", "2"]
    for bad, word in ((["-r", "0.5", "-k", "2"], "one of the two"), ([], "-f merges"), (["-f", "csv"], "-f merges"),
                      (["-r", "nan"], "nan"), (["-r", "high"], "high"), (["-k", "0"], "'0'"), (["-k", "-1"], "'-1'"),
                      (["-k", "2.5"], "2.5"), (["-k", "two"], "two"), (cut + ["-o", "directed"], "-o directed"),
                      (cut + ["-n", "5"], "-n 5"), (cut + ["-y"], "-y"), (cut + ["-y", "-t", "triples.txt"], "-y"),
                      (cut + ["-v", "lemmata"], "lemmata"), (cut + ["-s", "jaccard"], "jaccard"), (cut + ["-g", "4"], "-g 4"),
                      (cut + ["-g", "x"], "'x'"), (cut + ["-f", "gml"], "gml"), (cut + ["-b", "row"], "row")):
        rc, out = _east(bad + tail)
        assert rc == 1 and out.count("\n") == 1 and word in out, (bad, out)
    if command == "texts":
        rc, out = _east(cut + ["-b", "keyphrase"] + tail)
        assert rc == 1 and out.count("\n") == 1 and "-b keyphrase" in out
    monkeypatch.setenv("EAST_HIP_DEVICES", "2")
    rc, out = _east(cut + tail)
    assert rc == 1 and out.count("\n") == 1 and "-g 2" in out
    monkeypatch.delenv("EAST_HIP_DEVICES")
    monkeypatch.setenv("WORLD_SIZE", "2")
    rc, out = _east(cut + tail)
    assert rc == 1 and out.count("\n") == 1 and "WORLD_SIZE=2" in out
    monkeypatch.setenv("RANK", "1")                                           # (only rank 0 says it)
    assert _east(cut + tail) == (1, "")
    monkeypatch.delenv("RANK")
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("EAST_HIP_FORCE_DIST", "1")
    rc, out = _east(cut + tail)
    assert rc == 1 and out.count("\n") == 1 and "collective" in out
    monkeypatch.delenv("EAST_HIP_FORCE_DIST")
    rc, out = _east(cut + tail[:2])
    assert rc == 1 and "clusters" in out
    assert touched == []
    monkeypatch.undo()
    rc, out = _east(["texts", "alike", str(tmp_path)])
    assert rc == 1 and "'clusters'" in out
    (tmp_path / "k.txt").write_bytes(b"alpha\n")
    rc, out = _east(["keyphrases", "alike", str(tmp_path / "k.txt"), str(tmp_path / "k.txt")])
    assert rc == 1 and "'clusters'" in out
    assert "texts clusters" in main.__doc__ and "keyphrases clusters" in main.__doc__ and "k:" in main._OPTIONS


def test_cli_prints_the_result(tmp_path, monkeypatch, capsys):
    from east import applications, formatting, main, relevance
    for name in ("WORLD_SIZE", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST"):
        monkeypatch.delenv(name, raising=False)
    made = []

    def init(self, *a, **k):
        made.append((type(self).__name__,) + a)
        self.stopwords_source = "given"

    monkeypatch.setattr(relevance.CosineRelevanceMeasure, "__init__", init)
    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "__init__", init)
    (tmp_path / "t.txt").write_bytes(b"one\ntwo\n")
    (tmp_path / "k.txt").write_bytes(b"alpha\nbeta\n")
    seen = []
    result = applications.Clustering(["0", "1"], [0], [1], [0.5], [0, 0])

    monkeypatch.setattr(applications, "texts_clusters", lambda *a: seen.append(("texts",) + a[:3] + (a[4],)) or result)
    monkeypatch.setattr(applications, "keyphrases_clusters", lambda *a: seen.append(("keyphrases",) + a[:5] + (a[7],)) or result)
    texts = str(tmp_path / "t.txt")
    assert main.main(["-k", "1", "texts", "clusters", texts]) == 0
    assert capsys.readouterr().out == formatting.format_clusters(result, "xml") + "\n"
    assert seen[-1] == ("texts", {"0": b"one", "1": b"two"}, None, 1, "english") and made[-1] == ("ASTRelevanceMeasure", "easa", True)
    assert main.main(["-r", "0.25", "-s", "cosine", "-w", "tf", "-v", "words", "-f", "csv", "-l", "german", "texts", "clusters", texts]) == 0
    assert capsys.readouterr().out == formatting.format_clusters(result, "csv") + "\n"
    assert seen[-1][2:] == (0.25, None, "german") and made[-1] == ("CosineRelevanceMeasure", "words", "tf")
    assert main.main(["-f", "merges", "-d", "-b", "keyphrase", "keyphrases", "clusters", str(tmp_path / "k.txt"), texts]) == 0
    assert capsys.readouterr().out == formatting.format_clusters(result, "merges") + "\n"
    assert seen[-1] == ("keyphrases", ["alpha", "beta"], {"0": b"one", "1": b"two"}, "keyphrase", None, None, "english")
    assert made[-1] == ("ASTRelevanceMeasure", "easa", False)


# ---- the binding -------------------------------------------------------------------------------------------------------------
def test_binding_against_the_header():
    """Every entry point of the clusters is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        text = f.read()
    assert "Clusters (`east texts clusters`" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["east_hip_clusters_build_resident", "east_hip_clusters_build_host", "east_hip_clusters_fetch",
             "east_hip_clusters_cut_threshold", "east_hip_clusters_cut_count", "east_hip_last_clusters_ms"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp,
                "int32_t *": hip_backend._c_i32p, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
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
    assert lib.east_hip_last_clusters_ms(None) == -1.0
    assert lib.east_hip_clusters_fetch(None, None, None, None) == invalid
    assert lib.east_hip_clusters_build_resident(None, hip_backend.GRAPH_SOURCE_SIMILARITY, None) == invalid
    assert lib.east_hip_clusters_build_host(None, None, 0, None) == invalid
    assert lib.east_hip_clusters_cut_threshold(None, 0.5, None, None) == invalid
    assert lib.east_hip_clusters_cut_count(None, 1, None, None) == invalid
    for cls in (hip_backend.HipIndex, hip_backend.HipCosineIndex):
        for method in ("clusters_build", "clusters_build_host", "clusters_merges", "clusters_cut"):
            assert callable(getattr(cls, method)), (cls, method)
        assert isinstance(cls.last_clusters_ms, property)
    kernel = open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "clusters.h")).read()
    assert "SLOT_CLU" in kernel and "SLOT_CLU" in open(os.path.join(ROOT, "ast-text-analysis_amd", "csrc", "handle.h")).read()
    assert hip_backend.CLUSTERS_INFO_FIELDS == ("members", "merges", "rounds", "launches")


def test_the_three_linkages_share_one_frame():
    """clusters.h and linkage.h define the ten kernels; what single, complete and average linkage share is written once.  The
    one exception is counted as such: the rank counting loop stands in both *_rank_kernel, because as one template over the slot
    clu_rank_kernel measured about 1 % slower than its own body in three forms ("One frame for the three linkages")."""
    csrc = os.path.join(ROOT, "ast-text-analysis_amd", "csrc")
    both = open(os.path.join(csrc, "clusters.h")).read() + open(os.path.join(csrc, "linkage.h")).read()
    for kernel in ("clu_best_kernel", "clu_pick_kernel", "clu_merge_kernel", "clu_rank_kernel", "clu_symmetry_kernel",
                   "lnk_copy_kernel", "lnk_best_kernel", "lnk_pair_kernel", "lnk_update_kernel", "lnk_rank_kernel"):
        assert len(re.findall(r"__global__ __launch_bounds__\(BLOCK\) void %s\(" % kernel, both)) == 1, kernel
    assert both.count("for (u32 t = wv * 64u; t < wv * 64u + 64u; t++)") == 2, "the rank counting loop: the two rank kernels, nowhere else"
    once = {"the row-maximum loop": "for (u32 j0 = 0; j0 < M; j0 += 64u * CLU_UNROLL)",
            "the lanes' reduction of the row maximum": "ow == best && oj < best_j",
            "the tile minimum": "lds8[wv] = worst",
            "the tile read-back": "hipMemcpyAsync(host.data(), bad,",
            "the limit of the tiles": "more tiles than one launch takes",
            "the merge fetch": "hipMemcpyAsync(g.merge_w.data(), mw,",
            "the closing of a build": "out[3] = g.launches",
            "the upload": "consumer_upload<ClustersState>(",
            "the resident front": "consumer_resident_square<ClustersState>("}
    for what, line in once.items():
        assert both.count(line) == 1, what
    assert set(re.findall(r"EAST_HIP_GRAPH_SOURCE_\w+", both)) <= {"EAST_HIP_GRAPH_SOURCE_UPLOADED"}      # the frame knows the sources
    for entry in ("east_hip_clusters_build_resident", "east_hip_clusters_build_host", "east_hip_clusters_build_resident_linkage",
                  "east_hip_clusters_build_host_linkage"):
        assert len(re.findall(r"\bint %s\(" % entry, both)) == 1, entry
