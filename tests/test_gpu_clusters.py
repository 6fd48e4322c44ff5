"""GPU tier: single-linkage clusters on the device (csrc/clusters.h; include/east_hip.h, "Clusters").  Every case compares
the merges the C ABI gives with tests/clusters_exact.py byte for byte, and both cuts at several thresholds and counts.

The sizes are the edges of what the kernels choose: a wavefront's 64 columns, the 64 slots a workgroup ranks and the 64 x 64
tiles of the symmetry check (63, 64, 65), the 256 slots of a ranking tile and of a pass of the one-workgroup kernel (255, 256,
257), the 512 columns a wavefront has in flight twice over and one more (1 025), several of everything (2 049), and the sizes
without a launch (0, 1)."""
import numpy as np
import pytest

import clusters_exact as model

pytestmark = pytest.mark.gpu

INF = float("inf")

CASES = [("distinct", M) for M in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 2049)] + [
    ("ties", 65), ("ties", 257), ("ties", 1025),
    ("equal", 3), ("equal", 64), ("equal", 1025),
    ("chain", 63), ("chain", 257), ("chain", 1025),
    ("hierarchy", 64), ("hierarchy", 255), ("hierarchy", 1025),
    ("nan", 65), ("nan", 256), ("nan", 1025),
    ("inf", 3), ("inf", 63), ("inf", 257)]


@pytest.fixture(scope="module")
def index(hip):
    index = hip.HipIndex()
    yield index
    index.close()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def _check_cuts(index, M, want):
    a, b, w = want
    F = len(a)
    thresholds = [-INF, INF, 0.0]
    if F:
        present = float(w[F // 2])
        thresholds += [present, float(np.nextafter(present, INF)), float(np.nextafter(present, -INF)), float(w[0]), float(w[-1])]
    for t in thresholds:
        labels, clusters, applied = index.clusters_cut(threshold=t)
        ml, mc, mn = model.cut(M, a, b, w, threshold=t)
        assert (clusters, applied) == (mc, mn), t
        assert labels.dtype == np.int32 and labels.tobytes() == ml.tobytes(), t
    for k in sorted({1, 2, max(M // 2, 1), max(M - F, 1), max(M - 1, 1), max(M, 1), M + 5}):
        labels, clusters, applied = index.clusters_cut(k=k)
        ml, mc, mn = model.cut(M, a, b, w, k=k)
        assert (clusters, applied) == (mc, mn), k
        assert labels.tobytes() == ml.tobytes(), k
        assert clusters >= M - F


def _check_matrix(index, S, resident=None):
    """Clusters of the host array S (uploaded), or of the resident source whose fetched bytes are S."""
    M = S.shape[0]
    info = index.clusters_build(resident) if resident is not None else index.clusters_build_host(S)
    want = model.merges(S)
    assert info["members"] == M and info["merges"] == len(want[0])
    assert info["rounds"] <= max(M - 1, 0).bit_length() + 1        # ceil(log2 M) rounds that merge, one that may find nothing
    assert info["launches"] == 3 * info["rounds"] + (1 if len(want[0]) else 0) + (1 if resident is None and M >= 2 else 0)
    _same(index.clusters_merges(), want)
    _check_cuts(index, M, want)
    assert index.last_clusters_ms >= 0.0
    return info, want


@pytest.mark.parametrize("name,M", CASES)
def test_families(index, name, M):
    S = model.family(name, M)
    info, want = _check_matrix(index, S)
    if name == "equal":
        assert want[0].tolist() == [0] * (M - 1) and want[1].tolist() == list(range(1, M))     # the star from member 0
    if name == "chain":
        assert info["rounds"] == 1 and want[2].tolist() == [float(M - i) for i in range(M - 1)]
    if name == "hierarchy":
        assert info["rounds"] >= M.bit_length() - 1                   # the cluster of member 0 doubles a round, no faster
    if name == "nan":
        assert info["merges"] < M - 3                                # the all-NaN rows are clusters of their own


def test_the_sign_of_a_zero_comes_back(index):
    nan = float("nan")
    S = np.array([[nan, -0.0, 0.0, -1.0], [0.0, nan, nan, -0.0], [-0.0, nan, nan, nan], [-1.0, 0.0, nan, nan]])
    index.clusters_build_host(S)
    a, b, w = index.clusters_merges()
    assert (a.tolist(), b.tolist()) == ([0, 0, 1], [1, 2, 3])      # three zeros tie: by (a, b)
    assert np.signbit(w).tolist() == [True, False, True]            # the upper triangle's own bytes
    _same((a, b, w), model.merges(S))


def test_uploaded_copy_is_a_source_and_builds_repeat(index, hip):
    S = model.family("ties", 257)
    _, want = _check_matrix(index, S)
    first = [x.tobytes() for x in index.clusters_merges()]
    info = index.clusters_build(hip.GRAPH_SOURCE_UPLOADED)          # the clusters' own copy: no upload, no symmetry check
    assert info["launches"] == 3 * info["rounds"] + 1
    assert [x.tobytes() for x in index.clusters_merges()] == first
    other = hip.HipIndex()                                          # another handle, another build
    other.clusters_build_host(S)
    assert [x.tobytes() for x in other.clusters_merges()] == first
    other.close()


def test_asymmetric_upload_is_refused_with_the_pair(index, hip):
    lib = hip.load()
    good = model.family("distinct", 130)
    index.clusters_build_host(good)
    for value in (0.5, np.nan):
        bad = good.copy()
        bad[70, 3] = value                                         # (3, 70) is the first pair in row-major order ...
        bad[129, 100] = value                                      # ... (100, 129) the second
        with pytest.raises(hip.exceptions.HipBackendError) as e:
            index.clusters_build_host(bad)
        assert "S[3][70]" in str(e.value) and "code -2" in str(e.value)
        for call in (index.clusters_merges, lambda: index.clusters_cut(k=1), lambda: index.clusters_build(hip.GRAPH_SOURCE_UPLOADED)):
            with pytest.raises(hip.exceptions.HipBackendError) as e:
                call()
            assert "code -6" in str(e.value)
        assert lib.east_hip_last_clusters_ms(index._h) == -1.0
        index.clusters_build_host(good)
    zeros = good.copy()
    zeros[3, 70], zeros[70, 3] = 0.0, -0.0                          # +0.0 against -0.0 is symmetric
    _check_matrix(index, zeros)


def test_arguments(index, hip):
    index.clusters_build_host(model.family("distinct", 3))
    for call in (lambda: index.clusters_cut(threshold=float("nan")), lambda: index.clusters_cut(k=0), lambda: index.clusters_cut(k=-3),
                 lambda: index.clusters_build(hip.GRAPH_SOURCE_AST), lambda: index.clusters_build(hip.GRAPH_SOURCE_COSINE),
                 lambda: index.clusters_build(17)):
        with pytest.raises(hip.exceptions.HipBackendError) as e:
            call()
        assert "code -2" in str(e.value)
    _same(index.clusters_merges(), model.merges(model.family("distinct", 3)))     # a refused call leaves the clusters alone
    fresh = hip.HipIndex()
    for call in (fresh.clusters_merges, lambda: fresh.clusters_cut(k=1), lambda: fresh.clusters_build(hip.GRAPH_SOURCE_UPLOADED),
                 lambda: fresh.clusters_build(hip.GRAPH_SOURCE_SIMILARITY), lambda: fresh.clusters_build(hip.GRAPH_SOURCE_RELATED),
                 lambda: fresh.clusters_build(hip.GRAPH_SOURCE_COSINE_TEXTS)):
        with pytest.raises(hip.exceptions.HipBackendError) as e:
            call()
        assert "code -6" in str(e.value)
    assert fresh.last_clusters_ms == -1.0
    fresh.close()


# ---- resident sources ------------------------------------------------------------------------------------------------------
WORDS = ("suffix tree array text index cluster group merge forest edge graph vertex round kernel matrix cosine river bank "
         "quick brown lazy dog fox jumps over near today annotated relevance measure keyphrase document").split()


def _texts(D, seed):
    rng = np.random.RandomState(seed)
    return {"text %d" % d: " ".join(rng.choice(WORDS, size=rng.randint(6, 15)).tolist()) for d in range(D)}


KEYPHRASES = ["suffix tree", "cosine matrix", "quick fox", "river bank", "annotated suffix array", "lazy dog", "merge forest",
              "keyphrase relevance", "nothing here"]


@pytest.fixture(scope="module")
def ast_measure(hip):
    from east import relevance
    measure = relevance.ASTRelevanceMeasure("easa", True, device=0)
    measure.set_text_collection(list(_texts(70, 1).values()))
    yield measure
    measure.index.close()


@pytest.mark.parametrize("by", ("text", "keyphrase"))
def test_similarity_matrix_is_a_source(ast_measure, hip, by):
    from east import utils
    axis = ("text", "keyphrase").index(by)
    index = ast_measure.relevance_clusters([utils.prepare_text(kp) for kp in KEYPHRASES], axis)
    matrix, _ = index.similarity_matrix()
    assert matrix.shape[0] == (70 if by == "text" else len(KEYPHRASES))
    _check_matrix(index, matrix, hip.GRAPH_SOURCE_SIMILARITY)
    before = index.rank_similarity(5)
    index.clusters_build(hip.GRAPH_SOURCE_SIMILARITY)
    after = index.rank_similarity(5)                               # the ranking of the same matrix is unchanged
    assert [getattr(before, n).tobytes() for n in before.__slots__] == [getattr(after, n).tobytes() for n in after.__slots__]


def test_relatedness_is_a_source_symmetric_only(ast_measure, hip):
    index = ast_measure.relevance_clusters()
    matrix, _, _ = index.related_matrix()
    _, want = _check_matrix(index, matrix, hip.GRAPH_SOURCE_RELATED)
    index.related_build(True, hip.RELATED_DIRECTED)
    _same(index.clusters_merges(), want)                            # finished clusters outlive a rebuild of their source
    with pytest.raises(hip.exceptions.HipBackendError) as e:
        index.clusters_build(hip.GRAPH_SOURCE_RELATED)
    assert "directed" in str(e.value) and "code -2" in str(e.value)


def test_text_cosine_is_a_source_and_reset_releases(hip):
    from east import relevance
    measure = relevance.CosineRelevanceMeasure("words", "tf-idf", device=0, stopwords=())
    measure.set_text_collection(list(_texts(66, 2).values()))
    index = measure.relevance_clusters()
    matrix, _, _ = index.texts_matrix()
    _, want = _check_matrix(index, matrix, hip.GRAPH_SOURCE_COSINE_TEXTS)
    measure.set_text_collection(list(_texts(9, 3).values()))       # the source is withdrawn; the clusters are the host's
    _same(index.clusters_merges(), want)
    assert hip.load().east_hip_reset(index._h) == 0
    with pytest.raises(hip.exceptions.HipBackendError) as e:
        index.clusters_merges()
    assert "code -6" in str(e.value)
    index.close()


# ---- the applications on the device ----------------------------------------------------------------------------------------
def _check_clustering(found, names, matrix, threshold=None, k=None):
    a, b, w = model.merges(matrix)
    assert found.names == names
    assert found.merge_a.tobytes() == a.tobytes() and found.merge_b.tobytes() == b.tobytes() and found.merge_w.tobytes() == w.tobytes()
    assert found.merges == [(names[x], names[y], z) for x, y, z in zip(a.tolist(), b.tolist(), w.tolist())]
    if threshold is None and k is None:
        assert found.labels is None and found.clusters is None
        return
    labels = model.cut(len(names), a, b, w, threshold=threshold, k=k)[0].tolist()
    assert found.labels == labels
    assert found.clusters == [[names[v] for v in range(len(names)) if labels[v] == root] for root in sorted(set(labels))]


def test_applications_on_the_device(hip, monkeypatch):
    from east import applications, relevance
    monkeypatch.delenv("EAST_HIP_CLUSTERS", raising=False)
    texts = _texts(12, 4)
    names = list(texts)
    ast = relevance.ASTRelevanceMeasure("easa", True, device=0)
    found = applications.texts_clusters(texts, k=3, similarity_measure=ast)
    _check_clustering(found, names, ast.index.related_matrix()[0], k=3)
    assert len(found.clusters) == 3 and found.to_linkage().shape == (11, 4)
    middle = found.merge_w[5]
    found = applications.texts_clusters(texts, threshold=middle, similarity_measure=ast)
    _check_clustering(found, names, ast.index.related_matrix()[0], threshold=float(middle))
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="keyphrase", similarity_measure=ast)
    _check_clustering(found, KEYPHRASES, ast.index.similarity_matrix()[0])
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="text", threshold=0.5, similarity_measure=ast)
    _check_clustering(found, names, ast.index.similarity_matrix()[0], threshold=0.5)
    ast.index.close()
    cos = relevance.CosineRelevanceMeasure("words", "tf", device=0, stopwords=())
    found = applications.texts_clusters(texts, k=1, similarity_measure=cos)
    _check_clustering(found, names, cos.index.texts_matrix()[0], k=1)
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="text", k=4, similarity_measure=cos)
    _check_clustering(found, names, cos.index.similarity_matrix()[0], k=4)
    cos.index.close()
