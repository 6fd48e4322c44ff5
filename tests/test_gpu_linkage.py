"""GPU tier: complete and average linkage on the device (csrc/linkage.h; include/east_hip.h, "Clusters").  Every case compares
the merges the C ABI gives with tests/linkage_exact.py byte for byte, both cuts, the number of rounds and the launches.

The sizes are the edges of what the kernels choose: a wavefront's 64 columns, the 64 slots a workgroup ranks and the 64 x 64
tiles of the copy (63, 64, 65), the 256 slots of a ranking tile and of a pass of the one-workgroup kernel (255, 256, 257),
the 512 columns a wavefront has in flight twice over and one more (1 025), and the sizes without a launch (0, 1)."""
import numpy as np
import pytest

import clusters_exact
import linkage_exact as model

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")

CASES = [("distinct", M) for M in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)] + [
    ("ties", 65), ("ties", 257), ("equal", 3), ("equal", 64), ("equal", 257), ("chain", 63), ("chain", 257),
    ("hierarchy", 64), ("hierarchy", 255), ("zero_plateau", 65), ("zero_plateau", 257), ("dyadic", 130)]


@pytest.fixture(scope="module")
def index(hip):
    index = hip.HipIndex()
    yield index
    index.close()


_MODEL = {}


def _want(name, M, linkage):
    """The family's matrix and the model's result, computed once."""
    key = (name, M, linkage)
    if key not in _MODEL:
        S = model.family(name, M)
        _MODEL[key] = (S, model.rounds(S, linkage))
    return _MODEL[key]


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
        ml, mc, mn = clusters_exact.cut(M, a, b, w, threshold=t)
        assert (clusters, applied) == (mc, mn), t
        assert labels.dtype == np.int32 and labels.tobytes() == ml.tobytes(), t
    for k in sorted({1, 2, max(M // 2, 1), max(M - 1, 1), max(M, 1), M + 5}):
        labels, clusters, applied = index.clusters_cut(k=k)
        ml, mc, mn = clusters_exact.cut(M, a, b, w, k=k)
        assert (clusters, applied) == (mc, mn), k
        assert labels.tobytes() == ml.tobytes(), k


def _launches(M, rounds, merges, uploaded, probe=0):
    """Three a round; the symmetry check of an upload, the copy, the two launches of a round that found no pair at the floor
    (it launches no update), the ranking."""
    if M < 2:
        return 0
    return 3 * rounds + 2 * probe + 1 + (1 if uploaded else 0) + (1 if merges else 0)


def _check_matrix(index, S, linkage, want, resident=None):
    M = S.shape[0]
    info = index.clusters_build(resident, linkage) if resident is not None else index.clusters_build_host(S, linkage)
    assert info["members"] == M and info["merges"] == len(want[0]) == max(M - 1, 0)
    assert info["rounds"] == want[3]
    assert info["launches"] == _launches(M, want[3], len(want[0]), resident is None)
    _same(index.clusters_merges(), want[:3])
    _check_cuts(index, M, want[:3])
    assert index.last_clusters_ms >= 0.0
    return info


@pytest.mark.parametrize("linkage", model.LINKAGES)
@pytest.mark.parametrize("name,M", CASES)
def test_families(index, name, M, linkage):
    S, want = _want(name, M, linkage)
    info = _check_matrix(index, S, linkage, want)
    if name == "equal":
        assert info["rounds"] == M - 1                             # the worst case: one pair a round
        assert want[0].tolist() == [0] * (M - 1) and want[1].tolist() == list(range(1, M))


@pytest.mark.parametrize("M", (3, 63, 257))
def test_infinities_are_weights_of_complete_linkage(index, M):
    S, want = _want("inf", M, "complete")
    _check_matrix(index, S, "complete", want)


@pytest.mark.parametrize("linkage", model.LINKAGES)
def test_the_sign_of_a_zero_comes_back(index, linkage):
    S = np.array([[NAN, -0.0, 0.0], [0.0, NAN, -0.0], [-0.0, 0.0, NAN]])
    index.clusters_build_host(S, linkage)
    a, b, w = index.clusters_merges()
    assert (a.tolist(), b.tolist(), np.signbit(w).tolist()) == ([0, 0], [1, 2], [True, False])
    _same((a, b, w), model.merges(S, linkage))


@pytest.mark.parametrize("linkage", model.LINKAGES)
@pytest.mark.parametrize("name,M", (("distinct", 257), ("zero_plateau", 257), ("ties", 65)))
def test_a_floor_is_the_prefix(index, name, M, linkage):
    S, full = _want(name, M, linkage)
    w = full[2]
    present = float(w[len(w) // 2])
    for floor in (present, float(np.nextafter(present, INF)), float(np.nextafter(present, -INF)), INF, -INF, float(w[0]), float(w[-1])):
        n = clusters_exact.applied_by_threshold(w, floor)
        want = model.rounds(S, linkage, floor)
        assert [x.tobytes() for x in want[:3]] == [x[:n].tobytes() for x in full[:3]]
        info = index.clusters_build_host(S, linkage, floor)
        assert (info["merges"], info["rounds"]) == (n, want[3]), floor
        assert info["launches"] == _launches(M, want[3], n, True, probe=0 if n == M - 1 else 1), floor
        _same(index.clusters_merges(), want[:3])
        labels, clusters, applied = index.clusters_cut(threshold=-INF)
        assert (clusters, applied) == (M - n, n)
        assert labels.tobytes() == clusters_exact.labels_after(M, want[0], want[1], n).tobytes()


def _refused(index, hip, call, words, uploaded_gone):
    with pytest.raises(hip.exceptions.HipBackendError) as e:
        call()
    for word in words + ("code -2",):
        assert word in str(e.value), str(e.value)
    gone = [index.clusters_merges, lambda: index.clusters_cut(k=1)]
    if uploaded_gone:
        gone.append(lambda: index.clusters_build(hip.GRAPH_SOURCE_UPLOADED, "complete"))
    for after in gone:
        with pytest.raises(hip.exceptions.HipBackendError) as e:
            after()
        assert "code -6" in str(e.value)
    assert hip.load().east_hip_last_clusters_ms(index._h) == -1.0


def test_refusals_name_the_pair_and_leave_nothing(index, hip):
    good = model.family("distinct", 130)
    for linkage, value in (("complete", NAN), ("average", NAN), ("average", INF), ("average", -INF)):
        bad = good.copy()
        bad[3, 70] = bad[70, 3] = value                            # (3, 70) is the first pair in row-major order ...
        bad[100, 129] = bad[129, 100] = value                      # ... (100, 129) the second
        index.clusters_build_host(good, linkage)
        _refused(index, hip, lambda: index.clusters_build_host(bad, linkage), ("S[3][70]", linkage), True)
    for linkage in model.LINKAGES:
        bad = good.copy()
        bad[70, 3] = 0.5
        index.clusters_build_host(good, linkage)
        _refused(index, hip, lambda: index.clusters_build_host(bad, linkage), ("S[3][70]", "symmetric"), True)
    for linkage in (3, -1, 99):
        index.clusters_build_host(good, "average")
        _refused(index, hip, lambda: index.clusters_build_host(good, linkage), ("linkage",), False)
        index.clusters_build_host(good, "average")
        _refused(index, hip, lambda: index.clusters_build(hip.GRAPH_SOURCE_UPLOADED, linkage), ("linkage",), False)
    for linkage in model.LINKAGES:
        for source in (hip.GRAPH_SOURCE_AST, hip.GRAPH_SOURCE_COSINE, 17):
            with pytest.raises(hip.exceptions.HipBackendError) as e:
                index.clusters_build(source, linkage)
            assert "code -2" in str(e.value)
    infinite = good.copy()
    infinite[3, 70] = infinite[70, 3] = INF                        # an ordinary weight of complete linkage
    _check_matrix(index, infinite, "complete", model.rounds(infinite, "complete"))


def test_single_through_the_new_entry_point_is_the_old_build(index, hip):
    lib = hip.load()
    S = np.ascontiguousarray(clusters_exact.family("nan", 256))
    old_info = index.clusters_build_host(S)
    old = index.clusters_merges()
    _same(old, clusters_exact.merges(S))
    out = np.zeros(4, dtype=np.int64)
    matrix = S.ctypes.data_as(hip._c_dblp)
    assert lib.east_hip_clusters_build_host_linkage(index._h, matrix, 256, hip.LINKAGE_SINGLE, NAN, out.ctypes.data_as(hip._c_i64p)) == 0
    assert dict(zip(hip.CLUSTERS_INFO_FIELDS, out.tolist())) == old_info
    _same(index.clusters_merges(), old)
    assert lib.east_hip_clusters_build_resident_linkage(index._h, hip.GRAPH_SOURCE_UPLOADED, hip.LINKAGE_SINGLE, NAN,
                                                        out.ctypes.data_as(hip._c_i64p)) == 0
    assert out[1] == old_info["merges"]
    _same(index.clusters_merges(), old)
    floor = float(old[2][100])
    n = clusters_exact.applied_by_threshold(old[2], floor)
    info = index.clusters_build_host(S, "single", floor)           # a floor keeps the prefix
    assert info["merges"] == n < len(old[0])
    _same(index.clusters_merges(), tuple(x[:n] for x in old))
    assert index.clusters_cut(threshold=-INF)[1:] == (256 - n, n)


@pytest.mark.parametrize("linkage", model.LINKAGES)
def test_builds_repeat_and_the_uploaded_copy_is_a_source(index, hip, linkage):
    S, want = _want("ties", 257, linkage)
    _check_matrix(index, S, linkage, want)
    first = [x.tobytes() for x in index.clusters_merges()]
    _check_matrix(index, S, linkage, want, hip.GRAPH_SOURCE_UPLOADED)          # the clusters' own copy, unchanged by the build before
    other = hip.HipIndex()                                          # another handle, another build
    other.clusters_build_host(S, linkage)
    assert [x.tobytes() for x in other.clusters_merges()] == first
    other.close()


# ---- resident sources ------------------------------------------------------------------------------------------------------
WORDS = ("suffix tree array text index cluster group merge forest edge graph vertex round kernel matrix cosine river bank "
         "quick brown lazy dog fox jumps over near today annotated relevance measure keyphrase document").split()


def _texts(D, seed):
    rng = np.random.RandomState(seed)
    return {"text %d" % d: " ".join(rng.choice(WORDS, size=rng.randint(6, 15)).tolist()) for d in range(D)}


KEYPHRASES = ["suffix tree", "cosine matrix", "quick fox", "river bank", "annotated suffix array", "lazy dog", "merge forest",
              "keyphrase relevance"]


@pytest.fixture(scope="module")
def ast_measure(hip):
    from east import relevance
    measure = relevance.ASTRelevanceMeasure("easa", True, device=0)
    measure.set_text_collection(list(_texts(70, 1).values()))
    yield measure
    measure.index.close()


def _check_resident(index, matrix, source, linkage):
    assert model.refused(matrix, linkage) is None
    _check_matrix(index, matrix, linkage, model.rounds(matrix, linkage), source)


@pytest.mark.parametrize("linkage", model.LINKAGES)
@pytest.mark.parametrize("by", ("text", "keyphrase"))
def test_similarity_matrix_is_a_source_and_stays_as_it_is(ast_measure, hip, by, linkage):
    from east import utils
    axis = ("text", "keyphrase").index(by)
    index = ast_measure.relevance_clusters([utils.prepare_text(kp) for kp in KEYPHRASES], axis, linkage)
    matrix, _ = index.similarity_matrix()
    assert matrix.shape[0] == (70 if by == "text" else len(KEYPHRASES))
    before = index.rank_similarity(5)
    _check_resident(index, matrix, hip.GRAPH_SOURCE_SIMILARITY, linkage)
    after = index.rank_similarity(5)                               # the source matrix is never written
    assert [getattr(before, n).tobytes() for n in before.__slots__] == [getattr(after, n).tobytes() for n in after.__slots__]
    assert index.similarity_matrix()[0].tobytes() == matrix.tobytes()


@pytest.mark.parametrize("linkage", model.LINKAGES)
def test_relatedness_is_a_source_symmetric_only(ast_measure, hip, linkage):
    index = ast_measure.relevance_clusters(linkage=linkage)
    matrix, _, _ = index.related_matrix()
    _check_resident(index, matrix, hip.GRAPH_SOURCE_RELATED, linkage)
    want = [x.tobytes() for x in index.clusters_merges()]
    index.related_build(True, hip.RELATED_DIRECTED)
    assert [x.tobytes() for x in index.clusters_merges()] == want  # finished clusters outlive a rebuild of their source
    with pytest.raises(hip.exceptions.HipBackendError) as e:
        index.clusters_build(hip.GRAPH_SOURCE_RELATED, linkage)
    assert "directed" in str(e.value) and "code -2" in str(e.value)


@pytest.mark.parametrize("linkage", model.LINKAGES)
def test_text_cosine_is_a_source_and_reset_releases(hip, linkage):
    from east import relevance
    measure = relevance.CosineRelevanceMeasure("words", "tf-idf", device=0, stopwords=())
    measure.set_text_collection(list(_texts(66, 2).values()))
    index = measure.relevance_clusters(linkage=linkage)
    matrix, _, _ = index.texts_matrix()
    _check_resident(index, matrix, hip.GRAPH_SOURCE_COSINE_TEXTS, linkage)
    want = [x.tobytes() for x in index.clusters_merges()]
    measure.set_text_collection(list(_texts(9, 3).values()))       # the source is withdrawn; the clusters are the host's
    assert [x.tobytes() for x in index.clusters_merges()] == want
    assert hip.load().east_hip_reset(index._h) == 0
    with pytest.raises(hip.exceptions.HipBackendError) as e:
        index.clusters_merges()
    assert "code -6" in str(e.value)
    index.close()


# ---- the applications on the device ----------------------------------------------------------------------------------------
def _check_clustering(found, names, matrix, linkage, threshold=None, k=None):
    assert model.refused(matrix, linkage) is None
    a, b, w = model.merges(matrix, linkage, threshold)
    assert found.names == names and found.linkage == linkage
    assert found.merge_a.tobytes() == a.tobytes() and found.merge_b.tobytes() == b.tobytes() and found.merge_w.tobytes() == w.tobytes()
    if threshold is None and k is None:
        assert found.labels is None and found.clusters is None
        return
    labels = clusters_exact.cut(len(names), a, b, w, threshold=threshold, k=k)[0].tolist()
    assert found.labels == labels
    assert found.clusters == [[names[v] for v in range(len(names)) if labels[v] == root] for root in sorted(set(labels))]


@pytest.mark.parametrize("linkage", model.LINKAGES)
def test_applications_on_the_device(hip, monkeypatch, linkage):
    from east import applications, relevance
    monkeypatch.delenv("EAST_HIP_CLUSTERS", raising=False)
    texts = _texts(12, 4)
    names = list(texts)
    ast = relevance.ASTRelevanceMeasure("easa", True, device=0)
    found = applications.texts_clusters(texts, k=3, similarity_measure=ast, linkage=linkage)
    _check_clustering(found, names, ast.index.related_matrix()[0], linkage, k=3)
    assert len(found.clusters) == 3 and found.to_linkage().shape == (11, 4)
    middle = float(found.merge_w[5])
    found = applications.texts_clusters(texts, threshold=middle, similarity_measure=ast, linkage=linkage)
    _check_clustering(found, names, ast.index.related_matrix()[0], linkage, threshold=middle)
    assert 0 < len(found.merge_w) < 11                              # the floor: the dendrogram ends at the threshold
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="keyphrase", similarity_measure=ast, linkage=linkage)
    _check_clustering(found, KEYPHRASES, ast.index.similarity_matrix()[0], linkage)
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="text", threshold=0.5, similarity_measure=ast, linkage=linkage)
    _check_clustering(found, names, ast.index.similarity_matrix()[0], linkage, threshold=0.5)
    ast.index.close()
    cos = relevance.CosineRelevanceMeasure("words", "tf", device=0, stopwords=())
    found = applications.texts_clusters(texts, k=1, similarity_measure=cos, linkage=linkage)
    _check_clustering(found, names, cos.index.texts_matrix()[0], linkage, k=1)
    found = applications.keyphrases_clusters(KEYPHRASES, texts, by="text", k=4, similarity_measure=cos, linkage=linkage)
    _check_clustering(found, names, cos.index.similarity_matrix()[0], linkage, k=4)
    cos.index.close()
