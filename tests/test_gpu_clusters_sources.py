"""GPU tier: what the four build entry points of the clusters say of their source, word for word (csrc/clusters.h:
clusters_entry_resident, clusters_entry_host; csrc/consumer.h: consumer_resident_square).  Both resident entry points -- the
newer one under each linkage -- refuse the same sources with the same code and the same line of east_hip_last_error() and
leave the last result as it was; each of the four matrix sources, built symmetric, clusters through both; both host entry
points treat no members, a bad size and an asymmetric matrix alike.  The lines are literals: what the library said before
the entry points had one body."""
import numpy as np
import pytest

import clusters_exact
import linkage_exact

pytestmark = pytest.mark.gpu

NAN = float("nan")
OK, INVALID, NOT_BUILT = 0, -2, -6
LINKAGES = ("single", "complete", "average")
ENTRIES = [None, 0, 1, 2]                       # east_hip_clusters_build_*: the older entry point, the newer one with each linkage
ENTRY_IDS = ["old"] + ["linkage-%s" % name for name in LINKAGES]

TEXTS = ["the quick brown fox jumps over the lazy dog near the river bank",
         "a lazy dog sleeps near the river bank while the quick fox jumps",
         "suffix trees index every substring of the text in linear space",
         "suffix arrays index every substring of the text in less memory",
         "the river bank floods when the quick brown river rises over the lazy dog"]
KEYPHRASES = ["quick fox", "lazy dog", "suffix index", "river bank", "every substring", "brown river"]

NOT_SQUARE = "clusters: the source is not a square matrix of members"


def _resident(hip, index, entry, source):
    """-> (code, the line of east_hip_last_error(), out)"""
    lib, out = hip.load(), np.zeros(4, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)
    if entry is None:
        rc = lib.east_hip_clusters_build_resident(index._h, source, p_out)
    else:
        rc = lib.east_hip_clusters_build_resident_linkage(index._h, source, entry, NAN, p_out)
    return rc, lib.east_hip_last_error().decode() if rc else "", out.tolist()


def _host(hip, index, entry, matrix, m):
    lib, out = hip.load(), np.zeros(4, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)
    pointer = matrix.ctypes.data_as(hip._c_dblp) if matrix is not None else None
    if entry is None:
        rc = lib.east_hip_clusters_build_host(index._h, pointer, m, p_out)
    else:
        rc = lib.east_hip_clusters_build_host_linkage(index._h, pointer, m, entry, NAN, p_out)
    return rc, lib.east_hip_last_error().decode() if rc else "", out.tolist()


def _fetch(hip, index, merges):
    """-> (code, the bytes of the three lists)"""
    a, b, w = np.zeros(merges, dtype=np.int32), np.zeros(merges, dtype=np.int32), np.zeros(merges, dtype=np.float64)
    rc = hip.load().east_hip_clusters_fetch(index._h, a.ctypes.data_as(hip._c_i32p), b.ctypes.data_as(hip._c_i32p), w.ctypes.data_as(hip._c_dblp))
    return rc, [a.tobytes(), b.tobytes(), w.tobytes()]


def _refused_and_the_last_result_stays(hip, index, entry, source, code, line):
    S = clusters_exact.family("distinct", 17)
    index.clusters_build_host(S, "average")
    rc, before = _fetch(hip, index, 16)
    assert rc == OK and before == [x.tobytes() for x in linkage_exact.rounds(S, "average")[:3]]
    assert _resident(hip, index, entry, source)[:2] == (code, line)
    assert _fetch(hip, index, 16) == (OK, before)


@pytest.fixture(scope="module")
def fresh(hip):
    """A handle on which no matrix was ever built."""
    index = hip.HipIndex()
    yield index
    index.close()


@pytest.fixture(scope="module")
def ast_measure(hip):
    from east import relevance
    measure = relevance.ASTRelevanceMeasure("easa", True, device=0)
    measure.set_text_collection(TEXTS)
    yield measure
    measure.index.close()


@pytest.fixture(scope="module")
def cosine_measure(hip):
    from east import relevance
    measure = relevance.CosineRelevanceMeasure("words", "tf-idf", device=0, stopwords=())
    measure.set_text_collection(TEXTS)
    yield measure
    measure.index.close()


# ---- what is no source ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
@pytest.mark.parametrize("source,code,line", (
    ("GRAPH_SOURCE_AST", INVALID, NOT_SQUARE), ("GRAPH_SOURCE_COSINE", INVALID, NOT_SQUARE), (17, INVALID, NOT_SQUARE),
    ("GRAPH_SOURCE_SIMILARITY", NOT_BUILT, "clusters: no similarity matrix has been built on this handle"),
    ("GRAPH_SOURCE_RELATED", NOT_BUILT, "clusters: no relatedness matrix has been built on this handle"),
    ("GRAPH_SOURCE_COSINE_TEXTS", NOT_BUILT, "clusters: no text similarity matrix has been built on this handle"),
    ("GRAPH_SOURCE_OVERLAP", NOT_BUILT, "clusters: no overlap matrix has been built on this handle")))
def test_what_is_no_matrix_or_was_never_built(hip, fresh, entry, source, code, line):
    source = getattr(hip, source) if isinstance(source, str) else source
    _refused_and_the_last_result_stays(hip, fresh, entry, source, code, line)


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_directed_relatedness_is_refused_in_its_own_words(hip, ast_measure, entry):
    index = ast_measure.index
    index.related_build(True, hip.RELATED_DIRECTED)
    _refused_and_the_last_result_stays(hip, index, entry, hip.GRAPH_SOURCE_RELATED, INVALID,
                                       "clusters: the relatedness matrix is directed (build it with EAST_HIP_RELATED_SYMMETRIC)")


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_directed_overlap_is_refused_in_its_own_words(hip, cosine_measure, entry):
    index = cosine_measure.index
    index.overlap_build(2, hip.OVERLAP_DIRECTED)
    _refused_and_the_last_result_stays(hip, index, entry, hip.GRAPH_SOURCE_OVERLAP, INVALID,
                                       "clusters: the overlap matrix is directed (build it with EAST_HIP_OVERLAP_SYMMETRIC)")


# ---- the four matrix sources ---------------------------------------------------------------------------------------------------
def _matrix_of(hip, name, ast_measure, cosine_measure):
    """Builds the source symmetric -> (the index, the source's number, the matrix fetched)."""
    from east import utils
    if name == "similarity":
        index = ast_measure.relevance_clusters([utils.prepare_text(kp) for kp in KEYPHRASES], hip.TOP_BY_KEYPHRASE)
        return index, hip.GRAPH_SOURCE_SIMILARITY, index.similarity_matrix()[0]
    if name == "related":
        index = ast_measure.index
        index.related_build(True, hip.RELATED_SYMMETRIC)
        return index, hip.GRAPH_SOURCE_RELATED, index.related_matrix()[0]
    index = cosine_measure.index
    if name == "cosine_texts":
        index.texts_build(True)
        return index, hip.GRAPH_SOURCE_COSINE_TEXTS, index.texts_matrix()[0]
    index.overlap_build(2, hip.OVERLAP_SYMMETRIC)
    return index, hip.GRAPH_SOURCE_OVERLAP, index.overlap_matrix()[0]


@pytest.mark.parametrize("name", ("similarity", "related", "cosine_texts", "overlap"))
def test_every_matrix_source_clusters_through_both_entry_points(hip, ast_measure, cosine_measure, name):
    index, source, S = _matrix_of(hip, name, ast_measure, cosine_measure)
    M = S.shape[0]
    assert 2 <= M <= 70 and S.shape == (M, M)
    single = [x.tobytes() for x in clusters_exact.merges(S)]
    for entry in ENTRIES:
        rc, line, out = _resident(hip, index, entry, source)
        assert (rc, line) == (OK, ""), (entry, line)
        if entry in (None, 0):
            want, rounds = single, out[2]
        else:
            assert linkage_exact.refused(S, LINKAGES[entry]) is None
            result = linkage_exact.rounds(S, LINKAGES[entry])
            want, rounds = [x.tobytes() for x in result[:3]], result[3]
        assert out[:3] == [M, len(want[0]) // 4, rounds], entry
        assert _fetch(hip, index, out[1]) == (OK, want), entry      # (single linkage: the same merges through either)


# ---- the host entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_no_members_is_an_empty_result_and_no_uploaded_source(hip, fresh, entry):
    fresh.clusters_build_host(clusters_exact.family("distinct", 17))
    assert _resident(hip, fresh, entry, hip.GRAPH_SOURCE_UPLOADED)[0] == OK
    assert _host(hip, fresh, entry, None, 0) == (OK, "", [0, 0, 0, 0])
    assert _fetch(hip, fresh, 0) == (OK, [b"", b"", b""])
    labels, out = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int64)
    assert hip.load().east_hip_clusters_cut_count(fresh._h, 1, labels.ctypes.data_as(hip._c_i32p), out.ctypes.data_as(hip._c_i64p)) == OK
    assert out.tolist() == [0, 0]
    assert _resident(hip, fresh, entry, hip.GRAPH_SOURCE_UPLOADED)[:2] == (NOT_BUILT, "clusters: no host table has been uploaded to this handle")


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_a_bad_size_or_no_matrix_is_refused_and_touches_nothing(hip, fresh, entry):
    S = clusters_exact.family("distinct", 17)
    fresh.clusters_build_host(S)
    rc, before = _fetch(hip, fresh, 16)
    assert rc == OK
    for matrix, m in ((S, -1), (S, -(2 ** 31)), (S, 0x7FFFFFF0), (None, 17), (None, 1)):
        assert _host(hip, fresh, entry, matrix, m)[:2] == (INVALID, "clusters: null matrix or bad size")
        assert _fetch(hip, fresh, 16) == (OK, before)               # refused before the build began
    assert _resident(hip, fresh, entry, hip.GRAPH_SOURCE_UPLOADED)[0] == OK   # and the uploaded copy is still the source


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_an_asymmetric_matrix_is_no_source_afterwards(hip, fresh, entry):
    good = clusters_exact.family("distinct", 130)
    fresh.clusters_build_host(good)
    bad = good.copy()
    bad[70, 3] = 0.5
    assert _host(hip, fresh, entry, bad, 130)[:2] == (INVALID, "clusters: the matrix is not symmetric: S[3][70] differs from S[70][3]")
    assert _fetch(hip, fresh, 0)[0] == NOT_BUILT                    # the build had begun: the last result is gone
    assert hip.load().east_hip_last_clusters_ms(fresh._h) == -1.0
    for other in ENTRIES:
        assert _resident(hip, fresh, other, hip.GRAPH_SOURCE_UPLOADED)[:2] == (NOT_BUILT, "clusters: no host table has been uploaded to this handle")
