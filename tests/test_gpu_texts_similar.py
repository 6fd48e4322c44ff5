"""GPU tier: text-to-text cosine similarity on the device (csrc/cosine_texts.h; include/east_hip.h, "Text-to-text cosine
similarity").  Every case checks the fetched matrix, self and postings against tests/texts_cosine_exact.py: the bound
(t_ab + ceil(p_a / 64) + ceil(p_b / 64) + 176) * 2^-52 * exact, the exact zeros as +0.0, the NaN diagonal and C == C.T bit
for bit.  The collections are the ones tests/test_texts_similar_host.py holds plain doubles to a tenth of the bound on.

Largest error-to-bound ratio seen over all cases on an MI355X: see DESIGN.md 15, "Measured"."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import cosine_exact
import texts_cosine_exact as model
from conftest import load_golden

pytestmark = pytest.mark.gpu

INF = float("inf")
OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6


def _index(hip, name, chunk=None, seg=None):
    """A cosine index of a collection of the model, in its vector space -> (index, stems)."""
    chunk, seg = chunk or hip.COSINE_TEXTS_CHUNK, seg or hip.COSINE_TEXTS_SEG
    texts, stop, stems = model.collections(chunk, seg)[name]
    index = hip.HipCosineIndex()
    index.build_texts(list(texts), sorted(cosine_exact.prepared_stopwords(stop)))
    if stems:
        m = model.model_of(name, chunk, seg)
        assert index.terms() == m.terms
        index.set_classes(m.term_class, m.n_classes)
    return index, stems


def _check(hip, index, name, tfidf):
    info = index.texts_build(tfidf)
    chunk, seg = info["chunk_units"], info["segment_units"]
    assert (chunk, seg) == (hip.COSINE_TEXTS_CHUNK, hip.COSINE_TEXTS_SEG)
    ex = model.exact_of(name, chunk, seg, tfidf)
    m = model.model_of(name, chunk, seg)
    stems = model.collections(chunk, seg)[name][2]
    D = ex.p.size
    tiles = -(-D // 64)
    assert info["n_docs"] == D and info["units"] == m.space(stems)[2] and info["postings"] == m.space(stems)[3]
    assert info["tiles"] == tiles * (tiles + 1) // 2 and info["segments"] == -(-info["units"] // seg)
    matrix, own, postings = index.texts_matrix()
    assert matrix.dtype == np.float64 and own.dtype == np.float64 and postings.dtype == np.int32
    model.check(matrix, own, postings, ex)
    assert index.last_texts_ms() > 0.0
    return matrix, own


@pytest.mark.parametrize("D", model.TILE_EDGE_D)
def test_tile_edges(hip, D):
    index, _ = _index(hip, "tile edges %d" % D)
    for tfidf in (True, False):
        _check(hip, index, "tile edges %d" % D, tfidf)
    index.close()


@pytest.mark.parametrize("which", range(7))
def test_chunk_and_segment_edges(hip, which):
    U = model.unit_edge_sizes(hip.COSINE_TEXTS_CHUNK, hip.COSINE_TEXTS_SEG)[which]
    name = "units %d" % U
    index, _ = _index(hip, name)
    for tfidf in (True, False):
        matrix, _ = _check(hip, index, name, tfidf)
        assert matrix[2, 3] > 0.0                                 # the very last unit is the only common one
        assert (matrix[1, [0]] > 0.0).all()                       # the text of two postings, astride two segments where there are two
    index.close()


@pytest.mark.parametrize("name", ("document shapes", "cursor skew", "long text", "stems"))
def test_shapes_of_documents_and_both_spaces(hip, name):
    index, _ = _index(hip, name)
    for tfidf in (False, True, False):                            # one build after the other on one handle, alternating weightings
        matrix, own = _check(hip, index, name, tfidf)
    if name == "document shapes":
        assert own[:2].tolist() == [0.0, 0.0] and abs(matrix[3, 4] - 1.0) < 1e-13 and matrix[5, 6].tobytes() == np.float64(0.0).tobytes()
        found = index.rank_texts(3)
        assert found.index[2].tolist() == [3, 4, 0] and found.score[2, 0] == found.score[2, 1] > 0.0     # a tie, in the order of the texts
        assert found.score[2, 2].tobytes() == np.float64(0.0).tobytes()
    index.close()


def test_same_bytes_across_builds_and_batches(hip):
    U = model.unit_edge_sizes(hip.COSINE_TEXTS_CHUNK, hip.COSINE_TEXTS_SEG)[-1]
    name = "units %d" % U
    index, _ = _index(hip, name)
    lib = hip.load()
    want = {}
    for tfidf in (True, False):
        first = index.texts_build(tfidf)
        want[tfidf] = [a.tobytes() for a in index.texts_matrix()]
        assert first["segments"] == 3
        assert index.texts_build(tfidf)["launches"] == first["launches"]
        assert [a.tobytes() for a in index.texts_matrix()] == want[tfidf]
    try:
        for batch in (1, 2):
            assert lib.east_hip_debug_set_text_similarity_batch(batch) == OK
            for tfidf in (True, False):
                info = index.texts_build(tfidf)
                assert info["launches"] == 2 * -(-3 // batch) + 1      # a tile launch and a fold a batch, the finish
                assert [a.tobytes() for a in index.texts_matrix()] == want[tfidf], batch
    finally:
        lib.east_hip_debug_set_text_similarity_batch(0)
    other = hip.HipCosineIndex()                                   # another handle, another build of the index
    other.build_texts(list(model.collections(hip.COSINE_TEXTS_CHUNK, hip.COSINE_TEXTS_SEG)[name][0]))
    other.texts_build(True)
    assert [a.tobytes() for a in other.texts_matrix()] == want[True]
    other.close()
    index.close()


def _select(matrix, n, threshold):
    from east import applications
    return applications._top_select(matrix, 1, n, threshold)


def test_ranking_against_numpy_selection(hip):
    for name in ("tile edges 129", "document shapes"):
        index, _ = _index(hip, name)
        index.texts_build(True)
        matrix = index.texts_matrix()[0]
        finite = matrix[np.isfinite(matrix) & (matrix > 0.0)]
        for n, threshold in ((1, -INF), (10, -INF), (1024, -INF), (10, float(np.median(finite))), (1024, 0.0), (3, 2.0)):
            found = index.rank_texts(n, threshold)
            want = _select(matrix, n, threshold)
            assert found.count.tolist() == [len(w) for w in want]
            for s, w in enumerate(want):
                assert found.index[s, :len(w)].tolist() == [i for i, _ in w]
                assert found.score[s, :len(w)].tobytes() == np.array([v for _, v in w], dtype=np.float64).tobytes()
        again = index.texts_similar(True, 10)
        assert again.index.tobytes() == index.rank_texts(10).index.tobytes()
        index.close()


def test_lifetime(hip):
    lib = hip.load()
    index = hip.HipCosineIndex()
    h = index._h
    none = [None] * 3
    out = np.zeros(8, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)
    top_out = np.zeros(2, dtype=np.int64)

    def ranked():
        return lib.east_hip_top_build_resident(h, hip.GRAPH_SOURCE_COSINE_TEXTS, hip.TOP_BY_KEYPHRASE, 3, -INF, top_out.ctypes.data_as(hip._c_i64p))

    assert lib.east_hip_text_similarity_build(h, 1, p_out) == ERR_NOT_BUILT        # no cosine index
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and ranked() == ERR_NOT_BUILT
    assert lib.east_hip_last_text_similarity_ms(h) == -1.0
    texts = model.document_shapes()
    stop = sorted(cosine_exact.prepared_stopwords(model.STOPWORDS))
    index.build_texts(list(texts), stop)
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and ranked() == ERR_NOT_BUILT
    assert lib.east_hip_text_similarity_build(h, 2, p_out) == ERR_INVALID and lib.east_hip_text_similarity_build(h, -1, p_out) == ERR_INVALID
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and lib.east_hip_last_text_similarity_ms(h) == -1.0
    index.texts_build(True)
    want = [a.tobytes() for a in index.texts_matrix()]
    assert index.last_texts_ms() > 0.0 and ranked() == OK

    # a score call, a `keyphrases similar` build, a ranking of it and an EASA build in between leave the matrix alone
    ids = np.array([0, 1, 2], dtype=np.int32)
    index.score_table(ids, np.array([0, 2, 3], dtype=np.int64), True)
    index.similar(hip.TOP_BY_TEXT, 2)
    index.index.build_texts([b"some text for the suffix arrays here", b"another text of the same kind"])
    assert [a.tobytes() for a in index.texts_matrix()] == want and index.last_texts_ms() > 0.0 and ranked() == OK

    # the classes change the space under it; so does going back to the terms
    V = index.n_terms
    index.set_classes(np.arange(V, dtype=np.int32) // 2, (V + 1) // 2)
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and ranked() == ERR_NOT_BUILT
    assert lib.east_hip_last_text_similarity_ms(h) == -1.0
    index.texts_build(True)
    merged = index.texts_matrix()[0]
    assert merged.tobytes() != want[0]
    index.set_classes([], 0)
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT
    index.texts_build(True)
    assert [a.tobytes() for a in index.texts_matrix()] == want

    # a rebuild of the index, and a reset
    index.build_texts(list(texts), stop)
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and ranked() == ERR_NOT_BUILT
    index.texts_build(True)
    assert [a.tobytes() for a in index.texts_matrix()] == want
    assert lib.east_hip_reset(h) == OK
    assert lib.east_hip_text_similarity_fetch(h, *none) == ERR_NOT_BUILT and ranked() == ERR_NOT_BUILT
    assert lib.east_hip_text_similarity_build(h, 1, p_out) == ERR_NOT_BUILT and lib.east_hip_last_text_similarity_ms(h) == -1.0
    index.close()


def _hse():
    """The fixture's texts, as test_gpu_similar loads them.  They are Cyrillic: what the comparison of the two paths needs of
    them is that no character changes the length of the text under upper() (Python's and the device's 1:1 upper-casing
    differ on such characters only), which ASCII would guarantee and which is checked here."""
    g = load_golden("hse_config1.json")
    assert all(len(c.upper()) == 1 for text in g["texts"].values() for c in set(text))
    return {name: g["texts"][name].encode("utf-8") for name in sorted(g["texts"])}


def test_device_against_host_on_the_hse_fixture(hip, monkeypatch):
    """applications.texts_similar on both paths: the values agree to the bound, and the names wherever neighbouring values lie
    further apart than twice the bound."""
    from east import applications, relevance
    texts = _hse()
    names = list(texts)
    D = len(names)
    for space, weighting in (("words", "tf-idf"), ("stems", "tf")):
        make = lambda: relevance.CosineRelevanceMeasure(space, weighting, stopwords=model.STOPWORDS, stemmer=cosine_exact.ToyStemmer())
        m = cosine_exact.build_model(list(texts.values()), model.STOPWORDS, cosine_exact.ToyStemmer())
        ex = model.exact(m, weighting == "tf-idf", space == "stems")
        monkeypatch.delenv("EAST_HIP_TEXTS_SIMILAR", raising=False)
        measure = make()
        device = applications.texts_similar(texts, 1024, None, measure)
        model.check(*measure.text_similarity_matrix(), ex)
        monkeypatch.setenv("EAST_HIP_TEXTS_SIMILAR", "host")
        host = applications.texts_similar(texts, 1024, None, make())
        assert list(device) == list(host) == names
        compared = 0
        for a, name in enumerate(names):
            assert len(device[name]) == len(host[name]) == D - 1
            limit = {o: float(ex.bound[a, names.index(o)]) * model.ULP * v for o, v in host[name]}
            values = [v for _, v in host[name]]
            for i, ((od, vd), (oh, vh)) in enumerate(zip(device[name], host[name])):
                assert abs(vd - vh) <= 2.0 * max(limit[od], limit[oh]), (name, i)      # (each path within the bound of the exact value)
                # (twice the bound between the exact values is four times between the host's own)
                apart = all(abs(values[j] - vh) > 4.0 * limit[oh] for j in (i - 1, i + 1) if 0 <= j < D - 1)
                if apart:
                    assert od == oh, (name, i)
                    compared += 1
        print("%s %s: %d of %d entries compared by name" % (space, weighting, compared, D * (D - 1)))
        assert compared > 0


def test_cli_end_to_end(hip, tmp_path, monkeypatch):
    from east import applications, formatting, main, relevance
    for name in ("WORLD_SIZE", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST", "EAST_HIP_TEXTS_SIMILAR"):
        monkeypatch.delenv(name, raising=False)
    files = {"a": b"alpha beta gamma delta", "b": b"beta gamma epsilon", "c": b"zeta eta theta", "d": b"alpha alpha zeta"}
    for name, text in files.items():
        (tmp_path / (name + ".txt")).write_bytes(text)
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main.main(["-v", "words", "-n", "2", "texts", "similar", str(tmp_path)])
    want = applications.texts_similar(files, 2, None, relevance.CosineRelevanceMeasure("words", "tf-idf"))
    assert rc == 0 and buf.getvalue() == formatting.format_similar(want, "text", "xml") + "\n"
    assert sorted(o for o, _ in want["a"]) == ["b", "d"] and want["c"][0][0] == "d" and want["c"][1] == ("a", 0.0)
