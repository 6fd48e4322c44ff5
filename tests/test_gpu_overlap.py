"""GPU tier: the shingle overlap on the device (csrc/overlap.h; include/east_hip.h, "Shingle overlap").  Every case compares
the matrix, self and shingles with the model of tests/overlap_exact.py -- Python sets of word tuples, int / int -- with == on
the bytes, under route 1 (the integer matrix-core kernel), route 2 (the f64 tile kernel on unit weights) and from a second
build.  Nothing here has a tolerance."""
import numpy as np
import pytest

import clusters_exact
import cosine_exact
import overlap_exact as model

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6


def _index(hip, texts, stop=model.STOP):
    index = hip.HipCosineIndex()
    index.build_texts(list(texts), sorted(cosine_exact.prepared_stopwords(stop)))
    return index


def _fetch(index, w, symmetric):
    info = index.overlap_build(w, 1 if symmetric else 0)
    return info, tuple(a.tobytes() for a in index.overlap_matrix())


def _check(hip, index, texts, stop, w, symmetric, batches=(0,), want=None):
    """The three builds of a case against the model -> (the build's info, the model's (matrix, self, shingles, I))."""
    lib = hip.load()
    want = want or model.exact(texts, stop, w, symmetric)
    want_bytes = tuple(a.tobytes() for a in want[:3])
    info = None
    try:
        for batch in batches:
            assert lib.east_hip_debug_set_overlap_batch(batch) == OK
            for route in (1, 2, 0):                                   # (0: the default, the second build of its route)
                assert lib.east_hip_debug_set_overlap_route(route) == OK
                info, got = _fetch(index, w, symmetric)
                assert info["route"] == (route or info["route"]) and info["route"] in (1, 2)
                for name, g, e in zip(("matrix", "self", "shingles"), got, want_bytes):
                    assert g == e, (name, "route", route, "batch", batch, "w", w, "symmetric", symmetric)
    finally:
        lib.east_hip_debug_set_overlap_route(0)
        lib.east_hip_debug_set_overlap_batch(0)
    assert info["n_docs"] == len(texts) and info["words"] == w and index.last_overlap_ms() > 0.0
    return info, want


def _units(texts, stop, w):
    return model.shared_units(model.shingle_sets(texts, stop, w))


@pytest.mark.parametrize("D", (1, 2, 63, 64, 65, 129))
def test_tile_edges(hip, D):
    texts = model.tile_edge_texts(D)
    index = _index(hip, texts)
    for w in (1, 2, 3):
        for symmetric in (True, False):
            info, _ = _check(hip, index, texts, model.STOP, w, symmetric)
            distinct, shared, postings = _units(texts, model.STOP, w)
            assert (info["distinct_shingles"], info["shared_shingles"], info["postings"]) == (distinct, shared, postings)
            assert info["tiles"] == (D + 63) // 64 * ((D + 63) // 64 + 1) // 2
    index.close()


@pytest.mark.parametrize("U", (0, 1, 63, 64, 65, 8191, 8192, 8193))
def test_unit_range_edges(hip, U):
    """The i8 chunk of 64 units and the segment of 8 192: exactly U shared shingles, batches of 1, 2 and the default."""
    texts = model.unit_edge_texts(U)
    index = _index(hip, texts)
    for symmetric in (True, False):
        info, want = _check(hip, index, texts, model.STOP, 2, symmetric, batches=(1, 2, 0))
        assert info["shared_shingles"] == U and info["segments"] == (U + 8191) // 8192
        assert want[3][0, 1] == (U + 1) // 2 and want[3][0, 0] == U + 6       # (three passages of two shingles of its own)
    index.close()


def test_orientation_of_the_tile(hip):
    """130 texts, every pair a passage of its own: I[a][64 + b] != I[b][64 + a] for 80 % of the pairs, so a swapped
    row / column map or the f64 C/D map in the integer kernel cannot pass."""
    texts = model.orientation_texts()
    want = model.exact(texts, model.STOP, 2, True)
    I = want[3]
    pairs = [(a, b) for a in range(64) for b in range(64) if a != b]
    assert sum(1 for a, b in pairs if I[a, 64 + b] != I[b, 64 + a]) >= len(pairs) / 2
    index = _index(hip, texts)
    _check(hip, index, texts, model.STOP, 2, True, want=want)
    _check(hip, index, texts, model.STOP, 2, False)
    index.close()


def test_content_cases(hip):
    texts = model.content_texts()
    index = _index(hip, texts)
    for w in (1, 2, 4, 8):
        _check(hip, index, texts, model.STOP, w, True)
        _check(hip, index, texts, model.STOP, w, False)
    index.overlap_build(2, 1)
    matrix, own, shingles = index.overlap_matrix()
    assert matrix[0, 1] == 1.0 and shingles[0] == shingles[1] == 9                 # identical texts
    assert 0.0 < matrix[2, 0] < 1.0 and 0.0 < matrix[3, 0] < 1.0                  # contained: resemblance below 1
    for empty in (4, 5, 6):                                                        # empty, fewer than w words, stopwords only
        assert shingles[empty] == 0 and own[empty] == 0.0 and not np.signbit(own[empty])
        assert (np.delete(matrix[empty], empty) == 0.0).all() and not np.signbit(np.delete(matrix[empty], empty)).any()
    index.overlap_build(2, 0)
    directed = index.overlap_matrix()[0]
    assert directed[2, 0] == 1.0 and directed[0, 3] == 1.0 and directed[0, 2] == 3 / 9
    info = index.overlap_build(8, 1)                                               # w = 8: only the long texts have a shingle
    assert info["levels"] == 8 and index.overlap_matrix()[2].tolist() == [3, 3, 0, 9, 0, 0, 0, 0]
    index.close()
    # w larger than every text: no shingle position at all
    short = ("aaa bbb ccc", "aaa bbb ccc", "ddd")
    index = _index(hip, short)
    info, _ = _check(hip, index, short, model.STOP, 4, True)
    assert info["shingle_positions"] == 0 and info["shared_shingles"] == 0
    index.close()


def test_a_run_across_a_scan_tile(hip):
    """One shingle held by 4 097 one-shingle texts: a run of 4 097 postings, a matrix of ones."""
    D = 4097
    texts = ("alpha beta",) * D
    index = _index(hip, texts)
    lib = hip.load()
    try:
        for route in (1, 2, 1):
            assert lib.east_hip_debug_set_overlap_route(route) == OK
            info = index.overlap_build(2, 1)
            matrix, own, shingles = index.overlap_matrix()
            assert (info["shared_shingles"], info["postings"], info["distinct_shingles"]) == (1, D, 1)
            assert (shingles == 1).all() and (own == 1.0).all() and np.isnan(matrix.diagonal()).all()
            np.fill_diagonal(matrix, 1.0)
            assert (matrix == 1.0).all()
    finally:
        lib.east_hip_debug_set_overlap_route(0)
    index.close()


def test_wide_keys(hip):
    """70 000 distinct words at w = 2: more than 2^16 survivors below level 2 and 17 bits of terms, 34-bit keys."""
    texts = model.wide_key_texts()
    index = _index(hip, texts, ())
    info, want = _check(hip, index, texts, (), 2, True)
    assert info["shared_shingles"] == want[3][0, 1] == 34999 and info["segments"] == 5      # (the half that keeps its order)
    _check(hip, index, texts, (), 2, False)
    index.close()


def test_sweep_of_words_and_orientations(hip):
    texts = model.zipf_texts()
    index = _index(hip, texts)
    shared = []
    for w in range(1, model.MAX_WORDS + 1):
        for symmetric in (True, False):
            info, _ = _check(hip, index, texts, model.STOP, w, symmetric)
        shared.append(info["shared_shingles"])
        assert info["shared_shingles"] == _units(texts, model.STOP, w)[1] and info["kept_tokens"] >= 19000
    assert shared[1] > shared[3] > shared[7] > 0                                   # (the copied passages reach w = 8)
    index.close()


def test_fuzz_documents(hip):
    for i, r in enumerate(cosine_exact.fuzz_rounds()[:40]):
        index = _index(hip, r["texts"], r["stopwords"])
        _check(hip, index, r["texts"], r["stopwords"], 1 + i % 3, i % 2 == 0)
        index.close()


def test_lifecycle(hip):
    lib = hip.load()
    index = hip.HipCosineIndex()
    h = index._h
    out = np.zeros(14, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)

    def build(words=2, orientation=1, handle=h, out=p_out):
        return lib.east_hip_overlap_build(handle, words, orientation, out), lib.east_hip_last_error().decode()

    def fetch():
        return lib.east_hip_overlap_fetch(h, None, None, None)

    assert build() == (ERR_NOT_BUILT, "overlap: no cosine index has been built on this handle")
    assert fetch() == ERR_NOT_BUILT and lib.east_hip_last_error().decode() == "no overlap matrix has been built on this handle"
    assert lib.east_hip_last_overlap_ms(h) == -1.0
    assert build(handle=None)[0] == ERR_INVALID
    assert lib.east_hip_debug_set_overlap_route(3) == ERR_INVALID and lib.east_hip_debug_set_overlap_route(-1) == ERR_INVALID
    texts = model.tile_edge_texts(65)
    stop = sorted(cosine_exact.prepared_stopwords(model.STOP))
    index.build_texts(list(texts), stop)
    assert fetch() == ERR_NOT_BUILT
    want = _fetch(index, 2, True)[1]
    assert want == tuple(a.tobytes() for a in model.exact(texts, model.STOP, 2, True)[:3])

    # every refusal names what is wrong and leaves the earlier matrix fetchable
    for arguments, said in ((dict(words=0), "words must lie in 1 .. 8"), (dict(words=9), "words must lie in 1 .. 8"),
                            (dict(orientation=2), "unknown orientation"), (dict(orientation=-1), "unknown orientation"),
                            (dict(out=None), "out is null")):
        rc, message = build(**arguments)
        assert rc == ERR_INVALID and said in message and message.startswith("overlap: "), (arguments, message)
        assert fetch() == OK and tuple(a.tobytes() for a in index.overlap_matrix()) == want and index.last_overlap_ms() > 0.0

    # an extracted-phrases result is untouched by an overlap build, and the overlap by an extraction
    phrases = index.phrases(0, 3, 1, 2, 1)
    before = (phrases.words.tobytes(), phrases.count.tobytes(), phrases.first.tobytes(), phrases.strings())
    assert _fetch(index, 3, False)[1] == tuple(a.tobytes() for a in model.exact(texts, model.STOP, 3, False)[:3])
    R = len(phrases.words)
    words, count = np.empty(R, np.int32), np.empty(R, np.int32)
    assert lib.east_hip_phrases_fetch(h, words.ctypes.data_as(hip._c_i32p), count.ctypes.data_as(hip._c_i32p), *[None] * 6) == OK
    assert (words.tobytes(), count.tobytes()) == before[:2] and R > 0
    index.phrases(0, 3, 1, 2, 1)
    assert fetch() == OK and _fetch(index, 2, True)[1] == want

    # score calls and the classes leave it alone; a cosine build withdraws it, and so does a reset
    index.score_table(np.array([0, 1, 2], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64), True)
    V = index.n_terms
    index.set_classes(np.arange(V, dtype=np.int32) // 2, (V + 1) // 2)
    assert fetch() == OK and tuple(a.tobytes() for a in index.overlap_matrix()) == want
    assert _fetch(index, 2, True)[1] == want                       # (shingles are made of words whatever the vector space)
    index.set_classes([], 0)
    index.build_texts(list(texts), stop)
    assert fetch() == ERR_NOT_BUILT and lib.east_hip_last_overlap_ms(h) == -1.0
    assert _fetch(index, 2, True)[1] == want
    assert lib.east_hip_reset(h) == OK
    assert fetch() == ERR_NOT_BUILT and build()[0] == ERR_NOT_BUILT and lib.east_hip_last_overlap_ms(h) == -1.0
    index.close()


def test_consumers_of_the_matrix(hip):
    lib = hip.load()
    texts = model.tile_edge_texts(65)
    index = _index(hip, texts)
    h = index._h
    out = np.zeros(4, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)
    assert lib.east_hip_top_build_resident(h, hip.GRAPH_SOURCE_OVERLAP, hip.TOP_BY_KEYPHRASE, 3, 0.0, p_out) == ERR_NOT_BUILT
    assert lib.east_hip_last_error().decode().endswith(": no overlap matrix has been built on this handle")
    assert lib.east_hip_clusters_build_resident(h, hip.GRAPH_SOURCE_OVERLAP, p_out) == ERR_NOT_BUILT
    for symmetric in (True, False):
        matrix = model.exact(texts, model.STOP, 2, symmetric)[0]
        for n, threshold in ((5, -np.inf), (3, 0.2), (64, 0.0)):
            found = index.texts_overlap(2, 1 if symmetric else 0, n, threshold)
            count, at, score = model.ranking(matrix, n, threshold)
            assert np.array_equal(found.count, count) and np.array_equal(found.index, at)
            assert found.score.tobytes() == score.tobytes()
    # the clusters of the symmetric matrix, by both builders
    index.overlap_build(2, hip.OVERLAP_SYMMETRIC)
    S = index.overlap_matrix()[0]
    index.clusters_build(hip.GRAPH_SOURCE_OVERLAP)
    a, b, w = index.clusters_merges()
    ea, eb, ew = clusters_exact.merges(S)
    assert np.array_equal(a, ea) and np.array_equal(b, eb) and w.tobytes() == np.asarray(ew, np.float64).tobytes()
    for linkage in ("complete", "average"):
        index.clusters_build(hip.GRAPH_SOURCE_OVERLAP, linkage, None)
        from east import applications
        ha, hb, hw = applications._linkage_rounds(S, linkage)[:3]
        a, b, w = index.clusters_merges()
        assert np.array_equal(a, ha) and np.array_equal(b, hb) and w.tobytes() == hw.tobytes(), linkage
    # a directed matrix is refused by both, in the contract's line; source 7 stays unknown
    index.overlap_build(2, hip.OVERLAP_DIRECTED)
    line = "clusters: the overlap matrix is directed (build it with EAST_HIP_OVERLAP_SYMMETRIC)"
    assert lib.east_hip_clusters_build_resident(h, hip.GRAPH_SOURCE_OVERLAP, p_out) == ERR_INVALID
    assert lib.east_hip_last_error().decode() == line
    assert lib.east_hip_clusters_build_resident_linkage(h, hip.GRAPH_SOURCE_OVERLAP, 1, float("nan"), p_out) == ERR_INVALID
    assert lib.east_hip_last_error().decode() == line
    assert lib.east_hip_top_build_resident(h, hip.GRAPH_SOURCE_OVERLAP, hip.TOP_BY_KEYPHRASE, 3, 0.0, p_out) == OK
    assert lib.east_hip_top_build_resident(h, 7, hip.TOP_BY_KEYPHRASE, 3, 0.0, p_out) == ERR_INVALID
    assert "unknown table source" in lib.east_hip_last_error().decode()
    index.close()


def test_applications_device_against_host(hip, monkeypatch):
    from east import applications, relevance
    texts = {"t%02d" % d: text for d, text in enumerate(model.zipf_texts(3000, 9))}
    texts.update({"c%d" % d: text for d, text in enumerate(model.content_texts())})
    make = lambda: relevance.CosineRelevanceMeasure("words", stopwords=model.STOP)
    for arguments in (dict(n=4, words=2), dict(n=3, words=4, orientation="directed", overlap_threshold=0.01), dict(n=17, words=1)):
        monkeypatch.delenv("EAST_HIP_OVERLAP", raising=False)
        device = applications.texts_overlap(texts, similarity_measure=make(), **arguments)
        monkeypatch.setenv("EAST_HIP_OVERLAP", "host")
        host = applications.texts_overlap(texts, similarity_measure=make(), **arguments)
        assert device == host and list(device) == list(texts) and any(device.values())
    for arguments in (dict(words=2, threshold=0.3), dict(words=2, k=5, linkage="average"), dict(words=3, threshold=0.2, linkage="complete"),
                      dict(words=1)):
        monkeypatch.delenv("EAST_HIP_OVERLAP", raising=False)
        device = applications.texts_overlap_clusters(texts, similarity_measure=make(), **arguments)
        monkeypatch.setenv("EAST_HIP_OVERLAP", "host")
        host = applications.texts_overlap_clusters(texts, similarity_measure=make(), **arguments)
        assert device.merges == host.merges and device.clusters == host.clusters and device.labels == host.labels
        if arguments.get("threshold") == 0.3:
            assert ["c0", "c1", "c2", "c3"] in device.clusters     # (identical texts, the one they contain: 3 / 9, the one that quotes them: 9 / 15)
