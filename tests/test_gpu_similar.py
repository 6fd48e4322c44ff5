"""gpu tier: similar texts and keyphrases on the device (csrc/similarity.h through include/east_hip.h, "Similar texts and
keyphrases").  The yardstick is tests/similar_exact.py and never the project's host path: the VALUES of the fetched matrix
are compared to the contract in extended precision with the bound (2 L + 16) * 2^-53 and no other; the SELECTION is the
ranking's contract (np.lexsort, as tests/test_gpu_top.py) applied to the device's own fetched matrix -- indices compared
with ==, ranked scores as bytes of that matrix.

The exact-sum cases (entries j / 16) came out IDENTICAL to numpy's four operations when run on an MI355X;
the test asks for the derivable 4 ulp."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import similar_exact as model
from conftest import load_golden

pytestmark = pytest.mark.gpu

INF = float("inf")
OK, ERR_INVALID, ERR_OOM, ERR_NOT_BUILT = 0, -2, -3, -6
NS = (1, 2, 10, 64, 65, 1024)
MS = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 129, 193)       # the MFMA block, the quadrant, the tile; three tiles a side
LS = (1, 3, 4, 5, 16, 17, 31, 32, 33, 63, 64, 65, 257, 1000)    # the MFMA's k-step, the staging chunk of 32, two chunks


def exact_or_skip(P):
    found = model.exact(P)
    if found is None:
        pytest.skip("np.longdouble is no wider than a double here and the Fraction model takes M * M * L <= 10^6 only")
    return found


def check_values(S, q, P, want=None):
    """The fetched matrix and norms of the M x L profiles P against the model; -> the model's (S, q)."""
    M, L = P.shape
    want_S, want_q = exact_or_skip(P) if want is None else want
    assert S.shape == (M, M) and q.shape == (M,) and S.dtype == np.float64 and q.dtype == np.float64
    assert np.isnan(np.diag(S)).all()
    assert np.array_equal(np.isnan(S), np.isnan(want_S)), "NaN anywhere but where the contract puts it"
    assert S.tobytes() == S.T.copy().tobytes(), "S[a][b] and S[b][a] differ"
    worst = float(np.nanmax(np.abs(S - want_S), initial=0.0))
    assert worst <= model.bound(L), (M, L, worst, model.bound(L))
    ok = np.isfinite(want_q)
    assert (np.abs(q[ok] - want_q[ok]) <= model.gamma(L + 2) * want_q[ok]).all(), (M, L)
    return want_S, want_q


def agree(found, want, what=None):
    count, index, score = want
    assert found.count.dtype == np.int32 and found.index.dtype == np.int32 and found.score.dtype == np.float64
    assert found.index.shape == index.shape and found.score.shape == score.shape, what
    assert found.count.tolist() == count.tolist(), what
    assert np.array_equal(found.index, index), what
    assert found.score.tobytes() == score.tobytes(), what


def both_axes(index, P):
    """The profiles once as rows (by keyphrase) and once as columns (by text) -> [(S, q)] in that order."""
    M, L = P.shape
    found = []
    for axis, table in ((1, P), (0, np.ascontiguousarray(P.T))):
        assert index.similarity_from_table(table, axis) == (M, L)
        found.append(index.similarity_matrix())
    return found


def sparse_profiles(rng, M, L):
    P = rng.random((M, L))
    P[rng.random((M, L)) < 0.1] = 0.0
    return P


@pytest.mark.parametrize("M", MS)
def test_every_edge_of_block_quadrant_tile_and_chunk(hip, M):
    """Nothing is sampled: every M with every L, both axes; the two matrices agree with the model and with each other."""
    index = hip.HipIndex()
    for L in LS:
        P = sparse_profiles(np.random.default_rng(1000 * M + L), M, L)
        want = exact_or_skip(P)
        (S_rows, q_rows), (S_cols, q_cols) = both_axes(index, P)
        check_values(S_rows, q_rows, P, want)
        check_values(S_cols, q_cols, P, want)
        assert float(np.nanmax(np.abs(S_rows - S_cols), initial=0.0)) <= model.bound(L), (M, L)
    assert 0.0 < index.last_similarity_ms < 1000.0
    index.close()


@pytest.mark.parametrize("M,L", [(33, 5), (65, 1000), (130, 257)])
def test_exact_sums(hip, M, L):
    """Entries j / 16: every product and every partial sum is exact in any order, so q must be the integer model's bytes
    and S within 4 ulp of numpy's same four operations (each is within one)."""
    index = hip.HipIndex()
    J = np.random.default_rng(M + L).integers(0, 16, size=(M, L))
    J[min(7, M - 1)] = 0                                      # (a zero profile among them)
    P = J / 16.0
    q_int = (J.astype(np.int64) ** 2).sum(axis=1)
    G_int = J.astype(np.int64) @ J.astype(np.int64).T
    want_q = q_int / 256.0
    root = np.sqrt(want_q)
    with np.errstate(invalid="ignore", divide="ignore"):
        want_S = (G_int / 256.0) / (root[:, None] * root[None, :])
    want_S[(q_int == 0)[:, None] | (q_int == 0)[None, :]] = 0.0
    np.fill_diagonal(want_S, np.nan)
    for S, q in both_axes(index, P):
        assert q.tobytes() == want_q.tobytes()
        check_values(S, q, P)
        off = ~np.eye(M, dtype=bool)
        ulps = np.abs(S[off] - want_S[off]) / np.spacing(np.abs(want_S[off]))
        print("exact sums %d x %d: %d of %d entries differ from numpy's, at most %.1f ulp" % (M, L, int((ulps > 0).sum()), ulps.size, ulps.max()))
        assert ulps.max() <= 4.0
    index.close()


def test_signs_and_special_values(hip):
    index = hip.HipIndex()
    rng = np.random.default_rng(17)
    # negative entries; two opposite profiles
    P = rng.random((70, 37)) - 0.5
    P[66] = -P[3]
    for S, q in both_axes(index, P):
        check_values(S, q, P)
        assert abs(S[3, 66] + 1.0) <= model.bound(37) and (S < 0).any()
    # a profile of -0.0 is a zero profile: +0.0 in its row and column
    P = rng.random((67, 21)) - 0.25
    P[64] = -0.0
    for S, q in both_axes(index, P):
        check_values(S, q, P)
        others = np.arange(67) != 64
        assert not S[64, others].any() and not S[others, 64].any()
        assert not np.signbit(S[64, others]).any() and not np.signbit(S[others, 64]).any() and q[64] == 0.0
    # one NaN entry: NaN in exactly that member's row and column, every other entry still within the bound
    P = rng.random((66, 40))
    P[65, 33] = np.nan
    for S, q in both_axes(index, P):
        check_values(S, q, P)
        assert np.isnan(S[65]).all() and np.isnan(S[:, 65]).all() and np.isnan(q[65])
        assert np.isnan(S).sum() == 66 + 2 * 65
    # M = 1: the matrix is one NaN, nobody is ranked
    for axis, table in ((1, rng.random((1, 9))), (0, rng.random((9, 1)))):
        assert index.similarity_from_table(table, axis) == (1, 9)
        S, q = index.similarity_matrix()
        assert S.shape == (1, 1) and np.isnan(S[0, 0]) and q[0] > 0.0
        found = index.rank_similarity(10)
        assert found.count.tolist() == [0] and (found.index == -1).all() and not found.score.any()
    index.close()


@pytest.mark.parametrize("axis", [0, 1])
def test_ranking_the_matrix(hip, axis):
    index = hip.HipIndex()
    rng = np.random.default_rng(23 + axis)
    P = sparse_profiles(rng, 131, 29)
    P[77] = 0.0
    table = P if axis == 1 else np.ascontiguousarray(P.T)
    index.similarity_from_table(table, axis)
    S, q = index.similarity_matrix()
    check_values(S, q, P)
    present = float(S[5, 9])
    for threshold in (-INF, present, np.nextafter(present, 2.0)):
        for n in NS:
            found = index.rank_similarity(n, threshold)
            agree(found, model.select(S, n, threshold), (axis, n, threshold))
            assert found.count.max() <= 130 and not (found.index == np.arange(131)[:, None]).any()
    assert index.rank_similarity(1024).count.tolist() == [130] * 131
    # many equal profiles (exact entries: equal profiles give equal bytes): ties, broken by the member index
    kinds = rng.integers(0, 16, size=(5, 12)) / 16.0
    P = kinds[rng.integers(0, 5, size=150)]
    table = P if axis == 1 else np.ascontiguousarray(P.T)
    index.similarity_from_table(table, axis)
    S, _ = index.similarity_matrix()
    assert max(np.unique(row[~np.isnan(row)]).size for row in S) <= 5
    for n in (1, 10, 65, 1024):
        agree(index.rank_similarity(n), model.select(S, n, -INF), (axis, n))
    index.close()


def _hse():
    g = load_golden("hse_config1.json")
    return g["keyphrases"], {name: g["texts"][name].encode("utf-8") for name in sorted(g["texts"])}


def _resident(measure, keyphrases, texts):
    from east import utils
    measure.set_text_collection(list(texts.values()))
    prepared = [utils.prepare_text(kp) for kp in keyphrases]
    table = np.ascontiguousarray(measure.relevance_table(prepared), dtype=np.float64)
    assert table.shape == (len(keyphrases), len(texts))
    for axis in (0, 1):
        P = model.profiles_of(table, axis)
        for n, threshold in ((3, -INF), (64, 0.5)):
            found = measure.relevance_similar(prepared, axis, n, threshold)
            S, q = measure.index.similarity_matrix()
            check_values(S, q, P)
            agree(found, model.select(S, n, threshold), (axis, n, threshold))
    assert measure.index.last_similarity_ms > 0.0
    return table


def test_resident_ast_table_on_the_hse_fixture(hip):
    from east import relevance
    keyphrases, texts = _hse()
    table = _resident(relevance.ASTRelevanceMeasure("easa", True), keyphrases, texts)
    assert table.shape == (10, 30) and table.max() > 0.25
    _resident(relevance.ASTRelevanceMeasure("easa", False), keyphrases, texts)


def test_resident_cosine_table(hip):
    from east import relevance
    _, texts = _hse()
    keyphrases = load_golden("cosine.json")["cli"]["keyphrases"]
    table = _resident(relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[]), keyphrases, texts)
    assert table.max() > 0.0


def test_the_uploaded_copy_is_kept(hip):
    index = hip.HipIndex()
    P = sparse_profiles(np.random.default_rng(31), 70, 45)
    assert index.similarity_from_table(P, 1) == (70, 45)
    by_rows = index.similarity_matrix()
    assert index.similarity_from_uploaded(0) == (45, 70)      # the other axis of the same copy: no upload
    S, q = index.similarity_matrix()
    check_values(S, q, np.ascontiguousarray(P.T))
    assert index.similarity_from_uploaded(1) == (70, 45)
    again = index.similarity_matrix()
    assert again[0].tobytes() == by_rows[0].tobytes() and again[1].tobytes() == by_rows[1].tobytes()
    index.top_from_table(np.zeros((3, 4)), 0, 2)              # the ranking's uploaded table is another one
    assert index.similarity_from_uploaded(1) == (70, 45)
    index.close()


def test_two_builds_give_the_same_bytes(hip):
    index = hip.HipIndex()
    table = sparse_profiles(np.random.default_rng(21), 333, 130) - 0.2
    for axis in (0, 1):
        index.similarity_from_table(table, axis)
        one = index.similarity_matrix()
        other = hip.HipIndex()
        other.similarity_from_table(table, axis)
        two = other.similarity_matrix()
        other.close()
        index.similarity_from_uploaded(axis)
        three = index.similarity_matrix()
        for k in (0, 1):
            assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes(), (axis, k)
    index.close()


def test_lifetime_and_errors(hip):
    from east import exceptions
    lib = hip.load()
    dblp, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    index = hip.HipIndex()
    out = np.zeros(2, dtype=np.int64)
    out_p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    # before any score call, on every source; the ranking's source 3 before a similarity build; the fetch
    assert lib.east_hip_similarity_fetch(index._h, None, None) == ERR_NOT_BUILT
    assert index.last_similarity_ms == -1.0
    for source in (hip.GRAPH_SOURCE_AST, hip.GRAPH_SOURCE_COSINE, hip.GRAPH_SOURCE_UPLOADED):
        assert lib.east_hip_similarity_build_resident(index._h, source, 0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_similarity_build_resident(index._h, 7, 0, out_p) == ERR_INVALID
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_SIMILARITY, 0, out_p) == ERR_INVALID
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_SIMILARITY, 1, 3, 0.0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_top_build_resident(index._h, 7, 0, 3, 0.0, out_p) == ERR_INVALID
    texts = [b"alpha beta gamma delta", b"beta gamma epsilon", b"gamma delta alpha alpha"]
    index.build_texts(texts)
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_AST, 0, out_p) == ERR_NOT_BUILT
    cosine = hip.HipCosineIndex(index=index)
    cosine.build_texts(texts)
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_COSINE, 0, out_p) == ERR_NOT_BUILT
    with pytest.raises(exceptions.HipBackendError):
        index.similar(0, 3)
    with pytest.raises(exceptions.HipBackendError):
        cosine.similar(0, 3)
    with pytest.raises(exceptions.HipBackendError):
        index.similarity_matrix()
    qs, qo = hip.pack_queries(["BETA", "GAMMA", "ALPHA", "DELTA"])
    ast_table = index.score_table(qs, qo, True)
    cos_ids, cos_off = cosine.lookup(["BETA", "GAMMA", "ALPHA", "DELTA"]), np.arange(5, dtype=np.int64)
    cos_table = cosine.score_table(cos_ids, cos_off, True)
    tables = index.tables(1)
    # bad arguments build nothing
    for axis in (2, -1):
        assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_AST, axis, out_p) == ERR_INVALID
        assert lib.east_hip_similarity_build_host(index._h, ast_table.ctypes.data_as(dblp), 4, 3, axis, out_p) == ERR_INVALID
    assert lib.east_hip_similarity_build_host(index._h, None, 4, 3, 0, out_p) == ERR_INVALID
    assert lib.east_hip_similarity_build_host(index._h, ast_table.ctypes.data_as(dblp), 0, 3, 0, out_p) == ERR_INVALID
    assert lib.east_hip_similarity_fetch(index._h, None, None) == ERR_NOT_BUILT
    with pytest.raises(exceptions.HipBackendError):
        index.similarity_from_table(np.zeros(5), 0)
    # more members than any device holds a matrix of: refused with the sizes, nothing is allocated
    assert lib.east_hip_similarity_build_host(index._h, np.zeros((1 << 20) + 1).ctypes.data_as(dblp), (1 << 20) + 1, 1, 1, out_p) == ERR_OOM
    message = lib.east_hip_last_error().decode()
    assert "1048577" in message and "bytes" in message
    # a graph, then similarities and their rankings: the graph is still fetchable, unchanged
    rows = np.arange(4, dtype=np.int32)
    graph = index.graph(rows, 0.2, 1, 0.5)
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_AST, 0, out_p) == OK and out.tolist() == [3, 4]
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_AST, 1, out_p) == OK and out.tolist() == [4, 3]
    found = index.similar(1, 2)
    S, q = index.similarity_matrix()
    check_values(S, q, ast_table)
    agree(found, model.select(S, 2, -INF))
    found = cosine.similar(0, 5, 0.0)
    S_cos, q_cos = cosine.similarity_matrix()
    check_values(S_cos, q_cos, np.ascontiguousarray(cos_table.T))
    agree(found, model.select(S_cos, 5, 0.0))
    again = hip.GraphArrays(*(np.empty_like(getattr(graph, name)) for name in hip.GraphArrays.__slots__))
    assert lib.east_hip_graph_fetch(index._h, *(getattr(again, name).ctypes.data_as(i32p) for name in hip.GraphArrays.__slots__)) == OK
    for name in hip.GraphArrays.__slots__:
        assert np.array_equal(getattr(again, name), getattr(graph, name)), name
    # a ranking of the score table made after the similarity ranking is the one fetched: the ranking is the handle's last
    top = index.top(0, 2)
    fetched = hip.TopArrays(*(np.empty_like(getattr(top, name)) for name in hip.TopArrays.__slots__))
    assert lib.east_hip_top_fetch(index._h, fetched.count.ctypes.data_as(i32p), fetched.index.ctypes.data_as(i32p),
                                  fetched.score.ctypes.data_as(dblp)) == OK
    for name in hip.TopArrays.__slots__:
        assert getattr(fetched, name).tobytes() == getattr(top, name).tobytes(), name
    assert top.index.shape == (3, 2) and top.count.tolist() == [2, 2, 2]
    # ... and the matrix is still there, ranked again without a new build
    agree(index.rank_similarity(5, 0.0), model.select(S_cos, 5, 0.0))
    # new keyphrases withdraw the score table, not a finished matrix
    index.set_keyphrases(qs, qo)
    with pytest.raises(exceptions.HipBackendError):
        index.similarity(1)
    kept = index.similarity_matrix()
    assert kept[0].tobytes() == S_cos.tobytes() and kept[1].tobytes() == q_cos.tobytes()
    index.score_resident(True)
    assert index.similarity(1) == (4, 3)
    assert index.similarity_matrix()[0].tobytes() == S.tobytes()
    # the EASA tables, the AST scores and the cosine index are what they were
    after = index.tables(1)
    assert all(np.array_equal(tables[name], after[name]) for name in tables)
    assert index.score_table(qs, qo, True).tobytes() == ast_table.tobytes()
    assert cosine.score_table(cos_ids, cos_off, True).tobytes() == cos_table.tobytes()
    # after east_hip_reset the matrix and the uploaded table are gone
    index.similarity_from_table(ast_table, 0)
    assert lib.east_hip_reset(index._h) == 0
    assert lib.east_hip_similarity_fetch(index._h, None, None) == ERR_NOT_BUILT
    assert index.last_similarity_ms == -1.0
    assert lib.east_hip_similarity_build_resident(index._h, hip.GRAPH_SOURCE_UPLOADED, 0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_SIMILARITY, 1, 3, 0.0, out_p) == ERR_NOT_BUILT
    assert index.similarity_from_table(ast_table, 1) == (4, 3)             # ... and the handle builds the next one
    assert index.similarity_matrix()[0].tobytes() == S.tobytes()
    cosine.close()
    index.close()


def _gaps_allow_a_comparison(table, axis):
    """The precondition of comparing two paths by name: within every segment of the exact matrix neighbouring
    similarities lie further apart than twice the bound (and there is no zero profile)."""
    P = model.profiles_of(table, axis)
    S, q = exact_or_skip(P)
    assert (q > 0).all()
    smallest = INF
    for row in S:
        values = np.sort(row[~np.isnan(row)])
        smallest = min(smallest, float(np.diff(values).min()))
    print("axis %d: smallest gap %.3g, bound %.3g" % (axis, smallest, model.bound(P.shape[1])))
    assert smallest > 2.0 * model.bound(P.shape[1])
    return model.bound(P.shape[1])


def test_device_against_host_on_the_hse_fixture(hip, tmp_path, monkeypatch):
    from east import applications, formatting, main, relevance, utils
    keyphrases, texts = _hse()
    measure = relevance.ASTRelevanceMeasure("easa", True)
    measure.set_text_collection(list(texts.values()))
    table = np.ascontiguousarray(measure.relevance_table([utils.prepare_text(kp) for kp in keyphrases]), dtype=np.float64)
    bounds = {by: _gaps_allow_a_comparison(table, axis) for axis, by in ((0, "text"), (1, "keyphrase"))}
    calls = []
    real = relevance.ASTRelevanceMeasure.relevance_similar

    def counting(self, *a):
        calls.append(1)
        return real(self, *a)

    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "relevance_similar", counting)
    for by, n, threshold in (("text", 3, None), ("keyphrase", 5, 0.2), ("text", 1024, None), ("keyphrase", 1024, None)):
        monkeypatch.delenv("EAST_HIP_SIMILAR", raising=False)
        device = applications.keyphrases_similar(keyphrases, texts, n, by, threshold, relevance.ASTRelevanceMeasure("easa", True))
        monkeypatch.setenv("EAST_HIP_SIMILAR", "host")
        host = applications.keyphrases_similar(keyphrases, texts, n, by, threshold, relevance.ASTRelevanceMeasure("easa", True))
        assert list(device) == list(host) == (list(texts) if by == "text" else keyphrases)
        for member in device:
            assert [o for o, _ in device[member]] == [o for o, _ in host[member]], (by, member)
            assert member not in [o for o, _ in device[member]]
            assert all(abs(a - b) <= bounds[by] for (_, a), (_, b) in zip(device[member], host[member]))
        assert any(device.values())
    assert len(calls) == 4                                    # the default path went through the device, the host path did not
    # the command line, both directions and both formats
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, text in texts.items():
        (tdir / (name + ".txt")).write_bytes(text)
    kp = tmp_path / "kp.txt"
    kp.write_bytes("\n".join(keyphrases).encode("utf-8"))
    decimals = len((formatting._SCORE % 0.5).split(".")[1])
    for options in (["-n", "3"], ["-n", "3", "-f", "csv"], ["-n", "3", "-b", "keyphrase"], ["-n", "3", "-b", "keyphrase", "-f", "csv", "-r", "0.0"]):
        printed = {}
        for mode in ("device", "host"):
            monkeypatch.setenv("EAST_HIP_SIMILAR", mode)
            buf = io.StringIO()
            with redirect_stdout(buf):
                assert main.main(options + ["keyphrases", "similar", str(kp), str(tdir)]) == 0
            printed[mode] = buf.getvalue()
        by = "keyphrase" if "keyphrase" in options else "text"
        strip = (lambda s: s) if decimals < 12 else (lambda s: "\n".join(line.rsplit(",", 1)[0].split(">")[0] for line in s.split("\n")))
        assert strip(printed["device"]) == strip(printed["host"]) and printed["device"].count("\n") > 10, options
        if "csv" in options:
            assert printed["device"].count('",1,') == (len(keyphrases) if by == "keyphrase" else len(texts))
        else:
            assert printed["device"].startswith('<similar by="%s">\n' % by) and 'rank="3"' in printed["device"]
    # -s cosine reaches the device path too
    monkeypatch.setenv("EAST_HIP_SIMILAR", "device")
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main.main(["-n", "2", "-s", "cosine", "-v", "words", "-f", "csv", "keyphrases", "similar", str(kp), str(tdir)]) == 0
    assert buf.getvalue().count("\n") > 10
