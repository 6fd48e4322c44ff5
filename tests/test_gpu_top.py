"""gpu tier: ranked keyphrases selected on the device (csrc/top.h through include/east_hip.h, "Ranked keyphrases").  The
yardstick is the contract written out here -- per segment the members with score >= threshold (a NaN never), by score
descending and member index ascending among equal scores (-0.0 == 0.0), the first n -- with np.lexsort over the eligible
members; it never calls the project's own host path.  Counts and indices are compared with ==, scores as bytes."""
import ctypes
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

INF = float("inf")
OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
NS = (1, 2, 10, 64, 65, 1024)


def orders(table, axis, threshold):
    """Per segment (axis 0: a column, axis 1: a row) the eligible members in the contract's order."""
    found = []
    with np.errstate(invalid="ignore"):
        for values in (table.T if axis == 0 else table):
            eligible = np.flatnonzero(values >= threshold)
            found.append(eligible[np.lexsort((eligible, -values[eligible]))])
    return found


def expected(table, axis, order, n):
    """(count[S], index[S, n], score[S, n]) of the first n of every order: -1 and 0.0 behind the count."""
    segments = table.T if axis == 0 else table
    S = len(order)
    count = np.zeros(S, dtype=np.int32)
    index = np.full((S, n), -1, dtype=np.int32)
    score = np.zeros((S, n), dtype=np.float64)
    for s, o in enumerate(order):
        c = min(n, o.size)
        count[s] = c
        index[s, :c] = o[:c]
        score[s, :c] = segments[s][o[:c]]
    return count, index, score


def agree(found, want, what=None):
    count, index, score = want
    assert found.count.dtype == np.int32 and found.index.dtype == np.int32 and found.score.dtype == np.float64
    assert found.index.shape == index.shape and found.score.shape == score.shape, what
    assert found.count.tolist() == count.tolist(), what
    assert np.array_equal(found.index, index), what
    assert found.score.tobytes() == score.tobytes(), what


def check_uploaded(index, table, ns=NS, thresholds=(-INF,), what=None):
    """Upload once, then every axis, n and threshold from the uploaded copy."""
    first = True
    for axis in (0, 1):
        for threshold in thresholds:
            order = orders(table, axis, threshold)
            for n in ns:
                found = index.top_from_table(table, axis, n, threshold) if first else index.top_from_uploaded(axis, n, threshold)
                first = False
                agree(found, expected(table, axis, order, n), (what, table.shape, axis, n, threshold))


def mixed_table(rng, K, D):
    """Random scores with many exact ties, a few negative ones and both zeros."""
    table = rng.random((K, D))
    ties = rng.random((K, D))
    table[ties < 0.3] = rng.choice([0.0, -0.0, 0.25, 0.5, -0.5], size=int((ties < 0.3).sum()))
    return table


@pytest.mark.parametrize("K,D", [(1, 1), (2, 63), (63, 64), (64, 65), (65, 256), (257, 1000), (1000, 64), (1000, 4097),
                                 (1, 4097), (1000, 1), (257, 65)])
def test_host_tables_on_both_axes(hip, K, D):
    """Every segment length around the 64-member tiles and the 64-column strips, n below, at and above the tile and above
    the segment, with and without a threshold that occurs in the table."""
    index = hip.HipIndex()
    table = mixed_table(np.random.default_rng(100 * K + D), K, D)
    big = K * D > 500000
    check_uploaded(index, table, ns=(1, 10, 65, 1024) if big else NS, thresholds=(-INF,) if big else (-INF, 0.25))
    assert 0.0 < index.last_top_ms < 1000.0
    index.close()


def test_ties_are_decided_by_the_member_index(hip):
    index = hip.HipIndex()
    rng = np.random.default_rng(3)
    # one value everywhere: the first n members in index order
    same = np.full((300, 70), 0.125)
    found = index.top_from_table(same, 0, 65, -INF)
    assert np.array_equal(found.index, np.tile(np.arange(65, dtype=np.int32), (70, 1))) and found.count.tolist() == [65] * 70
    found = index.top_from_uploaded(1, 10, -INF)
    assert np.array_equal(found.index, np.tile(np.arange(10, dtype=np.int32), (300, 1)))
    check_uploaded(index, same, ns=(1, 64, 65, 1024))
    # three values
    check_uploaded(index, rng.choice([0.0, 0.25, 0.5], size=(257, 130)), thresholds=(-INF, 0.25, 0.5))
    # -0.0 and +0.0 are equal: the index decides, and the bytes that come back keep the sign
    zeros = np.where(rng.random((200, 66)) < 0.5, -0.0, 0.0)
    zeros[::7] = -1.0
    zeros[5::11, ::3] = 0.5
    check_uploaded(index, zeros, ns=(1, 2, 10, 65, 1024), thresholds=(-INF, 0.0, -0.0))
    found = index.top_from_table(np.array([[-0.0], [0.0], [-0.0], [1.0]]), 0, 3, 0.0)
    assert found.index.tolist() == [[3, 0, 1]] and np.signbit(found.score).tolist() == [[False, True, False]]
    index.close()


def test_nan_thresholds_and_infinities(hip):
    index = hip.HipIndex()
    rng = np.random.default_rng(4)
    table = rng.random((130, 67))
    table[rng.random(table.shape) < 0.3] = np.nan
    table[17] = np.nan                                       # a NaN row and a NaN column: never eligible
    table[:, 5] = np.nan
    table[64, 64] = INF
    table[65, 65] = -INF
    table[3, 66] = -np.nan
    present = float(table[20][np.isfinite(table[20])][0])
    check_uploaded(index, table, ns=(1, 10, 65, 1024), thresholds=(-INF, present, np.nextafter(present, 2.0), INF, 2.0))
    found = index.top_from_uploaded(0, 10, 2.0)              # above everything but +inf
    assert found.count.sum() == 1 and found.count[64] == 1 and found.index[64, 0] == 64
    found = index.top_from_uploaded(0, 1024, -INF)
    with np.errstate(invalid="ignore"):
        assert found.count.tolist() == (table >= -INF).sum(axis=0).tolist() and found.count[5] == 0
    assert (found.index[5] == -1).all() and found.score[5].tobytes() == np.zeros(1024).tobytes()
    found = index.top_from_table(rng.random((40, 30)), 1, 5, 1.5)      # a threshold above all: every count is 0
    assert found.count.tolist() == [0] * 40 and (found.index == -1).all() and not found.score.any()
    index.close()


def _tiled_table():
    """1000 x 70.  Even columns: the ten best members are the last ten rows, the last tile of every tiling.  Odd columns:
    one good member in every tile of 7 (and so in every tile of 64), 143 of them, better the later they come."""
    rng = np.random.default_rng(9)
    table = rng.random((1000, 70)) * 0.4
    table[990:, 0::2] = 0.9 + 0.01 * np.arange(10)[:, None]
    spread = np.arange(5, 1000, 7)
    table[spread, 1::2] = 0.5 + spread[:, None] / 4096.0
    return table


def test_the_result_does_not_depend_on_the_tile(hip):
    lib = hip.load()
    index = hip.HipIndex()
    table = _tiled_table()
    n = 100                                                  # more than a tile holds
    try:
        for source, axis in ((table, 0), (np.ascontiguousarray(table.T), 1)):
            want = expected(source, axis, orders(source, axis, 0.45), n)
            assert want[0].tolist() == [10, 100] * 35
            assert want[1][0, :10].tolist() == list(range(999, 989, -1)) and want[1][1, :3].tolist() == [999, 992, 985]
            seen = []
            for tile in (7, 64, 1000, 0):
                assert lib.east_hip_debug_set_top_tile(tile) == 0
                found = index.top_from_table(source, axis, n, 0.45)
                agree(found, want, (axis, tile))
                seen.append(found.count.tobytes() + found.index.tobytes() + found.score.tobytes())
                agree(index.top_from_uploaded(axis, 1024, -INF), expected(source, axis, orders(source, axis, -INF), 1024), (axis, tile))
            assert len(set(seen)) == 1
        assert lib.east_hip_debug_set_top_tile(1) == 0       # a member a tile: the merge does everything
        small = mixed_table(np.random.default_rng(12), 70, 9)
        check_uploaded(index, small, ns=(1, 10, 65))
    finally:
        lib.east_hip_debug_set_top_tile(0)
    index.close()


def test_two_builds_give_the_same_bytes(hip):
    index = hip.HipIndex()
    table = mixed_table(np.random.default_rng(21), 777, 300)
    for axis in (0, 1):
        one = index.top_from_table(table, axis, 65, 0.25)
        other = hip.HipIndex()
        two = other.top_from_table(table, axis, 65, 0.25)
        three = index.top_from_uploaded(axis, 65, 0.25)
        other.close()
        for name in hip.TopArrays.__slots__:
            assert getattr(one, name).tobytes() == getattr(two, name).tobytes() == getattr(three, name).tobytes(), name
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
    present = float(np.sort(table.ravel())[table.size // 2])
    for axis in (0, 1):
        for threshold in (-INF, present, 0.25):
            order = orders(table, axis, threshold)
            for n in (1, 3, 10, 64):
                found = measure.relevance_top(prepared, axis, n, threshold)
                agree(found, expected(table, axis, order, n), (axis, n, threshold))
    assert measure.index.last_top_ms > 0.0
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
    for weighting in ("tf-idf", "tf"):
        table = _resident(relevance.CosineRelevanceMeasure("words", weighting, stopwords=[]), keyphrases, texts)
        assert table.max() > 0.0


def test_rankings_and_graphs_live_side_by_side(hip):
    lib = hip.load()
    i32p, dblp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    index = hip.HipIndex()
    texts = [b"alpha beta gamma delta", b"beta gamma epsilon", b"gamma delta alpha alpha"]
    index.build_texts(texts)
    cosine = hip.HipCosineIndex(index=index)
    cosine.build_texts(texts)
    qs, qo = hip.pack_queries(["BETA", "GAMMA", "ALPHA", "DELTA"])
    ast_table = index.score_table(qs, qo, True)
    cos_ids, cos_off = cosine.lookup(["BETA", "GAMMA", "ALPHA", "DELTA"]), np.arange(5, dtype=np.int64)
    cos_table = cosine.score_table(cos_ids, cos_off, True)
    tables = index.tables(1)
    rows = np.arange(4, dtype=np.int32)

    def fetch_graph(like):
        again = hip.GraphArrays(*(np.empty_like(getattr(like, name)) for name in hip.GraphArrays.__slots__))
        assert lib.east_hip_graph_fetch(index._h, *(getattr(again, name).ctypes.data_as(i32p) for name in hip.GraphArrays.__slots__)) == OK
        return again

    def fetch_top(like):
        again = hip.TopArrays(*(np.empty_like(getattr(like, name)) for name in hip.TopArrays.__slots__))
        assert lib.east_hip_top_fetch(index._h, again.count.ctypes.data_as(i32p), again.index.ctypes.data_as(i32p),
                                      again.score.ctypes.data_as(dblp)) == OK
        return again

    # a graph, then rankings of all three sources: the graph is still fetchable, unchanged
    graph = index.graph(rows, 0.2, 1, 0.5)
    other = mixed_table(np.random.default_rng(8), 90, 70)
    agree(index.top(0, 3), expected(ast_table, 0, orders(ast_table, 0, -INF), 3))
    agree(cosine.top(1, 2, 0.05), expected(cos_table, 1, orders(cos_table, 1, 0.05), 2))
    top = index.top_from_table(other, 0, 10, 0.25)
    agree(top, expected(other, 0, orders(other, 0, 0.25), 10))
    for name in hip.GraphArrays.__slots__:
        assert np.array_equal(getattr(fetch_graph(graph), name), getattr(graph, name)), name
    # graphs of a resident and of an uploaded table, then the ranking again: unchanged; the two uploaded tables are apart
    index.graph(rows, 0.3, 1, 0.6)
    index.graph_from_table(ast_table, rows, 0.2, 1, 0.5)
    for name in hip.TopArrays.__slots__:
        assert getattr(fetch_top(top), name).tobytes() == getattr(top, name).tobytes(), name
    agree(index.top_from_uploaded(1, 5, -INF), expected(other, 1, orders(other, 1, -INF), 5))
    graph_2 = index.graph_from_uploaded(rows, 0.2, 1, 0.5)
    for name in hip.GraphArrays.__slots__:
        assert np.array_equal(getattr(graph_2, name), getattr(graph, name)), name
    # the EASA tables, the AST scores and the cosine index are what they were
    after = index.tables(1)
    assert all(np.array_equal(tables[name], after[name]) for name in tables)
    assert index.score_table(qs, qo, True).tobytes() == ast_table.tobytes()
    assert cosine.score_table(cos_ids, cos_off, True).tobytes() == cos_table.tobytes()
    cosine.close()
    index.close()


def test_lifetime_and_errors(hip):
    from east import exceptions
    lib = hip.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    index = hip.HipIndex()
    count = np.zeros(4, dtype=np.int32)
    out = np.zeros(2, dtype=np.int64)
    out_p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    # before any score call, on every source; after a build; after new keyphrases
    assert lib.east_hip_top_fetch(index._h, count.ctypes.data_as(i32p), None, None) == ERR_NOT_BUILT
    assert index.last_top_ms == -1.0
    for source in (hip.GRAPH_SOURCE_AST, hip.GRAPH_SOURCE_COSINE, hip.GRAPH_SOURCE_UPLOADED):
        assert lib.east_hip_top_build_resident(index._h, source, 0, 3, 0.0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_top_build_resident(index._h, 7, 0, 3, 0.0, out_p) == ERR_INVALID
    index.build_texts([b"alpha beta gamma delta", b"beta gamma epsilon"])
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_AST, 0, 3, 0.0, out_p) == ERR_NOT_BUILT
    cosine = hip.HipCosineIndex(index=index)
    cosine.build_texts([b"alpha beta gamma delta", b"beta gamma epsilon"])
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_COSINE, 0, 3, 0.0, out_p) == ERR_NOT_BUILT
    with pytest.raises(exceptions.HipBackendError):
        index.top(0, 3)
    with pytest.raises(exceptions.HipBackendError):
        cosine.top(0, 3)
    qs, qo = hip.pack_queries(["BETA", "GAMMA", "ALPHA"])
    table = index.score_table(qs, qo, True)
    # bad arguments: nothing is built by them
    for axis, n, threshold in ((0, 0, 0.0), (0, 1025, 0.0), (1, -1, 0.0), (0, 3, float("nan")), (2, 3, 0.0), (-1, 3, 0.0)):
        assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_AST, axis, n, threshold, out_p) == ERR_INVALID, (axis, n, threshold)
        dblp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert lib.east_hip_top_build_host(index._h, dblp, 3, 2, axis, n, threshold, out_p) == ERR_INVALID
    assert lib.east_hip_top_build_host(index._h, None, 3, 2, 0, 3, 0.0, out_p) == ERR_INVALID
    assert lib.east_hip_top_build_host(index._h, table.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0, 2, 0, 3, 0.0, out_p) == ERR_INVALID
    with pytest.raises(exceptions.HipBackendError):
        index.top_from_table(np.zeros(5), 0, 3)
    # out[0] = the segments, out[1] = the sum of the counts
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_AST, 0, 2, -INF, out_p) == OK and out.tolist() == [2, 4]
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_AST, 1, 1024, -INF, out_p) == OK and out.tolist() == [3, 6]
    first = index.top(1, 2, 0.1)
    agree(first, expected(table, 1, orders(table, 1, 0.1), 2))
    assert out.tolist() == [3, 6]
    index.set_keyphrases(qs, qo)                               # new keyphrases: the table of the old ones is withdrawn
    with pytest.raises(exceptions.HipBackendError):
        index.top(1, 2, 0.1)
    assert lib.east_hip_top_fetch(index._h, None, None, None) == OK         # ... the last ranking is still there
    index.score_resident(True)
    agree(index.top(1, 2, 0.1), (first.count, first.index, first.score))
    # after east_hip_reset the ranking and the uploaded table are gone
    index.top_from_table(table, 0, 2)
    assert lib.east_hip_reset(index._h) == 0
    assert lib.east_hip_top_fetch(index._h, None, None, None) == ERR_NOT_BUILT
    assert index.last_top_ms == -1.0
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_UPLOADED, 0, 3, 0.0, out_p) == ERR_NOT_BUILT
    agree(index.top_from_table(table, 1, 2, 0.1), (first.count, first.index, first.score))      # ... and the handle builds the next one
    cosine.close()
    index.close()


def _both_paths(monkeypatch, make_measure, keyphrases, texts, n, by, threshold):
    from east import applications
    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    device = applications.keyphrases_top(keyphrases, texts, n, by, threshold, make_measure())
    monkeypatch.setenv("EAST_HIP_TOP", "host")
    host = applications.keyphrases_top(keyphrases, texts, n, by, threshold, make_measure())
    monkeypatch.delenv("EAST_HIP_TOP")
    assert device == host
    assert [repr(s) for e in device.values() for _, s in e] == [repr(s) for e in host.values() for _, s in e]
    return device


def test_keyphrases_top_on_the_device_is_the_host_path(hip, monkeypatch):
    from east import relevance
    keyphrases, texts = _hse()
    listed = keyphrases[:4] + ["", keyphrases[1]] + keyphrases[4:]
    calls = []
    real = relevance.ASTRelevanceMeasure.relevance_top

    def counting(self, *a):
        calls.append(1)
        return real(self, *a)

    monkeypatch.setattr(relevance.ASTRelevanceMeasure, "relevance_top", counting)
    for by, n, threshold in (("text", 3, None), ("keyphrase", 5, 0.2), ("text", 1024, 0.1), ("keyphrase", 1, None)):
        top = _both_paths(monkeypatch, lambda: relevance.ASTRelevanceMeasure("easa", True), listed, texts, n, by, threshold)
        assert list(top) == (list(texts) if by == "text" else keyphrases)
        assert all(len(e) <= n for e in top.values()) and any(top.values())
    assert len(calls) == 4                                   # the default path went through the device, the host path did not
    cos = load_golden("cosine.json")["cli"]["keyphrases"]
    top = _both_paths(monkeypatch, lambda: relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[]), cos, texts, 3, "text", 0.01)
    assert any(top.values())


def test_cli_top_in_both_formats(hip, tmp_path, monkeypatch):
    from east import main
    keyphrases, texts = _hse()
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, text in texts.items():
        (tdir / (name + ".txt")).write_bytes(text)
    kp = tmp_path / "kp.txt"
    kp.write_bytes("\n".join(keyphrases).encode("utf-8"))
    for options in (["-n", "3"], ["-n", "3", "-f", "csv"], ["-n", "3", "-b", "keyphrase", "-r", "0.2"],
                    ["-n", "3", "-b", "keyphrase", "-f", "csv"], ["-n", "2", "-s", "cosine", "-v", "words", "-f", "csv"]):
        printed = {}
        for mode in ("device", "host"):
            monkeypatch.setenv("EAST_HIP_TOP", mode)
            buf = io.StringIO()
            with redirect_stdout(buf):
                assert main.main(options + ["keyphrases", "top", str(kp), str(tdir)]) == 0
            printed[mode] = buf.getvalue()
        assert printed["device"] == printed["host"] and printed["device"].count("\n") > 10, options
        by = "keyphrase" if "keyphrase" in options else "text"
        if "csv" in options:
            assert printed["device"].count(",3,") == (0 if "2" in options else len(keyphrases) if by == "keyphrase" else len(texts))
        else:
            assert printed["device"].startswith('<top by="%s">\n' % by) and 'rank="3"' in printed["device"]
