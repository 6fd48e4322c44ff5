"""gpu tier: the graph, the ranking and the similarity on ONE handle, each with an uploaded table of its own (csrc/consumer.h;
include/east_hip.h: the ranking's and the similarity's uploaded copies are "NOT the graph's table").  Three different tables
whose shapes lie on both sides of the 64-column word and of the 64-member tile -- 5 x 70, 3 x 130, 70 x 45 -- so that a
consumer that read another's pointer, K or D would give another result or refuse its rows.  The yardsticks are the numpy
contracts of east/applications.py (_graph_from_array, _top_select) and tests/similar_exact.py; the graph and the ranking
are compared exactly, the similarity within the bound it is documented with."""
import ctypes

import numpy as np
import pytest

import similar_exact as model

pytestmark = pytest.mark.gpu

INF = float("inf")
OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
RT, ST, RC = 0.5, 1, 0.4                                    # the graph's thresholds: about half of all pairs are edges
NS = (3, 65)                                                # places per segment: inside one tile, more than one tile holds
DBLP, I32P, I64P = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_int32, ctypes.c_int64))


def _graph_rows(K):
    """Every row once and row 1 a second time, as a keyphrase listed twice."""
    return np.array(list(range(K)) + [1], dtype=np.int32)


def check_graph(found, table):
    from east import applications
    rows = _graph_rows(table.shape[0])
    uniq = ["kp%d" % k for k in range(table.shape[0])]
    kps = [uniq[r] for r in rows]
    want = applications._graph_from_array(kps, applications.ScoreTable(uniq, ["t%d" % d for d in range(table.shape[1])], table),
                                          RC, RT, ST)
    assert found.support.tolist() == (table[rows] >= RT).sum(axis=1).tolist()
    assert len(want["edges"]) > 0
    assert applications.KeyphraseGraph.from_device(kps, found, RC, RT, ST).to_dict() == want


def check_top(found, table, axis, n, threshold=-INF):
    from east import applications
    want = applications._top_select(table, axis, n, threshold)
    assert found.count.tolist() == [len(entries) for entries in want]
    for s, entries in enumerate(want):
        assert found.index[s, :len(entries)].tolist() == [m for m, _ in entries], (axis, n, s)
        assert found.score[s, :len(entries)].tobytes() == np.array([v for _, v in entries], dtype=np.float64).tobytes(), (axis, n, s)
        assert (found.index[s, len(entries):] == -1).all() and (found.score[s, len(entries):] == 0.0).all()


def check_similarity(index, table, axis):
    """The matrix the handle holds is that of `table` by `axis`; -> the fetched matrix."""
    P = model.profiles_of(table, axis)
    S, q = index.similarity_matrix()
    want_S, want_q = model.exact(P)                         # (M * M * L <= 10^6 for all three tables: never None)
    assert S.shape == want_S.shape and np.array_equal(np.isnan(S), np.isnan(want_S))
    worst = float(np.nanmax(np.abs(S - want_S), initial=0.0))
    assert worst <= model.bound(P.shape[1]), (P.shape, worst, model.bound(P.shape[1]))
    assert (np.abs(q - want_q) <= model.gamma(P.shape[1] + 2) * want_q).all()
    return S


def check_rank_of_matrix(found, S, n):
    count, index, score = model.select(S, n, -INF)
    assert found.count.tolist() == count.tolist() and np.array_equal(found.index, index)
    assert found.score.tobytes() == score.tobytes()


def check_all_from_uploaded(index, graph_table, top_table, sim_table):
    """Interleaved: every consumer answers from its own copy, whatever the others did in between."""
    assert index.similarity_from_uploaded(0) == sim_table.shape[::-1]
    check_top(index.top_from_uploaded(1, NS[0]), top_table, 1, NS[0])
    check_graph(index.graph_from_uploaded(_graph_rows(graph_table.shape[0]), RT, ST, RC), graph_table)
    check_similarity(index, sim_table, 0)
    check_top(index.top_from_uploaded(0, NS[1]), top_table, 0, NS[1])
    assert index.similarity_from_uploaded(1) == sim_table.shape
    check_graph(index.graph_from_uploaded(_graph_rows(graph_table.shape[0]), RT, ST, RC), graph_table)
    check_top(index.top_from_uploaded(1, NS[1], 0.5), top_table, 1, NS[1], 0.5)
    check_similarity(index, sim_table, 1)
    check_top(index.top_from_uploaded(0, NS[0]), top_table, 0, NS[0])


def test_frame_messages(hip):
    """The messages of the consumer frame (csrc/consumer.h), word for word, through east_hip_last_error(): what a fetch and
    a *_build_resident call say on a fresh handle, and what the matrix's limit says.  Nothing is launched; the one upload
    is the (2^20 + 1) x 1 table whose matrix is refused before anything is allocated for it."""
    lib = hip.load()
    index = hip.HipIndex()
    h = index._h
    ERR_OOM = -3
    out = np.zeros(4, dtype=np.int64)
    out_p = out.ctypes.data_as(I64P)
    rows = np.zeros(1, dtype=np.int32)

    def said(rc, code, message):
        assert (rc, lib.east_hip_last_error().decode()) == (code, message)

    said(lib.east_hip_graph_fetch(h, None, None, None, None, None), ERR_NOT_BUILT, "no keyphrase graph has been built on this handle")
    said(lib.east_hip_top_fetch(h, None, None, None), ERR_NOT_BUILT, "no keyphrase ranking has been built on this handle")
    said(lib.east_hip_similarity_fetch(h, None, None), ERR_NOT_BUILT, "no similarity matrix has been built on this handle")
    said(lib.east_hip_related_fetch(h, None, None, None), ERR_NOT_BUILT, "no relatedness matrix has been built on this handle")
    said(lib.east_hip_text_similarity_fetch(h, None, None, None), ERR_NOT_BUILT, "no text similarity matrix has been built on this handle")
    said(lib.east_hip_clusters_fetch(h, None, None, None), ERR_NOT_BUILT, "no clusters have been built on this handle")

    resident = {
        "keyphrase graph": lambda s: lib.east_hip_graph_build_resident(h, s, rows.ctypes.data_as(I32P), 1, RT, float(ST), RC, out_p),
        "ranked keyphrases": lambda s: lib.east_hip_top_build_resident(h, s, 0, 3, 0.0, out_p),
        "similarity": lambda s: lib.east_hip_similarity_build_resident(h, s, 0, out_p),
        "clusters": lambda s: lib.east_hip_clusters_build_resident(h, s, out_p),
    }
    missing = {0: "no score table is resident (score the keyphrases first)",
               1: "no cosine score table is resident (score the keyphrases first)",
               2: "no host table has been uploaded to this handle",
               3: "no similarity matrix has been built on this handle",
               4: "no relatedness matrix has been built on this handle",
               5: "no text similarity matrix has been built on this handle"}
    for who, call in resident.items():
        takes_matrices = who in ("ranked keyphrases", "clusters")
        for source in (0, 1, 2, 3, 4, 5, 7):
            if who == "clusters" and source in (0, 1, 7):       # (the clusters refuse what is no matrix in their own words)
                said(call(source), ERR_INVALID, "clusters: the source is not a square matrix of members")
            elif source in (0, 1, 2) or (takes_matrices and source in (3, 4, 5)):
                said(call(source), ERR_NOT_BUILT, "%s: %s" % (who, missing[source]))
            else:
                said(call(source), ERR_INVALID, "%s: unknown table source" % who)

    M = (1 << 20) + 1
    column = np.zeros((M, 1))
    said(lib.east_hip_similarity_build_host(h, column.ctypes.data_as(DBLP), M, 1, 1, out_p), ERR_OOM,
         "similarity: the matrix of 1048577 x 1048577 members needs 8796109799432 bytes, which the device does not have")
    index.close()


def test_three_uploaded_tables_on_one_handle(hip):
    lib = hip.load()
    index = hip.HipIndex()
    h = index._h
    rng = np.random.default_rng(5070)
    graph_table, top_table, sim_table = rng.random((5, 70)), rng.random((3, 130)), rng.random((70, 45))
    out = np.zeros(2, dtype=np.int64)
    out_p = out.ctypes.data_as(I64P)
    rows = _graph_rows(5)

    # ---- the uploads, each checked as it is made
    check_graph(index.graph_from_table(graph_table, rows, RT, ST, RC), graph_table)
    check_top(index.top_from_table(top_table, 0, NS[0]), top_table, 0, NS[0])
    assert index.similarity_from_table(sim_table, 1) == (70, 45)
    check_similarity(index, sim_table, 1)
    # ---- each consumer reads its own copy
    check_all_from_uploaded(index, graph_table, top_table, sim_table)

    # ---- a refused host call leaves every copy usable
    other = rng.random((7, 66))
    assert lib.east_hip_top_build_host(h, other.ctypes.data_as(DBLP), 7, 66, 2, 3, 0.0, out_p) == ERR_INVALID
    assert lib.east_hip_similarity_build_host(h, other.ctypes.data_as(DBLP), 7, 66, -1, out_p) == ERR_INVALID
    check_all_from_uploaded(index, graph_table, top_table, sim_table)
    # (the graph checks its rows behind the upload: the call is refused, its table IS the uploaded one from then on, and
    # the graph in front of it is withdrawn)
    bad_rows = np.array([0, 7], dtype=np.int32)
    assert lib.east_hip_graph_build_host(h, other.ctypes.data_as(DBLP), 7, 66, bad_rows.ctypes.data_as(I32P), 2, RT, float(ST), RC,
                                         out_p) == ERR_INVALID
    assert lib.east_hip_graph_fetch(h, None, None, None, None, None) == ERR_NOT_BUILT
    check_graph(index.graph_from_uploaded(_graph_rows(7), RT, ST, RC), other)
    check_all_from_uploaded(index, other, top_table, sim_table)

    # ---- the matrix as a ranking source; the ranking's own table is untouched by it
    assert index.similarity_from_uploaded(0) == (45, 70)
    S = check_similarity(index, sim_table, 0)
    for n in NS:
        check_rank_of_matrix(index.rank_similarity(n), S, n)
    check_top(index.top_from_uploaded(1, NS[1]), top_table, 1, NS[1])
    check_rank_of_matrix(index.rank_similarity(NS[0]), S, NS[0])

    # ---- reset drops the three results and the three copies (and the synonyms' time with them)
    synonyms = hip.HipSynonyms(index=index)
    synonyms.build([0, 1, 2], [0, 0, 0], [1, 2, 0], [0], 3)
    synonyms.pairs([0, 1, 2], 0.0)
    assert min(index.last_graph_ms, index.last_top_ms, index.last_similarity_ms, synonyms.last_ms) > 0.0
    assert lib.east_hip_reset(h) == OK
    uploaded = hip.GRAPH_SOURCE_UPLOADED
    assert lib.east_hip_graph_build_resident(h, uploaded, rows.ctypes.data_as(I32P), rows.size, RT, float(ST), RC, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_top_build_resident(h, uploaded, 0, 3, 0.0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_similarity_build_resident(h, uploaded, 0, out_p) == ERR_NOT_BUILT
    assert lib.east_hip_graph_fetch(h, None, None, None, None, None) == ERR_NOT_BUILT
    assert lib.east_hip_top_fetch(h, None, None, None) == ERR_NOT_BUILT
    assert lib.east_hip_similarity_fetch(h, None, None) == ERR_NOT_BUILT
    assert (index.last_graph_ms, index.last_top_ms, index.last_similarity_ms, synonyms.last_ms) == (-1.0, -1.0, -1.0, -1.0)

    # ---- and the handle takes the next tables
    check_graph(index.graph_from_table(graph_table, rows, RT, ST, RC), graph_table)
    check_top(index.top_from_table(top_table, 1, NS[1]), top_table, 1, NS[1])
    assert index.similarity_from_table(sim_table, 0) == (45, 70)
    check_similarity(index, sim_table, 0)
    check_all_from_uploaded(index, graph_table, top_table, sim_table)
    index.close()
