"""GPU tier: the characteristic terms on the device (csrc/terms.h; include/east_hip.h, "Characteristic terms").  Every case
does three checks: (1) east_hip_terms_fetch_vectors against tests/terms_exact.py -- the same (group, unit, texts) structure
exactly, every value within (texts_gu + max ceil(p_d / 64) / 2 + 48) * 2^-53 * exact; (2) east_hip_terms_fetch compared with ==
against the model's ranking function applied to the device's own vectors, nothing skipped for closeness; (3) the same bytes
under east_hip_debug_set_terms_select(1) and from a second build.

Largest share of the bound seen over all cases on an MI355X: see README, "Characteristic terms"."""
import numpy as np
import pytest

import cosine_exact
import terms_exact as model

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
SHARES = {}


def _index(hip, name):
    """A cosine index of a collection of the model, in its vector space."""
    texts, stop, stems = model.collections()[name]
    index = hip.HipCosineIndex()
    index.build_texts(list(texts), sorted(cosine_exact.prepared_stopwords(stop)))
    if stems:
        m = model.model_of(name)
        assert index.terms() == m.terms
        index.set_classes(m.term_class, m.n_classes)
    return index


def _result(index, tfidf, n, min_texts, group, G):
    found = index.terms(tfidf, n, min_texts, group, G)
    return found, tuple(a.tobytes() for a in (found.members, found.count, found.unit, found.value, found.texts, found.df))


def _three_checks(hip, index, name, tfidf, grouping=(None, None), n=10, min_texts=1, ex=None):
    """-> (TermArrays, its bytes, the model)"""
    group, G = grouping
    stems = model.collections()[name][2]
    m = model.model_of(name)
    ex = ex or model.exact(m, tfidf, group, G, stems)
    found, first = _result(index, tfidf, n, min_texts, group, G)
    info = found.info
    assert info["n_docs"] == m.n_docs and info["groups"] == len(ex.members) and info["units"] == m.space(stems)[2]
    assert info["postings"] == m.space(stems)[3] and info["entries"] == ex.unit.size
    assert info["passing"] == int((ex.texts >= min_texts).sum()) and info["sorted"] <= info["passing"]
    assert info["grouping_sort_skipped"] == (1 if group is None else 0) and info["launches"] > 0
    assert np.array_equal(found.members, ex.members)
    # (1) the sums
    offsets, unit, value, texts = index.terms_vectors()
    share = model.check_vectors(offsets, unit, value, texts, ex)
    SHARES[name] = max(SHARES.get(name, 0.0), share)
    print("%s, %s, G = %d, n = %d: %.3g of the bound (largest so far over all cases: %.3g)"
          % (name, "tf-idf" if tfidf else "tf", len(ex.members), n, share, max(SHARES.values())))
    # (2) the ranking, of the device's own vectors
    count, r_unit, r_value, r_texts, r_df = model.ranked(offsets, unit, value, texts, ex.df, min_texts, n)
    assert np.array_equal(found.count, count) and np.array_equal(found.unit, r_unit) and np.array_equal(found.texts, r_texts)
    assert np.array_equal(found.df, r_df)
    assert np.array_equal(np.isnan(found.value), np.isnan(r_value))
    assert found.value[~np.isnan(r_value)].tobytes() == r_value[~np.isnan(r_value)].tobytes()
    # (3) without the pre-selection, and again
    lib = hip.load()
    try:
        assert lib.east_hip_debug_set_terms_select(1) == OK
        plain, second = _result(index, tfidf, n, min_texts, group, G)
        assert plain.info["sorted"] == plain.info["passing"]
    finally:
        lib.east_hip_debug_set_terms_select(0)
    assert second == first and _result(index, tfidf, n, min_texts, group, G)[1] == first
    assert index.last_terms_ms() > 0.0
    return found, first, ex


@pytest.mark.parametrize("name", ("tile edges 64", "spread"))
def test_groupings(hip, name):
    index = _index(hip, name)
    D = len(model.collections()[name][0])
    for tfidf in (True, False):
        _, null, ex = _three_checks(hip, index, name, tfidf)
        for label, grouping in model.groupings(D).items():
            found, explicit, _ = _three_checks(hip, index, name, tfidf, grouping, ex=ex if label == "identity" else None)
            if label == "identity":
                assert explicit == null                           # (the same bytes; the info says which path ran)
            if label == "one group" and name == "spread":         # (40 values, all different: the selection leaves few to sort)
                assert found.info["sorted"] < found.info["passing"]
            if label == "empty groups":
                assert found.count[[0, 3, 7, 8]].tolist() == [0] * 4 and (found.unit[[0, 3, 7, 8]] == -1).all()
                assert np.isnan(found.value[[0, 3, 7, 8]]).all() and (found.count[[1, 2, 4, 5, 6]] > 0).all()
    index.close()


@pytest.mark.parametrize("L", model.RUN_LENGTHS)
def test_run_lengths(hip, L):
    """A run across a wavefront, a workgroup and a scan tile: one word shared by L one-word texts of one group."""
    name = "runs %d" % L
    index = _index(hip, name)
    for tfidf in (False, True):
        found, _, _ = _three_checks(hip, index, name, tfidf, model.run_group(L))
        assert found.count.tolist() == [1, 2] and found.texts[0, 0] == L and found.df[0, 0] == L
        if not tfidf:
            assert found.value[0, 0] == 1.0                       # (L times 1.0, divided by L)
    _three_checks(hip, index, name, True)                         # (per text: L + 1 segments of one and two entries)
    index.close()


def test_segment_lengths(hip):
    """n - 1, n and n + 1 entries for n = 1, 10, 1024; a histogram tile's entries and one either side."""
    index = _index(hip, "segments")
    for n in model.SEGMENT_N:
        for tfidf in (False, True):
            found, _, _ = _three_checks(hip, index, "segments", tfidf, n=n)
            assert found.count.tolist() == [min(n, m) for m in model.SEGMENT_LENGTHS]
    _three_checks(hip, index, "segments", True, ([0] * len(model.SEGMENT_LENGTHS), 1), n=10)
    index.close()


def test_long_segment_beside_short_ones(hip):
    index = _index(hip, "long text")
    D = len(model.collections()["long text"][0])
    _three_checks(hip, index, "long text", True)
    _three_checks(hip, index, "long text", False, n=1024)
    _three_checks(hip, index, "long text", True, ([0] * D, 1), n=10)
    index.close()


def test_ties(hip):
    """A group all of whose entries have one value (one digest bin, longer than a tile: the cut goes by unit id); equal values
    across the n-th place; two groups with identical vectors."""
    index = _index(hip, "ties")
    for n in (2, 4, 10):
        found, _, _ = _three_checks(hip, index, "ties", False, n=n)
        assert found.unit[0].tolist() == list(range(n)) and len(set(found.value[0].tolist())) == 1
        assert found.info["sorted"] >= 5000                       # (the whole bin goes through the sort)
        assert found.unit[2, :min(n, 3)].tobytes() == found.unit[3, :min(n, 3)].tobytes()
        assert found.value[2, :min(n, 3)].tobytes() == found.value[3, :min(n, 3)].tobytes()
    assert found.value[1, 0] == found.value[1, 2] > found.value[1, 3] == found.value[1, 5]
    _three_checks(hip, index, "ties", True, n=4)
    _three_checks(hip, index, "ties", False, ([0, 1, 2, 2], 3), n=2)
    index.close()


def test_min_texts(hip):
    name = "tile edges 64"
    index = _index(hip, name)
    grouping = model.groupings(64)["four equal"]
    ex = model.exact(model.model_of(name), True, *grouping)
    for min_texts in (1, 2, 16, 17):
        found, _, _ = _three_checks(hip, index, name, True, grouping, min_texts=min_texts, ex=ex)
        assert found.members.tolist() == [16] * 4
        if min_texts == 17:                                       # no entry: count 0 and nothing else touched
            assert found.count.tolist() == [0] * 4 and (found.unit == -1).all() and (found.texts == -1).all() and (found.df == -1).all()
            assert np.isnan(found.value).all() and found.info["passing"] == 0 and found.info["entries"] > 0
        else:
            assert (found.texts[found.unit >= 0] >= min_texts).all()
    index.close()


@pytest.mark.parametrize("name", ("document shapes", "stems"))
def test_document_shapes_and_both_spaces(hip, name):
    index = _index(hip, name)
    D = len(model.collections()[name][0])
    for tfidf in (False, True, False):                            # one build after the other on one handle, alternating weightings
        found, _, _ = _three_checks(hip, index, name, tfidf)
        for label in ("one group", "empty groups", "permuted"):
            _three_checks(hip, index, name, tfidf, model.groupings(D)[label])
    if name == "document shapes":                                 # the empty text, the stopwords, one kept token, the twins
        found, _, _ = _three_checks(hip, index, name, True)
        assert found.count[:3].tolist() == [0, 0, 1] and found.value[2, 0] == 1.0
        assert found.unit[3].tobytes() == found.unit[4].tobytes() and found.value[3].tobytes() == found.value[4].tobytes()
    index.close()


def test_lifecycle(hip):
    lib = hip.load()
    index = hip.HipCosineIndex()
    h = index._h
    out = np.zeros(10, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)

    def build(weighting=1, group=None, G=None, n=3, min_texts=1):
        g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
        rc = lib.east_hip_terms_build(h, weighting, None if g is None else g.ctypes.data_as(hip._c_i32p),
                                      index.n_docs if G is None else G, n, min_texts, p_out)
        return rc, lib.east_hip_last_error().decode()

    def fetch():
        return lib.east_hip_terms_fetch(h, *[None] * 6), lib.east_hip_terms_fetch_vectors(h, *[None] * 4)

    assert build(G=1) == (ERR_NOT_BUILT, "no cosine index has been built on this handle")
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT)
    assert lib.east_hip_last_error().decode() == "no characteristic terms have been built on this handle"
    assert lib.east_hip_last_terms_ms(h) == -1.0
    assert lib.east_hip_terms_build(None, 1, None, 1, 3, 1, p_out) == ERR_INVALID
    assert lib.east_hip_debug_set_terms_select(2) == ERR_INVALID
    texts = model.tce.document_shapes()
    stop = sorted(cosine_exact.prepared_stopwords(model.tce.STOPWORDS))
    index.build_texts(list(texts), stop)
    D = len(texts)
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT)
    want = _result(index, True, 3, 1, None, None)[1]

    # every refusal names what is wrong and leaves the earlier result fetchable
    refused = [(dict(weighting=2), "unknown weighting"), (dict(weighting=-1), "unknown weighting"), (dict(n=0), "n must be 1 .. 1024"),
               (dict(n=1025), "n must be 1 .. 1024"), (dict(min_texts=0), "min_texts must be at least 1"),
               (dict(G=0), "n_groups must be at least 1"), (dict(G=D + 1), "%d, not %d" % (D, D + 1)),
               (dict(group=[0] * (D - 1) + [2], G=2), "group[%d] = 2" % (D - 1)), (dict(group=[0, -1] + [0] * (D - 2), G=2), "group[1] = -1")]
    for arguments, said in refused:
        rc, message = build(**arguments)
        assert rc == ERR_INVALID and said in message and message.startswith("characteristic terms: "), (arguments, message)
        assert fetch() == (OK, OK) and index.last_terms_ms() > 0.0

    def fetched():
        found = hip.TermArrays(np.empty(D, np.int32), np.empty(D, np.int32), np.empty((D, 3), np.int32), np.empty((D, 3), np.float64),
                               np.empty((D, 3), np.int32), np.empty((D, 3), np.int32))
        assert lib.east_hip_terms_fetch(h, *[a.ctypes.data_as(t) for a, t in (
            (found.members, hip._c_i32p), (found.count, hip._c_i32p), (found.unit, hip._c_i32p), (found.value, hip._c_dblp),
            (found.texts, hip._c_i32p), (found.df, hip._c_i32p))]) == OK
        return tuple(a.tobytes() for a in (found.members, found.count, found.unit, found.value, found.texts, found.df))

    assert fetched() == want

    # score calls, a text-similarity matrix, a ranking and clusters leave it alone; a build after them gives the same bytes
    index.score_table(np.array([0, 1, 2], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64), True)
    index.texts_similar(True, 2)
    index.clusters_build(hip.GRAPH_SOURCE_COSINE_TEXTS)
    labels = index.clusters_cut(None, 3)[0]
    assert fetched() == want and _result(index, True, 3, 1, None, None)[1] == want
    roots = sorted(set(labels.tolist()))
    grouped = index.terms(True, 3, 1, [roots.index(r) for r in labels.tolist()], len(roots))
    assert grouped.members.sum() == D and len(grouped.members) == len(roots) >= 3

    # the classes change the space under it; so do a rebuild of the index and a reset
    V = index.n_terms
    index.set_classes(np.arange(V, dtype=np.int32) // 2, (V + 1) // 2)
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT) and lib.east_hip_last_terms_ms(h) == -1.0
    assert _result(index, True, 3, 1, None, None)[1] != want
    index.set_classes([], 0)
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT)
    assert _result(index, True, 3, 1, None, None)[1] == want
    index.build_texts(list(texts), stop)
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT)
    assert _result(index, True, 3, 1, None, None)[1] == want
    assert lib.east_hip_reset(h) == OK
    assert fetch() == (ERR_NOT_BUILT, ERR_NOT_BUILT) and build(G=1)[0] == ERR_NOT_BUILT and lib.east_hip_last_terms_ms(h) == -1.0
    index.close()


def test_device_against_host_end_to_end(hip, monkeypatch):
    """applications.texts_terms on both paths, per text and with k: the same cluster memberships; the values agree to the
    bound, and the names wherever the model's neighbouring values lie further apart than twice the bound (at most 5 % of all
    list positions are left undecided by that rule)."""
    from east import applications, relevance
    texts = {"t%02d" % d: text for d, text in enumerate(model.spread_texts())}
    m = model.model_of("spread")
    positions = undecided = 0
    for weighting, cut in (("tf-idf", {}), ("tf", {}), ("tf-idf", dict(k=4, linkage="average")), ("tf", dict(k=3))):
        make = lambda: relevance.CosineRelevanceMeasure("words", weighting, stopwords=())
        monkeypatch.delenv("EAST_HIP_TERMS", raising=False)
        measure = make()
        device = applications.texts_terms(texts, 10, 1, measure, **cut)
        monkeypatch.setenv("EAST_HIP_TERMS", "host")
        host = applications.texts_terms(texts, 10, 1, make(), **cut)
        assert [g.names for g in device] == [g.names for g in host] and sum(len(g.names) for g in device) == len(texts)
        assert len(device) == (cut["k"] if cut else len(texts))
        titles = list(texts)
        group = [0] * len(titles)
        for g, found in enumerate(device):
            for name in found.names:
                group[titles.index(name)] = g
        ex = model.exact(m, weighting == "tf-idf", group, len(device))
        for g, (want, flags) in enumerate(model.decided(ex, 1, 10)):
            assert len(device[g].terms) == len(host[g].terms) == len(want)
            for r, ok in enumerate(flags):
                positions += 1
                undecided += not ok
                if ok:
                    i = want[r]
                    limit = ex.bound[i] * model.U * ex.value[i]
                    for path in (device, host):
                        t = path[g].terms[r]
                        assert t.text == m.terms[ex.unit[i]] and abs(t.value - ex.value[i]) <= limit, (weighting, cut, g, r)
                        assert (t.texts, t.df) == (ex.texts[i], ex.df[ex.unit[i]])
    print("%d of %d list positions undecided" % (undecided, positions))
    assert positions > 400 and undecided <= 0.05 * positions
