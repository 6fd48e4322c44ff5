# -*- coding: utf-8 -*-
"""gpu tier: synonym extraction (csrc/synonyms.h) on id arrays at the sizes and ids where its index arithmetic matters,
against the exact model on id arrays of tests/synonyms_exact.py (`array_model`, `pairs_model`, `similarity_model`).

  a. scale: 740 000 distinct triples (the marginals kernel's loop takes a second turn, a group lies across its stride),
     groups (w1, r) longer than a wavefront and than a workgroup, f^2, F_r and F_w1r above 2^32, all 64 relation counters,
     self-inverse relations, two complete bipartite blocks whose q is 1.0 exactly;
  b. the top of every field of the 64-bit key: n_words = 2^26, n_relations = 4096, ids at the bottom, the middle and the top;
  c. word counts on both sides of a power of two (the sort's width), the highest id as w1 and as w2;
  d. distinct-triple counts on both sides of the workgroup (keep[D] is thread D's);
  e. the pair pass at 1 300 and 4 097 candidates in no id order (two scan tiles of counts; 17 target tiles), a row longer
     than 16 chunks, thresholds 0.1 and 0.0, the chunk lengths 128 and 24, and 100 000 look-ups.

Every case compares info(), the offsets, relation and word arrays with ==, I, the row sums and the similarities per element
within the bounds derived in synonyms_exact's docstring, pair ids and order with ==, and prints the worst deviations in
ulp in front of the assertions (run with -s to see them).  tests/test_synonyms_host.py asserts, from the model alone, that
each generated case holds what it is here for."""
import time

import numpy as np
import pytest

import synonyms_exact as sx

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sx.WIDE, reason=sx.NARROW_REASON)]

INVALID = "(code -2)"


def check_build(dev, model, name, sparse=False):
    """info() and the CSR rows against the model.  sparse: n_words is large and nearly every row empty -- the offsets are
    compared through the rows that are not, as are the row sums."""
    assert dev.info() == model.info()
    offsets, relation, word, value, row_sum = dev.rows()
    assert offsets.size == model.n_words + 1 and row_sum.size == model.n_words
    if sparse:
        lengths = np.diff(offsets)
        occupied = np.flatnonzero(lengths)
        assert np.array_equal(occupied, model.row_words) and np.array_equal(lengths[occupied], model.row_len)
        assert np.array_equal(offsets[occupied], model.row_begin) and offsets[0] == 0 and offsets[-1] == model.row.size
        assert np.array_equal(np.flatnonzero(row_sum), model.row_words)
    else:
        assert np.array_equal(offsets, model.offsets())
        assert np.array_equal(np.flatnonzero(row_sum), model.row_words)            # an empty row sums to 0.0 exactly
    assert np.array_equal(relation, model.relation) and np.array_equal(word, model.word)
    want_I = model.I.astype(np.float64)
    off_I = sx.ulps(value, want_I)
    got_sum, want_sum = row_sum[model.row_words], model.row_sum.astype(np.float64)
    off_sum = sx.ulps(got_sum, want_sum)
    print("%s: %d features, worst |I - model| %.2f ulp; %d rows (longest %d), worst |row sum - model| %.2f ulp"
          % (name, want_I.size, off_I.max(initial=0.0), want_sum.size, model.info()["longest_row"], off_sum.max(initial=0.0)))
    assert (off_I <= sx.FEATURE_BOUND_ULP).all()
    assert (np.abs(got_sum - want_sum) <= sx.row_sum_bound(model.row_len) * want_sum).all()
    return off_I.max(initial=0.0), off_sum.max(initial=0.0)


def check_pairs(dev, joined, candidates, threshold, name):
    """The pair list at `threshold` against the joined model (pairs_model's result for these candidates): ids and order
    with ==, similarities within the derived bound.  Above 0 the model's own margin is asserted first: no similarity
    within 1e-9 of the threshold (a seed's business, not a tolerance of the comparison)."""
    a, b, sim, shared, n_a, n_b = joined
    if threshold > 0.0:
        assert (np.abs(sim - threshold) > sx.PAIR_MARGIN).all(), "the generated case has a similarity at the threshold"
    above = sim > threshold
    got_a, got_b, got_sim = dev.pairs(candidates, threshold)
    assert np.array_equal(got_a, a[above]) and np.array_equal(got_b, b[above])
    off = sx.ulps(got_sim, sim[above])
    print("%s: threshold %.2f, %d pairs of %d candidates (%d share a feature), worst |similarity - model| %.2f ulp"
          % (name, threshold, int(above.sum()), len(candidates), a.size, off.max(initial=0.0)))
    assert (np.abs(got_sim - sim[above]) <= sx.similarity_bound(shared, n_a, n_b)[above] * sim[above]).all()
    return got_a, got_b, got_sim


def check_lookups(dev, model, a, b, name):
    sim, shared, n_a, n_b = sx.similarity_model(model, a, b)
    got = dev.similarity(a, b)
    off = sx.ulps(got, sim)
    print("%s: %d look-ups, %d above 0, worst |similarity - model| %.2f ulp" % (name, sim.size, int((sim > 0).sum()), off.max(initial=0.0)))
    assert np.array_equal(got == 0.0, sim == 0.0)
    assert (np.abs(got - sim) <= sx.similarity_bound(shared, n_a, n_b) * sim).all()
    assert np.array_equal(dev.similarity(b, a), got)                    # symmetric, bit for bit
    return got


def check_small(hip, case, name):
    """Build, rows, every pair of the words in use at 0.0 (descending ids) and through the look-up."""
    w1, rel, w2, inverse, W = case
    model = sx.array_model(*case)
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        check_build(dev, model, name)
        used = np.unique(np.concatenate([w1, w2]))[::-1].astype(np.int32)
        check_pairs(dev, sx.pairs_model(model, used), used, 0.0, name)
        i, j = np.triu_indices(used.size, 0)                            # (with a == b: 1.0 where the row is not empty)
        check_lookups(dev, model, used[i], used[j], name)
    finally:
        dev.close()
    return model


# ---- a. scale ------------------------------------------------------------------------------------------------------------
def test_scale(hip):
    (w1, rel, w2, inverse, W), model = sx.scale_case()
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        check_build(dev, model, "scale")
        rng = np.random.default_rng(5)
        blocks = np.unique(np.concatenate([np.concatenate([w1[rel == r], w2[rel == r]]) for r, _, _ in sx.SCALE_BLOCKS]))
        cand = rng.permutation(np.union1d(rng.choice(W, size=600, replace=False), blocks)).astype(np.int32)
        joined = sx.pairs_model(model, cand)
        check_pairs(dev, joined, cand, 0.05, "scale")
        check_pairs(dev, joined, cand, 0.0, "scale")
        check_lookups(dev, model, rng.integers(0, W, size=20000), rng.integers(0, W, size=20000), "scale")
    finally:
        dev.close()


# ---- b. the top of every key field -----------------------------------------------------------------------------------------
def test_key_field_tops(hip):
    t0 = time.perf_counter()
    w1, rel, w2, inverse, W = case = sx.top_case()
    assert W == 1 << 26 and inverse.size == 1 << 12
    model = sx.array_model(*case)
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        check_build(dev, model, "key tops", sparse=True)
        used = np.unique(np.concatenate([w1, w2]))[::-1].astype(np.int32)
        check_pairs(dev, sx.pairs_model(model, used), used, 0.0, "key tops")
        i, j = np.triu_indices(used.size, 0)
        check_lookups(dev, model, used[i], used[j], "key tops")
        # one more word or relation than the key holds: refused before the device is touched, the build stays
        for n_words, inv in ((W + 1, inverse), (W, np.arange((1 << 12) + 1, dtype=np.int32))):
            with pytest.raises(hip.exceptions.HipBackendError) as e:
                dev.build(w1, rel, w2, inv, n_words)
            assert INVALID in str(e.value)
            assert dev.info() == model.info()
        check_pairs(dev, sx.pairs_model(model, used), used, 0.0, "key tops, after the refusals")
    finally:
        dev.close()
    print("key tops: %.1f s" % (time.perf_counter() - t0))


# ---- c. word counts around powers of two -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", sx.WORD_COUNTS)
def test_word_counts_around_powers_of_two(hip, W):
    check_small(hip, sx.word_count_case(W), "W = %d" % W)


# ---- d. distinct counts around the workgroup -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sx.DISTINCT_COUNTS)
def test_distinct_counts_around_the_block(hip, D):
    model = check_small(hip, sx.distinct_count_case(D), "D = %d" % D)
    assert model.key.size == D


# ---- e. the pair pass ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def chunk_knob(hip):
    lib = hip.load()
    try:
        yield lib.east_hip_debug_set_synonyms_chunk
    finally:
        lib.east_hip_debug_set_synonyms_chunk(0)


@pytest.mark.parametrize("C", sx.PAIR_CANDIDATES)
def test_pair_pass(hip, chunk_knob, C):
    (w1, rel, w2, inverse, W), model = sx.pair_case()
    cand = sx.pair_candidates(model, C)
    hub = int(model.row_words[np.argmax(model.row_len)])
    assert hub in cand.tolist() and model.row_len.max() > 16 * 128
    joined = sx.pairs_model(model, cand)
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        check_build(dev, model, "pair pass")
        lists = {}
        for chunk in (128, 24):
            chunk_knob(chunk)
            name = "C = %d, chunk %d" % (C, chunk)
            lists[chunk] = check_pairs(dev, joined, cand, sx.PAIR_THRESHOLD, name) + check_pairs(dev, joined, cand, 0.0, name)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(lists[128], lists[24]))     # the same bytes at both chunk lengths
        assert lists[128][3].size == joined[0].size                     # at 0.0: exactly the pairs that share a feature
    finally:
        dev.close()


def test_look_ups(hip):
    (w1, rel, w2, inverse, W), model = sx.pair_case()
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, W, size=100000), rng.integers(0, W, size=100000)
    hub = int(model.row_words[np.argmax(model.row_len)])
    a[:300] = hub                                                       # the longest row against 300 others, and against itself
    b[0] = hub
    dev = hip.HipSynonyms()
    try:
        dev.build(w1, rel, w2, inverse, W)
        got = check_lookups(dev, model, a, b, "pair case")
        assert got[0] == 1.0 and (got > 0.0).sum() > 1000
    finally:
        dev.close()
