# -*- coding: utf-8 -*-
"""An exact host model of synonym extraction (include/east_hip.h, "Synonym extraction"), and the generated
triples that tests/test_synonyms_host.py (CPU) and tests/test_gpu_synonyms.py (GPU) share.  A plain module: no test, no
fixture, and nothing of east.synonyms -- the model works on the strings of the triples.

`Model(triples)` goes from the raw triples (w1, relation, w2) to

  * the integers: every triple entered with its inverse, f(t) = its occurrences in the doubled list, and the marginals
    F_r, F_w1r, F_rw2 as sums of f^2 over the distinct triples (the reference adds f once per occurrence);
  * q = float(f) * F_r / F_w1r / F_rw2 in Python doubles, the three operations in that order -- what the reference computes
    and what the device is specified to compute bit for bit; a feature (r, w2) belongs to T(w1) iff q > 1.0;
  * I = ln(q), the row sums, the numerators and the similarities in `decimal` at 50 digits (q, a double, converts
    exactly); ONE rounding to double at the end of each.  The model's I and similarity are the correctly rounded values
    of the exact ones unless those lie within 1e-48 of a rounding boundary.

What a double implementation may differ by: each log by an ulp or so of a value of at most ln(2^64 * 2^30) < 66, the sums
of n such terms by n roundings, one division -- a few hundred ulp of values in [0, 1] for rows of a few hundred terms,
that is 1e-13 at the outside, under the 1e-12 the tests ask for.

`array_model(w1, rel, w2, inverse, n_words)` is the same model on id arrays, in numpy alone, for the sizes the strings do
not reach (tests/test_gpu_synonyms_scale.py): the doubled keys w1 << 38 | r << 26 | w2 as uint64, np.unique for the distinct
triples and f, np.add.at on uint64 squares for F_w1r and F_r, F_rw2 read from the group of the inverse triple (asserted to
be there), q with the contract's three double operations -- so membership is compared with == and needs no margin --,
I = log(q) and the row sums in np.longdouble (a 64-bit significand: a sum of n terms is off by about n * 2^-64 relative,
2^-11 of the bounds below; the tests that use it skip where np.longdouble is no wider than a double).  `pairs_model` joins
the candidates' rows through their features; `similarity_model` answers listed pairs.  The decimal Model pins it
(tests/test_synonyms_host.py: q bit-equal, the rest to 1e-15 relative).

The bounds the scale tests assert per element, u = 2^-53, derived and not fitted:

  * one feature: |I_dev - I| <= 2 ulp(I) -- the device's log is within 1 ulp of ln(q) (q itself is the model's bit for
    bit), the model's value is ln(q) rounded once more (half an ulp, and the extended logarithm's own last place);
  * a row sum of n entries, relative: (n + 1) u + 2^-51 -- the device adds n positive doubles one after another, n - 1
    roundings each at most u of a partial sum that never exceeds the total; every term carries its log's error, at most
    2^-52 of itself and so of the total; the model's final rounding is one more u; 2^-51 holds the 2^-52 and the
    second-order terms;
  * a similarity of s shared features between rows of n_a and n_b entries, relative: (s + max(n_a, n_b) + 4) u + 2^-50 --
    the numerator is s sums I_a + I_b (one rounding each, at most u of the numerator together, as the terms are positive)
    added one after another (s - 1 roundings); the divisor is the sum of two row sums, each off by its own bound, which
    weighs in with at most the larger, (max + 1) u, plus one addition; one division; the model's final rounding:
    s + max + 4 in all; the logs' 2^-52 enter numerator and divisor once each, and 2^-50 holds those and the second order.
"""
import collections
import decimal
import functools
import random

import numpy as np

CTX = decimal.Context(prec=50)
ABS_TOL = 1e-12


def inverse_relation(relation):
    return relation[:-3] if relation.endswith("_of") else relation + "_of"


class Model(object):
    """words, relations: sorted lists (the relations with every inverse); rows[w] = [((r, w2), I as Decimal)] in
    ascending (r, w2) order; q[(w1, r, w2)] for every distinct triple."""

    def __init__(self, triples):
        doubled = []
        for w1, r, w2 in triples:
            doubled.append((w1, r, w2))
            doubled.append((w2, inverse_relation(r), w1))
        self.f = collections.Counter(doubled)
        self.words = sorted(set(t[0] for t in doubled))
        self.relations = sorted(set(t[1] for t in doubled))
        F_r, F_w1r, F_rw2 = collections.Counter(), collections.Counter(), collections.Counter()
        for (w1, r, w2), f in self.f.items():
            F_r[r] += f * f
            F_w1r[(w1, r)] += f * f
            F_rw2[(r, w2)] += f * f
        self.F_r, self.F_w1r, self.F_rw2 = F_r, F_w1r, F_rw2
        self.q = {}
        rows = collections.defaultdict(list)
        for (w1, r, w2), f in self.f.items():
            q = float(f) * F_r[r] / F_w1r[(w1, r)] / F_rw2[(r, w2)]
            self.q[(w1, r, w2)] = q
            if q > 1.0:
                rows[w1].append(((r, w2), CTX.ln(decimal.Decimal(q))))
        self.rows = {w: sorted(rows[w]) for w in self.words}
        self.row_sum = {w: sum((v for _, v in self.rows[w]), decimal.Decimal(0)) for w in self.words}
        self._dict = {w: dict(self.rows[w]) for w in self.words}

    def I(self, w1, r, w2):
        return float(self._dict.get(w1, {}).get((r, w2), 0.0))

    def shared(self, a, b):
        return set(self._dict[a]) & set(self._dict[b])

    def similarity(self, a, b):
        den = self.row_sum[a] + self.row_sum[b]
        if not den:
            return 0.0
        da, db = self._dict[a], self._dict[b]
        num = sum((CTX.add(da[k], db[k]) for k in self.shared(a, b)), decimal.Decimal(0))
        return float(CTX.divide(num, den))

    def sharing_pairs(self, candidates):
        """The pairs (a in front of b in `candidates`) whose rows have a feature in common, in pair order -- found
        through the features, not by trying every pair."""
        position = {w: i for i, w in enumerate(candidates)}
        by_feature = collections.defaultdict(list)
        for w in candidates:
            for k in self._dict[w]:
                by_feature[k].append(position[w])
        found = set()
        for members in by_feature.values():
            for x in range(len(members)):
                for y in range(x + 1, len(members)):
                    found.add((members[x], members[y]))
        return [(candidates[i], candidates[j]) for i, j in sorted(found)]

    def pairs(self, candidates, threshold):
        """[(a, b, similarity)] for a in front of b in `candidates`, similarity > threshold >= 0, in pair order (a pair
        without a common feature has similarity 0.0)."""
        assert threshold >= 0.0
        out = []
        for a, b in self.sharing_pairs(candidates):
            s = self.similarity(a, b)
            if s > threshold:
                out.append((a, b, s))
        return out


def candidate_words(words, word_frequencies, number_of_texts):
    floor = number_of_texts // 50
    return [w for w in sorted(words) if len(w) > 2 and word_frequencies.get(w, 0) > floor]


def synonyms_of(pairs):
    """{word: [synonyms]} in the order the pairs come in."""
    out = collections.defaultdict(list)
    for a, b, _ in pairs:
        out[a].append(b)
        out[b].append(a)
    return dict(out)


# ---- generated triples -------------------------------------------------------------------------------------------------
def word_name(i):
    return "W%05d" % i


def zipf_triples(seed, n_words, n_relations, n_triples, exponent=1.0):
    """Seeded triples whose words follow a Zipf-like law; relations r0 .. , some of them given as `r_of`."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) ** exponent for k in range(n_words)]
    names = [word_name(i) for i in range(n_words)]
    rng.shuffle(names)
    rels = ["r%d" % i for i in range(n_relations)]
    rels = [r + "_of" if i % 3 == 2 else r for i, r in enumerate(rels)]
    a = rng.choices(names, weights, k=n_triples)
    b = rng.choices(names, weights, k=n_triples)
    return [(a[i], rng.choice(rels), b[i]) for i in range(n_triples)]


def row_length_triples(lengths, seed=0, shared_pool=24, max_shared=4):
    """One word (word_name(i)) per entry of `lengths` whose row has exactly that many features: up to `max_shared` of
    them are words of a small pool under relation `has` (so that rows intersect; `has` sorts behind `big`, so they are the
    LAST columns of the row), the rest the word's own under relation `big`.  Every triple occurs once, so
    q = F_r / (F_w1r * F_rw2) > 1 as long as no row is all of its relation; Model(...).rows says what came out, and the
    tests assert the lengths they rely on.  The feature words get short rows of their own (has_of, big_of)."""
    rng = random.Random(seed)
    triples = []
    pool = ["P%02d" % i for i in range(shared_pool)]
    for i, n in enumerate(lengths):
        w = word_name(i)
        take = rng.sample(pool, min(n, rng.randint(1, max_shared))) if n else []
        for t in take:
            triples.append((w, "has", t))
        for k in range(n - len(take)):
            triples.append((w, "big", "F%d_%d" % (i, k)))
    return triples


# ---- the model on id arrays ----------------------------------------------------------------------------------------------
# numpy only; what tests/test_gpu_synonyms_scale.py compares the device with.  The key is the device's: w1 << 38 | r << 26 | w2.
WORD_BITS, REL_BITS = 26, 12
FEAT_BITS = WORD_BITS + REL_BITS
U = 2.0 ** -53
WIDE = np.finfo(np.longdouble).nmant >= 63
NARROW_REASON = "np.longdouble is no wider than a double here: the extended-precision model has nothing to measure with"


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def pack_keys(w1, rel, w2):
    return (_u64(w1) << np.uint64(FEAT_BITS)) | (_u64(rel) << np.uint64(WORD_BITS)) | _u64(w2)


class ArrayModel(object):
    """What array_model returns.  Per distinct triple, in key order: key, w1, rel, w2 (int64), f (int64), gid (its group
    (w1, r)), q (float64), keep.  Per group: g_key (w1 << 12 | r), F_w1r (uint64).  F_r[r] (uint64).  The CSR rows of the kept
    features: row (the word), relation, word (int64), feature (r << 26 | w2, uint64), I (longdouble); row_words = the words
    with a row, row_begin / row_len / row_sum (longdouble) of each.  Nothing here is n_words long: offsets() and sums() are."""

    def offsets(self):
        return np.searchsorted(self.row, np.arange(self.n_words + 1, dtype=np.int64)).astype(np.int64)

    def sums(self):
        s = np.zeros(self.n_words, dtype=np.longdouble)
        s[self.row_words] = self.row_sum
        return s

    def info(self):
        return {"raw_triples": self.n_raw, "distinct_triples": int(self.key.size), "words": self.n_words, "relations": self.n_relations,
                "features": int(self.row.size), "longest_row": int(self.row_len.max()) if self.row_len.size else 0}

    def rows_of(self, words):
        """(index into `words` of every entry, entry index) of the rows of `words`, word by word, a row in column order."""
        words = np.asarray(words, dtype=np.int64)
        if not self.row_words.size:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        j = np.minimum(np.searchsorted(self.row_words, words), self.row_words.size - 1)
        has = self.row_words[j] == words
        begin, length = np.where(has, self.row_begin[j], 0), np.where(has, self.row_len[j], 0)
        owner = np.repeat(np.arange(words.size, dtype=np.int64), length)
        first = np.cumsum(length) - length
        return owner, np.arange(int(length.sum()), dtype=np.int64) - first[owner] + begin[owner]

    def length_and_sum(self, words):
        words = np.asarray(words, dtype=np.int64)
        if not self.row_words.size:
            return np.zeros(words.size, dtype=np.int64), np.zeros(words.size, dtype=np.longdouble)
        j = np.minimum(np.searchsorted(self.row_words, words), self.row_words.size - 1)
        has = self.row_words[j] == words
        return np.where(has, self.row_len[j], 0), np.where(has, self.row_sum[j], np.longdouble(0))


def array_model(w1, rel, w2, inverse, n_words):
    w1, rel, w2, inverse = (np.asarray(x, dtype=np.int64) for x in (w1, rel, w2, inverse))
    assert w1.size and 0 <= min(w1.min(), w2.min()) and max(w1.max(), w2.max()) < n_words <= 1 << WORD_BITS
    assert inverse.size <= 1 << REL_BITS and 0 <= rel.min() and rel.max() < inverse.size
    assert np.array_equal(inverse[inverse], np.arange(inverse.size))
    m = ArrayModel()
    m.n_raw, m.n_words, m.n_relations, m.inverse = int(w1.size), int(n_words), int(inverse.size), inverse
    m.key, f = np.unique(np.concatenate([pack_keys(w1, rel, w2), pack_keys(w2, inverse[rel], w1)]), return_counts=True)
    assert m.key.dtype == np.uint64
    m.f = f.astype(np.int64)
    m.w1 = (m.key >> np.uint64(FEAT_BITS)).astype(np.int64)
    m.rel = ((m.key >> np.uint64(WORD_BITS)) & np.uint64((1 << REL_BITS) - 1)).astype(np.int64)
    m.w2 = (m.key & np.uint64((1 << WORD_BITS) - 1)).astype(np.int64)
    m.g_key, m.gid = np.unique(m.key >> np.uint64(WORD_BITS), return_inverse=True)
    squares = m.f.astype(np.uint64) * m.f.astype(np.uint64)
    m.F_w1r = np.zeros(m.g_key.size, dtype=np.uint64)
    np.add.at(m.F_w1r, m.gid, squares)
    m.F_r = np.zeros(m.n_relations, dtype=np.uint64)
    np.add.at(m.F_r, m.rel, squares)
    inverse_group = (_u64(m.w2) << np.uint64(REL_BITS)) | _u64(inverse[m.rel])
    at = np.searchsorted(m.g_key, inverse_group)
    assert at.max() < m.g_key.size and np.array_equal(m.g_key[at], inverse_group), "the inverse of a triple is not listed"
    m.F_rw2 = m.F_w1r[at]
    m.q = m.f.astype(np.float64) * m.F_r[m.rel].astype(np.float64) / m.F_w1r[m.gid].astype(np.float64) / m.F_rw2.astype(np.float64)
    m.keep = m.q > 1.0
    m.row, m.relation, m.word = m.w1[m.keep], m.rel[m.keep], m.w2[m.keep]
    m.feature = m.key[m.keep] & np.uint64((1 << FEAT_BITS) - 1)
    m.I = np.log(m.q[m.keep].astype(np.longdouble))
    m.row_words, m.row_begin, m.row_len = np.unique(m.row, return_index=True, return_counts=True)
    at = np.searchsorted(m.row_words, m.row)
    m.row_sum = np.zeros(m.row_words.size, dtype=np.longdouble)
    np.add.at(m.row_sum, at, m.I)
    return m


def pairs_model(model, candidates):
    """Every pair (a in front of b in `candidates`) whose rows share a feature, in pair order ->
    (a, b word ids, similarity rounded once to float64, shared = the number of common features, n_a, n_b = the row lengths).
    The entries of the candidates' rows sorted by (feature, position in the list); all position pairs inside a feature's
    group; I_a + I_b added per pair in longdouble; one division by the sum of the two row sums."""
    candidates = np.asarray(candidates, dtype=np.int64)
    C = candidates.size
    position, entry = model.rows_of(candidates)
    order = np.lexsort((position, model.feature[entry]))
    position, entry = position[order], entry[order]
    feature = model.feature[entry]
    heads = np.flatnonzero(np.concatenate([[True], feature[1:] != feature[:-1]])) if feature.size else np.zeros(0, dtype=np.int64)
    sizes = np.diff(np.concatenate([heads, [feature.size]]))
    codes, values = [], []
    for size in np.unique(sizes[sizes > 1]).tolist():           # np.triu_indices once per group size, all groups of that size at once
        i, j = np.triu_indices(size, 1)
        start = heads[sizes == size][:, None]
        x, y = (start + i).ravel(), (start + j).ravel()
        codes.append(position[x] * C + position[y])             # position[x] < position[y]: a feature occurs once a row
        values.append(model.I[entry[x]] + model.I[entry[y]])
    if not codes:
        e = np.zeros(0, dtype=np.int64)
        return e, e, np.zeros(0), e, e, e
    code, which = np.unique(np.concatenate(codes), return_inverse=True)
    numerator = np.zeros(code.size, dtype=np.longdouble)
    np.add.at(numerator, which, np.concatenate(values))
    shared = np.bincount(which, minlength=code.size)
    length, total = model.length_and_sum(candidates)
    pa, pb = code // C, code % C
    similarity = (numerator / (total[pa] + total[pb])).astype(np.float64)
    return candidates[pa], candidates[pb], similarity, shared, length[pa], length[pb]


def similarity_model(model, a, b):
    """similarity(a[i], b[i]) -> (float64 rounded once, shared, n_a, n_b); 0.0 where the two row sums are zero."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert a.size < 1 << (64 - FEAT_BITS)
    pair_a, entry_a = model.rows_of(a)
    pair_b, entry_b = model.rows_of(b)
    code_a = (_u64(pair_a) << np.uint64(FEAT_BITS)) | model.feature[entry_a]
    code_b = (_u64(pair_b) << np.uint64(FEAT_BITS)) | model.feature[entry_b]
    _, ia, ib = np.intersect1d(code_a, code_b, assume_unique=True, return_indices=True)
    numerator = np.zeros(a.size, dtype=np.longdouble)
    np.add.at(numerator, pair_a[ia], model.I[entry_a[ia]] + model.I[entry_b[ib]])
    shared = np.bincount(pair_a[ia], minlength=a.size)
    (n_a, sum_a), (n_b, sum_b) = model.length_and_sum(a), model.length_and_sum(b)
    den = sum_a + sum_b
    similarity = np.where(den != 0, numerator / np.where(den != 0, den, 1), 0).astype(np.float64)
    return similarity, shared, n_a, n_b


# the derived bounds (the module's docstring), as functions of what the model counts
def ulps(got, want):
    """|got - want| in units of the last place of `want` (float64)."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))


FEATURE_BOUND_ULP = 2.0


def row_sum_bound(n):
    return (np.asarray(n, dtype=np.float64) + 1.0) * U + 2.0 ** -51


def similarity_bound(shared, n_a, n_b):
    return (np.asarray(shared, dtype=np.float64) + np.maximum(n_a, n_b) + 4.0) * U + 2.0 ** -50


# ---- generated id triples ------------------------------------------------------------------------------------------------
def zipf_ids(seed, n_words, n_relations, n_triples):
    """(w1, rel, w2) int32: both words Zipf (weight 1 / rank) through a seeded permutation of the ids, the relation uniform."""
    rng = np.random.default_rng(seed)
    weights = 1.0 / np.arange(1, n_words + 1)
    cdf = np.cumsum(weights / weights.sum())
    names = rng.permutation(n_words)
    w1 = names[np.minimum(np.searchsorted(cdf, rng.random(n_triples)), n_words - 1)]
    w2 = names[np.minimum(np.searchsorted(cdf, rng.random(n_triples)), n_words - 1)]
    rel = rng.integers(0, n_relations, size=n_triples)
    return w1.astype(np.int32), rel.astype(np.int32), w2.astype(np.int32)


def paired_inverse(n_relations, self_inverse=()):
    inverse = np.arange(n_relations, dtype=np.int32) ^ 1
    for r in self_inverse:                                      # whole pairs: (r, r ^ 1) both become their own inverse
        inverse[r], inverse[r ^ 1] = r, r ^ 1
    assert np.array_equal(inverse[inverse], np.arange(n_relations))
    return inverse


SCALE_WORDS, SCALE_RELATIONS, SCALE_STRIDE = 40000, 64, 2048 * 256
SCALE_SELF_INVERSE = (62, 63)
SCALE_BLOCKS = ((56, 3, 5), (58, 64, 65))                     # (relation, |A|, |B|): A x B once each under a pair of its own
SCALE_REPEATED, SCALE_REPEATS = (123, 4, 31999), 70000


def straddles(model, boundary):
    """Does a group (w1, r) hold the distinct triples boundary - 1 and boundary?"""
    return boundary < model.key.size and model.gid[boundary - 1] == model.gid[boundary]


@functools.lru_cache(maxsize=None)
def scale_case(seed=2024, boundary=SCALE_STRIDE):
    """W = 40 000, R = 64 (inv = r ^ 1, 62 and 63 their own inverses), about 420 000 Zipf raw triples under the relations
    0 .. 55 and 60 .. 63, one triple 70 000 times, two complete bipartite blocks under 56/57 and 58/59 (q == 1.0 exactly), and
    one planted triple that makes a group lie across distinct triple 524 288 where the draw has none that does (recomputed
    after planting: the planted triple and its inverse shift the order).  -> ((w1, rel, w2, inverse, n_words), its model)."""
    W, R = SCALE_WORDS, SCALE_RELATIONS
    inverse = paired_inverse(R, (SCALE_SELF_INVERSE[0],))
    w1, rel, w2 = zipf_ids(seed, W, R - 4, 420000)
    rel = np.where(rel >= 56, rel + 4, rel).astype(np.int32)    # 56 .. 59 are the blocks' own
    parts = [(w1, rel, w2)]
    a, r, b = SCALE_REPEATED
    parts.append(tuple(np.full(SCALE_REPEATS, x, dtype=np.int32) for x in (a, r, b)))
    rng = np.random.default_rng(seed + 1)
    for r, na, nb in SCALE_BLOCKS:
        members = rng.choice(W, size=na + nb, replace=False).astype(np.int32)
        parts.append((np.repeat(members[:na], nb), np.full(na * nb, r, dtype=np.int32), np.tile(members[na:], na)))
    w1, rel, w2 = (np.concatenate([p[i] for p in parts]) for i in range(3))
    model = array_model(w1, rel, w2, inverse, W)
    if not straddles(model, boundary):
        # one more member for the group that ends at boundary - 1: a word above w1 (its inverse sorts behind the
        # boundary) that the group does not hold yet
        d = boundary - 1
        group = set(model.w2[model.gid == model.gid[d]].tolist())
        new = next(w for w in range(W - 1, int(model.w1[d]), -1) if w not in group)
        w1, rel, w2 = (np.append(x, np.int32(v)) for x, v in ((w1, model.w1[d]), (rel, model.rel[d]), (w2, new)))
        model = array_model(w1, rel, w2, inverse, W)
    assert straddles(model, boundary), "no group lies across the marginals kernel's stride"
    return (w1, rel, w2, inverse, W), model


TOP_WORDS, TOP_RELATIONS = 1 << WORD_BITS, 1 << REL_BITS
TOP_WORD_IDS = (0, 1, 2, 77, (1 << 13) + 5, (1 << 25) - 1, 1 << 25, (1 << 25) + (1 << 24) + 3, (1 << 26) - 2, (1 << 26) - 1)
TOP_RELATION_IDS = (0, 1, 2047, 2048, 4094, 4095)


def top_case(n_words=TOP_WORDS, seed=10, n_triples=320):
    """A few hundred triples over word ids at the bottom, the middle and the top of the 26 bits and relation ids likewise of
    the 12, paired 0-1, 2047-2048, 4094-4095 (every other relation id is its own inverse and unused)."""
    rng = np.random.default_rng(seed)
    ids = np.array([w for w in TOP_WORD_IDS if w < n_words] + ([n_words - 2, n_words - 1] if n_words < TOP_WORDS else []), dtype=np.int64)
    inverse = np.arange(TOP_RELATIONS, dtype=np.int32)
    for a, b in ((0, 1), (2047, 2048), (4094, 4095)):
        inverse[a], inverse[b] = b, a
    w1 = ids[rng.integers(0, ids.size, size=n_triples)]
    w2 = ids[rng.integers(0, ids.size, size=n_triples)]
    rel = np.array(TOP_RELATION_IDS)[rng.integers(0, len(TOP_RELATION_IDS), size=n_triples)]
    return w1.astype(np.int32), rel.astype(np.int32), w2.astype(np.int32), inverse, n_words


WORD_COUNTS = (1, 2, 3, 255, 256, 257, 65535, 65536, 65537)


def word_count_case(W, n_triples=200):
    """About 200 triples of W words, 6 relations (4 and 5 their own inverses); the id W - 1 is both a w1 and a w2."""
    rng = np.random.default_rng(1000 + W)
    inverse = paired_inverse(6, (4,))
    pool = np.unique(np.concatenate([[0, W - 1, W // 2, max(W - 2, 0)], rng.integers(0, W, size=20)]))
    w1, w2 = pool[rng.integers(0, pool.size, size=n_triples)], pool[rng.integers(0, pool.size, size=n_triples)]
    rel = rng.integers(0, 6, size=n_triples)
    w1[0], w2[0], w1[1], w2[1] = W - 1, 0, 0, W - 1
    return w1.astype(np.int32), rel.astype(np.int32), w2.astype(np.int32), inverse, W


DISTINCT_COUNTS = (255, 256, 257, 511, 512, 513)
SCAN_TILE_DISTINCT = (4094, 4095, 4096, 4097)   # around the 4096 elements a workgroup of the device's prefix sums takes: 4094, 4096, 4096, 4098 sorted keys


def distinct_count_case(D):
    """D distinct triples: D // 2 different raw triples under the relations 0 and 2 (their inverses 1 and 3 are given to no
    raw triple, so no inverse meets a raw triple), and for an odd D one self-loop under relation 4, its own inverse."""
    rng = np.random.default_rng(2000 + D)
    W = 48
    inverse = paired_inverse(6, (4,))
    code = rng.choice(W * 2 * W, size=D // 2, replace=False)
    w1, rel, w2 = code // (2 * W), 2 * (code // W % 2), code % W
    if D % 2:
        w1, rel, w2 = np.append(w1, 5), np.append(rel, 4), np.append(w2, 5)
    return w1.astype(np.int32), rel.astype(np.int32), w2.astype(np.int32), inverse, W


PAIR_WORDS, PAIR_RELATIONS, PAIR_TRIPLES = 9000, 24, 90000
PAIR_CANDIDATES = (1300, 4097)
PAIR_THRESHOLD, PAIR_MARGIN = 0.1, 1e-9


@functools.lru_cache(maxsize=None)
def pair_case(seed=31):
    """-> ((w1, rel, w2, inverse, n_words), its model)"""
    case = zipf_ids(seed, PAIR_WORDS, PAIR_RELATIONS, PAIR_TRIPLES) + (paired_inverse(PAIR_RELATIONS), PAIR_WORDS)
    return case, array_model(*case)


def pair_candidates(model, C, seed=31):
    """C of the words in a seeded order of no kind, the word with the longest row among them."""
    rng = np.random.default_rng(seed * 100000 + C)
    hub = int(model.row_words[np.argmax(model.row_len)])
    others = rng.permutation(np.setdiff1d(np.arange(model.n_words), [hub]))[:C - 1]
    cand = np.append(others, hub)
    return cand[rng.permutation(C)].astype(np.int32)
