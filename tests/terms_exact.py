# -*- coding: utf-8 -*-
"""An exact host model of the characteristic terms (include/east_hip.h, "Characteristic terms"), and the
generated collections that tests/test_terms_host.py (CPU) and tests/test_gpu_terms.py (GPU) share.  A plain module: no test,
no fixture.

Built on cosine_exact.build_model: the integer counts, df and the class map.  With c_ud the count of unit u in text d,
idf_u = 1 + ln(D / df_u) (1 under tf) and rad_d = sum_u c_ud^2 idf_u^2

    exact[g][u] = (sum over the texts d of g that hold u of c_ud idf_u / sqrt(rad_d)) / members[g]

-- n_d cancels.  ln, the roots, the quotients and the sums are taken at 50 digits (cosine_exact.MP) and rounded ONCE to
double.  The bound per entry, in units of 2^-53 relative to the exact value (p_d = the postings of d; DESIGN.md 19 derives
it, the model's own rounding included):

    texts_gu + (max over d in g of ceil(p_d / 64)) / 2 + 48
"""
import functools

import numpy as np

import cosine_exact
import texts_cosine_exact as tce

MP = cosine_exact.MP
U = 2.0 ** -53                                   # the unit roundoff: the bounds are counted in it
EXTRA_U = 48
TILE = 4096                                     # csrc/terms.h: TERMS_TILE, the entries of a histogram tile


class Exact(object):
    """members[G]; offsets[G + 1]; per entry in (group, unit) order unit, value, texts and bound (in units of 2^-53); df[units]."""


def exact(model, tfidf, group=None, n_groups=None, stems=False):
    counts, df, n_units, _ = model.space(stems)
    D = model.n_docs
    group = list(range(D)) if group is None else [int(g) for g in group]
    G = D if n_groups is None else int(n_groups)
    rad = model._radicands(stems, tfidf)
    sums, texts = {}, {}
    slices = [0] * G
    for d, c in enumerate(counts):                               # (ascending d; the order does not matter at 50 digits)
        g = group[d]
        slices[g] = max(slices[g], -(-len(c) // 64))
        if not c:
            continue
        root = MP.sqrt(MP.mpf(rad[d]))
        for u, n in c.items():
            key = (g, u)
            sums[key] = sums.get(key, 0) + n * model.idf(df[u], tfidf) / root
            texts[key] = texts.get(key, 0) + 1
    e = Exact()
    e.members = np.bincount(np.asarray(group, dtype=np.int64), minlength=G).astype(np.int32)
    keys = sorted(sums)
    e.unit = np.array([u for _, u in keys], dtype=np.int32)
    e.value = np.array([float(sums[k] / int(e.members[k[0]])) for k in keys], dtype=np.float64)
    e.texts = np.array([texts[k] for k in keys], dtype=np.int32)
    e.bound = np.array([texts[k] + slices[k[0]] / 2.0 + EXTRA_U for k in keys], dtype=np.float64)
    e.offsets = np.searchsorted(np.array([g for g, _ in keys], dtype=np.int64), np.arange(G + 1)).astype(np.int64)
    e.df = np.asarray(df, dtype=np.int32)
    return e


def rank(unit, value, texts, min_texts, n):
    """The contract's ranking of one group's entries, over any (unit, value, texts) arrays: the entries with
    texts >= min_texts by value descending, then unit ascending; the first n -> their indexes."""
    keep = [i for i in range(len(unit)) if texts[i] >= min_texts]
    keep.sort(key=lambda i: (-float(value[i]), int(unit[i])))
    return keep[:n]


def ranked(offsets, unit, value, texts, df, min_texts, n):
    """The result of east_hip_terms_fetch from the vectors: (count[G], unit, value, texts, df as [G, n]; -1 and NaN behind count)."""
    G = len(offsets) - 1
    count = np.zeros(G, dtype=np.int32)
    r_unit, r_texts, r_df = (np.full((G, n), -1, dtype=np.int32) for _ in range(3))
    r_value = np.full((G, n), np.nan, dtype=np.float64)
    for g in range(G):
        a, e = int(offsets[g]), int(offsets[g + 1])
        best = np.asarray(rank(unit[a:e], value[a:e], texts[a:e], min_texts, n), dtype=np.int64) + a
        count[g] = best.size
        r_unit[g, :best.size], r_value[g, :best.size], r_texts[g, :best.size] = unit[best], value[best], texts[best]
        r_df[g, :best.size] = df[unit[best]]
    return count, r_unit, r_value, r_texts, r_df


def check_vectors(offsets, unit, value, texts, ex):
    """The vectors against the model: the same structure exactly, every value within its bound -> the largest share of it."""
    assert np.array_equal(np.asarray(offsets, dtype=np.int64), ex.offsets)
    assert np.array_equal(unit, ex.unit) and np.array_equal(texts, ex.texts)
    assert (np.asarray(value) > 0.0).all()
    if not ex.value.size:
        return 0.0
    share = float((np.abs(value - ex.value) / (ex.bound * U * ex.value)).max())
    assert share <= 1.0, "error %.3g of its bound" % share
    return share


def decided(ex, min_texts, n):
    """Per group the model's list of n (as indexes into the entries) and, per position, whether the twice-the-bound rule
    decides it: the value lies further than twice the bound from both neighbours in the model's full order."""
    out = []
    for g in range(len(ex.offsets) - 1):
        a, e = int(ex.offsets[g]), int(ex.offsets[g + 1])
        order = [a + i for i in rank(ex.unit[a:e], ex.value[a:e], ex.texts[a:e], min_texts, e - a)]
        apart = [ex.value[i] - ex.value[j] > 2.0 * U * (ex.bound[i] * ex.value[i] + ex.bound[j] * ex.value[j])
                 for i, j in zip(order, order[1:])]
        flags = [(r == 0 or apart[r - 1]) and (r + 1 >= len(order) or apart[r]) for r in range(min(n, len(order)))]
        out.append((order[:n], flags))
    return out


# ---- generated collections (the same for both tiers) ---------------------------------------------------------------------
word = tce.word
RUN_LENGTHS = (1, 63, 64, 65, 257, 4097)
SEGMENT_N = (1, 10, 1024)
SEGMENT_LENGTHS = tuple(sorted({m for n in SEGMENT_N for m in (n - 1, n, n + 1)} | {TILE - 1, TILE, TILE + 1}))


@functools.lru_cache(maxsize=None)
def run_texts(L):
    """One word shared by L one-word texts (group 0), beside one text of two other words (group 1)."""
    return [word(1)] * L + [word(2) + " " + word(3)]


def run_group(L):
    return [0] * L + [1], 2


@functools.lru_cache(maxsize=None)
def segment_texts():
    """A text of exactly m distinct words for every m of SEGMENT_LENGTHS (0: the empty text), each word 1 .. 3 times."""
    rng = np.random.default_rng(600)
    return [tce._text(rng, rng.choice(5000, size=m, replace=False)) if m else "" for m in SEGMENT_LENGTHS]


@functools.lru_cache(maxsize=None)
def tie_texts():
    """A text whose 5 000 words all occur once (one value, more entries than a tile); a text with three words twice and three
    once (equal values across the 2nd and the 4th place); two identical texts."""
    twin = " ".join(word(6000 + i) for i in (3, 1, 2, 1, 3, 3))
    return [" ".join(word(i) for i in range(5000)),
            " ".join(word(7000 + i) for i in (0, 0, 1, 1, 2, 2, 3, 4, 5)), twin, twin]


@functools.lru_cache(maxsize=None)
def spread_texts(D=24):
    """D texts over 40 words whose counts inside a text are all different (1 .. m in a random order): neighbouring values
    lie far apart, per text and in groups."""
    rng = np.random.default_rng(700)
    texts = []
    for _ in range(D):
        ids = rng.choice(40, size=int(rng.integers(6, 16)), replace=False)
        reps = rng.permutation(len(ids)) + 1
        tokens = np.repeat(ids, reps)
        rng.shuffle(tokens)
        texts.append(" ".join(word(i) for i in tokens.tolist()))
    return texts


def groupings(D):
    """{name: (group or None, G)}: the identity given as an array, one group, empty groups at the front, in the middle and at
    the end, G = D with a permuted assignment, and four groups of equal size (D a multiple of 4)."""
    rng = np.random.default_rng(800 + D)
    out = {"identity": (list(range(D)), D), "one group": ([0] * D, 1),
           "empty groups": ([(1, 2, 4, 5, 6)[i % 5] for i in range(D)], 9),
           "permuted": (rng.permutation(D).tolist(), D)}
    if D % 4 == 0:
        out["four equal"] = ([i % 4 for i in range(D)], 4)
    return out


@functools.lru_cache(maxsize=None)
def model_of(name):
    texts, stop, stems = collections()[name]
    return cosine_exact.build_model(list(texts), stop, cosine_exact.ToyStemmer() if stems else None, fast=not stems)


def collections():
    """{name: (texts, stopwords, stems)}: every collection of both tiers."""
    out = {"runs %d" % L: (run_texts(L), (), False) for L in RUN_LENGTHS}
    out["segments"] = (segment_texts(), (), False)
    out["ties"] = (tie_texts(), (), False)
    out["spread"] = (spread_texts(), (), False)
    out["tile edges 64"] = (tce.tile_edges(64), (), False)
    out["document shapes"] = (tce.document_shapes(), tce.STOPWORDS, False)
    out["long text"] = (tce.long_text(), (), False)
    out["stems"] = (tce.stem_texts(), tce.STOPWORDS, True)
    return out
