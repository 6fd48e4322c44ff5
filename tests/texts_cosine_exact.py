# -*- coding: utf-8 -*-
"""An exact host model of the text-to-text cosine similarity (include/east_hip.h, "Text-to-text cosine similarity";
DESIGN.md 15), and the generated collections that tests/test_texts_similar_host.py (CPU) and
tests/test_gpu_texts_similar.py (GPU) share.  A plain module: no test, no fixture.

Built on cosine_exact.build_model: the integer counts, df and the class map.  With c_ud the count of unit u in document d
and idf_u = 1 + ln(D / df_u) (1 under tf)

    exact[a][b] = sum_u c_ua c_ub idf_u^2  /  sqrt( (sum_u c_ua^2 idf_u^2) * (sum_u c_ub^2 idf_u^2) )

-- n_d cancels.  The integer sums per distinct df are exact (numpy int64 products of counts); ln, idf^2, the products with
the integers, their sums, the root and the quotient are taken at 50 digits (cosine_exact.MP) and rounded ONCE to double.

The bound, for a != b (t_ab = the common units, p_d = the postings of d):

    |got - exact| <= (t_ab + ceil(p_a / 64) + ceil(p_b / 64) + 128 + 48) * 2^-52 * exact

and the same with t_aa = p_a for |self[a] - 1|.  exact == 0 means got is +0.0, bit for bit.
"""
import functools

import numpy as np

import cosine_exact

MP = cosine_exact.MP
ULP = 2.0 ** -52
EXTRA_ULPS = 128 + 48


class Exact(object):
    """C[D, D] (NaN on the diagonal), t[D, D] = the common units, p[D] = the postings, bound[D, D] in ulps (the diagonal:
    the bound of self), has[D] = the document has postings."""


def dense_counts(model, stems):
    counts, _, n_units, _ = model.space(stems)
    dense = np.zeros((model.n_docs, max(n_units, 1)), dtype=np.int64)
    for d, c in enumerate(counts):
        if c:
            dense[d, list(c.keys())] = list(c.values())
    return dense


def exact(model, tfidf, stems=False):
    D = model.n_docs
    df = np.asarray(model.space(stems)[1], dtype=np.int64)
    dense = dense_counts(model, stems)
    present = (dense > 0).astype(np.int64)
    e = Exact()
    e.t = present @ present.T
    e.p = present.sum(axis=1)
    e.has = e.p > 0
    num = [[MP.mpf(0)] * D for _ in range(D)]
    for f in (np.unique(df[df > 0]).tolist() if tfidf else [None]):
        cols = dense[:, df == f] if tfidf else dense
        part = cols @ cols.T                                   # (exact: integers)
        w = model.idf(f, True) ** 2 if tfidf else 1
        for a, b in zip(*np.nonzero(np.triu(part))):
            num[a][b] = num[a][b] + int(part[a, b]) * w
    e.C = np.zeros((D, D), dtype=np.float64)
    for a in range(D):
        for b in range(a + 1, D):
            if e.t[a, b]:
                e.C[a, b] = e.C[b, a] = float(num[a][b] / MP.sqrt(MP.mpf(num[a][a]) * num[b][b]))
    np.fill_diagonal(e.C, np.nan)
    slices = np.ceil(e.p / 64.0)
    e.bound = e.t + slices[:, None] + slices[None, :] + EXTRA_ULPS
    return e


def errors(matrix, own, ex):
    """(the largest ratio of an error to its bound, off the diagonal and for self; the zeros are +0.0)."""
    D = ex.p.size
    off = ~np.eye(D, dtype=bool)
    nz = off & (ex.C != 0.0)
    ratio = 0.0
    if nz.any():
        ratio = float((np.abs(matrix[nz] - ex.C[nz]) / (ex.bound[nz] * ULP * ex.C[nz])).max())
    if ex.has.any():
        ratio = max(ratio, float((np.abs(own[ex.has] - 1.0) / (np.diag(ex.bound)[ex.has] * ULP)).max()))
    zeros = off & (ex.C == 0.0)
    return ratio, bool((matrix[zeros].view(np.uint64) == 0).all()) and bool((own[~ex.has].view(np.uint64) == 0).all())


def check(matrix, own, postings, ex, tenth=False):
    """Everything a result promises, against the model; tenth: within a tenth of the bound.  -> the ratio."""
    matrix, own = np.ascontiguousarray(matrix, dtype=np.float64), np.ascontiguousarray(own, dtype=np.float64)
    D = ex.p.size
    assert matrix.shape == (D, D) and own.shape == (D,)
    if postings is not None:
        assert np.array_equal(np.asarray(postings, dtype=np.int64), ex.p)
    assert np.isnan(matrix.diagonal()).all() and np.isnan(matrix).sum() == D
    assert matrix.tobytes() == matrix.T.copy().tobytes(), "C and its transpose are not the same bytes"
    ratio, zeros = errors(matrix, own, ex)
    print("text cosine %d x %d: error %.3g of its bound" % (D, D, ratio))
    assert zeros, "an exact zero is not +0.0"
    assert ratio <= (0.1 if tenth else 1.0), "error %.3g of its bound" % ratio
    return ratio


def plain_doubles(model, tfidf, stems=False):
    """The contract restated in plain doubles: the dot products in ascending unit order, the norms as the contract sums
    them -> (C, self)."""
    D = model.n_docs
    df = np.asarray(model.space(stems)[1], dtype=np.float64)
    dense = dense_counts(model, stems)
    n_d = np.maximum(np.asarray(model.n_d, dtype=np.float64), 1.0)
    x = dense.astype(np.float64) / n_d[:, None]
    if tfidf:
        with np.errstate(divide="ignore"):
            x = x * np.where(df > 0, 1.0 + np.log(float(D) / np.maximum(df, 1.0)), 0.0)[None, :]
    gram = np.zeros((D, D), dtype=np.float64)
    for u in range(x.shape[1]):
        gram += np.outer(x[:, u], x[:, u])
    norm = np.ones(D, dtype=np.float64)
    for d in range(D):                                         # the norm of the contract: 64 consecutive slices, then their sums in order
        sq = x[d, dense[d] > 0] ** 2
        if sq.size:
            width = -(-sq.size // 64)
            total = 0.0
            for b in range(0, sq.size, width):
                s = 0.0
                for v in sq[b:b + width].tolist():
                    s += v
                total += s
            norm[d] = np.sqrt(total)
    C = gram / (norm[:, None] * norm[None, :])
    own = C.diagonal().copy()
    np.fill_diagonal(C, np.nan)
    return C, own


# ---- generated collections (the same for both tiers) ---------------------------------------------------------------------
def word(i):
    return "W%05d" % i


def _text(rng, ids, most=3):
    """The units `ids`, each 1 .. most times, shuffled."""
    ids = np.repeat(np.asarray(ids, dtype=np.int64), rng.integers(1, most + 1, size=len(ids)))
    rng.shuffle(ids)
    return " ".join(word(i) for i in ids.tolist())


TILE_EDGE_D = (1, 2, 63, 64, 65, 129)
STOPWORDS = ("the", "and", "of")


@functools.lru_cache(maxsize=None)
def tile_edges(D):
    """D texts over 40 words: one tile, a diagonal tile with a ragged edge, off-diagonal tiles with mirror images."""
    rng = np.random.default_rng(100 + D)
    return [_text(rng, rng.choice(40, size=int(rng.integers(1, 25)), replace=False)) for _ in range(D)]


def unit_edge_sizes(chunk, seg):
    return (chunk - 1, chunk, chunk + 1, seg - 1, seg, seg + 1, 2 * seg + 1)


@functools.lru_cache(maxsize=None)
def unit_edges(U, seg):
    """65 texts over exactly U units.  Text 0 holds every unit in order, so unit i is word(i).  Text 1: only the last unit of
    a segment and the first of the next (U > seg), else the first and the last unit.  Texts 2 and 3: the very last unit is
    their only common one.  The rest: random subsets."""
    rng = np.random.default_rng(200 + U)
    texts = [" ".join(" ".join([word(i)] * (1 + i * 7 % 3)) for i in range(U))]
    texts.append(word(seg - 1) + " " + word(seg) if U > seg else word(0) + " " + word(U - 1))
    half = (U - 1) // 2
    texts.append(_text(rng, list(range(0, half, max(1, half // 20))) + [U - 1]))
    texts.append(_text(rng, list(range(half, U - 1, max(1, half // 20))) + [U - 1]))
    for _ in range(61):
        texts.append(_text(rng, rng.choice(U, size=min(U, int(rng.integers(1, 40))), replace=False)))
    return texts


@functools.lru_cache(maxsize=None)
def document_shapes():
    """An empty text, stopwords only, one kept token, two identical texts, two disjoint ones, ordinary ones."""
    rng = np.random.default_rng(300)
    twin = _text(rng, range(5, 25))
    return ["", "the and of the", word(7), twin, twin, _text(rng, range(100, 120)), _text(rng, range(200, 220)),
            _text(rng, range(0, 110, 3)) + " the of", "a to " + _text(rng, range(15, 30)), "12 ab"]


@functools.lru_cache(maxsize=None)
def cursor_skew():
    """One text holding every unit, beside 64 texts of one posting each."""
    return [" ".join(word(i) for i in range(200))] + [" ".join([word(3 * i)] * (1 + i % 3)) for i in range(64)]


@functools.lru_cache(maxsize=None)
def long_text():
    """A text of 20 000 postings, and three short ones."""
    rng = np.random.default_rng(400)
    return [_text(rng, range(20000), most=2), _text(rng, range(19990, 20010)), _text(rng, range(0, 20000, 997)), word(20005)]


@functools.lru_cache(maxsize=None)
def stem_texts():
    """Words with -S and -ING variants (cosine_exact.ToyStemmer merges them) over 9 texts."""
    rng = np.random.default_rng(500)
    bases = ["WORD%s" % chr(65 + i) * 2 for i in range(12)]
    vocab = [b + s for b in bases for s in ("", "S", "ING")]
    return [" ".join(vocab[i] for i in rng.integers(0, len(vocab), size=int(rng.integers(1, 30))).tolist()) for _ in range(9)]


def collections(chunk, seg):
    """{name: (texts, stopwords, stems)}: every collection of the gpu tier."""
    out = {"tile edges %d" % D: (tile_edges(D), (), False) for D in TILE_EDGE_D}
    out.update({"units %d" % U: (unit_edges(U, seg), (), False) for U in unit_edge_sizes(chunk, seg)})
    out["document shapes"] = (document_shapes(), STOPWORDS, False)
    out["cursor skew"] = (cursor_skew(), (), False)
    out["long text"] = (long_text(), (), False)
    out["stems"] = (stem_texts(), STOPWORDS, True)
    return out


@functools.lru_cache(maxsize=None)
def model_of(name, chunk, seg):
    texts, stop, stems = collections(chunk, seg)[name]
    return cosine_exact.build_model(list(texts), stop, cosine_exact.ToyStemmer() if stems else None, fast=not stems)


@functools.lru_cache(maxsize=None)
def exact_of(name, chunk, seg, tfidf):
    return exact(model_of(name, chunk, seg), tfidf, collections(chunk, seg)[name][2])
