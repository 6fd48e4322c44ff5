# -*- coding: utf-8 -*-
"""An exact host model of the BM25 score call (include/east_hip.h, "BM25"), standing on
cosine_exact.build_model: n_d, df, the counts and the class maps are that model's integers.  A plain module: no test, no
fixture, nothing of east.relevance.

    idf_u = log1p((D - df_u + 0.5) / (df_u + 0.5))
    w_ud  = idf_u * (c_ud * (k1 + 1)) / (c_ud + k1 * ((1 - b) + b * (n_d / avgdl))),   avgdl = N / D
    score(k, d) = sum of qtf_ku * w_ud over the distinct units of keyphrase k with a posting in d

What is exact and what is rounded.  k1 and b are taken as the doubles they are (exactly); D, df, c, n_d, N and qtf are
Python integers.  log1p, every quotient, product and sum are computed at 50 decimal digits (mpmath, cosine_exact's
context) -- 1e-50 relative each, a dozen per term -- and a score is rounded ONCE to double: the correctly rounded score
unless the exact value lies within 1e-48 relative of a rounding boundary, i.e. 0.5 units of 2^-53 (+ 1e-48) against a
bound of at least 25 units.  `avgdl` (the double every path shares) is N / D correctly rounded: Python's int / int.
"""
from collections import Counter

import numpy as np

from cosine_exact import MP

K1, B = 1.2, 0.75
UNIT = 2.0 ** -53
BOUND_EXTRA = 24                               # the issue's bound: (t + 24) * 2^-53 * exact (DESIGN.md 18 derives t + 16)
PARAMETERS = [(1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (2.0, 1.0), (0.001, 0.5), (100.0, 0.3)]


def total(model):
    return sum(model.n_d)


def avgdl(model):
    return total(model) / model.n_docs


def idf(n_docs, df):
    """log1p((D - df + 0.5) / (df + 0.5)) at 50 digits: (2 D - 2 df + 1) / (2 df + 1) is exact in integers."""
    return MP.log1p(MP.mpf(2 * n_docs - 2 * df + 1) / (2 * df + 1))


class Bm25(object):
    """The weights of one model, vector space and (k1, b), made per unit on first use."""

    def __init__(self, model, k1=K1, b=B, stems=False):
        self.model, self.stems = model, stems
        self.k1, self.b = MP.mpf(float(k1)), MP.mpf(float(b))
        self.counts, self.df, self.n_units, _ = model.space(stems)
        self.inv = model._inverted(stems)
        N = total(model)
        # k1 * ((1 - b) + b * (n_d / avgdl)), n_d / avgdl = n_d * D / N exactly
        self.norm = [self.k1 * ((1 - self.b) + self.b * (MP.mpf(n * model.n_docs) / N)) if N else None for n in model.n_d]
        self._idf, self._w = {}, {}

    def unit_weights(self, u):
        """[(document, w_ud)] of unit u, the documents ascending."""
        if u not in self._w:
            df = self.df[u]
            if df not in self._idf:
                self._idf[df] = idf(self.model.n_docs, df)
            f = self._idf[df] * (self.k1 + 1)
            self._w[u] = [(d, f * c / (c + self.norm[d])) for d, c in self.inv.get(u, ())]
        return self._w[u]

    def scores_from_ids(self, q_ids):
        """(K x D doubles, K x D contributing units t): q_ids[k] = the ids of keyphrase k's kept tokens, -1 outside."""
        out = np.zeros((len(q_ids), self.model.n_docs), dtype=np.float64)
        terms = np.zeros((len(q_ids), self.model.n_docs), dtype=np.int64)
        rows = {}
        for k, ids in enumerate(q_ids):
            c = Counter(int(i) for i in ids if i >= 0)
            if not c:
                continue
            key = tuple(sorted(c.items()))
            if key not in rows:
                acc, t = {}, {}
                for u, qtf in key:
                    for d, w in self.unit_weights(u):
                        acc[d] = acc.get(d, 0) + qtf * w
                        t[d] = t.get(d, 0) + 1
                docs = np.fromiter(acc.keys(), dtype=np.int64, count=len(acc))
                rows[key] = (docs, np.array([float(v) for v in acc.values()], dtype=np.float64),
                             np.fromiter((t[d] for d in acc), dtype=np.int64, count=len(acc)))
            docs, vals, ts = rows[key]
            out[k, docs] = vals
            terms[k, docs] = ts
        return out, terms

    def scores(self, prepared_queries):
        return self.scores_from_ids(self.model.query_ids(prepared_queries, self.stems))


def share_of_bound(got, exact, terms, extra=BOUND_EXTRA):
    """(the largest |got - exact| / ((t + extra) * 2^-53 * exact) over the scores above zero, their number, the zeros are
    the same and +0.0)."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    nz = exact != 0.0
    zeros_ok = bool(np.array_equal(got == 0.0, ~nz)) and not np.signbit(got[~nz]).any()
    if not nz.any():
        return 0.0, 0, zeros_ok
    bound = (terms[nz] + extra) * UNIT * exact[nz]
    return float((np.abs(got[nz] - exact[nz]) / bound).max()), int(nz.sum()), zeros_ok


def check(got, exact, terms, what="bm25"):
    share, n, zeros_ok = share_of_bound(got, exact, terms)
    print("%s %s: %d scores above zero, largest error %.3f of the bound (t + %d) * 2^-53" % (what, np.shape(got), n, share, BOUND_EXTRA))
    assert np.isfinite(np.asarray(got)).all()
    assert zeros_ok, "the zeros differ or are not +0.0"
    assert (np.asarray(got) >= 0.0).all()
    assert share <= 1.0, "error %.3f of the bound" % share
    return share


# ---- collections both tiers use ------------------------------------------------------------------------------------------
def small_collection():
    """(texts, stopwords): EVERY has df = D, several words df = 1, THOUSAND a count of 1 000, an empty text and a text of
    stopwords only (n_d = 0)."""
    texts = ["every alpha beta beta gamma", "every " + "thousand " * 1000 + "alpha", "", "the and the", "every delta alpha alpha alpha epsilon",
             "every beta zeta", "every"]
    return texts, ["the", "and"]


def small_collection_full_df():
    """As small_collection without the two texts that have no term: EVERY has df = D."""
    texts, stop = small_collection()
    return [t for i, t in enumerate(texts) if i not in (2, 3)], stop


WORKED_TEXTS = ["alpha beta beta", "alpha gamma"]
WORKED = {"BETA": (0.902321773509988, 0.0), "ALPHA": (0.1685325314902102, 0.19856803215183177), "GAMMA": (0.0, 0.7549127709068711),
          "BETA BETA ALPHA": (1.9731760785101862, None)}
