"""The yardstick of the similarity tests: the contract of include/east_hip.h ("Similar texts and keyphrases") in extended
precision, and the ranking's contract applied to a given matrix.  It is never the project's host path.

Profiles are taken as np.longdouble (a 64-bit significand here: sums of L products are off by about L * 2^-64 relative,
below 2^-10 of the bound (2 L + 16) * 2^-53), S = (P @ P.T) / outer(sqrt(q), sqrt(q)) is rounded ONCE to double, and the
contract's two special cases are written in: NaN on the diagonal, +0.0 where a q is zero.  Where np.longdouble is no
wider than a double, `exact` falls back to fractions.Fraction (exact sums, the root by integer square root at 2^-120)
for the cases with M * M * L <= 10^6 and says None for the others."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
WIDE = np.finfo(np.longdouble).nmant >= 63
FRACTION_MAX_WORK = 10 ** 6


def bound(L):
    """|S_device - S_exact| for finite tables."""
    return (2 * L + 16) * U


def gamma(n):
    return n * U / (1.0 - n * U)


def profiles_of(table, axis):
    """axis 0 (by text): the columns; axis 1 (by keyphrase): the rows.  -> M x L."""
    table = np.asarray(table, dtype=np.float64)
    return np.ascontiguousarray(table.T if axis == 0 else table)


def _finish(S, q_zero):
    S = np.array(S, dtype=np.float64)
    S[q_zero[:, None] | q_zero[None, :]] = 0.0
    np.fill_diagonal(S, np.nan)
    return S


def exact_wide(P):
    assert WIDE
    P = np.asarray(P, dtype=np.float64).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (P * P).sum(axis=1)
        root = np.sqrt(q)
        S = ((P @ P.T) / np.outer(root, root)).astype(np.float64)
    return _finish(S, np.asarray(q == 0)), q.astype(np.float64)


def exact_fraction(P):
    """Finite profiles only."""
    P = np.asarray(P, dtype=np.float64)
    M = P.shape[0]
    rows = [[Fraction(float(x)) for x in row] for row in P]
    q = [sum(x * x for x in row) for row in rows]
    S = np.zeros((M, M))
    for a in range(M):
        for b in range(a + 1, M):
            if q[a] == 0 or q[b] == 0:
                continue
            G = sum(x * y for x, y in zip(rows[a], rows[b]))
            r = G * G / (q[a] * q[b])
            root = Fraction(math.isqrt((r.numerator << 240) // r.denominator), 1 << 120)
            S[a, b] = S[b, a] = float(root if G >= 0 else -root)
    return _finish(S, np.array([x == 0 for x in q], dtype=bool)), np.array([float(x) for x in q])


def exact(P):
    """(S[M, M] rounded once to double, q[M] rounded to double) of the M x L profiles, or None where only the Fraction
    model is at hand and the case is too large for it."""
    if WIDE:
        return exact_wide(P)
    P = np.asarray(P)
    if P.shape[0] * P.shape[0] * P.shape[1] > FRACTION_MAX_WORK or not np.isfinite(P).all():
        return None
    return exact_fraction(P)


def select(matrix, n, threshold):
    """The ranking's contract on the rows of a matrix: per row the members with value >= threshold (a NaN never), by
    value descending and member index ascending among equal values, the first n.  -> (count[M], index[M, n], score[M, n]),
    -1 and 0.0 behind the count (np.lexsort as tests/test_gpu_top.py does it)."""
    M = matrix.shape[0]
    count = np.zeros(M, dtype=np.int32)
    index = np.full((M, n), -1, dtype=np.int32)
    score = np.zeros((M, n), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for s, values in enumerate(matrix):
            eligible = np.flatnonzero(values >= threshold)
            order = eligible[np.lexsort((eligible, -values[eligible]))][:n]
            count[s] = order.size
            index[s, :order.size] = order
            score[s, :order.size] = values[order]
    return count, index, score
