"""An exact host model of text-to-text relatedness (include/east_hip.h, "Text-to-text relatedness"; csrc/related.h).

Inputs: the strings of every text (collections[A] = a list of str) and a function score(s, B) that gives the double the
device computes for the string s against document B.  A string is scored when it is not empty once U+0020 is removed;
c_A = the scored strings of A.

    F[A][B] = (the sum over the scored strings s of A of score(s, B)) / c_A, 0 when c_A = 0
    directed (0):  R[A][B] = F[A][B];   symmetric (1):  R[A][B] = (F[A][B] + F[B][A]) / 2
    R[A][A] = NaN, self[A] = F[A][A]

Everything is evaluated with fractions.Fraction over the given doubles -- no rounding at all -- and rounded once at the
end.  The bound an implementation has to meet is per entry (max(c_A, c_B) + 4) * 2^-53 * exact: summing c finite
non-negative terms in any order is off by less than gamma_(c-1) relative, one rounding for the division, one for the
addition of the symmetric form; the halving is exact.
"""
from fractions import Fraction

import numpy as np

DIRECTED, SYMMETRIC = 0, 1
U = Fraction(1, 2 ** 53)


def scored_strings(strings):
    return [s for s in strings if s.replace(" ", "")]


class Exact(object):
    """The model's result: R, own (self), scored rounded once; x[a][b] / f[a] the exact values as Fractions (x[a][a] is
    None); c[a][b] the number of terms the bound counts."""

    def __init__(self, R, own, scored, x, f, c):
        self.R, self.own, self.scored, self.x, self.f, self.c = R, own, scored, x, f, c

    def allowed(self, a, b):
        return (self.c[a][b] + 4) * U * self.x[a][b]

    def allowed_self(self, a):
        return (int(self.scored[a]) + 4) * U * self.f[a]


def exact(collections, score, orientation):
    D = len(collections)
    kept = [scored_strings(strings) for strings in collections]
    scored = np.array([len(k) for k in kept], dtype=np.int32)
    F = [[Fraction(0)] * D for _ in range(D)]
    for a in range(D):
        if not kept[a]:
            continue
        for b in range(D):
            total = Fraction(0)
            for s in kept[a]:
                v = float(score(s, b))
                assert np.isfinite(v) and v >= 0.0, (s, b, v)
                total += Fraction(v)
            F[a][b] = total / len(kept[a])
    R = np.full((D, D), np.nan)
    x = [[None] * D for _ in range(D)]
    c = [[0] * D for _ in range(D)]
    own = np.array([float(F[a][a]) for a in range(D)], dtype=np.float64)
    for a in range(D):
        for b in range(D):
            if a == b:
                continue
            x[a][b] = (F[a][b] + F[b][a]) / 2 if orientation == SYMMETRIC else F[a][b]
            c[a][b] = max(int(scored[a]), int(scored[b]))
            R[a, b] = float(x[a][b])
    return Exact(R, own, scored, x, [F[a][a] for a in range(D)], c)


def check(matrix, own, scored, want, slack=1):
    """Asserts a result (matrix, self, scored) against exact()'s: every entry within slack x the bound of the exact value
    (slack 2: an implementation against another one's exact values), compared in exact arithmetic."""
    matrix = np.asarray(matrix, dtype=np.float64)
    D = len(want.scored)
    assert matrix.shape == (D, D)
    assert np.array_equal(np.asarray(scored), want.scored)
    worst = Fraction(0)
    for a in range(D):
        assert np.isnan(matrix[a, a])
        err = abs(Fraction(float(own[a])) - want.f[a])
        assert err <= slack * want.allowed_self(a), (a, float(err), float(want.allowed_self(a)))
        if want.scored[a] == 0:
            assert own[a] == 0.0 and not np.signbit(own[a])
        for b in range(D):
            if a == b:
                continue
            v = float(matrix[a, b])
            assert v == v, (a, b)
            err = abs(Fraction(v) - want.x[a][b])
            assert err <= slack * want.allowed(a, b), (a, b, float(err), float(want.allowed(a, b)))
            if want.x[a][b]:
                worst = max(worst, err / want.allowed(a, b))
    return float(worst)
