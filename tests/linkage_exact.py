"""The model of complete and average linkage (include/east_hip.h, "Clusters"): the contract's rounds, a row and a merged
pair at a time, and the exact cluster means as fractions over the original matrix.  Nothing is shared with the library or
with east.applications; the matrix families are those of clusters_exact and two more."""
from fractions import Fraction

import numpy as np

import clusters_exact

LINKAGES = ("complete", "average")
U = 2.0 ** -53


def refused(S, linkage):
    """The first pair a < b in row-major order whose S[a][b] the linkage does not take, or None."""
    S = np.asarray(S, dtype=np.float64)
    for a in range(S.shape[0]):
        row = S[a, a + 1:]
        bad = np.isnan(row) if linkage == "complete" else ~np.isfinite(row)
        if bad.any():
            return a, a + 1 + int(np.flatnonzero(bad)[0])
    return None


def _lw(linkage, x, y, n, n2):
    """x: the representative's values, y: its partner's; n, n2: their sizes before the round."""
    lo = np.where(y < x, y, x)
    if linkage == "complete":
        return lo
    hi = np.where(y < x, x, y)
    n, n2 = np.asarray(n, dtype=np.float64), np.asarray(n2, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = (n * x + n2 * y) / (n + n2)
    return np.where(r < lo, lo, np.where(r > hi, hi, r))


def rounds(S, linkage, floor=None):
    """-> (merge_a int32, merge_b int32, merge_w float64, the rounds that merged, members: per merge the two sets joined)."""
    assert linkage in LINKAGES and refused(S, linkage) is None
    S = np.asarray(S, dtype=np.float64)
    M = S.shape[0]
    W = np.zeros((M, M))
    for a in range(M):                                      # the upper triangle mirrored, byte for byte
        W[a, a + 1:] = S[a, a + 1:]
        W[a + 1:, a] = S[a, a + 1:]
    alive = list(range(M))
    size = [1] * M
    sets = {v: frozenset([v]) for v in range(M)}
    found, n_rounds = [], 0
    while len(alive) > 1:
        reps = np.asarray(alive)
        nn = {}
        for u in alive:
            others = reps[reps != u]
            nn[u] = int(others[np.argmax(W[u, others])])    # (the first of equal weights: the smallest other end; -0.0 == +0.0)
        pairs = [(u, nn[u]) for u in alive if nn[nn[u]] == u and u < nn[u]
                 and (floor is None or W[u, nn[u]] >= floor)]
        if not pairs:
            break
        partner = dict(pairs)
        gone = set(partner.values())
        for u, u2 in pairs:
            found.append((W[u, u2], n_rounds, u, u2, sets[u], sets[u2]))
        stay = [v for v in alive if v not in gone]
        new = W.copy()
        all_stay = np.asarray(stay, dtype=np.int64)
        all_has = np.asarray([v in partner for v in stay])
        all_other = np.asarray([partner.get(v, v) for v in stay], dtype=np.int64)
        all_n = np.asarray([size[v] for v in stay], dtype=np.float64)
        all_n2 = np.asarray([size[v] for v in all_other], dtype=np.float64)
        for i, u in enumerate(stay):                        # the pairs (u, v), u < v, of the representatives that stay
            later, has, other, n, n2 = all_stay[i + 1:], all_has[i + 1:], all_other[i + 1:], all_n[i + 1:], all_n2[i + 1:]
            if not later.size or (u not in partner and not has.any()):
                continue

            def c(x):
                return np.where(has, _lw(linkage, W[x, later], W[x, other], n, n2), W[x, later])

            value = _lw(linkage, c(u), c(partner[u]), size[u], size[partner[u]]) if u in partner else c(u)
            new[u, later] = value
            new[later, u] = value
        W = new
        for u, u2 in pairs:
            size[u] += size[u2]
            sets[u] = sets[u] | sets[u2]
        alive = stay
        n_rounds += 1
    found.sort(key=lambda m: (-(m[0] + 0.0), m[1], m[2]))
    return (np.asarray([m[2] for m in found], dtype=np.int32), np.asarray([m[3] for m in found], dtype=np.int32),
            np.asarray([m[0] for m in found], dtype=np.float64), n_rounds, [(m[4], m[5]) for m in found])


def merges(S, linkage, floor=None):
    return rounds(S, linkage, floor)[:3]


def exact_mean(S, A, B):
    """The mean of S[a][b] (the upper triangle's value) over a in A, b in B, as a Fraction."""
    total = Fraction(0)
    for a in A:
        for b in B:
            total += Fraction(float(S[min(a, b), max(a, b)]))
    return total / (len(A) * len(B))


def average_bound(S, A, B):
    """The contract's bound on |merge_w - exact mean| for the merge of A and B."""
    M = S.shape[0]
    biggest = float(np.max(np.abs(S[np.triu_indices(M, 1)])))
    return 4.0 * (len(A) + len(B)) * U * biggest


def share_of_bound(S, result):
    """The largest |merge_w - exact mean| / bound over the merges of an average-linkage result of rounds()."""
    worst = 0.0
    for w, (A, B) in zip(result[2].tolist(), result[4]):
        err = abs(Fraction(w) - exact_mean(S, A, B))
        bound = Fraction(average_bound(S, A, B))
        assert err <= bound, (w, sorted(A), sorted(B))
        if bound:
            worst = max(worst, float(err / bound))
    return worst


# ---- matrix families ------------------------------------------------------------------------------------------------------
def family(name, M, seed=0):
    rng = np.random.RandomState(seed + 104729 * M + 1)
    if name == "zero_plateau":                              # 90 % exact +0.0: texts without a common term
        vals = rng.rand(M, M)
        vals[rng.rand(M, M) < 0.9] = 0.0
        return clusters_exact.symmetric(vals)
    if name == "dyadic":                                    # distinct multiples of 2^-20 in [0, 1): 1 - s is exact, no ties
        n = M * (M - 1) // 2
        assert n <= 1 << 20
        S = np.zeros((M, M))
        S[np.triu_indices(M, 1)] = rng.permutation(1 << 20)[:n] / float(1 << 20)
        S = S + S.T
        np.fill_diagonal(S, np.nan)
        return S
    return clusters_exact.family(name, M, seed)
