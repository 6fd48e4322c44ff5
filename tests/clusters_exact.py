"""The model of the clusters (include/east_hip.h, "Clusters"): Kruskal's algorithm over all pairs that are not NaN, visited
strongest first, a plain union-find, and the two cuts.  Only comparisons; nothing is shared with the library or with
east.applications."""
import numpy as np


def sorted_edges(S):
    """Every pair a < b whose S[a][b] is not a NaN, strongest first -> (a, b, w): w descending with -0.0 == +0.0, then a
    ascending, then b ascending.  w is the upper triangle's own bytes."""
    S = np.asarray(S, dtype=np.float64)
    M = S.shape[0]
    a, b = np.triu_indices(M, 1)
    w = S[a, b]
    keep = ~np.isnan(w)
    a, b, w = a[keep], b[keep], w[keep]
    falling = -(w + 0.0)                    # (-0.0 + 0.0 is +0.0: both zeros become one key; infinities stay themselves)
    order = np.lexsort((b, a, falling))     # (the last key is the first to count)
    return a[order], b[order], w[order]


class _Sets(object):
    def __init__(self, M):
        self.parent = list(range(M))

    def find(self, v):
        p = self.parent
        while p[v] != v:
            p[v] = p[p[v]]
            v = p[v]
        return v

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        if b < a:
            a, b = b, a
        self.parent[b] = a                  # (the smaller root stays: a root is the smallest member of its set)
        return True


def merges(S):
    """The dendrogram -> (merge_a int32, merge_b int32, merge_w float64), strongest first: the edges Kruskal accepts."""
    S = np.asarray(S, dtype=np.float64)
    M = S.shape[0]
    a, b, w = sorted_edges(S)
    sets = _Sets(M)
    took = []
    for i in range(a.size):
        if len(took) == M - 1:
            break                           # (a spanning tree: every later edge closes a cycle)
        if sets.union(int(a[i]), int(b[i])):
            took.append(i)
    took = np.asarray(took, dtype=np.int64)
    return a[took].astype(np.int32), b[took].astype(np.int32), w[took].copy()


def applied_by_threshold(merge_w, t):
    """The merges with w >= t: a prefix of the list -> its length."""
    n = 0
    while n < len(merge_w) and merge_w[n] >= t:
        n += 1
    return n


def applied_by_count(M, F, k):
    return max(0, min(F, M - k))


def labels_after(M, merge_a, merge_b, n):
    """labels[v] = the smallest member of v's cluster after the first n merges (int32)."""
    sets = _Sets(M)
    for i in range(n):
        sets.union(int(merge_a[i]), int(merge_b[i]))
    return np.asarray([sets.find(v) for v in range(M)], dtype=np.int32)


def cut(M, merge_a, merge_b, merge_w, threshold=None, k=None):
    """-> (labels, clusters, merges applied)"""
    n = applied_by_threshold(merge_w, threshold) if threshold is not None else applied_by_count(M, len(merge_a), k)
    return labels_after(M, merge_a, merge_b, n), M - n, n


# ---- matrix families of the tests --------------------------------------------------------------------------------------
def symmetric(upper):
    """The upper triangle mirrored, NaN on the diagonal."""
    S = np.triu(upper, 1)
    S = S + S.T
    np.fill_diagonal(S, np.nan)
    return S


def family(name, M, seed=0):
    rng = np.random.RandomState(seed + 7919 * M)
    if name == "distinct":
        vals = rng.permutation(M * M).astype(np.float64).reshape(M, M) / max(M * M, 1)
        return symmetric(vals)
    if name == "ties":
        S = np.full((M, M), np.nan)
        iu = np.triu_indices(M, 1)
        w = rng.choice(np.array([-0.0, 0.0, 0.25, 0.5]), size=iu[0].size)
        S[iu] = w
        S[iu[1], iu[0]] = np.where(w == 0.0, rng.choice(np.array([-0.0, 0.0]), size=w.size), w)   # a zero's mirror image takes either sign
        return S
    if name == "equal":
        S = np.full((M, M), 0.375)
        np.fill_diagonal(S, np.nan)
        return S
    if name == "chain":
        S = np.zeros((M, M))
        for i in range(M - 1):
            S[i, i + 1] = S[i + 1, i] = float(M - i)
        np.fill_diagonal(S, np.nan)
        return S
    if name == "hierarchy":
        bits = max(int(M - 1).bit_length(), 1)
        idx = np.arange(M)
        x = (idx[:, None] ^ idx[None, :]).astype(np.float64)
        lead = bits - np.frexp(x)[1].astype(np.float64)      # (frexp's exponent of an integer is its bit length)
        return symmetric(lead)
    if name == "nan":
        vals = rng.rand(M, M)
        vals[rng.rand(M, M) < 0.15] = np.nan
        S = symmetric(np.where(np.isnan(vals), 0.0, vals))
        gone = np.triu(np.isnan(vals), 1)
        S[gone | gone.T] = np.nan
        for v in rng.choice(M, size=min(3, M), replace=False):
            S[v, :] = np.nan
            S[:, v] = np.nan
        return S
    if name == "inf":
        vals = rng.choice(np.array([-np.inf, np.inf, -1.0, 0.0, 1.0, 2.5]), size=(M, M))
        S = np.triu(vals, 1)
        S = S + S.T                         # (one of the two is 0 everywhere: no inf - inf)
        np.fill_diagonal(S, np.nan)
        return S
    raise ValueError(name)
