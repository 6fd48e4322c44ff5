"""Exact references of the radix sort, its spine and the scans (csrc/radix_sort.h, csrc/scan.h) in plain numpy with 64-bit
arithmetic: the witness of tests/test_gpu_sort_scan_forms.py, pinned to brute-force restatements by
tests/test_sort_exact_host.py.  Results that the device holds in 32-bit words are returned modulo 2^32, as uint32.
"""
import numpy as np

BINS = 256
FORMS = ("exclusive", "inclusive", "exclusive_in_place", "inclusive_in_place", "with_total")      # east_hip_debug_scan_ex, by number


def digits(keys, bits, begin_bit):
    """The part of every key that orders: the bits [begin_bit, bits)."""
    keys = np.asarray(keys)
    width = bits - begin_bit
    assert 0 <= begin_bit < bits <= keys.dtype.itemsize * 8
    k = keys.astype(np.uint64) >> np.uint64(begin_bit)
    return k if width == 64 else k & np.uint64((1 << width) - 1)


def sort_pairs(keys, vals, bits, begin_bit, doc_off=None):
    """Stable sort of the pairs on the key bits [begin_bit, bits), every document [doc_off[d], doc_off[d + 1]) -- or the
    whole array -- in its own range.  The other bits of a key travel with it and order nothing."""
    keys, vals = np.asarray(keys), np.asarray(vals)
    n = keys.size
    doc_off = [0, n] if doc_off is None else [int(o) for o in doc_off]
    assert doc_off[0] == 0 and doc_off[-1] == n and all(a < b for a, b in zip(doc_off, doc_off[1:]))
    d = digits(keys, bits, begin_bit)
    order = np.empty(n, dtype=np.int64)
    for a, b in zip(doc_off, doc_off[1:]):
        order[a:b] = a + np.argsort(d[a:b], kind="stable")
    return keys[order], vals[order]


def _exclusive(a, axis=0):
    a = np.asarray(a, dtype=np.uint64)
    return np.cumsum(a, axis=axis, dtype=np.uint64) - a


def doc_groups(doc_off, tile, group):
    """doc_group0 of a segmented sort: a document of m pairs has ceil(ceil(m / tile) / group) groups."""
    g0 = [0]
    for a, b in zip(doc_off, doc_off[1:]):
        tiles = -(-(int(b) - int(a)) // tile)
        g0.append(g0[-1] + -(-tiles // group))
    return g0


def spine(group_sum, digit_total, doc_group0, doc_off, shards):
    """group_prefix[g][digit] for the groups [doc_group0[d], doc_group0[d + 1]) of every document d: doc_off[d], plus the
    document's pairs with smaller digits -- its `shards` rows of digit_total added up --, plus the digit's sums in the
    document's earlier groups.  One segment: doc_group0 = [0, n_groups], doc_off = [0]."""
    group_sum = np.asarray(group_sum, dtype=np.uint64).reshape(-1, BINS)
    digit_total = np.asarray(digit_total, dtype=np.uint64).reshape(-1, BINS)
    n_docs = len(doc_group0) - 1
    assert digit_total.shape[0] == n_docs * shards and doc_group0[-1] == group_sum.shape[0]
    out = np.zeros(group_sum.shape, dtype=np.uint64)
    for d in range(n_docs):
        g0, g1 = int(doc_group0[d]), int(doc_group0[d + 1])
        total = digit_total[d * shards:(d + 1) * shards].sum(axis=0, dtype=np.uint64)
        out[g0:g1] = np.uint64(int(doc_off[d])) + _exclusive(total)[None, :] + _exclusive(group_sum[g0:g1], axis=0)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def scan(a, form):
    """The scan of `a` in one of FORMS: n words, n + 1 with the total."""
    a = np.asarray(a, dtype=np.uint64)
    inc = np.cumsum(a, dtype=np.uint64)
    if form in ("inclusive", "inclusive_in_place"):
        out = inc
    elif form in ("exclusive", "exclusive_in_place"):
        out = inc - a
    else:
        assert form == "with_total"
        out = np.concatenate([inc - a, inc[-1:]])
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def run_heads(keys, shift):
    """(inclusive scan of the run heads, their number): position i heads a run where i == 0 or the sorted keys i - 1 and i
    differ above bit `shift`."""
    k = np.asarray(keys, dtype=np.uint64) >> np.uint64(shift)
    head = np.ones(k.size, dtype=np.uint64)
    head[1:] = k[1:] != k[:-1]
    inc = np.cumsum(head, dtype=np.uint64)
    return inc.astype(np.uint32), int(inc[-1])


def pair_bounded(a, b, n_dev, extra):
    """(bound, exclusive scan of a, of b) over [0, bound), bound = min(n, n_dev + extra); nothing is defined behind it."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    bound = min(a.size, n_dev + extra)
    return bound, scan(a[:bound], "exclusive"), scan(b[:bound], "exclusive")


def ascending_offsets(sorted_values, n_values):
    """off[v], v = 0 .. n_values: the first index whose element is >= v (n where there is none)."""
    return np.searchsorted(np.asarray(sorted_values, dtype=np.uint64), np.arange(n_values + 1, dtype=np.uint64), side="left").astype(np.uint32)
