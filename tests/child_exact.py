"""The child tables and the lcp-interval lefts by their definitions, in plain Python over lists of ints: the witness of
tests/test_gpu_child_tables.py (csrc/tables.h: child_stream_kernel, child_wide_kernel, interval_left_kernel), pinned to
the oracle by tests/test_child_exact_host.py.

For a table v of n values in documents [seg, end) whose first ranks hold 0:
  PSE[k]  the nearest p < k with v[p] <= v[k] (-1: none -- only where a document's first rank is rank 0)
  NSE[k]  the nearest q > k with v[q] <= v[k], over the table extended by a 0 at n (so there always is one)
  up[k]   the leftmost position of the minimum of the open interval (PSE[k], k), if k > seg and k - PSE[k] > 1
  next[k] NSE[k], if NSE[k] < end and v[NSE[k]] == v[k]
  down[k] the leftmost position of the minimum of (k, NSE[k]), if NSE[k] < end and NSE[k] - k > 1
all three local to the document, 0 otherwise.
  anntab  as in the docstring of tests/test_gpu_annotation_search.py: NSV - PSE for a first l-index (v[k] > 0 and
          v[PSE[k]] < v[k]; NSV the nearest q > k with v[q] < v[k], n if none), n_d - m_d at a document's first rank, else 0
  left[r] the nearest p < k with v[p] < v[k], local to the document, for the ranks k = seg + r with r > 0 and anntab[k] > 0;
          NONE for every other rank (a document's first rank among them, whatever its annotation)

The path of a rank through the kernels, with dl = k - PSE[k] (0 at a document's first rank, which searches nothing to its
left), dr = NSE[k] - k and m = max(dl, dr): REGISTERS if m <= near, LANES (eight lanes with shuffles) if m <= local,
PYRAMID (listed for child_wide_kernel) otherwise.  near and local are the library's, handed in by the caller.

Nothing here knows of tiles, groups of 16 or a pyramid.
"""

NONE = 0xFFFFFFFF
REGISTERS, LANES, PYRAMID = 0, 1, 2


def nearest_not_larger(v):
    """(PSE, NSE) of every rank: two stack passes."""
    n = len(v)
    pse, nse = [-1] * n, [n] * n
    stack = []
    for k in range(n):
        while stack and v[stack[-1]] > v[k]:
            stack.pop()
        pse[k] = stack[-1] if stack else -1
        stack.append(k)
    stack = [n]                                 # (the 0 behind the table: never popped)
    for k in range(n - 1, -1, -1):
        while stack[-1] < n and v[stack[-1]] > v[k]:
            stack.pop()
        nse[k] = stack[-1]
        stack.append(k)
    return pse, nse


def next_smaller(v):
    """NSV of every rank: the nearest q > k with v[q] < v[k], n if none."""
    n = len(v)
    nsv = [n] * n
    stack = []
    for k in range(n - 1, -1, -1):
        while stack and v[stack[-1]] >= v[k]:
            stack.pop()
        nsv[k] = stack[-1] if stack else n
        stack.append(k)
    return nsv


def _leftmost_argmin(v, a, b):
    """Leftmost position of the minimum of the open interval (a, b), a + 1 < b."""
    seg = v[a + 1:b]
    return a + 1 + seg.index(min(seg))


class Child(object):
    """up, down, next, left (lists over all ranks, document-local values), ann, and pse / nse (global ranks)."""

    def __init__(self, lcp, doc_off=None, n_strings=None):
        v = [int(x) for x in lcp]
        n = len(v)
        doc_off = [0, n] if doc_off is None else [int(o) for o in doc_off]
        n_strings = [1] * (len(doc_off) - 1) if n_strings is None else [int(m) for m in n_strings]
        assert n >= 1 and doc_off[0] == 0 and doc_off[-1] == n and len(n_strings) == len(doc_off) - 1
        self.v, self.n, self.doc_off, self.n_strings = v, n, doc_off, n_strings
        self.pse, self.nse = nearest_not_larger(v)
        nsv = next_smaller(v)
        self.up, self.down, self.next = [0] * n, [0] * n, [0] * n
        self.ann, self.left = [0] * n, [NONE] * n
        self.seg_of = [0] * n
        for d in range(len(doc_off) - 1):
            seg, end = doc_off[d], doc_off[d + 1]
            assert seg < end and v[seg] == 0, "a document's first rank holds 0"
            self.ann[seg] = (end - seg - n_strings[d]) & 0xFFFFFFFF
            for k in range(seg, end):
                self.seg_of[k] = seg
                p, q = self.pse[k], self.nse[k]
                if k > seg:
                    assert p >= seg             # (the document's own zero at the latest)
                    if k - p > 1:
                        self.up[k] = _leftmost_argmin(v, p, k) - seg
                    if v[k] > 0 and v[p] < v[k]:
                        self.ann[k] = nsv[k] - p
                        self.left[k] = p - seg
                if q < end:
                    if v[q] == v[k]:
                        self.next[k] = q - seg
                    if q - k > 1:
                        self.down[k] = _leftmost_argmin(v, k, q) - seg
        for k in range(n):                      # left is none wherever the annotation is 0, and at every first rank
            assert (self.left[k] != NONE) == (self.ann[k] > 0 and k != self.seg_of[k])

    def reach(self, k):
        """(dl, dr): how far the searches of rank k go to either side."""
        return (k - self.pse[k] if k > self.seg_of[k] else 0), self.nse[k] - k

    def path(self, k, near, local):
        m = max(self.reach(k))
        return REGISTERS if m <= near else LANES if m <= local else PYRAMID

    def paths(self, near, local):
        """Number of ranks per path: [registers, lanes, pyramid]."""
        count = [0, 0, 0]
        for k in range(self.n):
            count[self.path(k, near, local)] += 1
        return count
