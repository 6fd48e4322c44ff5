"""gpu tier: the annotation pass on built tables (csrc/tables.h: ann_stream_kernel, ann_wide_kernel; csrc/build.h: annotate).

Everything goes through east_hip_debug_annotate, which uploads a caller's table and runs the function the build calls.
The witness is a stack pass in this file: for every rank the nearest value <= its own to the left and the nearest value
< its own to the right; anntab[k] = NSV - PSE for a first l-index, 0 where the left neighbour found is equal or missing,
n_d - m_d for the zero at a document's first rank and 0 for every other zero.  The model is defined for any table of
u32 values, LCP table or not.

The tile, the halo and the near reach come from the library (geometry_out), never from constants here.  The number of
ranks that went through ann_wide_kernel is compared with the model's count of ranks whose answer lies outside the staged
window (tile + halo to either side) in both directions: tables whose answers all lie inside it must list nothing, and no
table may list fewer or more ranks than the model says.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_u32p, _i64p, _i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)


def _annotate(hip, lcp, doc_off=None, n_strings=None):
    """(anntab, (tile, halo, near), listed) of the device's pass over `lcp`."""
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    n = int(lcp.size)
    doc_off = np.array([0, n] if doc_off is None else doc_off, dtype=np.int64)
    n_strings = np.array([1] * (doc_off.size - 1) if n_strings is None else n_strings, dtype=np.int32)
    ann = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    geo = np.zeros(3, dtype=np.uint32)
    listed = np.full(1, 0xDEADBEEF, dtype=np.uint32)
    rc = hip.load().east_hip_debug_annotate(0, lcp.ctypes.data_as(_u32p), n, doc_off.ctypes.data_as(_i64p), doc_off.size - 1,
                                            n_strings.ctypes.data_as(_i32p), ann.ctypes.data_as(_u32p),
                                            geo.ctypes.data_as(_u32p), listed.ctypes.data_as(_u32p))
    assert rc == 0, (rc, hip.load().east_hip_last_error())
    return ann, tuple(int(x) for x in geo), int(listed[0])


@pytest.fixture(scope="module")
def geometry(hip):
    _, geo, _ = _annotate(hip, np.zeros(1, dtype=np.uint32))
    tile, halo, near = geo
    assert tile % 16 == 0 and halo % 16 == 0 and 0 < near <= halo < tile
    return geo


def _model(lcp, doc_off, n_strings, tile, halo):
    """(anntab, number of ranks whose PSE -- or, for a first l-index, whose NSV -- lies outside the rank's staged window)."""
    v = [int(x) for x in lcp]
    n = len(v)
    pse, nsv = [-1] * n, [n] * n
    stack = []
    for k in range(n):                          # nearest p < k with v[p] <= v[k]
        while stack and v[stack[-1]] > v[k]:
            stack.pop()
        pse[k] = stack[-1] if stack else -1
        stack.append(k)
    stack = []
    for k in range(n - 1, -1, -1):              # nearest q > k with v[q] < v[k]
        while stack and v[stack[-1]] >= v[k]:
            stack.pop()
        nsv[k] = stack[-1] if stack else n
        stack.append(k)
    ann = np.zeros(n, dtype=np.uint32)
    starts = {int(o): d for d, o in enumerate(doc_off[:-1])}
    listed = 0
    for k in range(n):
        if v[k] == 0:
            if k in starts:
                d = starts[k]
                ann[k] = (int(doc_off[d + 1]) - k - int(n_strings[d])) & 0xFFFFFFFF
            continue
        p, q = pse[k], nsv[k]
        first = p >= 0 and v[p] < v[k]
        if first:
            ann[k] = q - p
        base = k // tile * tile
        if p < base - halo or (first and q >= base + tile + halo):
            listed += 1
    return ann, listed


def _check(hip, lcp, doc_off=None, n_strings=None, what="", inside=None):
    """The whole table against the model, and the listed count; inside=True / False: what the table was built for."""
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    n = int(lcp.size)
    doc_off = [0, n] if doc_off is None else doc_off
    n_strings = [1] * (len(doc_off) - 1) if n_strings is None else n_strings
    ann, (tile, halo, _), listed = _annotate(hip, lcp, doc_off, n_strings)
    want, want_listed = _model(lcp, doc_off, n_strings, tile, halo)
    bad = np.flatnonzero(ann != want)
    assert bad.size == 0, (what, n, "first differing ranks", bad[:8], ann[bad[:8]], want[bad[:8]])
    if inside is True:
        assert want_listed == 0, (what, "the table was built to stay inside the window", want_listed)
    if inside is False:
        assert want_listed > 0, (what, "the table was built to leave the window")
    assert listed == want_listed, (what, n, listed, want_listed)
    return want_listed


def _distances(tile, halo, near):
    return [1, near - 1, near, near + 1, 15, 16, 17, 63, 64, 65, halo - 1, halo, halo + 1, tile - 1, tile, tile + 1, 2 * tile + 3]


def _positions(tile):
    """Targets at 0, 1, 15, 16, tile - 1 mod tile in the first, a middle and the last tile of a table of 3 tiles + 5."""
    return [t * tile + r for t in (0, 1, 2) for r in (0, 1, 15, 16, tile - 1)]


def _distance_table(rng, n, at, d_left, d_right, v=5, equal_left=False):
    """Fillers > v everywhere, a few fillers == v to the right of the target, the value v at `at`, a smaller value (or, for a
    later l-index, an equal one) d_left before it and a smaller one d_right behind it -- where the table has the room; where it
    has not, the answer is the table's first entry (0) to the left and the table's end to the right."""
    lcp = rng.integers(v + 1, v + 4, size=n).astype(np.uint32)
    lcp[0] = 0
    if at == 0:
        return lcp                              # (rank 0 is the root: nothing to place)
    lcp[at] = v
    if at - d_left >= 1:
        lcp[at - d_left] = v if equal_left else v - 1
    hi = min(at + d_right, n)
    between = np.arange(at + 1, hi)
    if between.size:
        lcp[rng.choice(between, size=min(3, between.size), replace=False)] = v
    if at + d_right < n:
        lcp[at + d_right] = v - 1
    return lcp


def test_distances_to_both_neighbours(hip, geometry):
    """A rank whose PSV lies d_left before it and whose NSV lies d_right behind it, at every distance at which the kernel
    takes another path (the register pass, the rank's own group, the row of group minima, the halo's end, the next tile,
    past the window) and at every position class; every distance meets every position on either side."""
    tile, halo, near = geometry
    rng = np.random.default_rng(1)
    dist, n = _distances(tile, halo, near), 3 * tile + 5
    for i, at in enumerate(_positions(tile)):
        for j, d_left in enumerate(dist):
            d_right = dist[(i + j) % len(dist)]
            lcp = _distance_table(rng, n, at, d_left, d_right)
            _check(hip, lcp, what="at %d, PSV %d before, NSV %d behind" % (at, d_left, d_right))


def test_answers_inside_the_window_list_nothing(hip, geometry):
    """Tables built so that every answer lies in the staged window: nothing may go through ann_wide_kernel.  The model
    computes the condition (inside=True fails the test if a table is not what it was built to be).  All fillers are equal,
    so each finds its answer in its left neighbour, and what remains are the ranks placed here."""
    tile, halo, near = geometry
    n = 3 * tile + 5
    n_fit = 0
    for at in _positions(tile)[5:] + [tile + halo, 2 * tile + halo]:             # (the middle and the last tile)
        for d in (near + 1, 17, 65, halo - 1, halo):
            # zeros, then from at - d on: 4, fillers, the target 5 at `at`, fillers, 4 at at + d, zeros.  The second 4 finds the
            # first 2 d before it: inside its window if both lie in one tile, or d is short enough
            lcp = np.zeros(n, dtype=np.uint32)
            hi = min(at + d, n - 1)
            lcp[at - d:hi + 1] = 9
            lcp[at - d] = lcp[hi] = 4
            lcp[at] = 5
            # (... and the first 4 finds the zero behind the second, 2 d + 1 behind it)
            fits = (hi // tile == at // tile or at - d >= hi // tile * tile - halo) and hi + 1 < (at - d) // tile * tile + tile + halo
            n_fit += fits
            _check(hip, lcp, what="at %d, both neighbours %d away" % (at, d), inside=True if fits else None)
    assert n_fit >= 36, n_fit                   # (of 60: not a test that passes by building nothing that fits)
    # from a tile's second rank to its last, and from its last but one back to its first
    for t in (1, 2):
        lcp = np.zeros(n, dtype=np.uint32)
        lo, hi = t * tile, t * tile + tile - 1
        lcp[lo:hi + 1] = 9
        lcp[lo] = lcp[hi] = 4
        lcp[lo + 1] = lcp[hi - 1] = 5
        _check(hip, lcp, what="across tile %d" % t, inside=True)
    # ... and from the left halo's first rank to the tile's first, from the tile's last to the right halo's last
    lcp = np.zeros(n, dtype=np.uint32)
    lcp[tile - halo:tile + 1] = 9
    lcp[tile - halo] = 4
    lcp[tile] = 5
    lcp[2 * tile - 1:2 * tile + halo - 1] = 9
    lcp[2 * tile - 1] = 5
    _check(hip, lcp, what="the halo's ends", inside=True)


def test_answers_outside_the_window_are_listed(hip, geometry):
    tile, halo, near = geometry
    rng = np.random.default_rng(3)
    n = 3 * tile + 5
    for at in (tile + 1, 2 * tile + 16, 3 * tile - 1):
        for d_left, d_right in ((halo + 17, 1), (at - 1, 3)):
            lcp = _distance_table(rng, n, at, max(d_left, at % tile + halo + 1), d_right)
            _check(hip, lcp, what="left far, at %d" % at, inside=False)
    for at in (1, 16, tile - 1, tile + 15):
        lcp = _distance_table(rng, n, at, 1, tile - at % tile + halo + 1)
        _check(hip, lcp, what="right far, at %d" % at, inside=False)


def test_equal_value_chains(hip, geometry):
    """Later l-indices: the nearest value <= the rank's own is EQUAL to it and lies d before it -- the answer is 0 at any
    distance, and the rank is listed exactly when that neighbour lies outside the window."""
    tile, halo, near = geometry
    rng = np.random.default_rng(4)
    dist, n = _distances(tile, halo, near), 3 * tile + 5
    for i, at in enumerate(_positions(tile)):
        for j, d in enumerate(dist):
            lcp = _distance_table(rng, n, at, d, dist[(2 * i + j + 5) % len(dist)], equal_left=True)
            _check(hip, lcp, what="at %d, equal neighbour %d before" % (at, d))
    # a long chain: every 7th / every (halo + 1)th rank carries the same value, larger ones in between
    for step in (7, halo + 1, tile + halo + 1):
        lcp = rng.integers(6, 9, size=n).astype(np.uint32)
        lcp[0] = 0
        lcp[1::step] = 5
        _check(hip, lcp, what="chain of step %d" % step)


def _random_table(rng, n, kind):
    if kind == "geometric":
        lcp = (rng.geometric(0.3, size=n) - 1).astype(np.uint32)
    elif kind == "deep geometric":
        lcp = rng.geometric(0.02, size=n).astype(np.uint32)
    else:
        lcp = np.abs(np.cumsum(rng.integers(-3, 4, size=n))).astype(np.uint32)
    lcp[0] = 0
    return lcp


def test_table_sizes_and_ends(hip, geometry):
    """The end of the table inside a group, at a group's end, at a tile's end; the table's padding; a table without a
    level 1 (at most 16 entries)."""
    tile, halo, near = geometry
    rng = np.random.default_rng(5)
    for n in (1, 15, 16, 17, tile - 1, tile, tile + 1, 3 * tile + 5):
        for kind in ("geometric", "deep geometric", "walk"):
            _check(hip, _random_table(rng, n, kind), n_strings=[int(rng.integers(0, 4))], what="%s, n = %d" % (kind, n))
        # nothing smaller to the right: the interval ends with the table
        lcp = np.full(n, 7, dtype=np.uint32)
        lcp[0] = 0
        lcp[1:] += (np.arange(n - 1) % 3 == 0).astype(np.uint32)
        _check(hip, lcp, what="open to the right, n = %d" % n)


def test_documents_at_tile_seams(hip, geometry):
    """Two and five documents whose first ranks lie on, just before and just after a tile seam: the zero at a document's
    first rank bounds the searches of both neighbours and carries n_d - m_d."""
    tile, halo, near = geometry
    rng = np.random.default_rng(6)
    n = 3 * tile + 5
    for off in (-1, 0, 1):
        for starts in ([tile + off], [2 * tile + off], [16, tile + off, tile + off + 1, 2 * tile + off]):
            doc_off = [0] + starts + [n]
            for kind in ("geometric", "deep geometric", "walk"):
                lcp = _random_table(rng, n, kind)
                lcp[lcp == 0] = 1
                lcp[doc_off[:-1]] = 0
                m = [int(rng.integers(1, 5)) for _ in starts] + [1]
                _check(hip, lcp, doc_off, m, what="%s, documents at %s" % (kind, starts))
            # no other small value: every search runs to the document's ends
            lcp = rng.integers(3, 6, size=n).astype(np.uint32)
            lcp[doc_off[:-1]] = 0
            _check(hip, lcp, doc_off, [1] * (len(doc_off) - 1), what="flat documents at %s" % starts)


def test_ramps(hip, geometry):
    """Strictly ascending (the one-letter text: every NSV is the table's end, every rank of all but the last window is
    listed) and strictly descending (every PSV is rank 0)."""
    tile, halo, near = geometry
    n = 3 * tile + 5
    up = np.arange(n, dtype=np.uint32)
    assert _check(hip, up, what="ascending", inside=False) >= 2 * tile - halo - 8
    down = np.concatenate([[0], np.arange(n - 1, 0, -1)]).astype(np.uint32)
    assert _check(hip, down, what="descending", inside=False) >= 2 * tile - halo - 8


def test_tables_that_are_no_lcp_tables(hip, geometry):
    """What a speculative build can hand the pass after a wrong alphabet guess: arbitrary values, 0xFFFFFFFF among them,
    and no zero but the first entry.  The call returns and the result is the model's."""
    tile, halo, near = geometry
    rng = np.random.default_rng(8)
    for n in (17, tile + 1, 3 * tile + 5):
        for hi in (2, 5, 1 << 32):
            lcp = rng.integers(1, hi, size=n, dtype=np.uint64).astype(np.uint32)
            lcp[rng.integers(1, n, size=max(1, n // 50))] = 0xFFFFFFFF
            lcp[0] = 0
            _check(hip, lcp, what="values below %d, n = %d" % (hi, n))
        lcp = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        lcp[0] = 0
        _check(hip, lcp, what="all ones, n = %d" % n)
