"""gpu tier: the child tables and the lcp-interval lefts on hand-made tables (csrc/tables.h: child_stream_kernel,
child_wide_kernel, interval_left_kernel; csrc/build.h: child_tables, interval_lefts).

Everything goes through east_hip_debug_child_tables, which uploads a caller's table and runs annotate(), then the two
functions the read-back entry points call.  The witness is tests/child_exact.py (pinned to the oracle by
tests/test_child_exact_host.py): every check compares the four arrays in full and the number of ranks that went through
child_wide_kernel with the model's count of ranks on the pyramid path, exactly.

The tile, the halo and the two reaches come from the library (geometry_out), never from constants here.  The table
families below are functions of that geometry; each case carries a premise -- what the table was built to contain,
asserted of the model alone -- which tests/test_child_exact_host.py also runs at the default geometry, so that a
generator that drifts fails without a GPU.
"""
import ctypes

import numpy as np
import pytest

from child_exact import LANES, NONE, PYRAMID, REGISTERS, Child

pytestmark = pytest.mark.gpu

_u32p, _i64p, _i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
ERR_INVALID = -2


# ---- the table families (no GPU needed) -------------------------------------------------------------------------------
class Case(object):
    def __init__(self, what, lcp, doc_off=None, n_strings=None, premise=None):
        self.what = what
        self.lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
        n = int(self.lcp.size)
        self.doc_off = [0, n] if doc_off is None else [int(o) for o in doc_off]
        self.n_strings = [1] * (len(self.doc_off) - 1) if n_strings is None else [int(m) for m in n_strings]
        self.premise = premise

    def model(self, near, local):
        """The model of the case's table, with the case's premise asserted."""
        m = Child(self.lcp, self.doc_off, self.n_strings)
        if self.premise is not None:
            self.premise(m, near, local)
        return m


def distances(geo):
    tile, halo, near, local = geo
    return [1, 2, near - 1, near, near + 1, local - 1, local, local + 1, halo + 1, tile - 1, tile, tile + 1, 2 * tile + 3]


def positions(tile):
    """0, 1, 15, 16, tile - 1 mod tile in the first, a middle and the last full tile of a table of 3 tiles + 5."""
    return [t * tile + r for t in (0, 1, 2) for r in (0, 1, 15, 16, tile - 1)]


def _tier(d, near, local):
    return REGISTERS if d <= near else LANES if d <= local else PYRAMID


def distance_cases(geo, tile_index, equal):
    """A rank whose PSE lies d_left before it and whose NSE lies d_right behind it -- smaller than the rank's value or
    (equal) the same --, fillers above the value everywhere else.  Where the table has no room the neighbour is the
    table's first entry to the left and the table's end to the right.  Rank 0 searches to the right only, for a zero."""
    tile, halo, near, local = geo
    rng = np.random.default_rng(100 + 2 * tile_index + equal)
    dist, n, v = distances(geo), 3 * tile + 5, 5
    for i, at in enumerate(positions(tile)):
        if at // tile != tile_index:
            continue
        for j, d_left in enumerate(dist):
            d_right = dist[(i + j) % len(dist)]
            lcp = rng.integers(v + 1, v + 4, size=n).astype(np.uint32)
            lcp[0] = 0
            if at == 0:
                if d_right < n:
                    lcp[d_right] = 0
                want = (0, min(d_right, n))
            else:
                lcp[at] = v
                if at - d_left >= 1:
                    lcp[at - d_left] = v if equal else v - 1
                if at + d_right < n:
                    lcp[at + d_right] = v if equal else v - 1
                want = (min(d_left, at), min(d_right, n - at))

            def premise(m, near, local, at=at, want=want, d_left=d_left, d_right=d_right):
                assert m.reach(at) == want, (at, m.reach(at), want)
                assert m.path(at, near, local) == _tier(max(want), near, local)
                if at + d_right < n and (equal or at == 0):
                    assert m.next[at] == at + d_right
                if at - d_left >= 1:
                    assert (m.ann[at] == 0) == bool(equal)        # (a later l-index / a first one)
                    assert (m.left[at] == NONE) == bool(equal)
            yield Case("at %d, PSE %d before, NSE %d behind, %s" % (at, d_left, d_right, "equal" if equal else "smaller"),
                       lcp, premise=premise)


def _tie_candidates(lo, hi, k, near, local):
    """Where the copies of the minimum go in [lo, hi]: next to both ends, at the reaches' edges as seen from k, and at the
    first and last positions = 0 and 15 mod 16, = 0 and 255 mod 256.  An interval the registers hold: everywhere."""
    if hi - lo <= near:
        return list(range(lo, hi + 1))
    c = {lo, hi}
    for d in (near, near + 1, local, local + 1):
        c.update(x for x in (k - d, k + d) if lo <= x <= hi)
    for mod, res in ((16, 0), (16, 15), (256, 0), (256, 255)):
        first = lo + (res - lo) % mod
        if first <= hi:
            c.update((first, first + (hi - first) // mod * mod))
    return sorted(c)


def tie_distances(geo):
    tile, halo, near, local = geo
    return [near, near + 1, local, local + 1, 300, 4 * tile + 104]


def tie_cases(geo, side, dist):
    """The open interval between a rank k and its neighbour `dist` away on `side` holds its minimum two or three times:
    the answer is the leftmost copy.  Every pair of neighbouring candidate positions, the outermost pair and three triples."""
    tile, halo, near, local = geo
    rng = np.random.default_rng(200 + dist + (side == "left"))
    big = dist > 2 * tile
    n = (5 if big else 3) * tile + 5
    if side == "left":
        k = 4 * tile + 300 if big else 2 * tile + 7
        lo, hi = k - dist + 1, k - 1
    else:
        k = 203 if big else tile - 3
        lo, hi = k + 1, k + dist - 1
    c = _tie_candidates(lo, hi, k, near, local)
    combos = [c[i:i + 2] for i in range(len(c) - 1)] + [[c[0], c[-1]], c[:3], c[-3:], [c[0], c[len(c) // 2], c[-1]]]
    for combo in sorted(set(tuple(x) for x in combos if len(set(x)) >= 2)):
        lcp = rng.integers(9, 12, size=n).astype(np.uint32)
        lcp[0] = 0
        lcp[lo - 1] = lcp[hi + 1] = 3
        lcp[k] = 5
        lcp[k + 1 if side == "left" else k - 1] = 3
        lcp[list(combo)] = 7

        def premise(m, near, local, combo=combo):
            assert m.reach(k) == ((dist, 1) if side == "left" else (1, dist))
            assert m.path(k, near, local) == _tier(dist, near, local)
            assert (m.up[k] if side == "left" else m.down[k]) == combo[0]
            assert sum(int(x) == 7 for x in m.v[lo:hi + 1]) == len(set(combo)) >= 2
        yield Case("minimum of the %d ranks to the %s of %d at %s" % (dist - 1, side, k, combo), lcp, premise=premise)


def random_table(rng, n, kind):
    if kind == "geometric":                     # (many zeros)
        lcp = (rng.geometric(0.3, size=n) - 1).astype(np.uint32)
    elif kind == "deep geometric":
        lcp = rng.geometric(0.02, size=n).astype(np.uint32)
    else:
        lcp = np.abs(np.cumsum(rng.integers(-3, 4, size=n))).astype(np.uint32)
    lcp[0] = 0
    return lcp


KINDS = ("geometric", "deep geometric", "walk")


def sizes(geo):
    tile = geo[0]
    return [1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, tile - 1, tile, tile + 1, tile + 3, 4095, 4096, 4097]


def size_cases(geo, n):
    """The end of the table inside a quad, a group, a tile; tables without a level 1 or 2; interior zeros left in."""
    rng = np.random.default_rng(300 + n)
    for kind in KINDS:
        yield Case("%s, n = %d" % (kind, n), random_table(rng, n, kind), n_strings=[int(rng.integers(1, 4))])

    def ascending(m, near, local):
        assert all(m.nse[k] == n for k in range(1, n)) and not any(m.down) and not any(m.next) and not any(m.up)
        assert m.paths(near, local)[PYRAMID] == max(0, n - local)
    yield Case("ascending, n = %d" % n, np.arange(n), premise=ascending)

    def descending(m, near, local):
        assert all(m.pse[k] == 0 and m.up[k] == k - 1 for k in range(2, n))
        assert m.paths(near, local)[PYRAMID] == max(0, n - local)
    yield Case("descending, n = %d" % n, np.concatenate([[0], np.arange(n - 1, 0, -1)]), premise=descending)

    def flat(m, near, local):
        assert m.next[1:] == list(range(2, n)) + [0] * (n > 1) and not any(m.up) and not any(m.down[1:])
    yield Case("all equal behind the first, n = %d" % n, np.concatenate([[0], np.full(n - 1, 7)]), premise=flat)


def chain_cases(geo):
    """One value every 7th, (local + 1)th, (tile + local + 1)th rank, larger ones in between."""
    tile, halo, near, local = geo
    rng = np.random.default_rng(4)
    n = 3 * tile + 5
    for step in (7, local + 1, tile + local + 1):
        lcp = rng.integers(6, 9, size=n).astype(np.uint32)
        lcp[0] = 0
        lcp[1::step] = 5

        def premise(m, near, local, step=step):
            assert all(m.next[k] == k + step for k in range(1, n - step, step))
            assert (m.paths(near, local)[PYRAMID] > n // step // 2) == (step > local)
        yield Case("chain of step %d" % step, lcp, premise=premise)


def document_cases(geo):
    """First ranks on, one before and one after a tile seam and at every offset of a thread's quad; one-rank documents, a
    run of eight across a seam, at the table's ends; flat documents, whose searches all run to the document's ends.
    n_strings = 1 and more: n_d - m_d > 0 stands at the first rank of every document of several ranks."""
    tile, halo, near, local = geo
    rng = np.random.default_rng(6)
    n = 3 * tile + 5
    layouts = []
    for off in (-1, 0, 1):
        layouts += [[tile + off], [2 * tile + off], [21 + off, tile + off, tile + off + 1, 2 * tile + off]]
    layouts += [[tile + 40 + o, 2 * tile + 12 + o] for o in range(4)]
    layouts += [list(range(tile - 4, tile + 5)), [1, 2, tile, n - 1]]
    for starts in layouts:
        doc_off = [0] + starts + [n]
        lens = np.diff(doc_off)
        m = [int(rng.integers(1, min(4, ln) + 1)) if ln > 1 else 1 for ln in lens]

        def premise(mod, near, local, doc_off=doc_off, m=m):
            # (that left is none at these ranks is asserted by the model itself)
            assert all(mod.ann[s] == e - s - ms for s, e, ms in zip(doc_off[:-1], doc_off[1:], m)) and max(mod.ann[s] for s in doc_off[:-1]) > 0
        for kind in KINDS:
            lcp = random_table(rng, n, kind)
            lcp[doc_off[:-1]] = 0
            yield Case("%s, documents at %s" % (kind, starts), lcp, doc_off, m, premise)
        lcp = rng.integers(3, 6, size=n).astype(np.uint32)
        lcp[doc_off[:-1]] = 0

        def flat(mod, near, local, doc_off=doc_off, premise=premise):
            premise(mod, near, local)
            # the first rank of a long document searches its whole length to the right, and finds nothing
            for s, e in zip(doc_off[:-1], doc_off[1:]):
                assert mod.nse[s] == e and mod.next[s] == 0 and mod.down[s] == 0
        yield Case("flat documents at %s" % starts, lcp, doc_off, m, flat)


def local_cases(geo):
    """Tables whose answers all lie within `local`: nothing may be listed."""
    tile, halo, near, local = geo
    n = 3 * tile + 5

    def premise(m, near, local):
        count = m.paths(near, local)
        assert count[PYRAMID] == 0 and count[LANES] > n // local and count[REGISTERS] > 0, count
    for period in (near + 1, local // 2, local - 1, local):
        saw = np.arange(n) % period
        yield Case("sawtooth of period %d" % period, saw, premise=premise)
        yield Case("falling sawtooth of period %d" % period, np.where(saw == 0, 0, period - saw), premise=premise)
    # ... with documents: the same period, first ranks wherever a zero stands at the seams
    saw = np.arange(n) % local
    starts = [s for s in range(local, n, local) if s % tile < local or s % tile >= tile - local]
    yield Case("sawtooth of period %d in %d documents" % (local, len(starts) + 1), saw, [0] + starts + [n], premise=premise)


def families(geo):
    """{name: cases}: every table the gpu tier runs but the live build's."""
    fam = {}
    for t in (0, 1, 2):
        for equal in (0, 1):
            fam["distances-%d-%s" % (t, "equal" if equal else "smaller")] = lambda t=t, equal=equal: distance_cases(geo, t, equal)
    for side in ("left", "right"):
        for i, dist in enumerate(tie_distances(geo)):
            fam["ties-%s-%d" % (side, i)] = lambda side=side, dist=dist: tie_cases(geo, side, dist)
    for i, n in enumerate(sizes(geo)):
        fam["size-%d" % i] = lambda n=n: size_cases(geo, n)
    fam["chains"] = lambda: chain_cases(geo)
    fam["documents"] = lambda: document_cases(geo)
    fam["local"] = lambda: local_cases(geo)
    return fam


# ---- the device side ---------------------------------------------------------------------------------------------------
def _child_tables(hip, lcp, doc_off, n_strings, expect=0):
    """(up, down, next, left, (tile, halo, near, local), listed) of the device's passes over `lcp`."""
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    n = int(lcp.size)
    doc_off = np.array(doc_off, dtype=np.int64)
    n_strings = np.array(n_strings, dtype=np.int32)
    out = [np.full(n, 0xDEADBEEF, dtype=np.uint32) for _ in range(4)]
    geo = np.zeros(4, dtype=np.uint32)
    listed = np.full(1, 0xDEADBEEF, dtype=np.uint32)
    rc = hip.load().east_hip_debug_child_tables(0, lcp.ctypes.data_as(_u32p), n, doc_off.ctypes.data_as(_i64p), doc_off.size - 1,
                                                n_strings.ctypes.data_as(_i32p), *[a.ctypes.data_as(_u32p) for a in out],
                                                geo.ctypes.data_as(_u32p), listed.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    return out + [tuple(int(x) for x in geo), int(listed[0])]


@pytest.fixture(scope="module")
def geometry(hip):
    geo = _child_tables(hip, np.zeros(1, dtype=np.uint32), [0, 1], [1])[4]
    tile, halo, near, local = geo
    assert tile % 16 == 0 and halo % 4 == 0 and near % 4 == 0 and 0 < near < local <= halo < 256 < tile
    return geo


def _check(hip, geometry, case):
    tile, halo, near, local = geometry
    m = case.model(near, local)
    up, down, nxt, left, geo, listed = _child_tables(hip, case.lcp, case.doc_off, case.n_strings)
    assert geo == geometry
    for name, got, want in (("up", up, m.up), ("down", down, m.down), ("next", nxt, m.next), ("left", left, m.left)):
        want = np.array(want, dtype=np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (case.what, name, m.n, "first differing ranks", bad[:8], got[bad[:8]], want[bad[:8]],
                               [m.reach(int(k)) for k in bad[:8]])
    assert listed == m.paths(near, local)[PYRAMID], (case.what, m.n, listed, m.paths(near, local))


def _run(hip, geometry, name):
    n = 0
    for case in families(geometry)[name]():
        _check(hip, geometry, case)
        n += 1
    assert n > 0, name


@pytest.mark.parametrize("equal", ["smaller", "equal"])
@pytest.mark.parametrize("tile_index", [0, 1, 2])
def test_distances_to_both_sides(hip, geometry, tile_index, equal):
    """Every distance at which the search changes tier (registers, eight lanes, the pyramid; the halo's end, the next
    tile, past it) to either side of a rank at every position class; every distance meets every position on either side,
    so one side is far and the other near as often as both are."""
    _run(hip, geometry, "distances-%d-%s" % (tile_index, equal))


@pytest.mark.parametrize("tier", range(6))
@pytest.mark.parametrize("side", ["left", "right"])
def test_leftmost_minimum_under_ties(hip, geometry, side, tier):
    """up[] and down[] where the minimum stands two or three times: in the register scan (<= against <), in the eight
    lanes' 64-bit words (~dist against dist) and in pyr_leftmost_argmin, whose head, aligned middle and tail each hold the
    winner once and a losing copy once (tiers: an interval within near, just beyond, within local, just beyond, wider
    than a group of 256, wider than a group of 4 096)."""
    _run(hip, geometry, "ties-%s-%d" % (side, tier))


@pytest.mark.parametrize("i", range(18))
def test_sizes_and_ends(hip, geometry, i):
    """Three random kinds, the ascending and the descending ramp and the flat table at every size at which the tail of the
    table, the vector store or the pyramid's depth changes."""
    _run(hip, geometry, "size-%d" % i)


def test_equal_value_chains(hip, geometry):
    _run(hip, geometry, "chains")


def test_documents(hip, geometry):
    _run(hip, geometry, "documents")


def test_answers_within_local_list_nothing(hip, geometry):
    _run(hip, geometry, "local")


def test_the_live_path(hip, geometry):
    """A built handle's tables() and lcp_interval_lefts() against the debug entry on that handle's own lcptab: what the
    read-back entry points launch is what the tests above check."""
    tile, halo, near, local = geometry
    rng = np.random.default_rng(9)
    n, cut = 3 * tile + 5, tile + 1
    sym = rng.integers(65, 67, size=n).astype(np.uint32)
    sym[cut - 1] = sym[n - 1] = 0x0A00
    index = hip.HipIndex(device=0)
    try:
        index.build(sym, [0, cut, n], [1, 1])
        t = [index.tables(d) for d in (0, 1)]
        lefts = np.concatenate([index.lcp_interval_lefts(d) for d in (0, 1)])
    finally:
        index.close()
    lcp = np.concatenate([x["lcptab"] for x in t]).astype(np.uint32)
    up, down, nxt, left, _, _ = _child_tables(hip, lcp, [0, cut, n], [1, 1])
    for name, got in (("childtab_up", up), ("childtab_down", down), ("childtab_next_l_index", nxt)):
        assert np.array_equal(np.concatenate([x[name] for x in t]), got.astype(np.int64)), name
    assert np.array_equal(lefts, left.astype(np.int32).astype(np.int64))
    assert (lefts >= 0).sum() > n // 8 and np.count_nonzero(up) > n // 8


def test_rejections(hip, geometry):
    """Before any launch: a table that does not hold 0 at a document's first rank, offsets that do not increase, a value
    no LCP table holds."""
    lcp = np.array([0, 3, 1, 2, 0, 1], dtype=np.uint32)
    _child_tables(hip, lcp, [0, 4, 6], [1, 1])
    _child_tables(hip, lcp, [0, 3, 6], [1, 1], expect=ERR_INVALID)
    _child_tables(hip, lcp, [0, 4, 4, 6], [1, 1, 1], expect=ERR_INVALID)
    _child_tables(hip, lcp, [0, 5, 4, 6], [1, 1, 1], expect=ERR_INVALID)
    _child_tables(hip, np.array([1, 3], dtype=np.uint32), [0, 2], [1], expect=ERR_INVALID)
    _child_tables(hip, np.array([0, 0x7FFFFFF0], dtype=np.uint32), [0, 2], [1], expect=ERR_INVALID)
    _child_tables(hip, np.array([0, 0x7FFFFFEF], dtype=np.uint32), [0, 2], [1])
