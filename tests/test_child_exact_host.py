"""CPU tier: pin the witness of tests/test_gpu_child_tables.py (tests/child_exact.py) to the oracle, and the gpu file's
table generators to what they were written to contain.

The model must give what oracle.closed_form_tables gives on any single-document table, and what the faithful port of
the reference (OracleEASA) builds -- with the lcp-interval lefts accepted by the linear-time checker -- on the golden
fixtures, on random collections of several documents and on documents of several strings.  Then every table family of
the gpu file is built at the default geometry and its premises are asserted of the model: the gpu tier runs the same
premises at the library's geometry, but a generator that drifts is found here.
"""
import numpy as np
import pytest

from child_exact import LANES, NONE, PYRAMID, REGISTERS, Child
from conftest import load_golden
import test_gpu_child_tables as gpu_file

DEFAULT_GEOMETRY = (1024, 64, 8, 64)            # CH_TILE, CH_HALO, CH_NEAR, CH_LOCAL of csrc/tables.h


def _signed_left(m):
    return np.array([-1 if x == NONE else x for x in m.left], dtype=np.int64)


@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_against_the_closed_forms(oracle, n):
    rng = np.random.default_rng(n)
    for kind in gpu_file.KINDS * (8 if n > 2 else 2):
        lcp = gpu_file.random_table(rng, n, kind)
        m = Child(lcp, [0, n], [1])
        ann, nxt, up, down = oracle.closed_form_tables(lcp)
        ann[0] = n - 1
        assert (m.ann, m.next, m.up, m.down) == (ann.tolist(), nxt.tolist(), up.tolist(), down.tolist()), (kind, lcp[:20])


def _against_the_oracle(oracle, collections):
    """One model over the concatenated tables of `collections` (a document each) against each document's OracleEASA."""
    parts = [oracle.OracleEASA(sc) for sc in collections]
    off = np.concatenate([[0], np.cumsum([o.n for o in parts])]).astype(np.int64)
    ms = [o.m for o in parts]
    lcp = np.concatenate([o.lcptab for o in parts])
    m = Child(lcp, off, ms)
    for name, got in (("anntab", m.ann), ("childtab_up", m.up), ("childtab_down", m.down), ("childtab_next_l_index", m.next)):
        assert got == np.concatenate([getattr(o, name) for o in parts]).tolist(), (name, collections)
    oracle.check_tables(np.concatenate([o.symbols for o in parts]), off, ms,
                        {"left": _signed_left(m), "childtab_up": m.up, "childtab_down": m.down, "childtab_next_l_index": m.next},
                        verified_lcptab=lcp)
    return m


def test_against_the_oracle_on_the_golden_fixtures(oracle):
    cases = [load_golden("readme_example.json"), load_golden("test_base_case.json")] + load_golden("fuzz_small.json")["cases"]
    for case in cases:
        m = _against_the_oracle(oracle, [case["strings"]])
        assert (m.up, m.down, m.next) == (case["childtab_up"], case["childtab_down"], case["childtab_next_l_index"])
    # ... and all of them side by side, as the documents of one shard
    _against_the_oracle(oracle, [case["strings"] for case in cases])


def test_against_the_oracle_on_random_collections(oracle):
    rng = np.random.default_rng(11)
    firsts = 0
    for _ in range(30):
        docs = []
        for _ in range(int(rng.integers(2, 7))):
            n_strings = int(rng.integers(1, 5))
            alphabet = list("AB") if rng.integers(2) else list("ABCD")
            docs.append(["".join(rng.choice(alphabet, size=int(rng.integers(0, 40)))) for _ in range(n_strings)])
        m = _against_the_oracle(oracle, docs)
        firsts += sum(m.ann[s] > 0 for s in m.doc_off[:-1])
    assert firsts > 60                          # (n_d - m_d > 0 at the first ranks, where left must still be none)


def test_the_wrong_left_is_rejected(oracle):
    """(the checker this file leans on does look at `left`)"""
    o = oracle.OracleEASA(["XABXAC", "HI"])
    m = Child(o.lcptab, [0, o.n], [o.m])
    left = _signed_left(m)
    k = int(np.flatnonzero(left >= 0)[0])
    for wrong in (-1, int(left[k]) + 1):
        bad = left.copy()
        bad[k] = wrong
        with pytest.raises(oracle.TableMismatch):
            oracle.check_tables(o.symbols, [0, o.n], [o.m], {"left": bad}, verified_lcptab=o.lcptab)


def test_the_random_kinds_reach_every_path():
    """What the random tables of the gpu file are for: at 3 tiles + 5 every kind sends most ranks through the registers
    and some through the eight lanes, and the two deep kinds hundreds through the lanes and dozens through the pyramid
    (the shallow kind, three zeros in ten ranks, is there for the interior zeros: nothing of it is far)."""
    tile, halo, near, local = DEFAULT_GEOMETRY
    rng = np.random.default_rng(12)
    for kind in gpu_file.KINDS:
        count = Child(gpu_file.random_table(rng, 3 * tile + 5, kind)).paths(near, local)
        assert count[REGISTERS] > 1500 and count[LANES] > 50, (kind, count)
        if kind != "geometric":
            assert count[LANES] > 300 and count[PYRAMID] >= 20, (kind, count)


_FAMILIES = sorted(gpu_file.families(DEFAULT_GEOMETRY))


@pytest.mark.parametrize("name", _FAMILIES)
def test_the_gpu_files_tables_contain_what_they_were_built_for(name):
    tile, halo, near, local = DEFAULT_GEOMETRY
    cases = list(gpu_file.families(DEFAULT_GEOMETRY)[name]())
    assert cases
    seen = set()
    for case in cases:
        assert case.lcp.max() <= 0x7FFFFFEF and all(case.lcp[s] == 0 for s in case.doc_off[:-1]), case.what
        m = case.model(near, local)             # (asserts the case's premise)
        seen.update(m.path(k, near, local) for k in range(m.n))
    # what a family as a whole must reach, from the model alone
    if name.startswith("distances") or name in ("chains", "documents"):
        assert seen == {REGISTERS, LANES, PYRAMID}, (name, seen)
    if name == "local":
        assert seen == {REGISTERS, LANES}


def test_the_distance_tables_put_one_side_far_and_the_other_near():
    tile, halo, near, local = DEFAULT_GEOMETRY
    only_left = only_right = both = 0
    for t in (0, 1, 2):
        for case in gpu_file.distance_cases(DEFAULT_GEOMETRY, t, 0):
            m = Child(case.lcp)
            for k in range(1, m.n):
                dl, dr = m.reach(k)
                only_left += dl > local and dr <= near
                only_right += dr > local and dl <= near
                both += dl > local and dr > local
    assert only_left >= 30 and only_right >= 30 and both >= 30, (only_left, only_right, both)


def test_the_tie_tables_cover_the_three_parts_of_the_pyramid_walk():
    """For the intervals wider than a group of 256: the leftmost copy -- the answer -- stands in the unaligned head, in
    the aligned middle and in the unaligned tail of its interval at least once each, and so does a later, losing copy."""
    tile, halo, near, local = DEFAULT_GEOMETRY
    for side in ("left", "right"):
        for dist in gpu_file.tie_distances(DEFAULT_GEOMETRY)[4:]:
            win, lose = set(), set()
            for case in gpu_file.tie_cases(DEFAULT_GEOMETRY, side, dist):
                copies = np.flatnonzero(case.lcp == 7)
                lo = int(np.flatnonzero(case.lcp[:copies[0]] == 3)[-1]) + 1
                hi = int(copies[-1] + 1 + np.flatnonzero(case.lcp[copies[-1] + 1:] <= 5)[0]) - 1
                head_end, tail_start = (lo + 15) // 16 * 16, (hi + 1) // 16 * 16
                part = lambda x: "head" if x < head_end else "tail" if x >= tail_start else "middle"
                win.add(part(copies[0]))
                lose.update(part(x) for x in copies[1:])
            assert win == lose == {"head", "middle", "tail"}, (side, dist, win, lose)
