"""CPU tier: the linear-time checkers of oracle/easa_linear.c pinned to the faithful oracle.

The gpu tier checks large and deep builds in full with `check_tables()` and `score_table_fast()` (the reference's
annotation pass is quadratic on deep trees).  Here they must accept exactly what the faithful port (itself pinned to the
reference's own tables) builds -- every check compares every entry, so acceptance is equality -- on the golden fixtures,
the reference's fuzz collections and deep trees the faithful port still builds in seconds, and they must reject every
single corruption of those tables."""
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

TABLES = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")


def _psv_lefts(lcp, ann):
    """left[k] = the previous rank with a smaller lcp value, at the first l-indices k > 0 (ann[k] > 0), -1 elsewhere --
    what east_hip_get_lcp_intervals returns (a plain stack of previous smaller values)."""
    left = np.full(len(lcp), -1, dtype=np.int64)
    stack = []
    for k, v in enumerate(lcp.tolist()):
        while stack and lcp[stack[-1]] >= v:
            stack.pop()
        if k > 0 and ann[k] > 0:
            left[k] = stack[-1]
        stack.append(k)
    return left


def _faithful(oracle, sym, m):
    o = oracle.OracleEASA(symbols=sym, n_strings=m)
    t = {name: getattr(o, name) for name in TABLES}
    t["left"] = _psv_lefts(o.lcptab, o.anntab)
    return t


def _concat(parts):
    """[(symbols, n_strings, tables)] -> one multi-document input of check_tables."""
    sym = np.concatenate([p[0] for p in parts])
    off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)
    ms = np.array([p[1] for p in parts], dtype=np.int64)
    tables = {name: np.concatenate([p[2][name] for p in parts]) for name in parts[0][2]}
    return sym, off, ms, tables


def _fibonacci(n):
    a, b = np.array([65], np.uint32), np.array([65, 66], np.uint32)
    while b.size < n:
        a, b = b, np.concatenate([b, a])
    return b[:n]


def _one_string(body):
    return np.concatenate([body, [0x0A00]]).astype(np.uint32), 1


def _deep_inputs():
    """Deep suffix trees the faithful port builds in well under a second each."""
    from east import synthetic
    rng = np.random.default_rng(2024)
    passage = rng.integers(65, 91, size=700, dtype=np.uint32)
    out = {
        "one_letter": _one_string(np.full(20000, 65, np.uint32)),
        "period3": _one_string(np.resize(np.array([65, 66, 67], np.uint32), 20000)),
        "fibonacci": _one_string(_fibonacci(20000)),
        "worst_case_1e3": synthetic.worst_case_collection(rng, 100, 1000),
        "worst_case_1e4": synthetic.worst_case_collection(rng, 100, 10000),
        "passage_x16": _one_string(np.tile(passage, 16)),
    }
    strings = np.tile(passage, 16).reshape(4, -1)                     # the same 16 copies as four strings
    out["passage_x16_four_strings"] = (np.concatenate(
        [np.concatenate([s, [0x0A00 + i]]) for i, s in enumerate(strings)]).astype(np.uint32), 4)
    return out


@pytest.fixture(scope="module")
def deep(oracle):
    return {name: (sym, m, _faithful(oracle, sym, m)) for name, (sym, m) in _deep_inputs().items()}


def _golden_collections():
    from east import utils
    out = [load_golden("readme_example.json")["strings"], load_golden("test_base_case.json")["strings"]]
    out += [c["strings"] for c in load_golden("fuzz_small.json")["cases"]]
    out += [c["strings"] for c in load_golden("traversal_synonyms.json")["traversals"]]
    for fixture in ("sample_table.json", "hse_config1.json", "zipf_docs.json", "prose_like_docs.json"):
        out += [utils.text_to_strings_collection(t.encode("utf-8")) for t in load_golden(fixture)["texts"].values()]
    return [sc for sc in out if sc]


def test_checkers_accept_the_golden_fixtures(oracle):
    parts = []
    for sc in _golden_collections():
        sym = oracle.make_symbols(sc)
        parts.append((sym, len(sc), _faithful(oracle, sym, len(sc))))
        oracle.check_tables(sym, [0, sym.size], [len(sc)], parts[-1][2])       # one document ...
    assert len(parts) >= 70
    oracle.check_tables(*_concat(parts))                             # ... and all of them in one call


def test_checkers_accept_the_reference_tables_of_the_fuzz_collections(oracle):
    """reference_fuzz.json.gz holds the reference's own tables for 595 collections: every table and the scores, through
    the multi-document form and the batched walk."""
    with gzip.open(os.path.join(GOLDEN, "reference_fuzz.json.gz"), "rt", encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 595
    parts = []
    for case in cases:
        sym = np.array(case["string"], dtype=np.uint32)
        t = {name: np.array(case[name], dtype=np.int64) for name in TABLES}
        t["left"] = _psv_lefts(t["lcptab"], t["anntab"])
        parts.append((sym, len(case["strings"]), t))
        queries = [q["query"].replace(" ", "") for q in case["queries"]]
        queries = [q for q in queries if q]
        if not queries:
            continue
        qs = np.concatenate([oracle.query_symbols(q) for q in queries])
        qo = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
        recs = [q for q in case["queries"] if q["query"].replace(" ", "")]
        for i, norm in enumerate((True, False)):
            table, suf = oracle.score_table_fast(sym, [0, sym.size], [len(case["strings"])], t["suftab"], qs, qo,
                                                 norm, want_suffix=True)
            assert table[:, 0].tolist() == [q["score"][i] for q in recs], case["strings"]
            assert suf[0].tolist() == [v for q in recs for v in q["suffix"][i]], case["strings"]
    oracle.check_tables(*_concat(parts))


@pytest.mark.parametrize("name", list(_deep_inputs()))
def test_checkers_accept_deep_trees(oracle, deep, name):
    sym, m, t = deep[name]
    oracle.check_tables(sym, [0, sym.size], [m], t)
    assert int(t["lcptab"].max()) >= 996


def test_deep_trees_in_one_multi_document_call(oracle, deep):
    oracle.check_tables(*_concat(list(deep.values())))


def test_suffix_array_check_on_a_million_random_symbols(oracle):
    rng = np.random.default_rng(6)
    sym = rng.integers(65, 69, size=1 << 20).astype(np.uint32)
    sym[-1] = 0x0A00
    o = oracle.OracleEASA(symbols=sym, n_strings=1, tables=False)
    oracle.check_tables(sym, [0, sym.size], [1], {"suftab": o.suftab, "lcptab": o.lcptab})
    oracle.check_tables(sym, [0, sym.size], [1], {"suftab": o.suftab})


def _rejected(oracle, sym, m, tables, table, rank=None, **kw):
    with pytest.raises(oracle.TableMismatch) as e:
        oracle.check_tables(sym, [0, sym.size], [m], tables)
    assert e.value.table == table, (e.value, kw)
    if rank is not None:
        assert e.value.rank == rank, (e.value, kw)


def _mutated(t, name, fn):
    out = dict(t)
    out[name] = t[name].copy()
    fn(out[name])
    return out


def _first_l_indices(t):
    return np.flatnonzero(t["anntab"][1:] > 0) + 1


@pytest.mark.parametrize("name", ["fibonacci", "worst_case_1e3", "passage_x16_four_strings"])
def test_every_single_corruption_is_rejected(oracle, deep, name):
    sym, m, t = deep[name]
    n = sym.size
    sa, lcp = t["suftab"], t["lcptab"]
    rng = np.random.default_rng(len(name))

    # suffix array: adjacent entries swapped inside a tie group (lcp > 0) and across groups (lcp == 0), three rotated
    for r in (int(rng.choice(np.flatnonzero(lcp > 0))), int(rng.choice(np.flatnonzero(lcp[1:] == 0) + 1)), n - 1):
        def swap(a, r=r):
            a[r - 1], a[r] = a[r], a[r - 1]
        _rejected(oracle, sym, m, _mutated(t, "suftab", swap), "suftab", swap=r)    # (the inverse changes too: any rank)
    for r in (1, n // 2, n - 3):
        _rejected(oracle, sym, m, _mutated(t, "suftab", lambda a, r=r: a.__setitem__(slice(r, r + 3), np.roll(a[r:r + 3], 1))),
                  "suftab", rotate=r)
    _rejected(oracle, sym, m, _mutated(t, "suftab", lambda a: a.__setitem__(5, a[6])), "suftab", 5)     # not a permutation
    _rejected(oracle, sym, m, _mutated(t, "suftab", lambda a: a.__setitem__(9, n)), "suftab", 9)        # out of range

    # lcp: +-1 at one rank, the rank of the maximum among them
    for r in (1, int(np.argmax(lcp)), int(rng.integers(1, n)), n - 1):
        for d in (1, -1):
            if lcp[r] + d >= 0:
                _rejected(oracle, sym, m, _mutated(t, "lcptab", lambda a, r=r, d=d: a.__setitem__(r, a[r] + d)),
                          "lcptab", r, lcp=(r, d))
    _rejected(oracle, sym, m, _mutated(t, "lcptab", lambda a: a.__setitem__(0, 1)), "lcptab", 0)

    # annotation: +-1 at a first l-index, moved to a rank that is not one, changed at ann[0]
    first = _first_l_indices(t)
    others = np.setdiff1d(np.arange(1, n), first)
    for k in (int(first[0]), int(rng.choice(first)), int(first[-1])):
        for d in (1, -1):
            _rejected(oracle, sym, m, _mutated(t, "anntab", lambda a, k=k, d=d: a.__setitem__(k, a[k] + d)), "anntab", k)
        j = int(others[np.searchsorted(others, k) % others.size])

        def move(a, k=k, j=j):
            a[j], a[k] = a[k], 0
        _rejected(oracle, sym, m, _mutated(t, "anntab", move), "anntab", min(j, k), move=(k, j))
    for d in (1, -1):
        _rejected(oracle, sym, m, _mutated(t, "anntab", lambda a, d=d: a.__setitem__(0, a[0] + d)), "anntab", 0)

    # one entry of each child table, one left entry
    for name_t in ("childtab_up", "childtab_down", "childtab_next_l_index", "left"):
        for r in sorted({0, int(rng.integers(1, n)), int(rng.choice(first)), n - 1}):
            for d in (1, -1):
                _rejected(oracle, sym, m, _mutated(t, name_t, lambda a, r=r, d=d: a.__setitem__(r, a[r] + d)), name_t, r)

    # the later tables on an lcp table checked before
    derived = {k: v for k, v in t.items() if k not in ("suftab", "lcptab")}
    oracle.check_tables(sym, [0, n], [m], derived, verified_lcptab=lcp)
    with pytest.raises(oracle.TableMismatch) as e:
        oracle.check_tables(sym, [0, n], [m], _mutated(derived, "childtab_down", lambda a: a.__setitem__(n - 1, 3)),
                            verified_lcptab=lcp)
    assert (e.value.table, e.value.rank) == ("childtab_down", n - 1)

    # a table that only matches after a wrong earlier one is reported under the earlier one
    bad = _mutated(_mutated(t, "lcptab", lambda a: a.__setitem__(n // 2, a[n // 2] + 1)), "anntab",
                   lambda a: a.__setitem__(0, 0))
    _rejected(oracle, sym, m, bad, "lcptab", n // 2)


def test_the_multi_document_form_names_the_first_bad_document(oracle, deep):
    sym, off, ms, t = _concat(list(deep.values()))
    for d in (0, 3, len(ms) - 1):
        r = int(off[d]) + 7
        for name in ("suftab", "lcptab", "anntab", "childtab_down", "left"):
            bad = _mutated(t, name, lambda a, r=r: a.__setitem__(r, a[r] + 1))
            if name == "suftab":
                bad["suftab"][r - 1] += 1
            with pytest.raises(oracle.TableMismatch) as e:
                oracle.check_tables(sym, off, ms, bad)
            assert (e.value.doc, e.value.table) == (d, name), e.value
            if name not in ("suftab", "anntab"):
                assert e.value.rank == 7
    # two bad documents: the lower one is named
    bad = _mutated(t, "childtab_up", lambda a: a.__setitem__(int(off[4]) + 3, -5))
    bad["lcptab"] = bad["lcptab"].copy()
    bad["lcptab"][int(off[2]) + 9] += 1
    with pytest.raises(oracle.TableMismatch) as e:
        oracle.check_tables(sym, off, ms, bad)
    assert (e.value.doc, e.value.table, e.value.rank) == (2, "lcptab", 9)


def test_batched_score_walk_equals_the_single_walk(oracle, deep):
    """score_table_fast over K keyphrases x D documents: every entry and every per-suffix result is easa_score_fast's,
    normalized and -d, and a score one ulp away is told apart."""
    from east import synthetic
    names = list(deep)
    sym, off, ms, t = _concat([deep[k] for k in names])
    rng = np.random.default_rng(5)
    qs, qo = synthetic.keyphrases(rng, sym, 60)
    extra = [np.full(300, 65, np.uint32), np.resize(np.array([65, 66, 67], np.uint32), 70), np.array([90], np.uint32)]
    qs = np.concatenate([qs] + extra)
    qo = np.concatenate([qo, qo[-1] + np.cumsum([e.size for e in extra])])
    K = qo.size - 1
    for norm in (True, False):
        table, suf = oracle.score_table_fast(sym, off, ms, t["suftab"], qs, qo, norm, want_suffix=True)
        assert table.shape == (K, len(names)) and suf.shape == (len(names), qo[-1])
        assert np.array_equal(oracle.score_table_fast(sym, off, ms, t["suftab"], qs, qo, norm), table)
        for d, name in enumerate(names):
            o = oracle.OracleEASA(symbols=deep[name][0], n_strings=deep[name][1], tables=False)
            for k in range(K):
                want, want_suf = o.score_symbols(qs[qo[k]:qo[k + 1]], norm, fast=True, want_suffix=True)
                assert table[k, d] == want and np.array_equal(suf[d, qo[k]:qo[k + 1]], want_suf), (name, k, norm)
        assert (table > 0).any()
        k, d = np.argwhere(table > 0)[len(np.argwhere(table > 0)) // 2]
        moved = table.copy()
        moved[k, d] = np.nextafter(moved[k, d], np.inf)
        assert not np.array_equal(moved, table)
        moved[k, d] = np.nextafter(table[k, d], -np.inf)
        assert not np.array_equal(moved, table)
    with pytest.raises(ZeroDivisionError):
        oracle.score_table_fast(sym, off, ms, t["suftab"], qs[:3], np.array([0, 3, 3]))
