"""CPU tier: pin the witness of tests/test_gpu_dc3.py (tests/dc3_exact.py) to brute force on small strings -- suffixes
sorted by slicing, names as the dense ranks of sliced triples, the LCP table symbol by symbol -- and show, by the witness
and the model alone, that every generated case reaches what it claims to reach."""
import numpy as np
import pytest

import dc3_exact as D
import lcp_exact as L


def _random_small(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 61))
    sigma = int(rng.choice([1, 2, 3, 5, 26]))
    return rng.integers(1, sigma + 1, size=n), sigma


def _dense_ranks(rows):
    order = sorted(set(rows))
    rank = {r: i + 1 for i, r in enumerate(order)}
    return [rank[r] for r in rows]


def _sliced_names(s):
    """The names of the sample triples, in the order of the name string: mod-1 samples (the dummy at n among them when
    n mod 3 == 1), then mod-2 samples; a triple is a slice of the string with its three zero pads."""
    s = [int(x) for x in s]
    n = len(s)
    pad = s + [0, 0, 0]
    n0, n2 = (n + 2) // 3, n // 3
    pos = [3 * t + 1 for t in range(n0)] + [3 * t + 2 for t in range(n2)]
    return _dense_ranks([tuple(pad[p:p + 3]) for p in pos])


def test_suffix_array_and_names_against_slicing_form_0():
    for seed in range(300):
        s, sigma = _random_small(seed)
        lst = s.tolist()
        brute = sorted(range(len(lst)), key=lambda i: lst[i:])
        case = D.Case("small", 0, symbols=s, sigma=sigma)
        assert case.sa().tolist() == brute, lst
        cur = s
        for v in case.model():
            assert (v.n0, v.n1, v.n2) == ((v.n + 2) // 3, (v.n + 1) // 3, v.n // 3) and v.n02 == v.n0 + v.n2
            names = _sliced_names(cur)
            assert v.s12.tolist() == names and v.n_names == max(names), (lst, cur)
            assert v.max_group == max(names.count(x) for x in set(names))
            cur = v.s12
        assert case.model()[-1].branch in ("unique", "resolved")


def test_suffix_array_and_names_against_slicing_forms_1_and_2():
    """Terminators are symbols of their own, ascending with position: the plain slices of the u32 codes order the suffixes,
    and the dense ranks of the sliced triples are the names the terminator rule gives (a triple that holds a terminator is
    unique, and what follows the terminator cannot matter)."""
    for seed in range(200):
        rng = np.random.default_rng(5000 + seed)
        n = int(rng.integers(1, 61))
        sigma = int(rng.choice([1, 2, 3, 26, 254, 300]))
        t = D.cut_text("small", n, np.arange(1, sigma + 1), seed)
        assert t.n == n and t.codes[-1] >= t.term_first
        codes = t.codes.tolist()
        brute = sorted(range(n), key=lambda i: codes[i:])
        for form in ((1, 2) if sigma <= 254 else (1,)):
            case = D.Case("small", form, text=t)
            assert case.sa().tolist() == brute
            assert case.sigma == t.term_first - 1 + int(np.count_nonzero(t.codes >= t.term_first))
        m = D.Case("small", 1, text=t).model()
        assert m[0].s12.tolist() == _sliced_names(codes)
        cur = m[0].s12
        for v in m[1:]:
            assert v.s12.tolist() == _sliced_names(cur)
            cur = v.s12
        # the byte stream and its exact table, symbol by symbol
        if sigma <= 254:
            s8 = t.stream(1).tolist()
            assert all((b == 0xFF) == (c >= t.term_first) and (b == 0xFF or b == c) for b, c in zip(s8, codes))
            exact = t.exact(1)
            for r in range(1, n):
                p, q, h = brute[r], brute[r - 1], 0
                while max(p, q) + h < n and s8[p + h] == s8[q + h] and s8[p + h] != 0xFF:
                    h += 1
                assert exact[r] == h
            assert exact[0] == 0


def test_the_resolve_model_against_a_restatement_of_the_kernel():
    """dc3_resolve_ties_kernel thread by thread on small name strings, at a small geometry: the model's verdict (group size,
    longest run of shared names) is the kernel's."""
    geo = (16, 3, 4) + D.GEOMETRY[3:]
    seen = set()
    for seed in range(400):
        rng = np.random.default_rng(9000 + seed)
        n = int(rng.integers(12, 90))
        s = rng.integers(1, 3, size=n) if seed % 2 else np.resize(rng.integers(1, 4, size=int(rng.integers(1, 7))), n)
        if seed % 3 == 0:
            s = np.concatenate([rng.integers(1, 40, size=n), s[:20]])
        v = D.level(s, int(s.max()), geo=geo)
        if v.branch not in ("resolved", "failed"):
            continue
        order = np.lexsort((np.arange(v.n02), v.triples[:, 2], v.triples[:, 1], v.triples[:, 0]))
        names = v.s12[order].tolist()
        s12 = v.s12.tolist() + [0, 0, 0]
        fail = False
        for i, t in enumerate(order.tolist()):
            a, b = i, i + 1
            while a > 0 and names[a - 1] == names[i] and i - a <= geo[1]:
                a -= 1
            while b < v.n02 and names[b] == names[i] and b - i <= geo[1]:
                b += 1
            if b - a == 1:
                continue
            if b - a > geo[1]:
                fail = True
                continue
            for x in range(a, b):
                if x == i:
                    continue
                t2, h = int(order[x]), 1
                while True:
                    c1, c2 = s12[t + h], s12[t2 + h]
                    h += 1
                    if not (c1 == c2 and h <= geo[2]):
                        break
                fail |= c1 == c2
        assert fail == (v.branch == "failed"), s.tolist()
        seen.add((v.branch, v.max_group > geo[1], v.longest > geo[2]))
    assert {("resolved", False, False), ("failed", True, False), ("failed", False, True)} <= seen


def test_key_paths():
    assert [D.key_path(s) for s in (1, 1023, 1024, (1 << 21) - 1, 1 << 21, 1 << 22)] == ["u32", "u32", "u64", "u64", "two-stage", "two-stage"]


def test_the_merge_looks_at_its_caps_at_the_cut_points_of_the_byte_pass():
    """dc3_window_lcp hands a comparison that is equal over its window of 8 to lcp_bytes_capped at 8: two steps of 8, then
    strides of 32 -- the lengths at which lcp8_kernel's comparisons look at their caps, so lcp_exact.cut_point(cap, 1) is
    where the merge cuts."""
    looks = D.merge_looks(40000)
    assert looks[0] == L.BYTE_FIRST and set(np.diff(looks)) == {L.STEP[1]}
    for cap in list(range(24, 600)) + [D.GEOMETRY[3], D.GEOMETRY[4], D.GEOMETRY[4] + 1]:
        assert next(h for h in looks if h >= cap) == L.cut_point(cap, 1)
    assert D.lcp_geometry() == L.GEOMETRY


def test_merge_profile_on_a_small_tile():
    geo = (4,) + D.GEOMETRY[1:]
    sa = np.array([0, 3, 6, 1, 2, 4, 5, 7, 9, 8])
    prof = D.merge_profile(sa, geo)
    assert prof["tiles"] == 3 and prof["splits"] == [0, 1, 5, 6] and prof["b_only"] == 0 and prof["a_only"] == 1
    assert prof["first_a"] == 3 and prof["first_b"] == 0 and prof["switches"] == 3


CASES = D.all_cases()


def test_every_case_is_named_once_and_carries_a_claim():
    names = [c.what for c in CASES]
    assert len(set(names)) == len(names)
    assert all(c.claims for c in CASES)
    # every family of the gpu test is in the list the claims are checked on
    listed = set(names)
    for extra in D.scatter_cases():
        assert extra.what in listed
    assert {c.form for c in CASES} == {0, 1, 2}


@pytest.mark.parametrize("family", ["size", "keys", "term", "group", "length", "share", "all_same", "fibonacci", "period", "merge", "scatter",
                                    "lcp"])
def test_every_case_reaches_what_it_claims(family):
    mine = [c for c in CASES if c.what.startswith(family)]
    assert mine
    for c in mine:
        D.check_claims(c)


def test_no_case_is_outside_the_families_above():
    families = ("size", "keys", "term", "group", "length", "share", "all_same", "fibonacci", "period", "merge", "scatter", "lcp")
    assert all(c.what.startswith(families) for c in CASES)


def test_the_aimed_cases_straddle_their_bounds():
    by = {c.what: c for c in CASES}
    G, M = D.MAX_GROUP, D.MAX_LEN
    assert [by["group_%d" % k].model()[0].branch for k in (G - 1, G, G + 1)] == ["resolved", "resolved", "failed"]
    ok, bad = by["length_%d_0" % D.LENGTH_OK].model()[0], by["length_%d_0" % D.LENGTH_FAIL].model()[0]
    assert D.LENGTH_FAIL == D.LENGTH_OK + 1 and (ok.longest, bad.longest) == (M, M + 1) and (ok.branch, bad.branch) == ("resolved", "failed")
    assert ok.max_group <= G and bad.max_group <= G and bad.ties <= bad.n02 // 8        # (the length alone fails it)
    a, b = by["share_500"].model()[0], by["share_501"].model()[0]
    assert a.n02 == b.n02 and a.ties == a.n02 // 8 and b.ties == a.ties + 1 and (a.branch, b.branch) == ("resolved", "recurse")
    tops = [by["scatter_%d" % n].model()[0].rank_top for n in range(379, 386)]
    assert tops == sorted(tops) and set(tops) == {8, 9}
    deep = [x.rank_top for x in by["all_same"].model()]
    assert deep == sorted(deep, reverse=True) and deep[0] > 8 and deep[-1] <= 8         # (levels on both sides of the switch)
    paths = {by["keys_%d" % s].model()[0].keys for s in (1023, 1024, (1 << 21) - 1, 1 << 21, 1 << 22)}
    assert paths == {"u32", "u64", "two-stage"}
    assert {by["term_%d" % tf].model()[0].keys for tf in (1023, 1024)} == {"u32", "u64"}
