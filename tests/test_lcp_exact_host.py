"""CPU tier: pin the witness of tests/test_gpu_lcp_passes.py (tests/lcp_exact.py) to brute force on small texts -- suffixes
sorted by slicing, prefixes compared symbol by symbol, the finishing pass restated step by step at a small geometry --
and show, by the witness alone, that every generated case reaches what it claims to reach."""
import numpy as np
import pytest

import lcp_exact as L

SMALL = (8, 40, 64, 4, 4, 16)          # a geometry at which texts of a few hundred symbols meet every threshold


def _small_texts():
    out = []
    for seed, sigma in enumerate((1, 2, 3, 26, 254, 300)):
        rng = np.random.default_rng(100 + seed)
        docs = []
        for _ in range(int(rng.integers(1, 5))):
            docs.append([rng.integers(1, sigma + 1, size=int(rng.integers(0, 30))) for _ in range(int(rng.integers(1, 4)))])
        out.append(L.Text("small_%d" % sigma, docs))
    out.append(L.Text("identical", [[np.array([1, 2, 1, 2, 1])] * 4, [np.array([], dtype=np.uint32)], [np.full(40, 3)]]))
    out.append(L.pair_ladder("pairs", [7, 8, 9, 23, 24, 25, 41, 57, 90], 12, 5, residues=[(i % 8, (3 * i) % 8) for i in range(9)]))
    out.append(L.run_text("run", 1, 150, 5))
    out.append(L.run_text("period", 3, 151, 5))
    return out


def _brute_sa(t):
    codes = t.codes.tolist()
    sa = []
    for a, b in zip(t.doc_off[:-1], t.doc_off[1:]):
        sa += sorted(range(int(a), int(b)), key=lambda p: codes[p:int(b)])
    return np.array(sa, dtype=np.int64)


def _brute_lcp(t, width, sa):
    s = t.stream(width).tolist()
    first = set(int(o) for o in t.doc_off[:-1])
    out = []
    for r in range(t.n):
        h = 0
        if r not in first:
            p, q = int(sa[r]), int(sa[r - 1])
            while max(p, q) + h < t.n and s[p + h] == s[q + h] and not (width == 1 and s[p + h] == 0xFF):
                h += 1
        out.append(h)
    return np.array(out, dtype=np.int64)


def _simulate_finish(t, width, direct, geo):
    """The finishing pass as csrc/tables.h states it: classify, a wavefront per listed position for at most geo[3] lanes'
    worth of symbols, the long list in strides of geo[4] lanes, fill from the nearest anchor in front."""
    s = t.stream(width).tolist() + [0] * 64
    sa = t.sa()
    rank = L.inverse(sa)
    lcp = [int(v) for v in direct[:t.n]]
    stretch = L.STRETCH[width]

    def agree(p, q, h, lanes):                       # symbols of a step that agree before the first difference, or None
        for i in range(lanes * stretch):
            a, b = s[p + h + i], s[q + h + i]
            if a != b or (width == 1 and a == 0xFF):
                return i
        return None
    anchor, listed, long_list, rounds = [], [], [], 0
    for p in range(t.n):
        r = int(rank[p])
        if lcp[r] & L.PARTIAL:
            q = int(sa[r - 1])
            red = p > 0 and q > 0 and s[p - 1] == s[q - 1] and not (width == 1 and s[p - 1] == 0xFF)
            anchor.append(not red)
            if not red:
                listed.append(p)
        else:
            anchor.append(True)
    for p in listed:
        r = int(rank[p])
        q = int(sa[r - 1])
        h = lcp[r] & ~L.PARTIAL
        got = agree(p, q, h, geo[3])
        if got is None:
            lcp[r] = L.PARTIAL | (h + geo[3] * stretch)
            long_list.append(p)
        else:
            lcp[r] = h + got
    for p in long_list:
        r = int(rank[p])
        q = int(sa[r - 1])
        h = lcp[r] & ~L.PARTIAL
        it = 0
        while True:
            it += 1
            got = agree(p, q, h, geo[4])
            if got is not None:
                break
            h += geo[4] * stretch
        lcp[r] = h + got
        rounds = max(rounds, it)
    last = 0
    for p in range(t.n):
        if anchor[p]:
            last = p
        else:
            lcp[int(rank[p])] = lcp[int(rank[last])] - (p - last)
    return np.array(lcp, dtype=np.int64), len(listed), len(long_list), rounds


@pytest.mark.parametrize("text", _small_texts(), ids=lambda t: t.what)
def test_witness_equals_brute_force(text):
    sa = _brute_sa(text)
    assert np.array_equal(text.sa(), sa)
    for a, b in zip(text.doc_off[:-1], text.doc_off[1:]):
        assert np.array_equal(np.sort(sa[a:b]), np.arange(a, b))
    for width in text.widths():
        want = _brute_lcp(text, width, sa)
        assert np.array_equal(text.exact(width), want), width
        q = L.phi(sa, text.doc_off)
        s = text.stream(width).tolist()
        red = [p > 0 and q[p] > 0 and s[p - 1] == s[q[p] - 1] and not (width == 1 and s[p - 1] == 0xFF) for p in range(text.n)]
        assert np.array_equal(text.reducible(width), np.array(red, dtype=bool)), width
    if len(text.widths()) == 2:
        assert np.array_equal(text.exact(1), text.exact(4))         # (terminators are unique under either rule)
        assert np.array_equal(text.reducible(1), text.reducible(4))


def test_cut_points():
    assert [L.cut_point(c, 4) for c in (8, 256, 16384)] == [8, 256, 16384]
    assert [L.cut_point(c, 1) for c in (8, 24, 25, 256, 16384)] == [24, 24, 56, 280, 16408]
    for w in (1, 4):
        for cap in (256, 16384):
            assert cap <= L.cut_point(cap, w) < cap + L.STEP[w] and L.cut_point(cap, w) <= cap + L.THRESHOLD_STEP[w]


@pytest.mark.parametrize("text", _small_texts(), ids=lambda t: t.what)
@pytest.mark.parametrize("budget", [-1, 0])
def test_counters_equal_the_finishing_pass_step_by_step(text, budget):
    for width in text.widths():
        exact = text.exact(width)
        direct = L.model_direct(exact, text.n, width, budget, SMALL)
        L.check_direct(direct, int(((direct[:text.n] & L.PARTIAL) != 0).any()), exact, text.doc_off, width, budget, SMALL)
        final, listed, long_n, rounds = _simulate_finish(text, width, direct, SMALL)
        assert np.array_equal(final, exact), width
        assert L.counters(direct, exact, text.sa(), text.reducible(width), width, SMALL) == (listed, long_n), width
        assert L.long_rounds(direct, exact, text.sa(), text.reducible(width), width, SMALL) == rounds, width
        for fraction, zero in ((0.3, False), (1.0, False), (1.0, True)):
            table = L.partial_table(text, width, fraction, 7, zero=zero)
            final, listed, long_n, rounds = _simulate_finish(text, width, table, SMALL)
            assert np.array_equal(final, exact), (width, fraction, zero)
            assert L.counters(table, exact, text.sa(), text.reducible(width), width, SMALL) == (listed, long_n)


def test_the_small_texts_meet_the_small_geometry():
    texts = {t.what: t for t in _small_texts()}
    t = texts["pairs"]
    for width, rounds in ((1, 2), (4, 3)):
        direct = L.model_direct(t.exact(width), t.n, width, 0, SMALL)
        listed, long_n = L.counters(direct, t.exact(width), t.sa(), t.reducible(width), width, SMALL)
        assert listed > long_n > 0 and L.long_rounds(direct, t.exact(width), t.sa(), t.reducible(width), width, SMALL) >= rounds
    assert int(texts["run"].exact(4).max()) == 149 and int(texts["identical"].exact(1).max()) == 39


def _violations(text, width, budget):
    """Direct tables that break one clause of the contract each."""
    exact = text.exact(width)
    good = L.model_direct(exact, text.n, width, budget, SMALL)
    soft, cap = SMALL[0], SMALL[1]
    bit = (good[:text.n] & L.PARTIAL) != 0
    out = []
    plain = np.flatnonzero(~bit & (exact > 0))
    bad = good.copy(); bad[plain[0]] += 1; out.append(("a", bad, 1))
    cut = np.flatnonzero(bit)
    bad = good.copy(); bad[cut[0]] = L.PARTIAL | (soft - 1); out.append(("b-low", bad, 1))
    bad = good.copy(); bad[cut[0]] = L.PARTIAL | (int(exact[cut[0]]) + 1); out.append(("b-high", bad, 1))
    low = np.flatnonzero((exact < soft) & (exact > 0))
    bad = good.copy(); bad[low[0]] = L.PARTIAL | int(exact[low[0]]); out.append(("c", bad, 1))
    far = np.flatnonzero(exact >= cap + L.STEP[width])
    bad = good.copy(); bad[far[0]] = exact[far[0]]; out.append(("d", bad, 1))
    out.append(("f-capped", good, 0))
    bad = good.copy(); bad[0] = 1; out.append(("f-first", bad, 1))
    bad = good.copy(); bad[-1] = 0; out.append(("f-pad", bad, 1))
    return out


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("budget", [-1, 0])
def test_the_contract_refuses_every_violation(width, budget):
    text = L.run_text("run", 1, 150, 6)
    assert text.n % 16 != 0
    for what, table, capped in _violations(text, width, budget):
        with pytest.raises(AssertionError):
            L.check_direct(table, capped, text.exact(width), text.doc_off, width, budget, SMALL)
    exact = text.exact(width)
    with pytest.raises(AssertionError):                    # (e) a deep comparison although nothing is allowed
        L.check_direct(L.model_direct(exact, text.n, width, -1, SMALL), 1, exact, text.doc_off, width, 0, SMALL)
    with pytest.raises(AssertionError):                    # (e) a cut at the soft cap although nothing limits
        L.check_direct(L.model_direct(exact, text.n, width, 0, SMALL), 1, exact, text.doc_off, width, -1, SMALL)
    # a budget of b per slot lets SLOTS * b entries through and no more
    deep = np.flatnonzero(exact >= SMALL[0] + L.THRESHOLD_STEP[width])
    table = L.model_direct(exact, text.n, width, 0, SMALL)
    table[deep[:64]] = np.minimum(exact[deep[:64]], L.PARTIAL | L.cut_point(SMALL[1], width)).astype(np.uint32)
    cutoff = exact[deep[:64]] >= L.cut_point(SMALL[1], width)
    table[deep[:64]] = np.where(cutoff, L.PARTIAL | L.cut_point(SMALL[1], width), exact[deep[:64]]).astype(np.uint32)
    L.check_direct(table, 1, exact, text.doc_off, width, 1, SMALL)
    table[deep[64]] = L.PARTIAL | L.cut_point(SMALL[1], width) if exact[deep[64]] >= L.cut_point(SMALL[1], width) else exact[deep[64]]
    with pytest.raises(AssertionError):
        L.check_direct(table, 1, exact, text.doc_off, width, 1, SMALL)


CASES = L.cases()


@pytest.mark.parametrize("text", CASES, ids=lambda t: t.what)
def test_every_case_reaches_what_it_claims(text):
    assert 0 < text.n <= 70000
    assert set(text.claims) == set(text.widths())
    geo = L.GEOMETRY
    for width, claims in text.claims.items():
        exact, sa, red = text.exact(width), text.sa(), text.reducible(width)
        direct = L.model_direct(exact, text.n, width, 0)
        listed, long_n = L.counters(direct, exact, sa, red, width)
        got = {"listed": listed, "long": long_n, "rounds": L.long_rounds(direct, exact, sa, red, width), "max": int(exact.max()),
               "direct": int(np.count_nonzero(exact >= L.cut_point(geo[1], width))),
               "spent": int(np.count_nonzero(exact >= geo[0] + L.THRESHOLD_STEP[width])) > geo[2] * L.build_budget(text.n)}
        for key, want in claims.items():
            assert got[key] == want, (text.what, width, key, got[key], want)


def test_the_cases_cover_every_threshold():
    by = {t.what: t for t in CASES}
    soft, cap, wave, thr = L.GEOMETRY[0], L.GEOMETRY[1], L.GEOMETRY[3], L.GEOMETRY[4]
    assert sorted(t.claims[1]["rounds"] for t in CASES if 1 in t.claims and "rounds" in t.claims[1]) == [1, 2, 2, 2, 3, 3]
    assert by["ladder_u32"].claims[4]["rounds"] == 3 and by["ladder_u32"].sigma > 254
    # both sides of the direct cap's cut point, both widths
    for w in (1, 4):
        assert by["ladder_direct_0"].claims[w]["direct"] <= 1 < by["ladder_direct_1"].claims[w]["direct"]
        assert by["ladder_direct_2"].claims[w]["max"] == cap + 33
    # every pair of residues mod 8 on the byte stream
    t = by["ladder_residues"]
    starts = np.flatnonzero(np.isin(t.codes[:-1], (1, 2)) & (np.arange(t.n - 1) < t.n - 202)) + 1
    assert set((int(a) % 8, int(b) % 8) for a, b in zip(starts[0::2], starts[1::2])) == set((a, b) for a in range(8) for b in range(8))
    # documents: starts and ends next to multiples of 256 and 64
    assert sorted(int(t.doc_off[1]) - 4096 for t in CASES if t.what.startswith("documents_300")) == [-1, 1, 63, 65]
    for t in CASES:
        if t.what.startswith("documents"):                     # a long entry right behind a document's first rank, one in front
            for w in t.widths():                                  # of another document's first rank
                assert t.exact(w)[int(t.doc_off[1]) + 1] == 999 and t.n_strings.tolist() == [1, 1, 3, 1, 2]
                assert int(t.doc_off[4]) - int(t.doc_off[3]) == 1
    assert any(t.sigma > 254 and t.claims[4].get("long") for t in CASES)
    assert soft < wave < cap and thr * 8 < cap


def test_partial_tables():
    for text in L.mode_b_texts()[:3]:
        for width in text.widths():
            exact = text.exact(width)
            first = np.asarray(text.doc_off[:-1])
            for fraction, zero in ((0.01, False), (0.5, False), (1.0, False), (1.0, True)):
                table = L.partial_table(text, width, fraction, 3, zero=zero).astype(np.int64)
                bit = (table & L.PARTIAL) != 0
                k = table & ~np.int64(L.PARTIAL)
                assert not bit[first].any() and np.all(k <= exact) and np.array_equal(k[~bit], exact[~bit])
                if fraction == 1.0:
                    assert int(bit.sum()) == text.n - first.size and (not zero or not k[bit].any())
                else:
                    assert abs(int(bit.sum()) - fraction * text.n) < 0.2 * fraction * text.n + 30
    big = L.mode_b_texts()[3]
    table = L.partial_table(big, 4, 1.0, 3, zero=True)
    listed, _ = L.counters(table, big.exact(4), big.sa(), big.reducible(4), 4)
    assert listed > 8192 * 4                                  # more than one grid-stride round of lcp_phi_compare_kernel
