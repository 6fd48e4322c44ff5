"""gpu tier: the DC3 suffix sort at kernel level, in every form a build calls it in (csrc/dc3.h: the triple keys with and
without the terminator rule, the two-stage sort of wide alphabets, the naming, dc3_resolve_ties_kernel, the ranks plain and
bucketed, the merge on tuples and on byte records, the LCP table fused into the byte merge and dc3_lcp_heads_kernel;
csrc/level0.h: the sample mode of the byte stream's level 0).

Everything goes through east_hip_debug_suffix_array_ex, which runs dc3_suffix_array as build_impl calls it.  The witness is
tests/dc3_exact.py (pinned to brute force by tests/test_dc3_exact_host.py, which also shows that every case reaches what
it claims): the suffix array is array_equal to prefix doubling's, the guard behind every output is intact, the levels run
and resolved are the model's (forms 0 and 1), the fused LCP table is held to the contract of a direct table and, where its
cuts are determined, equal to the model.  The thresholds come from the library (geometry_out); the cases are made for
dc3_exact.GEOMETRY, and the first test fails if the two differ.
"""
import ctypes

import numpy as np
import pytest

import dc3_exact as D
import lcp_exact as L

pytestmark = pytest.mark.gpu

_u32p, _i64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)
ERR_INVALID = -2
EE = 0xEEEEEEEE
INFO = ("levels", "levels_resolved", "refine_rounds", "radix_passes_u32", "radix_passes_u64", "merge_elems")
CASES = {c.what: c for c in D.all_cases()}


def _call(hip, form, data, sigma, term_first, bucket=-1, lean=0, want_lcp=0, budget=-1, fill=0x5A, expect=0, n=None, lcp_null=False):
    data = np.ascontiguousarray(data, dtype=np.uint8 if form == 2 else np.uint32)
    guard = hip.DEBUG_GUARD
    sa, lcp = np.full(data.size + guard, 0x11111111, dtype=np.uint32), np.full(data.size + guard, 0x11111111, dtype=np.uint32)
    n = int(data.size) if n is None else n               # (another n: a call that is refused before it reads or writes)
    capped, info, geo = np.full(1, 0x11111111, dtype=np.uint32), np.full(6, -7, dtype=np.int64), np.full(7, 0x11111111, dtype=np.uint32)
    rc = hip.load().east_hip_debug_suffix_array_ex(0, form, data.ctypes.data_as(ctypes.c_void_p), n, sigma, term_first, bucket, lean,
                                                   want_lcp, budget, fill, sa.ctypes.data_as(_u32p),
                                                   None if lcp_null else lcp.ctypes.data_as(_u32p), capped.ctypes.data_as(_u32p),
                                                   info.ctypes.data_as(_i64p), geo.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.load().east_hip_last_error())
    if expect != 0:                                       # (nothing was launched, nothing was written)
        assert np.all(sa == 0x11111111) and np.all(lcp == 0x11111111) and capped[0] == 0x11111111
        assert np.all(info == -7) and np.all(geo == 0x11111111)
        return None
    assert np.all(sa[n:] == EE), "a write behind the suffix array"
    if want_lcp:
        assert np.all(lcp[n:] == EE), "a write behind the LCP table"
    elif not lcp_null:
        assert np.all(lcp == EE), "an LCP table nobody asked for"
    return sa[:n], lcp[:n], int(capped[0]), dict(zip(INFO, (int(x) for x in info))), tuple(int(g) for g in geo)


def _run(hip, case, **kw):
    return _call(hip, case.form, case.data(), case.sigma, case.term_first, **kw)


def _check(hip, case, **kw):
    sa, lcp, capped, info, geo = _run(hip, case, **kw)
    want = case.sa()
    if not np.array_equal(sa, want):
        bad = int(np.flatnonzero(sa != want)[0])
        raise AssertionError("%s: the suffix array differs at rank %d of %d: %d, want %d" % (case.what, bad, case.n, sa[bad], want[bad]))
    if case.form != 2:
        m = case.model(geo)
        assert info["levels"] == len(m), (case.what, info, [v.branch for v in m])
        assert info["levels_resolved"] == sum(v.branch == "resolved" for v in m), (case.what, info, [v.branch for v in m])
        assert info["merge_elems"] == sum(v.n for v in m)
        wide = [v.keys for v in m]
        assert (info["radix_passes_u64"] > 0) == any(k != "u32" for k in wide), (case.what, info, wide)
    return sa, lcp, capped, info, geo


def _check_lcp(case, lcp, capped, budget, geo):
    exact = case.text.exact(1)
    lgeo = D.lcp_geometry(geo)
    table = np.full(L.pyr_padded(case.n, lgeo[5]), L.NONE, dtype=np.uint32)     # (the merge does not write the padding)
    table[:case.n] = lcp
    L.check_direct(table, capped, exact, case.text.doc_off, 1, budget, lgeo)
    if budget <= 0:                                       # (where the cuts are determined, so is the whole table)
        want = L.model_direct(exact, case.n, 1, budget, lgeo)
        if not np.array_equal(table, want):
            bad = int(np.flatnonzero(table != want)[0])
            raise AssertionError("%s, budget %d: the table differs at rank %d: %#x, want %#x (exact %d)"
                                 % (case.what, budget, bad, table[bad], want[bad], exact[bad]))


def test_geometry(hip):
    c = CASES["size_f0_s2_n40"]
    geo = _check(hip, c)[4]
    assert geo == D.GEOMETRY, "tests/dc3_exact.py states the tile and the bounds its cases are made for: restate them"
    assert geo[6] == hip.DEBUG_GUARD and D.lcp_geometry(geo) == L.GEOMETRY


@pytest.mark.parametrize("sigma", [1, 2, 4])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_every_small_size_and_the_sizes_next_to_a_tile(hip, form, sigma):
    """n = 1 .. 40 -- the residues, the dummy sample, the base cases -- and k * MERGE_TILE + d."""
    for n in D.sizes():
        case = CASES["size_f%d_s%d_n%d" % (form, sigma, n)]
        _check(hip, case)
        if form == 2:
            sa, lcp, capped, info, geo = _check(hip, case, want_lcp=1)
            _check_lcp(case, lcp, capped, -1, geo)


@pytest.mark.parametrize("name", [c.what for c in D.key_path_cases()])
def test_key_paths_with_ties(hip, name):
    _check(hip, CASES[name])


@pytest.mark.parametrize("name", [c.what for c in D.term_cases()])
def test_terminator_rule_on_both_key_widths(hip, name):
    case = CASES[name]
    sa, lcp, capped, info, geo = _check(hip, case)
    assert (info["radix_passes_u64"] > 0) == (case.term_first > 1023)
    if case.term_first <= 255:                            # (the same strings on the byte stream)
        as_bytes = D.Case(name + "_bytes", 2, text=case.text)
        _check(hip, as_bytes)


@pytest.mark.parametrize("name", [c.what for c in D.resolve_cases()])
def test_resolve_ties_on_both_sides_of_each_bound(hip, name):
    case = CASES[name]
    sa, lcp, capped, info, geo = _check(hip, case)
    assert [v.branch for v in case.model(geo)] == list(case.claims["branch"])


@pytest.mark.parametrize("name", [c.what for c in D.depth_cases()])
def test_depth(hip, name):
    case = CASES[name]
    sa, lcp, capped, info, geo = _check(hip, case)
    assert info["levels"] == len(case.claims["branch"])


@pytest.mark.parametrize("name", [c.what for c in D.merge_cases(0) + D.merge_cases(2)])
def test_merge_shapes(hip, name):
    case = CASES[name]
    _check(hip, case)
    if case.form == 2:
        sa, lcp, capped, info, geo = _check(hip, case, want_lcp=1, budget=0)
        _check_lcp(case, lcp, capped, 0, geo)


@pytest.mark.parametrize("name", [c.what for c in D.scatter_cases()])
def test_bucketed_rank_scatter_gives_the_same(hip, name):
    """rank_bucket_bytes = 0 sends every level through dc3_rank_pairs_kernel, one radix pass on the top bits of the slot
    (from bit top - 8, or all of them where top <= 8) and dc3_rank_store_kernel."""
    case = CASES[name]
    a, b = _check(hip, case), _check(hip, case, bucket=0)
    assert np.array_equal(a[0], b[0]) and a[3]["levels"] == b[3]["levels"]
    assert b[3]["radix_passes_u32"] == a[3]["radix_passes_u32"] + a[3]["levels"]     # (one pass more per level)


@pytest.mark.parametrize("budget", ["none", "zero", "build"])
@pytest.mark.parametrize("name", [c.what for c in D.lcp_cases()])
def test_lcp_fused_into_the_byte_merge(hip, name, budget):
    case = CASES[name]
    b = {"none": -1, "zero": 0, "build": L.build_budget(case.n)}[budget]
    sa, lcp, capped, info, geo = _check(hip, case, want_lcp=1, budget=b)
    _check_lcp(case, lcp, capped, b, geo)
    if name == "lcp_run_heads" and b <= 0:                # (dc3_lcp_heads_kernel cuts at budget 0 and goes deep without one)
        heads = lcp[geo[0]::geo[0]]
        assert heads.size == 4
        assert np.all(heads == (L.PARTIAL | L.cut_point(geo[3], 1))) if b == 0 else np.array_equal(heads, case.text.exact(1)[geo[0]::geo[0]])


@pytest.mark.parametrize("name", ["lcp_run_heads", "lcp_window_edge", "lcp_term_in_window", "lcp_short_strings", "lcp_identical_strings_200",
                                  "merge_equal_strings_+1", "size_f2_s1_n1", "size_f2_s2_n7"])
def test_nothing_depends_on_what_lies_behind_the_pad(hip, name):
    """The windows and the comparisons read past the stream's end, and the u32 stream of form 2 holds the fill byte: what
    they find there decides nothing."""
    case = CASES[name]
    for b in (0, -1):
        a, z = _check(hip, case, want_lcp=1, budget=b, fill=0x5A), _check(hip, case, want_lcp=1, budget=b, fill=0xFF)
        for x, y in zip(a, z):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        _check_lcp(case, a[1], a[2], b, a[4])
    for form in (0, 1):
        other = CASES["size_f%d_s2_n%d" % (form, 1025)]
        a, z = _check(hip, other, fill=0x5A), _check(hip, other, fill=0xFF)
        assert np.array_equal(a[0], z[0]) and a[3] == z[3]


@pytest.mark.parametrize("name", ["lcp_identical_strings_200", "lcp_run_period3_200", "lcp_short_strings", "merge_equal_strings_-1"])
def test_lean_and_wide_window_keys(hip, name):
    """lean: the sample mode hands its names to the recursion without refinement rounds; window sort mode 3: 64-bit window
    keys at level 0 where 32 bits would do."""
    case = CASES[name]
    plain = _check(hip, case, want_lcp=1, budget=0)
    lean = _check(hip, case, want_lcp=1, budget=0, lean=1)
    assert np.array_equal(plain[1], lean[1]) and plain[2] == lean[2]
    assert lean[3]["refine_rounds"] == 0
    _check_lcp(case, lean[1], lean[2], 0, lean[4])
    if name.startswith("lcp_identical") or name.startswith("lcp_run"):
        assert lean[3]["levels"] >= 2                     # (a repetitive text: names went to the recursion)
    lib = hip.load()
    assert lib.east_hip_debug_set_window_sort(3) == 0
    try:
        wide = _check(hip, case, want_lcp=1, budget=0)
    finally:
        assert lib.east_hip_debug_set_window_sort(1) == 0
    assert np.array_equal(plain[1], wide[1]) and plain[2] == wide[2]
    assert wide[3]["radix_passes_u64"] > 0


def test_the_rank_bucket_knob_of_a_call_is_its_own(hip):
    """rank_bucket_bytes goes into the call's own knobs: a call without it runs the plain scatter again."""
    case = CASES["scatter_385"]
    a = _check(hip, case)
    b = _check(hip, case, bucket=0)
    c = _check(hip, case)
    assert a[3] == c[3] and b[3]["radix_passes_u32"] > a[3]["radix_passes_u32"]


def test_rejections(hip):
    """Every argument check answers EAST_HIP_ERR_INVALID before anything is launched; the outputs stay untouched."""
    t = L.Text("two_strings", [[np.array([1, 2, 1, 2, 3]), np.array([2, 1])]])
    codes, s8, tf, sigma = t.codes, t.stream(1), t.term_first, t.term_first - 1 + 2
    lib = hip.load()

    def bad(form, data, sigma_, tf_, message=None, **kw):
        assert _call(hip, form, data, sigma_, tf_, expect=ERR_INVALID, **kw) is None
        if message:
            assert message in lib.east_hip_last_error().decode(), lib.east_hip_last_error()
    plain = np.array([1, 2, 3, 1, 2], dtype=np.uint32)
    assert _call(hip, 0, plain, 3, 0) is not None and _call(hip, 1, codes, sigma, tf) is not None
    assert _call(hip, 2, s8, sigma, tf, want_lcp=1) is not None and _call(hip, 2, s8, sigma, tf, lcp_null=True) is not None
    bad(3, plain, 3, 0), bad(-1, plain, 3, 0)
    bad(0, plain, 3, 0, n=0), bad(0, plain, 3, 0, n=-1), bad(0, plain, 3, 0, n=0x7FFFFFF0)
    bad(0, plain, 0, 0)
    bad(0, plain, 2, 0, "symbol outside")
    z = plain.copy(); z[2] = 0
    bad(0, z, 3, 0, "symbol outside")
    bad(0, plain, 3, 4, "term_first belongs")
    bad(0, plain, 3, 0, "byte form", want_lcp=1), bad(1, codes, sigma, tf, "byte form", want_lcp=1)
    bad(2, s8, sigma, tf, want_lcp=1, lcp_null=True)
    bad(0, plain, 3, 0, bucket=-2), bad(0, plain, 3, 0, lean=2), bad(0, plain, 3, 0, want_lcp=2)
    bad(2, s8, sigma, tf, budget=-2, want_lcp=1), bad(0, plain, 3, 0, fill=256), bad(0, plain, 3, 0, fill=-1)
    # form 1
    bad(1, codes, sigma, 1, "term_first out of range"), bad(1, codes, sigma, 1 << 21, "term_first out of range")
    bad(1, codes[:-1], sigma - 1, tf, "does not end in a terminator")
    bad(1, codes, sigma + 1, tf, "sigma is not"), bad(1, codes, sigma - 1, tf, "sigma is not")
    s = codes.copy(); s[0] = 0
    bad(1, s, sigma, tf, "a code outside")
    s = codes.copy(); s[0] = tf + t.n
    bad(1, s, sigma, tf, "a code outside")
    s = codes.copy(); s[5], s[8] = s[8], s[5]
    bad(1, s, sigma, tf, "must ascend")
    s = codes.copy(); s[8] = s[5]
    bad(1, s, sigma, tf, "must ascend")
    # form 2
    bad(2, s8, sigma, 1, "term_first out of range"), bad(2, s8, sigma, 256, "term_first out of range")
    bad(2, s8[:-1], sigma - 1, tf, "does not end in a terminator")
    bad(2, s8, sigma + 1, tf, "sigma is not")
    s = s8.copy(); s[1] = 0
    bad(2, s, sigma, tf, "a zero byte")
    s = s8.copy(); s[1] = tf
    bad(2, s, sigma, tf, "neither a text code nor 0xFF")
    s = s8.copy(); s[1] = 0xFE
    bad(2, s, sigma, tf, "neither a text code nor 0xFF")
