"""Exact witness of the DC3 suffix sort (csrc/dc3.h: dc3_suffix_array) in the three forms a build calls it in, and a model
of its driver's decisions, in plain numpy and Python integers: the witness of tests/test_gpu_dc3.py, pinned to brute force
by tests/test_dc3_exact_host.py, which also shows -- by this module alone -- that every case reaches what it claims.

The forms (include/east_hip.h, east_hip_debug_suffix_array_ex): (0) plain u32 symbols in [1, sigma], every recursion
level; (1) u32 codes, text below term_first and the terminators ascending from term_first, level 0 of wide-alphabet text;
(2) the byte stream, 0xFF for every terminator.

The suffix array comes from lcp_exact.suffix_array: prefix doubling, which shares nothing with DC3, orders a shorter
prefix first and terminators by position.  The exact LCP table and the contract of a direct table come from lcp_exact
(kasai, check_direct, model_direct) at width 1: the merge's comparison (dc3_window_lcp, then lcp_bytes_capped from 8) looks
at its caps at 8, after two steps of 8, and then in strides of 32 -- merge_looks() below restates that, and the lengths it
looks at from 24 on are the cut points of lcp_exact.cut_point(cap, 1).  The merge does not write the table's padding: a test
pads with NONE before it calls check_direct.

The model restates, level by level, what the host driver decides (dc3.h, from "sort the sample triples, name them" to
"recurse on the name string"): n0, n1, n2, n02; the sample triples (at level 0 of form 1 with the terminator rule of
dc3_triple_keys_term_kernel: every terminator is term_first in the key, what follows a triple's first terminator is
dropped, and a triple that holds one is a name of its own); the names and their number; the key path from bit_width; and
the branch -- unique names, resolved in place, tried and failed, recursed -- down to the bottom.
"""
import numpy as np

import lcp_exact as L

# MERGE_TILE, RESOLVE_MAX_GROUP, RESOLVE_MAX_LEN, LCP_SOFT_CAP, LCP_DIRECT_CAP, LCP_BUDGET_SLOTS, EAST_HIP_DEBUG_GUARD as the
# library was compiled at the time of writing; the gpu tests take them from east_hip_debug_suffix_array_ex
GEOMETRY = (1024, 32, 2048, 256, 16384, 64, 4096)
TILE, MAX_GROUP, MAX_LEN = GEOMETRY[0], GEOMETRY[1], GEOMETRY[2]
NONE = L.NONE


def lcp_geometry(geo=GEOMETRY):
    """The geometry lcp_exact's checks take (soft cap, direct cap, slots, -, -, fan), from this module's."""
    return (geo[3], geo[4], geo[5], L.GEOMETRY[3], L.GEOMETRY[4], L.GEOMETRY[5])


def bit_width(x):
    return int(x).bit_length()


def merge_looks(limit, soft=GEOMETRY[3]):
    """The lengths at which a comparison of the merge that is still equal looks at its caps (dc3_window_lcp: the window of
    8; common.h, lcp_bytes_capped from h = 8: two steps of 8 while below the soft cap, then strides of 4 x 8)."""
    h, out = 8, []
    for _ in range(2):
        if h < soft:
            h += 8
    while h <= limit:
        out.append(h)
        h += 32
    return out


# ---- the driver, level by level ------------------------------------------------------------------------------------------
class Level(object):
    pass


def level(s, sigma, term_first=0, geo=GEOMETRY):
    s = np.asarray(s, dtype=np.int64)
    n = int(s.size)
    v = Level()
    v.n, v.sigma = n, int(sigma)
    v.n0, v.n1, v.n2 = (n + 2) // 3, (n + 1) // 3, n // 3
    v.n02 = n02 = v.n0 + v.n2
    pad = np.concatenate([s, [0, 0, 0]])
    t = np.arange(n02)
    p = np.where(t < v.n0, 3 * t + 1, 3 * (t - v.n0) + 2)            # dc3_sample_pos
    c0, c1, c2 = pad[p], pad[p + 1], pad[p + 2]
    if term_first:
        bits = 3 * bit_width(term_first)
        v.keys = "u32" if bits <= 32 else "u64"
        c0 = np.minimum(c0, term_first)
        c1 = np.where(c0 == term_first, 0, np.minimum(c1, term_first))
        c2 = np.where((c0 == term_first) | (c1 == term_first), 0, np.minimum(c2, term_first))
        has_term = (c0 == term_first) | (c1 == term_first) | (c2 == term_first)
        v.term_at = (int(np.count_nonzero(c0 == term_first)), int(np.count_nonzero(c1 == term_first)),
                     int(np.count_nonzero(c2 == term_first)))
        order = np.lexsort((p, c2, c1, c0))                          # (enumerated in text order, sorted stably)
    else:
        bits = 3 * bit_width(sigma)
        v.keys = "u32" if bits <= 32 else "u64" if bits <= 64 else "two-stage"
        has_term = np.zeros(n02, dtype=bool)
        order = np.lexsort((t, c2, c1, c0))
    v.triples = np.stack([c0, c1, c2], axis=1)
    a0, a1, a2, ht = c0[order], c1[order], c2[order], has_term[order]
    new = np.ones(n02, dtype=bool)
    new[1:] = (a0[1:] != a0[:-1]) | (a1[1:] != a1[:-1]) | (a2[1:] != a2[:-1]) | ht[1:]
    # (equal keys that hold a terminator: what a naming without the terminator rule would give one name)
    v.term_ties = int(np.count_nonzero(ht[1:] & (a0[1:] == a0[:-1]) & (a1[1:] == a1[:-1]) & (a2[1:] == a2[:-1])))
    names = np.cumsum(new)
    v.n_names = int(names[-1])
    v.s12 = np.empty(n02, dtype=np.int64)
    v.s12[order] = names
    v.max_group = int(np.bincount(names).max())
    v.ties = n02 - v.n_names
    # adjacent sorted triples that agree in the first two symbols and differ in the third, and names that share their third
    # symbol with another name: what a two-stage naming that ignored one of its two keys would merge
    same2 = (a0[1:] == a0[:-1]) & (a1[1:] == a1[:-1])
    v.third_only = int(np.count_nonzero(same2 & (a2[1:] != a2[:-1])))
    v.share_third = v.n_names - int(np.unique(a2).size)
    v.rank_top = bit_width(2 * v.n0 + 1)
    v.longest = None
    if v.n_names == n02:
        v.branch = "unique"
    elif v.ties <= n02 // 8:
        # dc3_resolve_ties_kernel: a group above RESOLVE_MAX_GROUP fails; two members are compared name by name at the
        # offsets 1 .. RESOLVE_MAX_LEN and fail if all agree, i.e. if the suffixes of the name string share RESOLVE_MAX_LEN + 1
        # names or more -- the largest such length over a group is the largest over neighbours in suffix order
        off = np.array([0, n02], dtype=np.int64)
        sa12 = L.suffix_array(v.s12, off)
        v.longest = int(L.kasai(v.s12, sa12, off, 4).max())
        v.branch = "resolved" if v.max_group <= geo[1] and v.longest <= geo[2] else "failed"
    else:
        v.branch = "recurse"
    return v


def model(symbols, sigma, term_first=0, geo=GEOMETRY):
    """Every level the driver runs for these symbols, from level 0 (term_first > 0: form 1) to the bottom."""
    out, s = [], np.asarray(symbols, dtype=np.int64)
    while True:
        v = level(s, sigma, term_first if not out else 0, geo)
        out.append(v)
        if v.branch in ("unique", "resolved"):
            return out
        s, sigma = v.s12, v.n_names


def merge_profile(sa, geo=GEOMETRY):
    """The level-0 merge as its tiles see it: A = the sample suffixes (positions not 0 mod 3), B the others; splits[i] = A
    elements among the first i tiles' outputs."""
    sa = np.asarray(sa, dtype=np.int64)
    n, tile = int(sa.size), geo[0]
    tiles = -(-n // tile)
    is_a = sa % 3 != 0
    cum = np.concatenate([[0], np.cumsum(is_a)])
    splits = cum[np.minimum(np.arange(tiles + 1) * tile, n)]
    na = np.diff(splits)
    count = np.minimum(tile, n - np.arange(tiles) * tile)
    first_a = int(np.flatnonzero(is_a)[0]) if is_a.any() else n
    first_b = int(np.flatnonzero(~is_a)[0]) if (~is_a).any() else n
    return {"tiles": tiles, "splits": [int(x) for x in splits], "b_only": int(np.count_nonzero(na == 0)),
            "a_only": int(np.count_nonzero(na == count)), "first_a": first_a, "first_b": first_b,
            "switches": int(np.count_nonzero(is_a[1:] != is_a[:-1]))}


# ---- a case --------------------------------------------------------------------------------------------------------------
class Case(object):
    """One call of the entry: the text in its form, the arguments, the claims.  Claims (every one is checked by the host
    test against the model; a case without any fails there): "keys" / "branch" -- per level, from level 0; "max_group" --
    the largest group of equal names at level 0; "ties" -- n02 - n_names at level 0; "longest" -- the longest run of names
    two tied suffixes share at level 0; "tiles" -- merge tiles at level 0; "split" -- items of merge_profile; "levels";
    "rank_top" -- bit_width(2 n0 + 1) at level 0; "term_at" -- level-0 triples with the terminator first / second / third,
    at least; "third_only", "share_third", "term_ties" -- at least; "residue" -- n mod 3; "lcp" -- {"max": ..., "heads_above_soft": ...}."""

    def __init__(self, what, form, text=None, symbols=None, sigma=None, claims=None):
        self.what, self.form, self.claims = what, form, dict(claims or {})
        self._cache = {}
        if form == 0:
            self.codes = np.asarray(symbols, dtype=np.uint32)
            self.sigma, self.term_first, self.text = int(sigma), 0, None
            assert self.codes.min() >= 1 and self.codes.max() <= self.sigma
        else:
            self.text = text
            self.codes = text.codes
            self.term_first = text.term_first
            self.sigma = text.term_first - 1 + int(text.n_strings.sum())
            assert len(text.docs) == 1 and (form == 1 or text.term_first <= 255)
        self.n = int(self.codes.size)

    def data(self):
        """What goes to the entry: u32 symbols / codes, or the byte stream."""
        return self.text.stream(1) if self.form == 2 else self.codes

    def sa(self):
        if "sa" not in self._cache:
            self._cache["sa"] = L.suffix_array(self.codes, np.array([0, self.n], dtype=np.int64)) if self.form == 0 else self.text.sa()
        return self._cache["sa"]

    def model(self, geo=GEOMETRY):
        """Forms 0 and 1.  (Level 0 of form 2 runs on window keys, csrc/level0.h, whose rounds are not modelled here.)"""
        if "model" not in self._cache:
            self._cache["model"] = model(self.codes, self.sigma, self.term_first if self.form == 1 else 0, geo)
        return self._cache["model"]

    def profile(self, geo=GEOMETRY):
        return merge_profile(self.sa(), geo)


def check_claims(case, geo=GEOMETRY):
    """AssertionError unless the case reaches, by the model and the witness, everything it claims."""
    c = case.claims
    assert c, "%s: a case without a claim" % case.what
    known = {"keys", "branch", "max_group", "ties", "longest", "tiles", "split", "levels", "rank_top", "term_at", "third_only",
             "share_third", "residue", "lcp", "levels_resolved", "term_ties"}
    assert set(c) <= known, (case.what, set(c) - known)
    need_model = set(c) - {"tiles", "split", "residue", "lcp"}
    if need_model:
        assert case.form != 2, "%s: level 0 of the byte form is not modelled" % case.what
        m = case.model(geo)
        v = m[0]
        for key in ("keys", "branch"):
            if key in c:
                got = [getattr(x, key) for x in m]
                assert got[:len(c[key])] == list(c[key]) and (key == "keys" or len(got) == len(c[key])), (case.what, key, got)
        for key in ("max_group", "ties", "longest", "rank_top"):
            if key in c:
                assert getattr(v, key) == c[key], (case.what, key, getattr(v, key))
        for key in ("third_only", "share_third", "term_ties"):
            if key in c:
                assert getattr(v, key) >= c[key], (case.what, key, getattr(v, key))
        if "term_at" in c:
            assert all(g >= w for g, w in zip(v.term_at, c["term_at"])), (case.what, v.term_at)
        if "levels" in c:
            assert len(m) == c["levels"], (case.what, len(m))
        if "levels_resolved" in c:
            assert sum(x.branch == "resolved" for x in m) == c["levels_resolved"], case.what
    if "residue" in c:
        assert case.n % 3 == c["residue"], case.what
    if "tiles" in c:
        assert -(-case.n // geo[0]) == c["tiles"], (case.what, case.n)
    if "split" in c:
        prof = case.profile(geo)
        for key, want in c["split"].items():
            assert prof[key] == want, (case.what, key, prof[key])
    if "lcp" in c:
        exact = case.text.exact(1)
        if "max" in c["lcp"]:
            assert int(exact.max()) == c["lcp"]["max"], (case.what, int(exact.max()))
        if "heads_above_soft" in c["lcp"]:
            heads = exact[geo[0]::geo[0]]
            assert int(np.count_nonzero(heads >= geo[3] + L.THRESHOLD_STEP[1])) == c["lcp"]["heads_above_soft"], (case.what, heads)
        if "values" in c["lcp"]:
            assert set(c["lcp"]["values"]) <= set(int(x) for x in exact), case.what


def key_path(sigma):
    b = 3 * bit_width(sigma)
    return "u32" if b <= 32 else "u64" if b <= 64 else "two-stage"


# ---- texts ---------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def with_term_first(text, term_first):
    """The same strings under a larger term_first: the letters keep their codes, the terminators move up."""
    assert term_first >= text.term_first
    text.codes = np.where(text.codes >= text.term_first, text.codes - text.term_first + term_first, text.codes).astype(np.uint32)
    text.term_first, text.sigma = term_first, term_first - 1
    text._cache = {}
    return text


def cut_text(what, n, letters, seed):
    """n symbols in all: random letters, cut into strings at random places (the last symbol is a terminator)."""
    rng = _rng(seed)
    letters = np.asarray(letters)
    is_term = rng.random(n) < 0.2
    is_term[-1] = True
    body = letters[rng.integers(0, letters.size, size=n)]
    strings, start = [], 0
    for e in np.flatnonzero(is_term):
        strings.append(body[start:e])
        start = int(e) + 1
    return with_term_first(L.Text(what, [strings]), int(letters.max()) + 1)


def short_strings(what, count, max_len, letters, seed):
    rng = _rng(seed)
    letters = np.asarray(letters)
    strings = [letters[rng.integers(0, letters.size, size=int(rng.integers(0, max_len + 1)))] for _ in range(count)]
    return with_term_first(L.Text(what, [strings]), int(letters.max()) + 1)


def sizes(geo=GEOMETRY):
    return list(range(1, 41)) + [k * geo[0] + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)]


def size_cases(form, sigma, geo=GEOMETRY):
    """Every n of sizes() over an alphabet of sigma letters: the three residues, the dummy sample, the base cases of the
    recursion, output counts next to a multiple of the merge tile."""
    out = []
    for n in sizes(geo):
        claims = {"residue": n % 3, "tiles": -(-n // geo[0])}
        what = "size_f%d_s%d_n%d" % (form, sigma, n)
        if form == 0:
            claims["keys"] = ["u32"]
            out.append(Case(what, 0, symbols=_rng(1000 * sigma + n).integers(1, sigma + 1, size=n), sigma=sigma, claims=claims))
        else:
            if form == 1:
                claims["keys"] = ["u32"]
            out.append(Case(what, form, text=cut_text(what, n, np.arange(1, sigma + 1), 2000 * sigma + n), claims=claims))
    return out


def key_path_cases():
    out = []
    for sigma in (1023, 1024, (1 << 21) - 1, 1 << 21, 1 << 22):
        s = _rng(sigma).integers(sigma - 2, sigma + 1, size=3000)
        out.append(Case("keys_%d" % sigma, 0, symbols=s, sigma=sigma,
                        claims={"keys": [key_path(sigma)], "branch": ["recurse", "resolved"], "tiles": 3, "third_only": 10, "share_third": 10}))
    for sigma in (1 << 21, 1 << 22):
        # (v, A, A) repeated: the triples at 3q + 1 are (A, A, v') -- tied but for the third symbol
        rng = _rng(sigma + 1)
        s = np.full(3000, sigma)
        s[0::3] = rng.integers(sigma - 2, sigma, size=1000)
        out.append(Case("keys_%d_third" % sigma, 0, symbols=s, sigma=sigma,
                        claims={"keys": ["two-stage"], "branch": ["recurse", "recurse", "recurse", "unique"], "third_only": 2, "tiles": 3}))
        # (A, v, w) repeated: the triples at 3q + 1 are (v, w, A) and share their third symbol, those at 3q + 2 are (w, A, v')
        s = np.full(3000, sigma)
        s[1::3] = rng.integers(sigma - 2, sigma, size=1000)
        s[2::3] = rng.integers(sigma - 2, sigma, size=1000)
        out.append(Case("keys_%d_first_two" % sigma, 0, symbols=s, sigma=sigma,
                        claims={"keys": ["two-stage"], "branch": ["recurse", "recurse", "unique"], "share_third": 3, "tiles": 3}))
    return out


def term_cases():
    out = []
    for tf in (2, 3, 255, 256, 1023, 1024, 2559):
        letters = np.arange(max(1, tf - 3), tf)
        t = short_strings("term_%d" % tf, 300, 11, letters, tf)
        out.append(Case("term_%d" % tf, 1, text=t, claims={"keys": ["u32" if tf <= 1023 else "u64"], "term_at": (100, 100, 100), "term_ties": 100}))
    return out


def group_case(k, seed=7):
    """A random background and one triple of three reserved symbols planted k times at positions 1 mod 3, 150 apart."""
    sigma, n = 1000, 6000
    s = _rng(seed).integers(1, sigma - 3, size=n)
    for i in range(k):
        s[1 + 150 * i:4 + 150 * i] = (sigma - 2, sigma - 1, sigma)
    ok = k <= MAX_GROUP
    return Case("group_%d" % k, 0, symbols=s, sigma=sigma,
                claims={"keys": ["u32"] if ok else ["u32", "u64"], "branch": ["resolved"] if ok else ["failed", "unique"],
                        "max_group": k, "ties": k - 1, "tiles": 6, "levels": 1 if ok else 2, "levels_resolved": 1 if ok else 0})


LENGTH_N = 120000


def length_case(B, distance, claims, seed=9, n=LENGTH_N):
    """A random background in which a passage of B symbols stands twice, `distance` apart."""
    sigma = 1000
    s = _rng(seed).integers(1, sigma + 1, size=n)
    at = 30001
    s[at + distance:at + distance + B] = s[at:at + B]
    return Case("length_%d_%d" % (B, distance % 3), 0, symbols=s, sigma=sigma, claims=claims)


def share_case(extra):
    """n02 = 4000, n02 / 8 = 500: 500 triples of reserved symbols, each planted twice at positions 1 mod 3 -- 500 ties; extra:
    one tie more, a pair of equal triples at positions 2 mod 3."""
    sigma, n, pairs = 1000, 6000, 500
    s = _rng(14).integers(1, 901, size=n)            # (a seed whose background has no tie of its own: the claims say so)
    for i in range(pairs):
        tri = (1000, 901 + i % 100, 901 + i // 100)
        for side in (0, 1):
            p = 6 * (2 * i + side) + 1
            s[p:p + 3] = tri
            s[p + 3] = 1 + side                          # (the triples behind the two copies differ)
    if extra:
        # every planted triple starts with 1000: (1000, 1000, 1000) twice at positions 2 mod 3, led by the two different
        # symbols above
        for p in (6 * 0 + 5, 6 * 3 + 5):
            s[p:p + 2] = 1000
    ties = pairs + (1 if extra else 0)
    return Case("share_%d" % ties, 0, symbols=s, sigma=sigma, claims={
        "keys": ["u32"] if not extra else ["u32", "u64"], "ties": ties, "max_group": 2, "tiles": 6,
        "branch": ["resolved"] if not extra else ["recurse", "unique"]})


def fibonacci(n):
    a, b = [1], [1, 2]
    while len(b) < n:
        a, b = b, b + a
    return np.array(b[:n])


def depth_cases(geo=GEOMETRY):
    n = 3 * geo[0] + 1
    return [
        Case("all_same", 0, symbols=np.ones(n), sigma=1, claims={"levels": 8, "branch": ["recurse"] * 7 + ["unique"], "tiles": 4,
                                                                  "keys": ["u32"] * 8}),
        Case("fibonacci", 0, symbols=fibonacci(5000), sigma=2, claims={"levels": 6, "branch": ["recurse"] * 5 + ["resolved"],
                                                                       "tiles": 5, "levels_resolved": 1}),
        Case("period2", 0, symbols=np.resize([1, 2], n), sigma=2, claims={"tiles": 4, "branch": ["recurse"] * 7 + ["unique"]}),
        Case("period3", 0, symbols=np.resize([2, 1, 1], n), sigma=2, claims={"tiles": 4, "branch": ["recurse"] * 7 + ["unique"]}),
    ]


def _byte_text(what, symbols):
    """One string: the symbols but the last, which becomes the terminator (n stays what it was)."""
    return L.Text(what, [[np.asarray(symbols)[:-1]]])


def merge_cases(form, geo=GEOMETRY):
    out = []
    for d in (-1, 0, 1):
        n = 3 * geo[0] + d
        n0 = (n + 2) // 3
        rng = _rng(50 + d)
        shapes = []
        s = rng.integers(2, 4, size=n)
        s[0::3] = 1
        shapes.append(("b_first", s, 3))
        s = rng.integers(1, 3, size=n)
        s[0::3] = 3
        shapes.append(("a_first", s, 3))
        shapes.append(("one_letter", np.ones(n, dtype=np.int64), 1))
        for name, s, sigma in shapes:
            what = "merge_%s_f%d_%+d" % (name, form, d)
            if form == 0:
                split = {"b_first": {"first_a": n0, "b_only": 1, "switches": 1}, "a_first": {"first_b": n - n0, "a_only": 1 if d < 0 else 2, "switches": 1},
                         "one_letter": {}}[name]
                out.append(Case(what, 0, symbols=s, sigma=sigma, claims={"tiles": 3 if d < 1 else 4, "split": split, "residue": n % 3}))
            else:
                # (the last symbol is the terminator, the largest: where it stands at 3q, the B side's last suffix)
                last_b = (n - 1) % 3 == 0
                split = {"b_first": {"first_a": n0 - 1 if last_b else n0}, "a_first": {"first_b": n - n0 if last_b else n - n0 - 1}, "one_letter": {}}[name]
                out.append(Case(what, 2, text=_byte_text(what, s), claims={"tiles": 3 if d < 1 else 4, "split": split, "residue": n % 3}))
    if form == 2:
        # runs of equal short strings: a$a$a$ ..., $$$ ..., ab$ab$ ...: the comparator's 0xFF rule decides at the first symbol
        # (two suffixes that start with a terminator) and at the second (a sample at 3q + 2 in front of one)
        for d in (-1, 0, 1):
            n = 3 * geo[0] + d
            kinds = [np.array([1]), np.array([], dtype=np.int64), np.array([1, 2]), np.array([2])]
            strings = [kinds[0]] * 300 + [kinds[1]] * 300 + [kinds[2]] * 200
            # ... and the same strings in random succession: what stands behind a terminator then orders against the positions,
            # so the rule (the earlier terminator first) and the ranks behind the terminators disagree
            strings += [kinds[k] for k in _rng(70 + d).integers(0, 4, size=650)]
            rest = n - sum(x.size + 1 for x in strings)
            strings += [np.array([2, 1, 1])] * (rest // 4) + [kinds[1]] * (rest % 4)
            what = "merge_equal_strings_%+d" % d
            out.append(Case(what, 2, text=L.Text(what, [strings]), claims={"tiles": 3 if d < 1 else 4, "residue": n % 3,
                                                                           "lcp": {"values": [0, 1, 2, 3]}}))
    return out


def scatter_cases():
    out = [Case("scatter_%d" % n, 0, symbols=_rng(n).integers(1, 5, size=n), sigma=4,
                claims={"rank_top": 8 if n <= 381 else 9, "tiles": 1}) for n in range(379, 386)]
    return out + [depth_cases()[0]]


def lcp_cases(geo=GEOMETRY):
    """The byte form with the fused LCP: the single-document byte cases of lcp_exact.cases(), and small texts at the edges
    of the merge's own window."""
    names = ("ladder_residues", "ladder_bytes_wave", "ladder_direct_0", "ladder_direct_1", "ladder_direct_2", "run_one_letter_200",
             "run_period3_200", "two_copies_200", "identical_strings_200")
    by_name = {t.what: t for t in L.cases(lcp_geometry(geo))}
    out = [Case("lcp_" + k, 2, text=by_name[k], claims={"lcp": {"max": by_name[k].claims[1]["max"]} if "max" in by_name[k].claims[1] else {},
                                                        "tiles": -(-by_name[k].n // geo[0])}) for k in names]
    out.append(Case("lcp_window_edge", 2, text=L.pair_ladder("window_edge", [6, 7, 8, 9], 20, 60, residues=[(1, 2), (3, 0), (5, 5), (7, 4)]),
                    claims={"lcp": {"values": [6, 7, 8, 9], "max": 9}, "tiles": 1}))
    # two equal strings of length j: the common prefix of their first suffixes is ended by the terminator at byte j
    strings = []
    for j in range(8):
        body = np.concatenate([[3 + j], np.full(max(j - 1, 0), 1)])[:j]
        strings += [body, body]
    out.append(Case("lcp_term_in_window", 2, text=L.Text("term_in_window", [strings + [np.arange(1, 11)]]),
                    claims={"lcp": {"values": list(range(8)), "max": 7}, "tiles": 1}))
    out.append(Case("lcp_short_strings", 2, text=short_strings("short_strings", 3000, 4, [1, 2], 61), claims={"lcp": {"max": 4}}))
    out.append(Case("lcp_run_heads", 2, text=L.run_text("run_heads", 1, 5000, 0), claims={"lcp": {"max": 4999, "heads_above_soft": 4}, "tiles": 5}))
    return out


# the neighbouring lengths of the copied passage, found with the model for the seed of length_case (see the host test)
LENGTH_OK, LENGTH_FAIL = 6146, 6147


def resolve_cases():
    out = [group_case(k) for k in (31, 32, 33)]
    out.append(length_case(LENGTH_OK, 30000, {"branch": ["resolved"], "longest": MAX_LEN, "keys": ["u32"], "max_group": 2}))
    out.append(length_case(LENGTH_FAIL, 30000, {"branch": ["failed", "resolved"], "longest": MAX_LEN + 1, "keys": ["u32", "u64"], "max_group": 2}))
    out.append(length_case(3000, 30001, {"branch": ["resolved"], "keys": ["u32"], "max_group": 2}))
    out += [share_case(0), share_case(1)]
    return out


def all_cases(geo=GEOMETRY):
    out = []
    for form in (0, 1, 2):
        for sigma in (1, 2, 4):
            out += size_cases(form, sigma, geo)
    out += key_path_cases() + term_cases() + resolve_cases() + depth_cases(geo) + merge_cases(0, geo) + merge_cases(2, geo)
    out += scatter_cases()[:-1] + lcp_cases(geo)
    return out
