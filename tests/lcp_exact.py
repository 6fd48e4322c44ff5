"""Exact references of the two passes that make the LCP table (csrc/tables.h: lcp_kernel, lcp8_kernel and the finishing
pass lcp_phi_*; csrc/build.h: direct_lcp, finish_capped_lcp) in plain numpy and Python integers: the witness of
tests/test_gpu_lcp_passes.py and tests/test_gpu_wide_repeats.py, pinned to brute force by tests/test_lcp_exact_host.py.

A text here is a list of documents, each a list of strings, each an array of text codes 1 .. sigma.  It has two
streams, as a build holds them: bytes (width 1: the codes, 0xFF for every terminator; sigma <= 254 only) and dense u32
codes (width 4: the codes, the terminators numbered term_first + i in the order of their positions).  The suffix array is
the same under both: terminators order by position.
"""
import numpy as np

PARTIAL = 0x80000000
NONE = 0xFFFFFFFF
# the geometry of the library as compiled at the time of writing; the gpu tests take it from east_hip_debug_lcp
GEOMETRY = (256, 16384, 64, 1024, 1024, 16)          # SOFT_CAP, DIRECT_CAP, BUDGET_SLOTS, WAVE_STEPS * WAVE, LONG_THREADS, FAN
# Symbols a direct comparison advances between two looks at its caps.  u32: 4 (csrc/tables.h, lcp_kernel: `h += 4;` in
# front of the two tests); bytes: 32 (csrc/common.h, lcp_bytes_capped: the loop `for (int k = 0; k < 4; k++)` of 8-byte
# steps between two passes through the tests at the top of `while (true)`).  A cut length k therefore lies in
# [cap, cap + STEP).  The tests on the exact value take THRESHOLD_STEP: 0 for u32 -- both caps are multiples of 4 and the
# comparison starts at 0, so it looks exactly at them --, 32 for bytes, which start their strides at 24 (a first window of
# 8 in lcp8_kernel, two single steps of 8 in lcp_bytes_capped).
STEP = {1: 32, 4: 4}
THRESHOLD_STEP = {1: 32, 4: 0}
BYTE_FIRST = 24
STRETCH = {1: 8, 4: 1}                               # symbols a lane compares per step of the finishing pass (lcp_phi_step)


def cut_point(cap, width):
    """Where a direct comparison that is cut at `cap` stops: the first length it looks at that is >= cap."""
    if width == 4:
        return -(-cap // 4) * 4
    return BYTE_FIRST + -(-(cap - BYTE_FIRST) // 32) * 32


def pyr_padded(n, fan=16):
    return -(-n // fan) * fan


class Text(object):
    def __init__(self, what, docs, claims=None):
        self.what = what
        self.docs = [[np.asarray(s, dtype=np.uint32) for s in d] for d in docs]
        assert all(len(d) >= 1 for d in self.docs)
        assert all(s.size == 0 or s.min() >= 1 for d in self.docs for s in d)
        self.sigma = max([int(s.max()) for d in self.docs for s in d if s.size] + [1])
        self.term_first = self.sigma + 1
        parts, off, t = [], [0], 0
        for d in self.docs:
            for s in d:
                parts += [s, np.array([self.term_first + t], dtype=np.uint32)]
                t += 1
            off.append(off[-1] + sum(s.size + 1 for s in d))
        self.codes = np.concatenate(parts).astype(np.uint32)
        self.n = int(self.codes.size)
        self.doc_off = np.array(off, dtype=np.int64)
        self.n_strings = np.array([len(d) for d in self.docs], dtype=np.int32)
        self.claims = dict(claims or {})
        self._cache = {}

    def widths(self):
        return (1, 4) if self.sigma <= 254 else (4,)

    def stream(self, width):
        if width == 4:
            return self.codes
        assert self.sigma <= 254
        return np.where(self.codes >= self.term_first, 0xFF, self.codes).astype(np.uint8)

    def sa(self):
        if "sa" not in self._cache:
            self._cache["sa"] = suffix_array(self.codes, self.doc_off)
        return self._cache["sa"]

    def exact(self, width):
        if ("lcp", width) not in self._cache:
            self._cache["lcp", width] = kasai(self.stream(width), self.sa(), self.doc_off, width)
        return self._cache["lcp", width]

    def reducible(self, width):
        if ("red", width) not in self._cache:
            self._cache["red", width] = reducible(self.stream(width), self.sa(), self.doc_off, width)
        return self._cache["red", width]

    def symbols(self, letters, tagged=False):
        """The text as a build takes it: code c spelled letters[c - 1], the i-th string of a document ended by U+0A00 + i
        (tagged: by 0x80000000 | i, the encoding for text at or above U+0A00)."""
        letters = np.asarray(letters, dtype=np.uint32)
        assert letters.size >= self.sigma and np.all(np.diff(letters.astype(np.int64)) > 0)
        parts = []
        for d in self.docs:
            for i, s in enumerate(d):
                parts += [letters[s.astype(np.int64) - 1], np.array([(0x80000000 | i) if tagged else 0x0A00 + i], dtype=np.uint32)]
        return np.concatenate(parts).astype(np.uint32)


# ---- suffix array, exact table, reducible positions ----------------------------------------------------------------------
def _doubling(s):
    n = s.size
    rank = np.unique(s, return_inverse=True)[1].astype(np.int64).reshape(-1)
    k = 1
    while True:
        second = np.full(n, -1, dtype=np.int64)
        if k < n:
            second[:n - k] = rank[k:]
        order = np.lexsort((second, rank))
        a, b = rank[order], second[order]
        new = np.empty(n, dtype=np.int64)
        new[order] = np.concatenate([[0], np.cumsum((a[1:] != a[:-1]) | (b[1:] != b[:-1]))])
        rank = new
        if n == 1 or int(rank.max()) == n - 1:
            return order.astype(np.int64)
        k *= 2


def suffix_array(codes, doc_off):
    """Per document, by prefix doubling on the u32 codes: positions in the shard, every document's ranks in its own range."""
    codes = np.asarray(codes)
    sa = np.empty(codes.size, dtype=np.int64)
    for a, b in zip(doc_off[:-1], doc_off[1:]):
        sa[a:b] = a + _doubling(codes[a:b])
    return sa


def kasai(stream, sa, doc_off, width):
    """The exact table: 0 at every document's first rank, else the common prefix of the suffixes at ranks r - 1 and r.
    width 1: a 0xFF byte ends a common prefix (equal 0xFF bytes are different terminators); width 4: plain equality."""
    s = np.asarray(stream).tolist()
    sa_l = np.asarray(sa).tolist()
    n = len(s)
    rank = [0] * n
    for r, p in enumerate(sa_l):
        rank[p] = r
    first = set(int(o) for o in doc_off[:-1])
    lcp = [0] * n
    h = 0
    for p in range(n):
        r = rank[p]
        if r in first:
            h = 0
            continue
        q = sa_l[r - 1]
        m = n - max(p, q)
        if width == 1:
            while h < m and s[p + h] == s[q + h] and s[p + h] != 0xFF:
                h += 1
        else:
            while h < m and s[p + h] == s[q + h]:
                h += 1
        lcp[r] = h
        if h:
            h -= 1
    return np.array(lcp, dtype=np.int64)


def inverse(sa):
    rank = np.empty(sa.size, dtype=np.int64)
    rank[sa] = np.arange(sa.size)
    return rank


def phi(sa, doc_off):
    """phi[p]: the suffix in front of p's in its document's order, -1 where p's is the document's first."""
    rank = inverse(sa)
    prev = np.concatenate([[-1], sa[:-1]])
    prev[np.asarray(doc_off[:-1], dtype=np.int64)] = -1
    return prev[rank]


def reducible(stream, sa, doc_off, width):
    """reducible[p]: p > 0, phi(p) > 0, the symbols in front of the two agree (and, on bytes, are no terminator)."""
    s = np.asarray(stream).astype(np.int64)
    q = phi(sa, doc_off)
    p = np.arange(s.size)
    ok = (p > 0) & (q > 0)
    a, b = s[np.maximum(p - 1, 0)], s[np.maximum(q - 1, 0)]
    ok &= a == b
    if width == 1:
        ok &= a != 0xFF
    return ok


# ---- the contract of a direct table, the counters ------------------------------------------------------------------------
def model_direct(exact, n, width, budget, geo=GEOMETRY):
    """The direct table where it is determined: no budget (budget < 0: cut at the direct cap only) or a budget of 0 (cut
    at the soft cap wherever a comparison reaches it)."""
    assert budget <= 0
    soft, direct, fan = geo[0], geo[1], geo[5]
    at = cut_point(direct if budget < 0 else soft, width)
    out = np.full(pyr_padded(n, fan), NONE, dtype=np.uint32)
    out[:n] = np.where(exact >= at, PARTIAL | at, exact).astype(np.uint32)
    return out


def check_direct(direct, capped, exact, doc_off, width, budget, geo=GEOMETRY):
    """The contract (a) .. (f) of a direct table against the exact one; budget: deep comparisons per slot, < 0 = none."""
    soft, direct_cap, slots, fan = geo[0], geo[1], geo[2], geo[5]
    n = exact.size
    direct = np.asarray(direct, dtype=np.uint32).astype(np.int64)
    assert direct.size == pyr_padded(n, fan)
    bit = (direct[:n] & PARTIAL) != 0
    k = direct[:n] & ~np.int64(PARTIAL)
    step, ts = STEP[width], THRESHOLD_STEP[width]
    assert np.array_equal(k[~bit], exact[~bit]), "(a) an entry without the bit differs from the exact value at rank %d" % \
        np.flatnonzero(~bit & (k != exact))[0]
    assert np.all((k[bit] >= soft) & (k[bit] <= exact[bit])), "(b) a cut entry below the soft cap or above the exact value"
    at_soft = (k >= soft) & (k < soft + step)
    at_direct = (k >= direct_cap) & (k < direct_cap + step)
    assert np.all(at_soft[bit] | at_direct[bit]), "(b) a cut entry that is at neither cap"
    if budget < 0:
        assert np.all(at_direct[bit]), "(d) a cut at the soft cap without a budget"
    assert not np.any(bit & (exact < soft)), "(c) a cut entry whose exact value is below the soft cap"
    far = exact >= direct_cap + ts
    assert np.all(bit[far]), "(d) an entry at or beyond the direct cap without the bit"
    deep = exact >= soft + ts
    if budget >= 0:
        assert int(np.count_nonzero(deep & ~bit)) <= slots * budget, "(e) more deep comparisons than the budget"
        assert int(np.count_nonzero(at_direct & bit)) <= slots * budget, "(e) more comparisons up to the direct cap than the budget"
    if budget == 0:
        assert np.all(bit[deep]) and np.all(k[deep] < soft + step), "(e) budget 0: a comparison went deep"
    if budget < 0:
        assert not np.any(bit & (exact < direct_cap)), "(e) no budget: a cut below the direct cap"
    assert (int(capped) != 0) == bool(bit.any()), "(f) capped"
    assert direct[0] == 0 and np.all(direct[np.asarray(doc_off[:-1], dtype=np.int64)] == 0), "(f) a document's first rank"
    assert np.all(direct[n:] == NONE), "(f) the padding"


def counters(direct, exact, sa, red, width, geo=GEOMETRY):
    """(positions listed, positions handed to the long kernel) for the direct table the finishing pass was given."""
    n = exact.size
    d = np.asarray(direct, dtype=np.uint32)[:n].astype(np.int64)
    bit = (d & PARTIAL) != 0
    k = d & ~np.int64(PARTIAL)
    listed = bit & ~red[sa]                              # by rank
    long_ = listed & (exact - k >= geo[3] * STRETCH[width])
    return int(np.count_nonzero(listed)), int(np.count_nonzero(long_))


def long_rounds(direct, exact, sa, red, width, geo=GEOMETRY):
    """The largest number of iterations lcp_phi_long_kernel makes for a listed position (0: nothing on the long list).
    It starts behind what the wavefront saw to agree: the compare kernel leaves LCP_PARTIAL_BIT | (k + its whole reach)."""
    n = exact.size
    d = np.asarray(direct, dtype=np.uint32)[:n].astype(np.int64)
    bit = (d & PARTIAL) != 0
    k = d & ~np.int64(PARTIAL)
    wave = geo[3] * STRETCH[width]
    rest = (exact - k)[bit & ~red[sa]]
    rest = rest[rest >= wave]
    return int((rest.max() - wave) // (geo[4] * STRETCH[width])) + 1 if rest.size else 0


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def pair_ladder(what, lengths, sigma, seed, residues=None, claims=None):
    """Pairs of equal passages of the given lengths in one string.  Every copy is led and followed by a symbol of its own
    pair and side (the two leads differ, the two followers differ), so that the pair's longest common prefix is its length
    and only the copies' first positions are irreducible.  The passages are random over the letters 5 .. sigma; 1 .. 4
    lead and follow.  residues: per pair, the two copies' start positions mod 8 (filled with letter 5 .. material)."""
    rng = _rng(seed)
    parts, pos = [], 0
    for i, L in enumerate(lengths):
        body = rng.integers(5, sigma + 1, size=L)
        for side in (0, 1):
            if residues is not None:
                fill = (residues[i][side] - (pos + 1)) % 8
                parts.append(rng.integers(5, sigma + 1, size=fill))
                pos += fill
            parts += [np.array([1 + side]), body, np.array([3 + side])]
            pos += L + 2
    parts.append(np.arange(1, sigma + 1))                # (every letter present: the alphabet is sigma)
    return Text(what, [[np.concatenate(parts)]], claims)


def run_text(what, period, repeats, fillers, claims=None):
    """`fillers` distinct letters, then a period of `period` letters `repeats` times."""
    unit = np.arange(1, period + 1)
    return Text(what, [[np.concatenate([np.arange(1, fillers + 1), np.resize(unit, repeats)])]], claims)


def two_copies(what, length, sigma, seed, claims=None):
    body = _rng(seed).integers(3, sigma + 1, size=length)
    return Text(what, [[np.concatenate([np.arange(1, sigma + 1), [1], body, [2], body])]], claims)


def identical_strings(what, count, length, sigma, seed, claims=None):
    body = _rng(seed).integers(1, sigma + 1, size=length)
    body[:min(sigma, length)] = np.arange(1, min(sigma, length) + 1)
    return Text(what, [[body] * count], claims)


def several_documents(what, sigma, seed, shift, claims=None):
    """Copies within and across documents, a document that is one run, a document of one symbol (its terminator).  The run
    is the second document and starts at 4096 + shift: its second rank holds the run's length - 1, a long entry right
    behind a document's first rank, which `shift` puts next to a multiple of 256 or 64."""
    rng = _rng(seed)
    passage = rng.integers(3, sigma + 1, size=1500)
    every = np.arange(1, sigma + 1)
    head = np.concatenate([every, [1], passage, [2], passage])
    d0 = [np.concatenate([head, rng.integers(3, sigma + 1, size=4096 + shift - head.size - 1)])]
    d1 = [np.full(1000, 9)]
    body2 = np.concatenate([[2], passage, [1], passage, np.full(700, 7)])
    d2 = [body2, rng.integers(3, sigma + 1, size=2 * 4096 + 64 - body2.size - 3), np.array([], dtype=np.uint32)]
    d3 = [np.array([], dtype=np.uint32)]
    d4 = [np.concatenate([passage, [1]]), passage]
    return Text(what, [d0, d1, d2, d3, d4], claims)


def random_text(what, n, sigma, seed, strings=3):
    rng = _rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), size=strings - 1, replace=False)) if strings > 1 else []
    return Text(what, [list(np.split(rng.integers(1, sigma + 1, size=n), cuts))])


def cases(geo=GEOMETRY):
    """Every text of the kernel-level tests, by name.  Claims: what a text was made to reach, shown by this witness alone
    (tests/test_lcp_exact_host.py) -- width -> {"listed": n at budget 0, "long": n at budget 0, "rounds": iterations of
    the long kernel at budget 0, "max": the largest exact value, "direct": entries at or beyond the direct cut point}."""
    soft, direct, wave, thr = geo[0], geo[1], geo[3], geo[4]
    out = []
    # u32: the soft cap, the wave bound behind it, one and two strides of the long kernel
    k4 = cut_point(soft, 4)
    lens = [soft + d for d in (-1, 0, 1, 3, 4)] + [k4 + m * wave + d for m in (1, 2, 3) for d in (-1, 0, 1)]
    out.append(pair_ladder("ladder_u32", lens, 300, 11,
                           claims={4: {"listed": len(lens) - 1, "long": 8, "rounds": 3, "max": lens[-1]}}))
    # bytes: the same distances behind the point at which the byte comparison is cut, eight symbols a lane
    k1 = cut_point(soft, 1)
    near = [soft - 1, soft, soft + 1, k1 - 1, k1, k1 + 1, k1 + 31, k1 + 32]
    res = [(a, b) for a in range(8) for b in range(8)]
    out.append(pair_ladder("ladder_residues", [near[i % len(near)] for i in range(64)], 200, 12, residues=res,
                           claims={1: {"listed": 32, "long": 0}, 4: {"listed": 56, "long": 0}}))
    out.append(pair_ladder("ladder_bytes_wave", [k1 + 8 * wave + d for d in (-1, 0, 1)] + [soft + 8 * wave], 200, 13,
                           residues=[(1, 6), (7, 2), (3, 3), (5, 0)],
                           claims={1: {"listed": 4, "long": 2, "rounds": 1}, 4: {"listed": 4, "long": 4, "rounds": 8}}))
    out.append(pair_ladder("ladder_bytes_long_1", [k1 + 8 * (wave + thr) - 1, k1 + 8 * (wave + thr)], 200, 14, residues=[(5, 2), (0, 7)],
                           claims={1: {"listed": 2, "long": 2, "rounds": 2}}))
    out.append(pair_ladder("ladder_bytes_long_2", [k1 + 8 * (wave + thr) + 1, soft + 4], 200, 15, residues=[(3, 4), (1, 1)],
                           claims={1: {"listed": 1, "long": 1, "rounds": 2}}))
    for i, d in enumerate((-1, 0, 1)):
        out.append(pair_ladder("ladder_bytes_long_%d" % (3 + i), [k1 + 8 * (wave + 2 * thr) + d], 200, 16 + i, residues=[(2 + i, 7 - i)],
                               claims={1: {"listed": 1, "long": 1, "rounds": 3 if d >= 0 else 2}}))
    # the direct cap, both widths
    for i, ds in enumerate(((-1, 0), (1, 31), (32, 33))):
        out.append(pair_ladder("ladder_direct_%d" % i, [direct + d for d in ds], 200, 20 + i, residues=[(1, 4), (6, 3)],
                               claims={w: {"listed": 2, "max": direct + ds[1],
                                           "direct": sum(max(0, direct + d - cut_point(direct, w) + 1) for d in ds)} for w in (1, 4)}))
    for fillers in (300, 200):
        ws = (4,) if fillers > 254 else (1, 4)
        out.append(run_text("run_one_letter_%d" % fillers, 1, 20000, fillers,
                            claims={w: {"listed": 1, "long": 1, "max": 19999, "direct": 20000 - cut_point(direct, w)} for w in ws}))
        out.append(run_text("run_period3_%d" % fillers, 3, 20001, fillers,
                            claims={w: {"listed": 1, "long": 1, "max": 19998} for w in ws}))
        out.append(two_copies("two_copies_%d" % fillers, 18000, fillers, 30,
                              claims={w: {"listed": 1, "long": 1, "max": 18000} for w in ws}))
        out.append(identical_strings("identical_strings_%d" % fillers, 60, 400, fillers, 31,
                                     claims={w: {"listed": 59, "long": 0, "max": 400} for w in ws}))
    for shift in (-1, 1, 63, 65):
        out.append(several_documents("documents_300_%+d" % shift, 300, 40, shift, claims={4: {"max": 1500, "listed": 5, "long": 3}}))
    out.append(several_documents("documents_200", 200, 41, 0, claims={1: {"max": 1500, "listed": 5}, 4: {"max": 1500, "listed": 5}}))
    for t in out:                                        # every one of them has more deep comparisons than a build's budget
        for w in t.widths():
            t.claims.setdefault(w, {})["spent"] = True
    return out


def build_budget(n, geo=GEOMETRY):
    """Deep comparisons per slot that a build of n symbols allows (csrc/build.h, build_impl: ctx.lcp_budget.per_slot)."""
    return max(n // 256 // geo[2], 4)


def mode_b_texts():
    return [random_text("random_2", 5000, 2, 50), random_text("random_26", 5000, 26, 51), random_text("random_300", 5000, 300, 52),
            random_text("random_300_long_list", 40000, 300, 53, strings=1)]


def partial_table(text, width, fraction, seed, zero=False):
    """Mode B: the exact table with a random `fraction` of the ranks that may be (all but the documents' first) made
    LCP_PARTIAL_BIT | k, k uniform in [0, exact] (zero: k = 0)."""
    exact = text.exact(width)
    rng = _rng(seed)
    may = np.ones(text.n, dtype=bool)
    may[text.doc_off[:-1]] = False
    pick = may & (rng.random(text.n) < fraction)
    k = np.zeros(text.n, dtype=np.int64) if zero else rng.integers(0, exact + 1)
    return np.where(pick, PARTIAL | k, exact).astype(np.uint32)
