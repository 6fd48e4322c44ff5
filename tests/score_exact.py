"""An exact host model of the keyphrase x document score (csrc/score.h), for exhaustive differential tests.

The contract.  A document is a list of strings s_1 .. s_m of text symbols (code points; no terminators).  For a
non-empty sequence u of symbols, f(u) is the number of occurrences of u as a substring of the strings, and
root = n_d - m_d = the number of text symbols of the document.  The walk of a keyphrase suffix q goes on while
f(q[:j]) > 0:

  * at depth 0 a node is always entered:              acc += f(q[:1]) / root;
  * deeper, a node is entered iff f(q[:j]) < f(q[:j-1]):  acc += f(q[:j]) / f(q[:j-1]);
  * the suffix result is (acc + depth) - nodes, divided by depth if normalized; 0.0 at depth 0;
  * the score is the sum of the suffix results, in suffix order, divided by |q|.

These are the reference's double operations in the reference's order (easa.py:91-139), so a correct implementation
equals the model bit for bit -- table entries and per-suffix results, normalized and not.  A query symbol that is no
text symbol of the document (absent from the corpus, a terminator code point, no code point at all) has f = 0.

The model shares nothing with the suffix-array code: it is a dict of substring counts up to a length L and a loop.
A walk that would need a count beyond L raises (the model never guesses).

The module also holds what the two test files share: the document families (seeded generators), the keyphrase sets,
the cases, and per case the coverage facts -- what its walks do at which table level, computed from the model alone.
"""
import itertools

import numpy as np

TERMINATOR_START = 0x0A00
TERMINATOR_TAG = 0x80000000
WALK_ENDGAME = 4                # csrc/score.h: intervals of at most that many suffixes are finished out of registers
FIRST_LETTER = 0x41             # letter i of a generated alphabet is FIRST_LETTER + 2 i: the odd code points are absent


def _key(seq):
    return np.asarray(seq, dtype="<u4").tobytes()


def substring_counts(strings, L):
    """{u (as little-endian uint32 bytes): f(u)} for every u of at most L symbols."""
    c = {}
    get = c.get
    for s in strings:
        b = _key(s)
        n = len(b) // 4
        for i in range(n):
            for j in range(i + 1, min(n, i + L) + 1):
                u = b[4 * i:4 * j]
                c[u] = get(u, 0) + 1
    return c


class ModelDepth(Exception):
    """A walk went deeper than the counts reach."""


class Document(object):
    """One document of the model: its strings, substring counts up to L, walks memoised per suffix."""

    def __init__(self, strings, L):
        self.strings = [[int(c) for c in s] for s in strings]
        self.m = len(self.strings)
        self.n = sum(len(s) for s in self.strings) + self.m
        self.root = self.n - self.m
        assert self.m >= 1 and self.root >= 1, "the score divides by the root annotation n_d - m_d"
        self.L = L
        self.counts = substring_counts(self.strings, L)
        self._walks = {}

    def f(self, u):
        return self.counts.get(u if isinstance(u, bytes) else _key(u), 0)

    def walk(self, qb):
        """(acc, depth, nodes) of the walk of the suffix qb (bytes of uint32)."""
        r = self._walks.get(qb)
        if r is None:
            get = self.counts.get
            acc, depth, nodes, parent = 0.0, 0, 0, self.root
            for j in range(4, len(qb) + 1, 4):
                if j > 4 * self.L:
                    raise ModelDepth("a walk passed depth %d" % self.L)
                f = get(qb[:j], 0)
                if f == 0:
                    break
                if depth == 0 or f < parent:
                    acc += f / parent
                    nodes += 1
                parent = f
                depth += 1
            r = self._walks[qb] = (acc, depth, nodes)
        return r

    def suffix_result(self, qb, normalized):
        acc, depth, nodes = self.walk(qb)
        if depth == 0:
            return 0.0
        r = (acc + depth) - nodes
        return r / depth if normalized else r

    def score(self, q, normalized):
        """(score, [suffix results]) of the keyphrase q."""
        qb = _key(q)
        suf = [self.suffix_result(qb[4 * i:], normalized) for i in range(len(qb) // 4)]
        total = 0.0
        for v in suf:
            total += v
        return total / len(suf), suf


def document_symbols(strings, tagged=False):
    """A document as east_hip_build takes it: string i followed by its terminator."""
    parts = []
    for i, s in enumerate(strings):
        parts.append(np.array(list(s) + [(TERMINATOR_TAG | i) if tagged else TERMINATOR_START + i], dtype=np.uint32))
    return np.concatenate(parts)


def score_tables(documents, keyphrases, normalized):
    """The (K, D) table and the (D, S) per-suffix array in HipIndex.score_table's layout."""
    K, D = len(keyphrases), len(documents)
    keys = [_key(q) for q in keyphrases]
    S = sum(len(b) for b in keys) // 4
    table = np.zeros((K, D), np.float64)
    suf = np.zeros((D, S), np.float64)
    for d, doc in enumerate(documents):
        res = doc.suffix_result
        row = suf[d]
        s = 0
        for k, b in enumerate(keys):
            n = len(b) // 4
            total = 0.0
            for i in range(n):
                v = res(b[4 * i:], normalized)
                row[s + i] = v
                total += v
            table[k, d] = total / n
            s += n
    return table, suf


def all_keyphrases(alphabet, max_len):
    """Every sequence of 1 .. max_len symbols of the alphabet, shorter ones first, in the alphabet's order."""
    out = []
    for n in range(1, max_len + 1):
        out.extend(list(q) for q in itertools.product(alphabet, repeat=n))
    return out


def pack(keyphrases):
    """[keyphrase] -> (q_symbols uint32, q_offsets int64)."""
    off = np.zeros(len(keyphrases) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in keyphrases], out=off[1:])
    return np.array([c for q in keyphrases for c in q], dtype=np.uint32), off


# ---- document families ----------------------------------------------------------------------------
def letters(sigma):
    return [FIRST_LETTER + 2 * i for i in range(sigma)]


def cut(rng, symbols, mean):
    """The symbols as strings of 1 .. 2 mean - 1 symbols."""
    out, i = [], 0
    while i < len(symbols):
        n = int(rng.integers(1, 2 * mean))
        out.append([int(c) for c in symbols[i:i + n]])
        i += n
    return out


def random_text(rng, alphabet, n, mean=9, p=None):
    return cut(rng, rng.choice(alphabet, size=n, p=p), mean)


def forbidden_bigrams(alphabet):
    """Every letter keeps a successor: (x, x) for the letters at even places, (x, next letter) for those at odd ones."""
    s = len(alphabet)
    out = set()
    if s >= 2:
        out.update((alphabet[i], alphabet[i]) for i in range(0, s, 2))
    if s >= 3:
        out.update((alphabet[i], alphabet[(i + 1) % s]) for i in range(1, s, 2))
    return out


def markov_text(rng, alphabet, n, mean=9):
    forb = forbidden_bigrams(alphabet)
    s = [int(alphabet[0])]
    while len(s) < n:
        c = int(rng.choice(alphabet))
        if (s[-1], c) not in forb:
            s.append(c)
    return cut(rng, s, mean)


def one_letter(letter):
    return [[letter] * n for n in (1, 2, 3, 7, 40)]


def period3(rng, alphabet, n, mean=30):
    unit = [alphabet[0], alphabet[-1], alphabet[-1]]
    return cut(rng, (unit * (n // 3 + 1))[:n], mean)


def tiny_documents(alphabet):
    """Documents of n_d = 2, 3, 4, 4, 5 symbols: the smallest the C ABI and the oracle take (n_d - m_d >= 1)."""
    a, b = alphabet[0], alphabet[-1]
    return [[[b]], [[a, b]], [[a, b, a]], [[a], [b]], [[b], [b, a]]]


def ladder_documents(alphabet, k):
    """One string a^(k + w - 1) each, w = 1 .. 5, and a^(k + 8): f(a^k) = w -- the width a walk of a^k.. leaves level k with."""
    a = alphabet[0]
    return [[[a] * (k + w - 1)] for w in (1, 2, 3, 4, 5, 9)]


def clamp_documents(alphabet, k):
    """One string each (so that the last ranks but one hold text).  With u = z a^(k-1), z the largest and a the smallest
    letter: `a z a^(k-1)` -- u once, at rank n_d - 2 --, and `z a^k z a^(k-1)` -- u twice, the ranks n_d - 3 and n_d - 2."""
    a, z = alphabet[0], alphabet[-1]
    assert a != z
    return [[[a, z] + [a] * (k - 1)], [[z] + [a] * k + [z] + [a] * (k - 1)]]


# ---- cases ----------------------------------------------------------------------------------------
ALL_WIDTHS = {1, 2, 3, 4, 5, 6}          # (6: more than 5)


class Case(object):
    """A collection with its keyphrases and what its walks are expected to show.

    docs        [[string]], string = [text code point]
    L           the keyphrases are all sequences of at most L symbols over the text alphabet + `absent` (+ `extra`)
    plans       [(k, pairs)]: the table depths the collection is meant to get (by whichever side builds the tables) and
                whether the pair layout is meant; the facts are asserted for each
    expect      {fact: value the fact must reach}, or {plan: {fact: value}}; see facts() and expected()
    model_docs  the documents the model covers (None: all)
    """

    def __init__(self, name, docs, L, plans, expect, tagged=False, extra=(), keyphrases=None, absent=None, model_docs=None,
                 model_L=None):
        self.name, self.docs, self.L, self.plans, self.expect, self.tagged = name, docs, L, list(plans), dict(expect), tagged
        self.letters = sorted(set(c for doc in docs for s in doc for c in s))
        self.sigma_t = len(self.letters)
        self.A = self.sigma_t + 2
        self.absent = absent if absent is not None else self.letters[0] + 1
        assert self.absent not in self.letters and self.absent >= 2
        self.extra = [list(q) for q in extra]
        self._keyphrases = keyphrases
        self.model_docs = list(range(len(docs))) if model_docs is None else list(model_docs)
        self.model_L = model_L if model_L is not None else L + 1
        self.window_sort = 1                 # east_hip_debug_set_window_sort for the build (1: the default)
        self.marked = False                  # the build marks the tables off its window keys
        self.with_long = None                # the packing case: its keyphrases + one longer than a workgroup
        self._documents = {}
        self._tables = {}

    def __repr__(self):
        return self.name

    def expected(self, plan):
        return self.expect[plan] if plan in self.expect else self.expect

    # the build's input
    def input(self):
        parts = [document_symbols(doc, self.tagged) for doc in self.docs]
        off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
        return np.concatenate(parts), off, np.array([len(doc) for doc in self.docs], dtype=np.int32)

    def keyphrases(self):
        if self._keyphrases is None:
            self._keyphrases = all_keyphrases(self.letters + [self.absent], self.L) + self.extra
        return self._keyphrases

    def document(self, d):
        if d not in self._documents:
            self._documents[d] = Document(self.docs[d], self.model_L)
        return self._documents[d]

    def tables_of(self, docs, normalized):
        """The model's table and per-suffix array of the documents `docs` alone, computed once."""
        key = (tuple(docs), normalized)
        if key not in self._tables:
            self._tables[key] = score_tables([self.document(d) for d in docs], self.keyphrases(), normalized)
        return self._tables[key]

    def tables(self, normalized):
        """The model's (K, len(model_docs)) table and per-suffix array, computed once."""
        if normalized not in self._tables:
            self._tables[normalized] = score_tables([self.document(d) for d in self.model_docs], self.keyphrases(), normalized)
        return self._tables[normalized]

    # the oracle's view: it knows text below U+0A00 only, and takes a terminator code point in a query for the terminator
    def oracle_input(self):
        """(symbols, offsets, n_strings, rename): the collection with its text renamed, order-preserving, to 2, 3, ... where
        it holds text at or above U+0A00 (else as it is); rename(q) = the query in those names, every symbol that is no
        text symbol of the corpus as the one absent symbol."""
        if self.tagged:
            name = {c: 2 + i for i, c in enumerate(self.letters)}
            unused = 2 + self.sigma_t
        else:
            name = {c: c for c in self.letters}
            unused = self.absent
        parts = []
        for doc in self.docs:
            for i, s in enumerate(doc):
                parts.append(np.array([name[c] for c in s] + [TERMINATOR_START + i], dtype=np.uint32))
        sym = np.concatenate(parts)
        _, off, ms = self.input()
        return sym, off, ms, lambda q: [name.get(c, unused) for c in q]

    # ---- coverage facts -------------------------------------------------------------------------
    def code(self, c):
        """The dense code of a text symbol in the k-gram tables: 1 .. sigma_t in code point order."""
        return self.letters.index(c) + 1

    def present_codes(self, d, k):
        """The sorted k-gram codes of the suffixes of document d (csrc/score.h: kgram_code -- the terminator class is
        A - 1, behind it pads)."""
        A = self.A
        rank = {c: i + 1 for i, c in enumerate(self.letters)}
        flat = []
        for s in self.docs[d]:
            flat.extend(rank[c] for c in s)
            flat.append(A - 1)
        x = np.array(flat + [0] * k, dtype=np.int64)
        n = len(flat)
        g = np.zeros(n, np.int64)
        ended = np.zeros(n, bool)
        for i in range(k):
            c = np.where(ended, 0, x[i:i + n])
            ended |= c == A - 1
            g = g * A + c
        return np.unique(g)

    def facts(self, k, pairs):
        """What the walks of the case's keyphrases do in its documents, for tables of depth k, from the model alone:

        ends_at_level   the levels j at which a walk ends because q[:j] is absent while q[:j-1] is present
        leave_widths    min(f(q[:k]), 6) of the walks that go on behind level k (k = 0: behind the first symbol)
        no_shrink       a step with f(q[:j]) == f(q[:j-1])
        clamp           a walk that goes on behind level max(k, 1) with at most WALK_ENDGAME suffixes whose interval starts
                        within the last 3 ranks of a document of at least WALK_ENDGAME symbols
        short_document  such a walk (any start) in a document of fewer than WALK_ENDGAME symbols
        max_depth       the deepest match
        and with pairs: empty_run -- the longest run of absent k-grams behind a present one that a walk reads; last_text_gram
        -- a walk reads the last present k-gram of a document that holds text only; tail_run -- the absent entries between
        the last present k-gram of a document and entry [bins], at least."""
        kk = max(k, 1)
        out = {"ends_at_level": set(), "leave_widths": set(), "no_shrink": False, "clamp": False, "short_document": False,
               "max_depth": 0}
        if pairs:
            out.update(empty_run=0, last_text_gram=False, tail_run=0)
        seen = set()
        suffixes = []
        for q in self.keyphrases():
            b = _key(q)
            for i in range(0, len(b), 4):
                if b[i:] not in seen:
                    seen.add(b[i:])
                    suffixes.append(b[i:])
        for d in self.model_docs:
            doc = self.document(d)
            get = doc.counts.get
            if pairs:
                present = self.present_codes(d, k)
                bins = self.A ** k
                out["tail_run"] = max(out["tail_run"], bins - 1 - int(present[-1]))
                digits = [(present // self.A ** i) % self.A for i in range(k)]
                all_text = np.logical_and.reduce([(x >= 1) & (x <= self.sigma_t) for x in digits])
                last_text = int(present[all_text][-1]) if all_text.any() else -1
            for b in suffixes:
                n = len(b) // 4
                prev = None
                for j in range(1, min(n, doc.L) + 1):
                    f = get(b[:4 * j], 0)
                    if f == 0:
                        if j == 1 or prev:
                            out["ends_at_level"].add(j)
                        break
                    out["max_depth"] = max(out["max_depth"], j)
                    if prev is not None and f == prev:
                        out["no_shrink"] = True
                    if j == kk and n > j:
                        out["leave_widths"].add(min(f, 6))
                    if j >= kk and n > j and f <= WALK_ENDGAME:
                        if doc.n < WALK_ENDGAME:
                            out["short_document"] = True
                        elif not out["clamp"] and doc.m + f <= 3 and self._starts_in_last_ranks(doc, b[:4 * j], f):
                            out["clamp"] = True
                    if pairs and j == k:
                        g = 0
                        for c in np.frombuffer(b[:4 * k], dtype="<u4"):
                            g = g * self.A + self.code(int(c))
                        at = int(np.searchsorted(present, g))
                        assert present[at] == g, "a k-gram the model counts is no k-gram of a suffix"
                        nxt = int(present[at + 1]) if at + 1 < present.size else bins
                        out["empty_run"] = max(out["empty_run"], nxt - g - 1)
                        out["last_text_gram"] |= g == last_text
                    prev = f
        return out

    @staticmethod
    def _starts_in_last_ranks(doc, ub, f):
        """Whether the suffixes that start with u (f of them) begin within the last 3 ranks: the terminators sort above all
        text, so that is m + f + (text suffixes above every one that starts with u) <= 3."""
        u = list(np.frombuffer(ub, dtype="<u4"))
        above = 0
        inf = 1 << 40
        for s in doc.strings:
            for i in range(len(s)):
                t = s[i:i + len(u)]
                t = t + [inf] * (len(u) - len(t))           # (the terminator, then nothing that matters)
                if t > u:
                    above += 1
        return doc.m + f + above <= 3


def expect_for(k, sigma_t, pairs=False, families=True):
    """What a mixed collection over sigma_t letters shows for tables of depth k."""
    e = {"ends_at_level": set(range(1, k + 2)), "leave_widths": set(ALL_WIDTHS)}
    if sigma_t >= 2:
        # (one letter: f(a^j) falls strictly with j, and every interval starts at rank 0)
        e.update(no_shrink=True, clamp=True)
    if pairs:
        e.update(empty_run=sigma_t + 2, last_text_gram=True, tail_run=1)
    return e


def small_k(sigma_t, n, n_docs):
    """The depth of the tables the score side builds itself (csrc/score_host.h: ensure_kgram): at most 3 levels, at most
    65 536 entries, 16 entries per symbol of an average document + 4 096."""
    A, k, bins = sigma_t + 2, 0, 1
    if sigma_t > 254:
        return 0
    while k < 3 and bins * A <= 65536 and bins * A * 16 <= n // n_docs + 4096:
        bins *= A
        k += 1
    return k


def marked_k(sigma_t, n, n_docs):
    """The depth of the tables the build marks off its window keys (csrc/build.h): at most 4 levels, at most 2^20 entries,
    two entries per symbol of an average document + 4 096."""
    A, k, bins = sigma_t + 2, 0, 1
    while k < 4 and bins * A <= 1048576 and bins * A <= 2 * (n // n_docs) + 4096:
        bins *= A
        k += 1
    return k


def _size(docs):
    return sum(len(s) + 1 for doc in docs for s in doc)


def extra_untagged(a):
    """Keyphrases that hold a terminator code point or a value that is no code point: both are absent symbols."""
    return [[TERMINATOR_START], [a, TERMINATOR_START], [a, a, TERMINATOR_START + 1, a], [TERMINATOR_START + 7, a],
            [0x110000], [a, 0x110000, a], [a, 0xFFFFFFFF], [a, a, a, TERMINATOR_TAG]]


def _exhaustive_L(sigma_t, k):
    """k + 2 where that stays below about 20 000 keyphrases, else k + 1."""
    count = lambda L: sum((sigma_t + 1) ** n for n in range(1, L + 1))
    return k + 2 if count(k + 2) < 20000 else k + 1


def mixed_documents(rng, alphabet, k, size=300):
    docs = [random_text(rng, alphabet, size), markov_text(rng, alphabet, size), one_letter(alphabet[0]),
            period3(rng, alphabet, size)]
    docs += tiny_documents(alphabet) + ladder_documents(alphabet, k)
    if len(alphabet) >= 2:
        docs += clamp_documents(alphabet, k)
    return docs


def _small_case(name, docs, expect=None, **kw):
    sigma_t = len(set(c for doc in docs for s in doc for c in s))
    k = small_k(sigma_t, _size(docs), len(docs))
    a = min(c for doc in docs for s in doc for c in s)
    kw.setdefault("extra", extra_untagged(a))
    return Case(name, docs, _exhaustive_L(sigma_t, k), [(k, False)], expect_for(k, sigma_t) if expect is None else expect(k), **kw)


_cases = {}


def _build_small_cases():
    out = []
    # the families mixed in one collection, over every alphabet (several documents: the tiled marking kernel)
    for sigma in (1, 2, 3, 4, 6, 14):
        rng = np.random.default_rng(1000 + sigma)
        k = {1: 3, 2: 3, 3: 3, 4: 3, 6: 2, 14: 2}[sigma]
        docs = mixed_documents(rng, letters(sigma), k, size=600 if sigma == 14 else 300)
        case = _small_case("mixed_sigma%d" % sigma, docs)
        assert case.plans == [(k, False)], (case.plans, k)
        if k <= 2:
            case.expect["short_document"] = True          # (tables of 3 levels end every walk in a document of 3 symbols)
        out.append(case)
    # every family alone; one document: kgram_mark_kernel
    rng = np.random.default_rng(2001)
    out.append(_small_case("random_alone", [random_text(rng, letters(3), 400)],
                           lambda k: {"ends_at_level": set(range(1, k + 2)), "leave_widths": {6}, "no_shrink": True}))
    out.append(_small_case("markov_alone", [markov_text(rng, letters(3), 400)],
                           lambda k: {"ends_at_level": set(range(1, k + 2)), "leave_widths": {6}, "no_shrink": True}))
    out.append(_small_case("one_letter_alone", [one_letter(FIRST_LETTER)],
                           lambda k: {"ends_at_level": set(range(1, k + 2)), "leave_widths": {6}, "max_depth": 5}))
    out.append(_small_case("period3_alone", [period3(rng, letters(2), 300, mean=1 << 20)],     # (one string)
                           lambda k: {"ends_at_level": set(range(1, k + 2)), "leave_widths": {6}, "no_shrink": True}))
    out.append(_small_case("tiny_alone_sigma2", tiny_documents(letters(2)),
                           lambda k: {"ends_at_level": {1, 2, 3}, "max_depth": 3}))
    out.append(_small_case("tiny_alone_sigma6", tiny_documents(letters(6)) + [[letters(6)]],
                           lambda k: {"ends_at_level": {1, 2, 3}, "short_document": True, "leave_widths": {1}}))
    # 70 documents, no multiple of 8: the XCD-aware order with a ragged last group
    rng = np.random.default_rng(2070)
    docs = [random_text(rng, letters(2), int(rng.integers(20, 120)), mean=6) for _ in range(56)]
    docs += tiny_documents(letters(2)) + ladder_documents(letters(2), 3) + clamp_documents(letters(2), 3) + [one_letter(FIRST_LETTER)]
    assert len(docs) == 70
    out.append(_small_case("seventy_documents", docs))
    # one long document over two letters: n / n_docs >= 256 bins -- the table entries by binary search.  (By DC3: the window
    # sort takes random text over two letters for repetitive, whatever its size, and then marks the tables itself.)
    rng = np.random.default_rng(2200)
    docs = [random_text(rng, letters(2), 20000, mean=40)]
    out.append(_small_case("search_kernel", docs, lambda k: {"ends_at_level": set(range(1, k + 2)), "leave_widths": {6}}))
    out[-1].window_sort = 0
    # more than 254 text symbols: the u32 symbol stream, no tables (k = 0), binary search + the u32 endgame
    rng = np.random.default_rng(2300)
    three = [0x30, 0x32, 0x34]
    fillers = [0x100 + 2 * i for i in range(252)]
    body = list(rng.choice(three, size=700))
    for i, c in enumerate(fillers):
        body.insert(int(rng.integers(0, len(body) + 1)), c)
    docs = [cut(rng, body, 12)] + tiny_documents(three) + clamp_documents(three, 1) + ladder_documents(three, 1)
    kp = all_keyphrases(three + [fillers[100], 0x31], 4) + extra_untagged(0x30)
    out.append(Case("u32_symbols", docs, 4, [(0, False)],
                    {"ends_at_level": {1, 2, 3, 4}, "leave_widths": set(ALL_WIDTHS), "no_shrink": True, "clamp": True,
                     "short_document": True}, keyphrases=kp, absent=0x31))
    # text at or above U+0A00: the tagged encoding; query symbols above and below the base, present and absent
    rng = np.random.default_rng(2400)
    high = [0x41, 0x43, 0x0A02, 0x4E2D, 0x10FFFF]
    docs = mixed_documents(rng, high, 2, size=300)
    kp = all_keyphrases(high + [0x42], 4) + all_keyphrases([0x0A02, 0x4E2D, 0x0A03, 0x0A00], 3) + \
        [[0x110000], [0x41, 0x110000, 0x41], [0x41, 0xFFFFFFFF], [0x41, TERMINATOR_TAG], [0x10FFFF, 0x10FFFE], [0x09FF, 0x0A02]]
    case = Case("tagged", docs, 4, [(2, False)], expect_for(2, 5), tagged=True, keyphrases=kp, absent=0x42)
    case.expect["short_document"] = True
    assert small_k(5, _size(docs), len(docs)) == 2           # (A = 7: 343 entries x 16 > 4 096 + a document's symbols)
    out.append(case)
    out.append(_packing_case())
    return out


PACK_BLOCK = 256                 # csrc: BLOCK, the suffixes of a workgroup of the walk


def _packing_case():
    """Keyphrases cut out of a periodic document: their lengths sum to 255, 256 and 257 suffixes per workgroup, one has
    exactly 256, the last has 1.  keyphrases(): all at most 256 long (the sums run inside the walk);
    with_long: the same + one of 257 (every sum falls back to the reduction kernel) + one of 1."""
    rng = np.random.default_rng(2500)
    ab = letters(2)
    unit = [ab[0], ab[1], ab[1]]
    body = (unit * 250)[:700]
    docs = [[body], random_text(rng, ab, 150, mean=20), [[ab[0]] * 300], tiny_documents(ab)[2]]
    lengths = [255, 200, 56, 200, 57, 256, 100, 100, 56, 1, 254, 2, 255, 1]
    kp = []
    for i, n in enumerate(lengths):
        start = (7 * i) % 50
        q = body[start:start + n]
        if i % 3 == 1:
            q = q[:-1] + [ab[0] + 1]                 # (ends in the absent symbol)
        kp.append(q)
    kp[6] = [ab[0]] * 100                            # (matches the one-letter document to the end)
    # (the window sort takes this text for repetitive and marks the tables itself, small as the input is: 4 levels, filled
    # layout -- pairs where they are forced)
    case = Case("packing", docs, PACK_BLOCK + 1, [(4, False), (4, True)],
                {"max_depth": PACK_BLOCK, "no_shrink": True, "leave_widths": {6}}, keyphrases=kp, model_L=PACK_BLOCK + 4)
    case.with_long = kp + [body[3:3 + PACK_BLOCK + 1], [ab[1]]]
    case.marked = True
    assert marked_k(2, _size(docs), len(docs)) == 4
    return case


def packing_blocks(lengths, block=PACK_BLOCK):
    """The suffixes per workgroup as set_keyphrases packs whole keyphrases (csrc/score_host.h), None if one is too long."""
    out, used = [], 0
    for n in lengths:
        if n > block:
            return None
        if used + n > block:
            out.append(used)
            used = 0
        used += n
    return out + [used]


def small_cases():
    if "small" not in _cases:
        _cases["small"] = _build_small_cases()
    return _cases["small"]


# ---- the collections just above the small-input limit of the window sort (the build marks the tables) ----
def sampled_keyphrases(docs, alphabet, absent, positions, seed):
    """Every 1- and 2-gram over the alphabet + the absent symbol; every distinct 3-, 4- and 5-gram at `positions` seeded
    places of the text, each also with its last symbol replaced by every other letter and by the absent symbol."""
    rng = np.random.default_rng(seed)
    syms = list(alphabet) + [absent]
    out = all_keyphrases(syms, 2)
    seen = set()
    strings = [s for doc in docs for s in doc if len(s) >= 5]
    for _ in range(positions):
        s = strings[int(rng.integers(0, len(strings)))]
        i = int(rng.integers(0, len(s) - 4))
        for n in (3, 4, 5):
            head = s[i:i + n - 1]
            for c in syms:
                q = tuple(head + [c])
                if q not in seen:
                    seen.add(q)
                    out.append(list(q))
    return out


def _skewed(sigma):
    p = 1.0 / np.sqrt(np.arange(sigma) + 1.0)
    return p / p.sum()


def _build_marked_cases():
    out = {}
    ab = letters(6)
    # 17 documents x 4 200 symbols over 6 letters + the small ones: A = 8, k = 4 marked (4 096 bins), k = 2 where the score
    # side builds the tables itself (512 entries x 16 > 4 096 + the symbols of an average document)
    rng = np.random.default_rng(3000)
    docs = [random_text(rng, ab, 4200, mean=12, p=_skewed(6) if i % 2 else None) for i in range(17)]
    docs += tiny_documents(ab) + ladder_documents(ab, 4) + ladder_documents(ab, 2) + clamp_documents(ab, 4) + clamp_documents(ab, 2)
    n, D = _size(docs), len(docs)
    assert n > 65536 and marked_k(6, n, D) == 4 and small_k(6, n, D) == 2 and D >= 16
    e4, e3 = expect_for(4, 6, pairs=True), expect_for(2, 6)
    out["pairs"] = Case("pairs_17_documents", docs, 5, [(4, True), (4, False), (2, False)],
                        {(4, True): e4, (4, False): expect_for(4, 6), (2, False): e3}, extra=extra_untagged(ab[0]))
    # the same with a periodic and a one-letter document: long runs of empty buckets
    rng = np.random.default_rng(3100)
    docs = [random_text(rng, ab, 4200, mean=12) for i in range(15)]
    docs += [period3(rng, ab, 4200, mean=60), [[ab[2]] * 1500, [ab[2]] * 2500, [ab[2]] * 7]]
    docs += ladder_documents(ab, 4) + clamp_documents(ab, 4) + ladder_documents(ab, 2) + clamp_documents(ab, 2)
    n, D = _size(docs), len(docs)
    assert n > 65536 and marked_k(6, n, D) == 4 and small_k(6, n, D) == 2 and D >= 16
    e = expect_for(4, 6, pairs=True)
    e["empty_run"] = 256                             # (the mixed collection: A; here runs of half a third-level bucket)
    out["pairs_runs"] = Case("pairs_periodic_and_one_letter", docs, 5, [(4, True), (2, False)],
                             {(4, True): e, (2, False): expect_for(2, 6)}, extra=extra_untagged(ab[0]))
    # fewer than 16 documents: the filled table, by chunks
    rng = np.random.default_rng(3200)
    docs = [random_text(rng, ab, 23800, mean=12, p=_skewed(6) if i == 1 else None) for i in range(2)]
    docs.append(markov_text(rng, ab, 23800, mean=400))       # (forbidden bigrams: whole stretches of the last level stay empty)
    n, D = _size(docs), len(docs)
    assert n > 65536 and marked_k(6, n, D) == 4 and small_k(6, n, D) == 3
    e = {"ends_at_level": {1, 2, 3, 4, 5}, "leave_widths": set(ALL_WIDTHS), "no_shrink": True}
    e3 = {"ends_at_level": {1, 2, 3, 4}, "leave_widths": {6}}    # (the score side's own tables: long documents, 3 levels)
    ep = dict(e, empty_run=8, last_text_gram=True, tail_run=1)      # (mode 4 forces the pair layout on it)
    out["chunks"] = Case("chunks_3_documents", docs, 5, [(4, False), (4, True), (3, False)],
                         {(4, False): e, (4, True): ep, (3, False): e3}, extra=extra_untagged(ab[0]))
    return out


def marked_cases():
    if "marked" not in _cases:
        _cases["marked"] = _build_marked_cases()
    return _cases["marked"]


def _large_case(name, sigma, n, seed, plans):
    rng = np.random.default_rng(seed)
    ab = letters(sigma)
    docs = [random_text(rng, ab, n, mean=60, p=_skewed(sigma))]
    kp = sampled_keyphrases(docs, ab, ab[3] + 1, 2000, seed + 1)
    e = {}
    for k, pairs in plans:
        e[(k, pairs)] = {"ends_at_level": set(range(1, k + 2)), "leave_widths": set(ALL_WIDTHS) if k == 4 else {6}, "no_shrink": True}
        if pairs:
            e[(k, pairs)].update(empty_run=sigma + 2, tail_run=1)
    case = Case(name, docs, 5, plans, e, keyphrases=kp + extra_untagged(ab[0]), absent=ab[3] + 1, model_L=6)
    for k, _ in plans:
        assert k in (marked_k(sigma, _size(docs), 1), small_k(sigma, _size(docs), 1)), (name, k)
    return case


def large_case(which):
    """chunks_274: one document of 140 000 symbols over 21 letters -- A = 23, k = 4, 279 841 bins = 274 chunks of the
    filled layout.  bins_limit: one document of 530 000 symbols over 30 letters -- A = 32, k = 4, bins = 2^20 = the limit
    exactly, the upper tables (1 058 words per document) too long for the LDS."""
    if which not in _cases:
        if which == "chunks_274":
            _cases[which] = _large_case("chunks_274", 21, 140000, 4000, [(4, False), (2, False)])
        else:
            _cases[which] = _large_case("bins_limit", 30, 530000, 5000, [(4, True), (3, False)])
    return _cases[which]
