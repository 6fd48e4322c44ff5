# -*- coding: utf-8 -*-
"""An exact host model of the cosine term index (include/east_hip.h, "The cosine relevance measure"), and
the generated collections that tests/test_cosine_exact_host.py (CPU) and tests/test_gpu_cosine_differential.py (GPU)
share.  A plain module: no test, no fixture, nothing of east.relevance and nothing of test_cosine_host.restate.

`build_model(texts, stopwords, stemmer)` goes from raw texts to

  * the kept tokens of every document: east.utils.prepare_text + east.utils.tokenize (the contract the device tables are
    derived from) and, written out here, "at least 3 code points, not a stopword";
  * the integer structures the index is specified to hold: the terms in first-occurrence order, `kept tokens` and
    `distinct words` (both with the stopwords included), the postings {(term, document): count}, n_d, df; with a
    stemmer the class map (classes numbered by their smallest term id) and the merged postings;
  * K x D scores in high precision (Model.scores_from_ids / Model.scores).

What is exact and what is rounded in a score.  With c_u the count of unit u in the query, n_ud its count in document d
and idf_u = 1 + ln(D / df_u) (1 under tf), the contract's dot / (|w_d| |q|) is

    sum_u c_u n_ud idf_u  /  sqrt( (sum_u n_ud^2 idf_u^2) * (sum_u c_u^2) )

-- n_d and the query's length cancel.  Exact (Python integers): every count, n_d, df, the products c_u n_ud, the sums of
n_ud^2 over the units of one df, sum c_u^2, and under tf the whole numerator and the whole radicand.  Rounded to 50
decimal digits (mpmath, a context of this module's own): ln, idf^2, the products of an integer with idf or idf^2, their
sums (at most one term per distinct df), the square root and the quotient -- each 1e-50 relative, a few dozen of them per
score.  Then ONE rounding to double.  The result is the correctly rounded score unless the exact value lies within
1e-48 relative of a rounding boundary: its error is 0.5 ulp (+ 1e-48), against tolerances of 1e-12 and of >= 97 ulp.

`fast=True` takes the integer-coded path for collections of MiB: the words are numbered through a dict and everything
else is numpy on the numbers.  It gives the same Model (test_cosine_exact_host pins it to the slow path).
"""
import functools
import random
from collections import Counter

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50
MIN_LEN = 3                                    # tokenize_and_filter's min_word_length
ULP = 2.0 ** -52
ABS_TOL = 1e-12                                # README: "Scores agree with the reference to 1e-12"
REL_EXTRA_ULPS = 32                            # log, sqrt, the divisions ("How it is tested")


class ToyStemmer(object):
    """tools/gen_cosine_golden.py's toy stemmer, restated: lower case, then a final ING or S stripped."""

    def stem(self, token):
        t = token.lower()
        for suffix in ("ing", "s"):
            if t.endswith(suffix) and len(t) > len(suffix) + 1:
                return t[:-len(suffix)]
        return t


def all_tokens(text):
    """Every [\\w']+ token of the prepared text, short ones included."""
    from east import utils
    return utils.tokenize(utils.prepare_text(text))


def prepared_stopwords(stopwords):
    from east import utils
    return frozenset(utils.prepare_text(w) for w in stopwords)


class Model(object):
    """The index of one collection.  Fields named after hip_backend.COSINE_INFO_FIELDS where they are one:
    n_docs, kept_tokens, words, terms (the list; len = the field), n_d[d], df[t], counts[d] = {term: count} in ascending
    term order, postings; with a stemmer term_class[t], n_classes, stem_class {stem: class}, cls_counts[d], cls_df,
    cls_postings."""

    def __init__(self):
        self.stemmer = None
        self.n_classes = 0
        self._idf = {}
        self._inv = {}
        self._rad = {}

    # ---- the integer structures --------------------------------------------------------------------------------------
    def _finish(self, stemmer):
        self.term_id = {t: i for i, t in enumerate(self.terms)}
        assert len(self.term_id) == len(self.terms)
        self.postings = sum(len(c) for c in self.counts)
        self.stemmer = stemmer
        if stemmer is not None:
            self.stem_class = {}
            self.term_class = [self.stem_class.setdefault(stemmer.stem(t), len(self.stem_class)) for t in self.terms]
            self.n_classes = len(self.stem_class)
            self.cls_counts = [merge_classes(c, self.term_class) for c in self.counts]
            self.cls_df = unit_df(self.cls_counts, self.n_classes)
            self.cls_postings = sum(len(c) for c in self.cls_counts)
        return self

    def structures(self):
        """Everything integer, for the comparison of the two paths."""
        s = dict(n_docs=self.n_docs, kept_tokens=self.kept_tokens, words=self.words, terms=self.terms, n_d=list(self.n_d),
                 df=list(self.df), counts=[list(c.items()) for c in self.counts], postings=self.postings)
        if self.stemmer is not None:
            s.update(term_class=list(self.term_class), n_classes=self.n_classes, cls_df=list(self.cls_df),
                     cls_counts=[list(c.items()) for c in self.cls_counts], cls_postings=self.cls_postings)
        return s

    def with_classes(self, term_class, n_classes):
        """A copy whose classes are the given map (east_hip_cosine_set_classes without a stemmer)."""
        m = Model()
        m.__dict__.update(self.__dict__)
        m._idf, m._inv, m._rad = {}, {}, {}
        m.term_class, m.n_classes = list(term_class), n_classes
        m.cls_counts = [merge_classes(c, m.term_class) for c in m.counts]
        m.cls_df = unit_df(m.cls_counts, n_classes)
        m.cls_postings = sum(len(c) for c in m.cls_counts)
        return m

    def space(self, stems):
        """(counts per document, df, units, postings) of a vector space."""
        if stems:
            return self.cls_counts, self.cls_df, self.n_classes, self.cls_postings
        return self.counts, self.df, len(self.terms), self.postings

    def info(self, stems=False):
        """The fields of east_hip_cosine_info that do not depend on the run."""
        return {"built": 1, "n_docs": self.n_docs, "kept_tokens": self.kept_tokens, "words": self.words,
                "terms": len(self.terms), "classes": self.n_classes if stems else 0,
                "postings": self.cls_postings if stems else self.postings}

    def postings_per_doc(self, stems=False):
        return [len(c) for c in self.space(stems)[0]]

    # ---- queries -------------------------------------------------------------------------------------------------------
    def query_tokens(self, prepared_query):
        return [t for t in all_tokens(prepared_query) if len(t) >= MIN_LEN and t not in self.stop]

    def query_ids(self, prepared_queries, stems=False):
        """Per query: its kept tokens as ids of the vector space, -1 outside it."""
        out = []
        for q in prepared_queries:
            tokens = self.query_tokens(q)
            if stems:
                out.append([self.stem_class.get(self.stemmer.stem(t), -1) for t in tokens])
            else:
                out.append([self.term_id.get(t, -1) for t in tokens])
        return out

    # ---- scores --------------------------------------------------------------------------------------------------------
    def idf(self, df, tfidf):
        if not tfidf:
            return 1
        if df not in self._idf:
            self._idf[df] = 1 + MP.log(MP.mpf(self.n_docs) / df)
        return self._idf[df]

    def _inverted(self, stems):
        if stems not in self._inv:
            inv = {}
            for d, c in enumerate(self.space(stems)[0]):
                for u, n in c.items():
                    inv.setdefault(u, []).append((d, n))
            self._inv[stems] = inv
        return self._inv[stems]

    def _radicands(self, stems, tfidf):
        """Per document: sum_u n_ud^2 idf_u^2 -- integer sums per distinct df, then one product and one term per df."""
        key = (stems, tfidf)
        if key not in self._rad:
            counts, df = self.space(stems)[:2]
            rad = []
            for c in counts:
                by_df = {}
                for u, n in c.items():
                    by_df[df[u]] = by_df.get(df[u], 0) + n * n
                if tfidf:
                    s = MP.mpf(0)
                    for f, sq in by_df.items():
                        s += sq * self.idf(f, True) ** 2
                else:
                    s = sum(by_df.values())
                rad.append(s)
            self._rad[key] = rad
        return self._rad[key]

    def scores_from_ids(self, q_ids, tfidf, stems=False):
        """K x D doubles: q_ids[k] = the ids of query k's kept tokens (-1 outside the vector space)."""
        df = self.space(stems)[1]
        inv, rad = self._inverted(stems), self._radicands(stems, tfidf)
        out = np.zeros((len(q_ids), self.n_docs), dtype=np.float64)
        rows = {}
        for k, ids in enumerate(q_ids):
            c = Counter(int(i) for i in ids if i >= 0)
            if not c:
                continue
            key = tuple(sorted(c.items()))
            if key not in rows:
                q2 = sum(n * n for n in c.values())
                num = {}
                for u, cu in key:
                    f = self.idf(df[u], tfidf)
                    for d, n in inv.get(u, ()):
                        num[d] = num.get(d, 0) + cu * n * f
                docs = np.fromiter(num.keys(), dtype=np.int64, count=len(num))
                vals = np.array([float(v / MP.sqrt(MP.mpf(rad[d]) * q2)) for d, v in num.items()], dtype=np.float64)
                rows[key] = (docs, vals)
            docs, vals = rows[key]
            out[k, docs] = vals
        return out

    def scores(self, prepared_queries, space, weighting):
        stems = space == "stems"
        return self.scores_from_ids(self.query_ids(prepared_queries, stems), weighting == "tf-idf", stems)


def merge_classes(counts, term_class):
    """{term: count} -> {class: count}, ascending."""
    merged = {}
    for t, n in counts.items():
        merged[term_class[t]] = merged.get(term_class[t], 0) + n
    return dict(sorted(merged.items()))


def unit_df(counts, n_units):
    df = [0] * n_units
    for c in counts:
        for u in c:
            df[u] += 1
    return df


def build_model(texts, stopwords=(), stemmer=None, fast=False):
    m = Model()
    m.stop = prepared_stopwords(stopwords)
    m.n_docs = len(texts)
    kept = [[t for t in all_tokens(text) if len(t) >= MIN_LEN] for text in texts]
    m.kept_tokens = sum(len(k) for k in kept)
    if fast:
        number = {}
        codes = [np.fromiter((number.setdefault(t, len(number)) for t in k), dtype=np.int64, count=len(k)) for k in kept]
        by_number = list(number)
        m.words = len(by_number)
        non_stop = np.array([w not in m.stop for w in by_number], dtype=bool)
        term_of = np.where(non_stop, np.cumsum(non_stop) - 1, -1)          # first-occurrence order survives the removal
        m.terms = [w for w, keep in zip(by_number, non_stop.tolist()) if keep]
        m.n_d, m.counts = [], []
        df = np.zeros(len(m.terms), dtype=np.int64)
        for c in codes:
            t = term_of[c] if c.size else c
            t = t[t >= 0]
            m.n_d.append(int(t.size))
            u, n = np.unique(t, return_counts=True)
            df[u] += 1
            m.counts.append(dict(zip(u.tolist(), n.tolist())))
        m.df = df.tolist()
    else:
        m.words = len(set(t for k in kept for t in k))
        docs = [[t for t in k if t not in m.stop] for k in kept]
        order = {}
        for doc in docs:
            for t in doc:
                order.setdefault(t, len(order))
        m.terms = list(order)
        m.n_d = [len(doc) for doc in docs]
        m.counts = [dict(sorted(Counter(order[t] for t in doc).items())) for doc in docs]
        m.df = unit_df(m.counts, len(m.terms))
    return m._finish(stemmer)


# ---- the bounds of the gpu tier ----------------------------------------------------------------------------------------
def relative_bound_ulps(p_d, q_len):
    """slices of ceil(p_d / 64) squared weights, 64 partial sums, a dot product of at most q terms; 32 ulp for
    log, sqrt and the divisions."""
    return (np.ceil(np.asarray(p_d, dtype=np.float64) / 64.0)[None, :] + 64.0 + np.asarray(q_len, dtype=np.float64)[:, None]
            + REL_EXTRA_ULPS)


def score_errors(got, exact, p_d, q_len):
    """(largest absolute error, largest ratio of the relative error to its bound, the zero patterns agree)."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    if got.size == 0:
        return 0.0, 0.0, True
    err = np.abs(got - exact)
    bound = relative_bound_ulps(p_d, q_len) * ULP * exact
    nz = exact != 0.0
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    return float(err.max()), ratio, bool(np.array_equal(got == 0.0, exact == 0.0))


def check_scores(got, exact, p_d, q_len):
    abs_err, ratio, zeros = score_errors(got, exact, p_d, q_len)
    print("cosine scores %s: absolute error %.3g, relative error %.3g of its bound" % (np.shape(got), abs_err, ratio))
    assert np.isfinite(np.asarray(got)).all()
    assert zeros, "the zero pattern differs"
    assert abs_err <= ABS_TOL, abs_err
    assert ratio <= 1.0, "relative error %.3g of its bound" % ratio
    return ratio


# ---- generated collections (the same for both tiers) ---------------------------------------------------------------------
# the character pools of test_gpu_parity.test_device_text_preparation_fuzz, restated
FUZZ_CHARS = list("abcXYZ'_ 019,.-\n\t") + ["ß", "é", "Ж", "ж", "λ", "Σ", "ς", "٣", "²", "½", "ŉ", "ǅ", "ſ", "ı",
                                              "\U0001F600", "—", "’", "﻿", " ", "İ", "ͅ"]
FUZZ_JUNK = [b"\x80", b"\xbf", b"\xc0", b"\xc1\x81", b"\xc2", b"\xe0\x80", b"\xe0\xa0", b"\xe4\xb8", b"\xed\xa0\x80",
             b"\xf0\x90\x80", b"\xf4\x90\x80\x80", b"\xf5", b"\xff", b"\xe2\x82", b"\xf0\x9f\x98"]
FUZZ_HIGH = ["中", "文", "ก", "ข", "ệ", "ქ", "Ɐ", "한", "\U00010428", "๓", "ⅷ",
             "ᾳ"]
# case variants, sigmas, sharp s, titlecase digraph, dotted I, apostrophe-only and digit-only tokens, Arabic-Indic digits;
# tokens of exactly 2 and 3 code points of 1, 2, 3 and 4 bytes each
FUZZ_WORDS = ["Fox", "FOX", "fox", "σας", "σασ", "ΣΑΣ", "σ", "ς", "Σ", "ß", "ßßß", "straße", "ǅ", "ǅǅǅ", "İ", "İİİ", "'", "''",
              "'''", "''''", "12", "123", "007", "٣٤", "٣٤٥", "٣", "don't", "ab", "abc", "éé", "ééé", "中文",
              "中文中", "\U00010428\U00010428", "\U00010428\U00010428\U00010400", "tests", "testing", "test"]
ABSENT = ["ABSENT", "NOWHERE", "ЖЖЖЖ", "QQ"]
MODES = [(s, w) for s in ("words", "stems") for w in ("tf", "tf-idf")]


@functools.lru_cache(maxsize=None)
def fuzz_rounds(n_rounds=150, seed=20241):
    """[{texts, space, weighting, stopwords, queries}]: 1 to 6 texts a round, empty ones among them."""
    rng = random.Random(seed)
    rounds = []
    for it in range(n_rounds):
        pool = FUZZ_CHARS + FUZZ_HIGH if it % 3 == 2 else FUZZ_CHARS
        texts = []
        for _ in range(rng.randint(1, 6)):
            parts = []
            for _ in range(0 if rng.random() < 0.15 else rng.randint(0, 40)):
                r = rng.random()
                if r < 0.12:
                    parts.append(rng.choice(FUZZ_JUNK))
                elif r < 0.32:
                    parts.append((" " + rng.choice(FUZZ_WORDS) + " ").encode("utf-8"))
                else:
                    parts.append("".join(rng.choice(pool) for _ in range(rng.randint(1, 6))).encode("utf-8"))
            texts.append(b"".join(parts))
        tokens = sorted(set(t for text in texts for t in all_tokens(text))) or ["EMPTY"]
        space, weighting = MODES[rng.randrange(4)]
        stopwords = []
        if rng.random() < 0.5:
            stopwords = [rng.choice(tokens) for _ in range(rng.randint(1, 6))] + rng.sample(ABSENT, 2)
        queries = []
        for _ in range(rng.randint(4, 12)):
            words = []
            for _ in range(rng.randint(0, 5)):
                r = rng.random()
                words.append(rng.choice(ABSENT) if r < 0.15 else rng.choice(words) if r < 0.3 and words else rng.choice(tokens))
            queries.append(" ".join(words))
        rounds.append(dict(texts=texts, space=space, weighting=weighting, stopwords=stopwords, queries=queries))
    return rounds


PIECE_LENGTHS = (3, 2047, 2048, 2049, 4095, 4096, 4097, 6145)


def _alphabet_word(rng, alphabet, n):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n).tolist())


def _other(alphabet, c):
    return alphabet[(alphabet.index(c) + 1) % len(alphabet)]


@functools.lru_cache(maxsize=None)
def piece_collection():
    """(texts, families, near_misses).  Tokens of the PIECE_LENGTHS over ASCII and over 3-byte code points; per long length
    a family: the token, and the token with its first / 2 047th / 2 048th / last code point changed, its last dropped,
    one appended.  Spread over five documents in different orders and numbers."""
    rng = np.random.default_rng(11)
    alphabets = ([chr(c) for c in range(65, 91)], [chr(c) for c in range(0x4E00, 0x4E40)])
    families, near = [], []
    for alphabet in alphabets:
        for n in PIECE_LENGTHS:
            w = _alphabet_word(rng, alphabet, n)
            fam = [w]
            if n >= 2047:
                for pos in (0, 2046, 2047, n - 1):
                    if pos < n:
                        fam.append(w[:pos] + _other(alphabet, w[pos]) + w[pos + 1:])
                fam += [w[:-1], w + alphabet[0]]
                near += [w[:1000] + _other(alphabet, w[1000]) + w[1001:], w + alphabet[0] + alphabet[1], w[:-2], w[1:]]
            else:
                near += [w + alphabet[0], w[:-1] + _other(alphabet, w[-1])]
            families.append(list(dict.fromkeys(fam)))
    members = [w for fam in families for w in fam]
    texts = []
    for d in range(5):
        order = rng.permutation(len(members)).tolist()
        take = order[: len(order) * (d + 2) // 6] + (order[:7] if d % 2 else [])
        texts.append(" ".join(members[i] for i in take).encode("utf-8") if d != 3 else
                     ("short ab " + " ".join(members[i] for i in take) + " tail").encode("utf-8"))
    return texts, families, near


def piece_queries(families, near):
    return [fam[0] for fam in families] + [" ".join(fam[1:3]) for fam in families if len(fam) > 2] + near[:8] + \
        [families[0][0] + " " + families[1][0] + " " + families[0][0]]


@functools.lru_cache(maxsize=None)
def prefix_chain():
    """(texts, the chain): one token of 4 097 code points and 303 of its prefixes, each shorter than the one before it in
    the collection.  Whatever the hash, the first occurrence in a set of colliding tokens is their longest, and every other
    is a prefix of it: they differ from it in length ALONE."""
    rng = np.random.default_rng(15)
    w = _alphabet_word(rng, [chr(c) for c in range(65, 91)], 4097)
    chain = [w[:n] for n in [4097, 4096, 4095, 2049, 2048, 2047] + list(range(300, 2, -1))]
    return [" ".join(chain[:100]), "", " ".join(chain[100:]) + " " + chain[0][:5] + " " + chain[3]], chain


@functools.lru_cache(maxsize=None)
def stopword_case():
    """(stopword list, normal texts, queries, long words): the list holds an absent word, a word of 2 code points, an
    empty string, a duplicate, non-ASCII entries, an entry of 4 097 code points that is in the collection and one that
    is not."""
    rng = np.random.default_rng(12)
    letters = [chr(c) for c in range(65, 91)]
    long_in, long_out = _alphabet_word(rng, letters, 4097), _alphabet_word(rng, letters, 4097)
    stop = ["the", "and", "the", "", "of", "absentword", "Жук", "straße", "٣٤٥", long_in, long_out]
    texts = ["the cat and the dog жук " + long_in, "the and Жук the THE straße ٣٤٥ of " + long_in + " AND",
             "dogs and cats of the world " + long_in + " " + long_in[:-1], "", "cat cat dog the"]
    queries = ["THE CAT", "DOG AND CATS", long_in, long_in[:-1] + " WORLD", "ЖУК", "NOTHING", "CAT CAT DOG", "OF"]
    return stop, texts, queries, (long_in.upper(), long_out.upper())


def all_stop_texts():
    """Every kept word is a stopword of stopword_case()'s list."""
    return ["the and the", "Жук of the straße", "", "and ٣٤٥ a to"]


def degenerate_collections():
    """{name: texts}."""
    return {"all empty": ["", "", ""], "short tokens only": ["a bc de", "to be or", "12 ' é"], "one document": ["alpha beta alpha"],
            "one empty text alone": [""], "empty first and last": ["", "alpha beta gamma", "beta delta", ""],
            "two identical": ["same words here twice same", "same words here twice same"]}


DEGENERATE_QUERIES = ["ALPHA BETA", "SAME", "NOPE NOTHING", "BETA BETA DELTA AB"]


def three_documents():
    return ["alpha beta gamma delta alpha alpha epsilon", "beta gamma zeta eta theta beta", "iota alpha kappa lambda gamma mu nu"]


def id_queries(K, n_units, seed, q_max=3):
    """K queries of 1 to q_max ids in [-1, n_units) as (flat ids, offsets)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, q_max + 1, size=K)
    offsets = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return rng.integers(-1, n_units, size=int(offsets[-1])).astype(np.int32), offsets


def split_ids(ids, offsets):
    ids, offsets = np.asarray(ids).tolist(), np.asarray(offsets).tolist()
    return [ids[a:e] for a, e in zip(offsets[:-1], offsets[1:])]


def one_line_documents(D):
    """D one-line documents: EVERY sits in all of them, SECOND in every second one, a word of df 1 in each, and a word
    shared by the 7 documents of a group."""
    return [("every %s only%d group%d" % ("second" if d % 2 == 0 else "odd", d, d // 7)) for d in range(D)]


SLICE_POSTINGS = (0, 1, 63, 64, 65, 127, 128, 129, 4097)


def slice_documents():
    """Documents of exactly SLICE_POSTINGS postings (the 64 slices of the norm), with counts above 1 and shared words."""
    texts = []
    for i, p in enumerate(SLICE_POSTINGS):
        words = ["w%05d" % ((j * (i + 1)) % 5003) for j in range(p)]
        assert len(set(words)) == p
        texts.append(" ".join(words + words[: p // 3] + ["a", "of"]))
    return texts


SLICE_QUERIES = ["W00000", "W00001 W00002", "W00064 W00063 W00000 W00000", "W05002 NOPE", "W00003 W00128 W04096"]

SCAN_TILE = 4096                                 # elements a workgroup of the device's prefix sums takes (csrc/scan.h)
SCAN_TILE_SIZES = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 2 * SCAN_TILE + 1)
SCAN_TILE_STOP = ("the",)


def scan_tile_collections(n):
    """{name: (texts, stopwords)} whose counts lie at n: one document of n distinct words of six letters (tokens = kept
    tokens = words = terms = postings = n); the same with the stopword and a token of two letters in its middle (tokens
    n + 2, kept tokens and words n + 1, terms and postings n); the same words dealt over three documents."""
    words = ["w%05d" % j for j in range(n)]
    return {"one document": ([" ".join(words)], ()),
            "a stopword and a short token": ([" ".join(words[: n // 2] + ["the", "ab"] + words[n // 2:])], SCAN_TILE_STOP),
            "three documents": ([" ".join(words[i::3]) for i in range(3)], ())}


def scan_tile_queries(n):
    """The first and the last word, the two on either side of a tile, a stopword and a short token, a word that is absent."""
    return ["W00000", "W%05d" % (n - 1), "W%05d W%05d" % (SCAN_TILE - 1, min(SCAN_TILE, n - 1)), "THE AB W00001 W00001",
            "NOPE W00002 W%05d" % (n // 2)]


def _zipf_words(rng, size):
    """A vocabulary in Zipf rank order: random bases (east.synthetic.zipf_vocabulary), every fifth rank an -S or -ING
    variant of the base before it (classes with several members), every seventh base mapped to Cyrillic or Greek."""
    from east import synthetic
    vocab = synthetic.zipf_vocabulary(rng, size=size)
    words = []
    for i in range(size):
        a, n = int(vocab["starts"][i]), int(vocab["lens"][i])
        w = vocab["letters"][a:a + n].tobytes().decode()
        if i % 7 == 3:
            base = 0x0410 if i % 2 else 0x0391
            w = "".join(chr(base + (ord(c) - 65) % 17) for c in w)
        if i % 5 == 1:
            w = words[i - 1] + "S"
        elif i % 5 == 2:
            w = words[i - 2] + "ING"
        words.append(w)
    return list(dict.fromkeys(words)), vocab["cdf"]


@functools.lru_cache(maxsize=None)
def zipf_collection(n_docs=64, largest=1 << 20, smallest=1 << 10, vocabulary=5000, n_queries=2000, seed=13):
    """(texts, queries, the 50 most frequent words): documents of `smallest` to `largest` bytes, geometrically spread and
    shuffled; queries of 1 to 4 words: in the vocabulary, absent, frequent (the stopwords of half the modes)."""
    rng = np.random.default_rng(seed)
    words, cdf = _zipf_words(rng, vocabulary)
    sizes = np.geomspace(smallest, largest, n_docs)
    rng.shuffle(sizes)
    texts = []
    for size in sizes:
        ids = np.searchsorted(cdf, rng.random(max(1, int(size / 7.5))), side="left").clip(0, len(words) - 1)
        texts.append(" ".join(words[i] for i in ids.tolist()).encode("utf-8")[: int(size)])
    queries = []
    for _ in range(n_queries):
        q = []
        for _ in range(int(rng.integers(1, 5))):
            r = rng.random()
            if r < 0.15:
                q.append("ABSENT%d" % int(rng.integers(0, 50)))
            elif r < 0.3:
                q.append(words[int(rng.integers(0, 50))])
            elif r < 0.65:
                q.append(words[int(np.searchsorted(cdf, rng.random())) % len(words)])
            else:
                q.append(words[int(rng.integers(0, len(words)))])
        queries.append(" ".join(q))
    return texts, queries, words[:50]


@functools.lru_cache(maxsize=None)
def zipf_model(stop):
    """The model of zipf_collection() without stopwords or with its 50 most frequent words as stopwords; both vector
    spaces."""
    texts, _, top = zipf_collection()
    return build_model(texts, top if stop else (), ToyStemmer(), fast=True)


@functools.lru_cache(maxsize=None)
def two_mib_collection():
    """2 MiB in 24 texts (both entry points take it)."""
    rng = np.random.default_rng(14)
    words, cdf = _zipf_words(rng, 5000)
    texts = []
    for d in range(24):
        ids = np.searchsorted(cdf, rng.random(12500), side="left").clip(0, len(words) - 1)
        texts.append(" ".join(words[i] for i in ids.tolist()).encode("utf-8"))
    queries = [" ".join(words[int(i)] for i in rng.integers(0, 600, size=int(rng.integers(1, 4)))) for _ in range(200)]
    return texts, queries


def lookup_probes(model, texts, sample=300, seed=3):
    """(words that are terms, words that must give -1): every term up to 10^5 (a fixed-seed sample of 10^5 beyond); the
    stopwords, the empty word, the short words of the texts, and `sample` terms with the last code point changed, with
    one appended, with the last dropped."""
    rng = random.Random(seed)
    terms = model.terms if len(model.terms) <= 10 ** 5 else rng.sample(model.terms, 10 ** 5)
    absent = list(model.stop) + [""]
    absent += sorted(set(t for text in texts[:64] for t in all_tokens(text[: 1 << 16]) if len(t) < MIN_LEN))[:1000]
    for t in (model.terms if len(model.terms) <= sample else rng.sample(model.terms, sample)):
        for cand in [t[:-1] + r for r in ("Q", "Z", "Ω", "7")] + [t + "Q", t + "Ω", t[:-1]]:
            if cand not in model.term_id:
                absent.append(cand)
    return terms, absent
