# -*- coding: utf-8 -*-
"""An exact host model of phrase extraction (include/east_hip.h, "Phrase extraction"), and the generated
collections that tests/test_phrases_host.py (CPU) and tests/test_gpu_phrases.py (GPU) share.  A plain module: no test, no
fixture.

The model is a dict from word tuple to occurrence list, built text by text, up to `longest` = max_words + 1 words: count,
texts, first, closedness and the order are the contract's own words.  It shares the tokenizer with cosine_exact
(all_tokens, MIN_LEN, prepared_stopwords) and nothing with sorting or naming: no ids, no levels, no keys.
"""
import functools
import random

import numpy as np

from cosine_exact import MIN_LEN, all_tokens, prepared_stopwords

MAX_WORDS = 8


class Expected(object):
    """What a build and its fetch must give, field for field (hip_backend.PhraseArrays)."""

    def __init__(self, rows, candidates, levels, domain, survivors):
        self.strings = [" ".join(g) for g, _, _, _, _, _ in rows]
        self.words = np.array([len(g) for g, _, _, _, _, _ in rows], dtype=np.int32)
        self.count = np.array([c for _, c, _, _, _, _ in rows], dtype=np.int32)
        self.texts = np.array([t for _, _, t, _, _, _ in rows], dtype=np.int32)
        self.first = np.array([f for _, _, _, f, _, _ in rows], dtype=np.int32)
        self.first_text = np.array([d for _, _, _, _, d, _ in rows], dtype=np.int32)
        self.term_ids = np.array([i for _, _, _, _, _, ids in rows for i in ids], dtype=np.int32)
        self.text_off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.strings], out=self.text_off[1:])
        self.text = np.frombuffer("".join(self.strings).encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.uint32)
        self.candidates, self.levels = candidates, levels
        self.domain = np.array(domain + [0] * (MAX_WORDS - len(domain)), dtype=np.int64)
        self.survivors = np.array(survivors + [0] * (MAX_WORDS - len(survivors)), dtype=np.int64)

    def tuples(self):
        return list(zip(self.strings, self.words.tolist(), self.count.tolist(), self.texts.tolist(), self.first.tolist()))


class PhraseModel(object):
    """The phrases of one collection up to `longest` words: extract() answers for every max_words < longest."""

    def __init__(self, texts, stopwords=(), longest=MAX_WORDS + 1):
        stop = prepared_stopwords(stopwords)
        self.longest = longest
        self.term_id = {}
        occ = {}                                        # word tuple -> [(position, text)], positions ascending
        base = 0
        for d, text in enumerate(texts):
            kept = [t for t in all_tokens(text) if len(t) >= MIN_LEN]
            for i, t in enumerate(kept):
                if t in stop:
                    continue
                self.term_id.setdefault(t, len(self.term_id))
                for n in range(1, longest + 1):
                    if i + n > len(kept) or kept[i + n - 1] in stop:
                        break                           # (no phrase contains a break, none leaves its text)
                    occ.setdefault(tuple(kept[i:i + n]), []).append((base + i, d))
            base += len(kept)
        self.kept_tokens = base
        self.phrases = list(occ)
        index = {g: k for k, g in enumerate(self.phrases)}
        self.n = np.array([len(g) for g in self.phrases], dtype=np.int64)
        self.count = np.array([len(occ[g]) for g in self.phrases], dtype=np.int64)
        self.texts = np.array([len(set(d for _, d in occ[g])) for g in self.phrases], dtype=np.int64)
        self.first = np.array([occ[g][0][0] for g in self.phrases], dtype=np.int64)
        self.first_text = np.array([occ[g][0][1] for g in self.phrases], dtype=np.int64)
        # an extension of g by one word, in front or behind, with the count of g
        self.extended = np.zeros(len(self.phrases), dtype=bool)
        # the count of the phrase without its last word (what decides whether an occurrence is looked at on the next level)
        self.prefix_count = np.zeros(len(self.phrases), dtype=np.int64)
        for k, g in enumerate(self.phrases):
            if len(g) > 1:
                for shorter in (g[:-1], g[1:]):
                    if self.count[index[shorter]] == self.count[k]:
                        self.extended[index[shorter]] = True
                self.prefix_count[k] = self.count[index[g[:-1]]]

    def extract(self, n=0, max_words=3, min_words=1, min_count=2, min_texts=1):
        assert max_words < self.longest
        # (an extension of n + 1 <= max_words words is in the dict: longest > max_words)
        closed = (self.n == max_words) | ~self.extended
        is_candidate = ((self.n >= min_words) & (self.n <= max_words) & (self.count >= min_count) & (self.texts >= min_texts) & closed)
        chosen = np.flatnonzero(is_candidate)
        score = self.count[chosen] * self.n[chosen]
        order = chosen[np.lexsort((self.first[chosen], self.n[chosen], -score))]
        cut = order[:n] if n else order
        rows = [(self.phrases[k], int(self.count[k]), int(self.texts[k]), int(self.first[k]), int(self.first_text[k]),
                 [self.term_id[w] for w in self.phrases[k]]) for k in cut.tolist()]
        domain, survivors = [], []
        for level in range(1, max_words + 1):
            at = self.n == level
            looked_at = at if level == 1 else at & (self.prefix_count >= min_count)
            domain.append(int(self.count[looked_at].sum()))
            survivors.append(int((at & (self.count >= min_count)).sum()))
            if survivors[-1] == 0:
                break
        return Expected(rows, int(order.size), len(domain), domain, survivors)


def check(found, expected, what=""):
    """Every fetched array byte-equal with the model."""
    assert found.strings() == expected.strings, (what, found.strings()[:5], expected.strings[:5])
    for name in ("words", "count", "texts", "first", "first_text", "term_ids", "text_off", "text", "domain", "survivors"):
        got, want = getattr(found, name), getattr(expected, name)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, name, got[:8], want[:8])
    assert (found.candidates, found.levels) == (expected.candidates, expected.levels), (what, found.candidates, found.levels)


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------
HEADER_EXAMPLE = ["abc bcd cde abc bcd cde abc bcd cde abc bcd"]
HEADER_EXPECTED = [("ABC BCD CDE", 3, 3, 1, 0), ("BCD CDE ABC", 3, 3, 1, 1), ("CDE ABC BCD", 3, 3, 1, 2), ("ABC BCD", 2, 4, 1, 0)]
REPEATS = (5, 256, 257, 4097)                       # a run across a workgroup and across a scan tile of 4 096


def one_word(times):
    return [" ".join(["aaa"] * times)]


def two_word_period(times=300):
    return [" ".join(["tick", "tock"] * times)]


def boundary_collections():
    """{name: (texts, stopwords)}."""
    seventy = ["only%d here shared phrase tail%d" % (d, d) for d in range(70)]
    return {
        "last and first token of neighbours": (["left middle edge", "next left middle edge", "next other"], ()),
        "empty and short-token texts between": (["red green blue", "", "a bc de", "red green blue", "", "to be", "green blue red green"], ()),
        "one text": (["solo piece solo piece solo"], ()),
        "seventy texts beside three hundred in one": (seventy + [" ".join(["inner loop"] * 300)], ()),
        "a word over three texts": ([" ".join(["www"] * 1500), " ".join(["www"] * 2000), " ".join(["www"] * 597)], ()),
    }


def break_collections():
    stop = ("the", "and")
    return {
        "stopwords inside, in front and behind": (["the quick fox and quick fox the the quick fox", "quick the fox quick fox and"], stop),
        "stopwords only": (["the and the", "and and the"], stop),
        "no kept token": (["a bc", "", "to be or"], stop),
        "one empty text": ([""], ()),
    }


@functools.lru_cache(maxsize=None)
def zipf_collection(tokens=20000, vocabulary=300, n_texts=16, seed=7):
    """About `tokens` tokens over `vocabulary` words, Zipf-distributed, in texts of uneven size; short tokens and the
    stopwords ("w000", "w001": the two most frequent words) in between."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocabulary + 1)
    ids = rng.choice(vocabulary, size=tokens, p=p / p.sum())
    cuts = np.sort(rng.choice(np.arange(1, tokens), size=n_texts - 1, replace=False))
    texts = []
    for part in np.split(ids, cuts):
        words = ["w%03d" % i for i in part.tolist()]
        for k in range(7, len(words), 23):
            words.insert(k, "ab")
        texts.append(" ".join(words))
    return texts, ("w000", "w001")


@functools.lru_cache(maxsize=None)
def ties_collection():
    """Dozens of candidates of one score across different n: six occurrences of single words, three of pairs, two of
    triples -- score 6 each --, kept apart by fillers that occur once."""
    rng = random.Random(5)
    units, filler = [], iter("f%04d" % i for i in range(100000))
    for k in range(12):
        units += [["single%d" % k]] * 6 + [["pair%da" % k, "pair%db" % k]] * 3 + [["tri%da" % k, "tri%db" % k, "tri%dc" % k]] * 2
    rng.shuffle(units)
    third = len(units) // 3                             # (the texts are cut between units)
    texts = []
    for part in (units[:third], units[third:2 * third], units[2 * third:]):
        texts.append(" ".join(w for u in part for w in u + [next(filler)]))
    return texts, ()


@functools.lru_cache(maxsize=None)
def wide_collection(words=70000):
    """`words` distinct words in a row, twice: every pair of neighbours occurs twice; term ids need more than 16 bits and the packed
    key of level 2 more than 32."""
    half = ["v%05d" % i for i in range(words)]
    return [" ".join(half), " ".join(half)], ()
