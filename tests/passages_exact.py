"""The model of the shared passages (include/east_hip.h, "Shared passages"): per text the token list of cosine_exact's
tokenizer, S_b as a Python set of word tuples, and a plain loop over the positions of a.  It shares nothing with sorting,
naming or bit words."""
import functools

import numpy as np

import cosine_exact
import overlap_exact

MAX_WORDS = 8
STOP = overlap_exact.STOP


def token_lists(texts, stopwords=()):
    """Per text its kept tokens (at least 3 code points) in order, None where the token is a stopword: a position each."""
    stop = cosine_exact.prepared_stopwords(stopwords)
    return [[None if t in stop else t for t in cosine_exact.all_tokens(text) if len(t) >= cosine_exact.MIN_LEN] for text in texts]


def text_starts(tokens):
    """The collection position of every text's first token, and the number of positions behind the last."""
    starts = [0]
    for t in tokens:
        starts.append(starts[-1] + len(t))
    return starts


def shingle_at(tokens, j, w):
    """The shingle that starts at position j of a token list, or None where w words of the text do not start there."""
    g = tuple(tokens[j:j + w])
    return g if len(g) == w and None not in g else None


def pair_exact(tokens, a, b, w, min_words=None, per_pair=0, starts=None):
    """One ordered pair -> (starts, covered, found, [(start, words, at), ...]) in collection positions, the passages in the
    contract's order and cut, and the set of the distinct shingles at the shared starts."""
    min_words = w if min_words is None else min_words
    starts = starts or text_starts(tokens)
    ta, tb = tokens[a], tokens[b]
    first_in_b = {}
    for j in range(len(tb)):
        g = shingle_at(tb, j, w)
        if g is not None and g not in first_in_b:
            first_in_b[g] = j
    shared = [False] * (len(ta) + 1)
    distinct = set()
    for j in range(len(ta)):
        g = shingle_at(ta, j, w)
        if g is not None and g in first_in_b:
            shared[j] = True
            distinct.add(g)
    covered = set()
    passages = []
    j = 0
    while j < len(ta):
        if not shared[j]:
            j += 1
            continue
        m = 0
        while shared[j + m]:
            covered.update(range(j + m, j + m + w))
            m += 1
        passages.append((starts[a] + j, m + w - 1, starts[b] + first_in_b[shingle_at(ta, j, w)]))
        j += m
    kept = sorted((p for p in passages if p[1] >= min_words), key=lambda p: (-p[1], p[0]))
    return sum(shared), len(covered), len(kept), kept[:per_pair] if per_pair else kept, distinct


def exact(texts, stopwords, pairs, w, min_words=None, per_pair=0):
    """-> dict of the arrays east_hip_passages_fetch fills, as Python lists."""
    tokens = token_lists(texts, stopwords)
    starts = text_starts(tokens)
    out = {"pair_off": [0], "starts": [], "covered": [], "found": [], "start": [], "words": [], "at": [], "text_start": starts}
    for a, b in pairs:
        s, c, f, kept, _ = pair_exact(tokens, a, b, w, min_words, per_pair, starts)
        out["starts"].append(s)
        out["covered"].append(c)
        out["found"].append(f)
        for start, words, at in kept:
            out["start"].append(start)
            out["words"].append(words)
            out["at"].append(at)
        out["pair_off"].append(len(out["start"]))
    return out


def all_pairs(D):
    return [(a, b) for a in range(D) for b in range(D) if a != b]


# ---- collections --------------------------------------------------------------------------------------------------------------
WORKED = ("abc bcd cde def xyz bcd cde", "qqq bcd cde def rrr")        # the header's example, w = 2


def word(i, prefix="w"):
    return "%s%05d" % (prefix, i)


def fresh(n, prefix):
    """n words nobody else has."""
    return [word(i, prefix) for i in range(n)]


@functools.lru_cache(maxsize=None)
def bit_edge_texts():
    """w = 2.  Text 0 has 130 shingle positions, bits 0 .. 129 of its row.  Every other text shares with it ONE run of
    shared starts placed at an edge of the row's 64-bit words, so that every pair (0, partner) isolates one edge.
    -> (texts, {name: (partner, (first shared start, last shared start))})."""
    base = fresh(131, "b")                                  # 131 tokens: 130 shingle positions at w = 2
    runs = {"ends at bit 63": (60, 63), "starts at bit 0 of the second word": (64, 70), "crosses a word boundary": (50, 80),
            "bit 63 and bit 64 alone": (63, 64), "the last position": (120, 129), "the first position": (0, 0),
            "two words whole": (0, 127)}
    texts, cases = [" ".join(base)], {}
    for k, (name, (lo, hi)) in enumerate(sorted(runs.items())):
        own = fresh(3, "o%d" % k)
        texts.append(" ".join(own + base[lo:hi + 2] + own[::-1]))
        cases[name] = (k + 1, (lo, hi))
    return tuple(texts), cases


@functools.lru_cache(maxsize=None)
def length_texts():
    """Texts of 63, 64, 65, 127, 128 and 129 shingle positions at w = 2 (one token more each), all cut from one stream of
    distinct words at staggered offsets, so that every pair shares a long stretch."""
    stream = fresh(400, "s")
    texts = [" ".join(stream[5 * k:5 * k + n + 1]) for k, n in enumerate((63, 64, 65, 127, 128, 129))]
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def row_border_texts():
    """Text 0 has exactly 64 positions, a row of one word, and ends in two words that text 2 holds; text 1 begins with two
    that text 2 holds: the pairs (0, 2), (1, 2) in this order put a row whose bit 63 is a shared start (w = 1) in front of a
    row whose bit 0 is one."""
    a = fresh(62, "a") + ["end1", "end2"]
    b = ["beg1", "beg2"] + fresh(40, "c")
    return (" ".join(a), " ".join(b), "xxx end1 end2 yyy beg1 beg2 zzz")


@functools.lru_cache(maxsize=None)
def neighbours_texts():
    """w = 1: the last word of every text and the first of the next are both shared with the last text, at adjacent
    collection positions; no passage may cross from one text into the next."""
    return ("aaa bbb ccc", "ddd eee fff", "ccc ddd", "fff aaa ccc ddd")


@functools.lru_cache(maxsize=None)
def held_by_many_texts(D=300):
    """One 2-word shingle held by D texts (a long text list on route 1), each with words of its own around it; the last
    text holds it three times."""
    texts = ["%s common shingle %s" % (word(d, "l"), word(d, "r")) for d in range(D - 1)]
    texts.append("common shingle mid1 common shingle mid2 common shingle")
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def order_texts():
    """Text 0 shares with text 1 passages of 3, 5, 3, 2, 5 and 3 words at w = 2, separated by words of its own: equal
    lengths are ordered by start."""
    pieces, a = [], []
    for k, n in enumerate((3, 5, 3, 2, 5, 3)):
        piece = fresh(n, "p%d" % k)
        pieces.append(piece)
        a += piece + [word(k, "gap")]
    b = []
    for k, piece in reversed(list(enumerate(pieces))):
        b += piece + [word(k, "sep")]
    return (" ".join(a), " ".join(b))


def content_texts():
    return overlap_exact.content_texts()


def generated():
    """{name: (texts, stopwords)}: the small collections the host path is held to the model on."""
    found = dict(overlap_exact.generated())
    found["worked"] = (WORKED, ())
    found["bit edges"] = (bit_edge_texts()[0], ())
    found["row borders"] = (row_border_texts(), ())
    found["neighbours"] = (neighbours_texts(), ())
    found["order"] = (order_texts(), ())
    return found


def some_pairs(D, limit=40, seed=3):
    """All ordered pairs of a small collection; of a larger one `limit` drawn ones, a duplicate and a mirrored one among them."""
    pairs = all_pairs(D)
    if len(pairs) <= limit:
        return pairs
    rng = np.random.default_rng(seed + D)
    chosen = [pairs[i] for i in rng.choice(len(pairs), size=limit, replace=False).tolist()]
    return chosen + [chosen[0], (chosen[1][1], chosen[1][0])]
