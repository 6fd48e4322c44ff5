"""The model of the shingle overlap (include/east_hip.h, "Shingle overlap"): per text a Python set of word tuples, built with
cosine_exact's tokenizer; the intersections by set intersection; every entry Python's int / int, which is the correctly
rounded quotient.  It shares nothing with sorting or naming.

Above SET_LIMIT texts the same integers are counted through the shingles' holders and divided by numpy (a float64 division
of integers below 2^53 is the same correctly rounded quotient); tests/test_overlap_host.py holds the two forms to each
other."""
import functools

import numpy as np

import cosine_exact

SET_LIMIT = 300                                 # texts up to which every pair's sets are intersected one by one
MAX_WORDS = 8


def shingle_sets(texts, stopwords=(), w=4):
    """Per text the set of its w-word shingles: tuples of w kept tokens (at least 3 code points) at consecutive positions,
    none of them a stopword."""
    stop = cosine_exact.prepared_stopwords(stopwords)
    sets = []
    for text in texts:
        kept = [t for t in cosine_exact.all_tokens(text) if len(t) >= cosine_exact.MIN_LEN]
        found = set()
        for j in range(len(kept) - w + 1):
            g = tuple(kept[j:j + w])
            if not any(t in stop for t in g):
                found.add(g)
        sets.append(found)
    return sets


def intersections(sets):
    """I[a][b] = |S_a n S_b| as an int64 array (the diagonal: |S_a|)."""
    D = len(sets)
    I = np.zeros((D, D), dtype=np.int64)
    if D <= SET_LIMIT:
        for a in range(D):
            for b in range(a, D):
                I[a, b] = I[b, a] = len(sets[a] & sets[b])
        return I
    holders = {}
    for a, s in enumerate(sets):
        for g in s:
            holders.setdefault(g, []).append(a)
    for at in holders.values():
        at = np.asarray(at, dtype=np.int64)
        I[at[:, None], at[None, :]] += 1
    return I


def quotients(I, symmetric, by_numpy=None):
    """(matrix with NaN on the diagonal, self, shingles) of the intersections."""
    D = I.shape[0]
    n = I.diagonal().copy()
    matrix = np.zeros((D, D), dtype=np.float64)
    if by_numpy is None:
        by_numpy = D > SET_LIMIT
    if by_numpy:
        den = (n[:, None] + n[None, :] - I) if symmetric else np.broadcast_to(n[:, None], (D, D))
        np.divide(I.astype(np.float64), den.astype(np.float64), out=matrix, where=den > 0)
    else:
        rows, size = I.tolist(), n.tolist()
        for a in range(D):
            for b in range(D):
                den = size[a] + size[b] - rows[a][b] if symmetric else size[a]
                if den:
                    matrix[a, b] = rows[a][b] / den
    np.fill_diagonal(matrix, np.nan)
    return matrix, (n > 0).astype(np.float64), n.astype(np.int32)


def exact(texts, stopwords=(), w=4, symmetric=True):
    """-> (matrix, self, shingles, I)."""
    I = intersections(shingle_sets(texts, stopwords, w))
    return quotients(I, symmetric) + (I,)


def shared_units(sets):
    """(distinct shingles of the collection, those held by two or more texts, the postings of the latter)."""
    held = {}
    for s in sets:
        for g in s:
            held[g] = held.get(g, 0) + 1
    shared = [c for c in held.values() if c > 1]
    return len(held), len(shared), sum(shared)


def ranking(matrix, n, threshold=-np.inf):
    """Per row the other members by value descending, index ascending among equals, the first n at or above the threshold:
    (count[D], index[D, n] with -1 behind, score[D, n] with 0.0 behind)."""
    D = matrix.shape[0]
    count, index, score = np.zeros(D, np.int32), np.full((D, n), -1, np.int32), np.zeros((D, n), np.float64)
    for a in range(D):
        row = matrix[a]
        eligible = [b for b in range(D) if row[b] >= threshold]          # (a NaN never is)
        eligible.sort(key=lambda b: (-(row[b] + 0.0), b))
        eligible = eligible[:n]
        count[a] = len(eligible)
        index[a, :len(eligible)] = eligible
        score[a, :len(eligible)] = row[eligible]
    return count, index, score


# ---- collections --------------------------------------------------------------------------------------------------------------
STOP = ("the",)
WORKED = ("abc bcd cde def", "bcd cde def efg")            # the header's example, w = 2

HAND = {
    # name: (texts, stopwords, w, I[0][1], shingles)
    "worked": (WORKED, (), 2, 2, [3, 3]),
    "no shingle spans a text boundary": (("aaa bbb", "ccc ddd", "bbb ccc"), (), 2, 0, [1, 1, 1]),
    "a stopword breaks a shingle": (("aaa the bbb ccc", "aaa bbb ccc"), STOP, 2, 1, [1, 2]),
    "one word 300 times is one shingle": ((" ".join(["aaa"] * 300), "aaa aaa"), (), 2, 1, [1, 1]),
}


def word(i, prefix="w"):
    return "%s%05d" % (prefix, i)


@functools.lru_cache(maxsize=None)
def tile_edge_texts(D, seed=5):
    """D short texts over a small vocabulary with a stopword among it: many shared pairs of words, uneven sets, and every
    seventh text empty or too short."""
    rng = np.random.default_rng(seed + D)
    vocab = [word(i, "v") for i in range(14)] + ["the"]
    texts = []
    for d in range(D):
        if d % 7 == 3:
            texts.append("" if d % 2 else "v00001")
            continue
        texts.append(" ".join(vocab[i] for i in rng.integers(0, len(vocab), size=int(rng.integers(3, 18))).tolist()))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def unit_edge_texts(U):
    """Three texts with exactly U shared 2-word shingles (P_i Q_i, a stopword between two of them): the first holds all,
    the second the even ones, the third the odd ones and every third; each has shingles of its own besides."""
    def passages(ids, own):
        return " the ".join(["%s %s" % (word(i, "p"), word(i, "q")) for i in ids] + ["%s%da %s%db %s%dc" % (own, k, own, k, own, k) for k in range(3)])
    ids = range(U)
    return (passages(ids, "xx"), passages([i for i in ids if i % 2 == 0], "yy"),
            passages([i for i in ids if i % 2 == 1 or i % 3 == 0], "zz"))


ORIENTATION_D = 130


def orientation_count(a, b):
    return 1 + (7 * a + 13 * b) % 5


@functools.lru_cache(maxsize=None)
def orientation_texts():
    """130 texts in which every pair a < b shares a passage of its own: orientation_count(a, b) 2-word shingles of words no
    other pair uses."""
    D = ORIENTATION_D
    parts = [[] for _ in range(D)]
    for a in range(D):
        for b in range(a + 1, D):
            passage = " ".join("s%03dt%03dn%d" % (a, b, i) for i in range(orientation_count(a, b) + 1))
            parts[a].append(passage)
            parts[b].append(passage)
    return tuple(" the ".join(p) for p in parts)


@functools.lru_cache(maxsize=None)
def zipf_texts(tokens=20000, D=16, vocabulary=400, seed=11):
    """A Zipf collection of `tokens` tokens in D uneven texts, a stopword among the frequent words, with passages of 12 to
    40 tokens copied from text to text (what long shingles can share)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocabulary + 1)
    p /= p.sum()
    sizes = np.maximum((tokens * np.geomspace(1.0, 24.0, D) / np.geomspace(1.0, 24.0, D).sum()).astype(int), 4)
    rng.shuffle(sizes)
    names = ["the" if i == 3 else word(i, "z") for i in range(vocabulary)]
    docs = [[names[i] for i in rng.choice(vocabulary, size=int(n), p=p).tolist()] for n in sizes]
    for _ in range(40):
        src, dst = rng.integers(0, D, size=2).tolist()
        length = int(rng.integers(12, 41))
        if src == dst or len(docs[src]) <= length or len(docs[dst]) <= length:
            continue
        s, t = int(rng.integers(0, len(docs[src]) - length)), int(rng.integers(0, len(docs[dst]) - length))
        docs[dst][t:t + length] = docs[src][s:s + length]
    return tuple(" ".join(d) for d in docs)


@functools.lru_cache(maxsize=None)
def wide_key_texts(n=70000):
    """n distinct words in two texts, every one twice in the collection: level 2 has more than 2^16 survivors below it and
    17 bits of terms, 34-bit keys.  The second text holds the first half in order and the second half reversed."""
    words = [word(i, "k") for i in range(n)]
    return (" ".join(words), " ".join(words[:n // 2] + words[n // 2:][::-1]))


def generated():
    """{name: (texts, stopwords)}: the small collections the host path is held to the model on."""
    found = {"tile edges %d" % D: (tile_edge_texts(D), STOP) for D in (1, 2, 5, 65)}
    found["unit edges 65"] = (unit_edge_texts(65), STOP)
    found["zipf"] = (zipf_texts(3000, 9), STOP)
    found["content"] = (content_texts(), STOP)
    for i, r in enumerate(cosine_exact.fuzz_rounds()[:12]):
        found["fuzz %d" % i] = (tuple(r["texts"]), tuple(r["stopwords"]))
    return found


def content_texts():
    base = "alpha beta gamma delta epsilon zeta eta theta iota kappa"
    return (base, base, "gamma delta epsilon zeta", "lead words here " + base + " and trailing words", "", "alpha", "the the the",
            "kappa iota theta eta zeta")
