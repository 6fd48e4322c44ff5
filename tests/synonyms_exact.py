# -*- coding: utf-8 -*-
"""An exact host model of synonym extraction (include/east_hip.h, "Synonym extraction"), and the generated
triples that tests/test_synonyms_host.py (CPU) and tests/test_gpu_synonyms.py (GPU) share.  A plain module: no test, no
fixture, and nothing of east.synonyms -- the model works on the strings of the triples.

`Model(triples)` goes from the raw triples (w1, relation, w2) to

  * the integers: every triple entered with its inverse, f(t) = its occurrences in the doubled list, and the marginals
    F_r, F_w1r, F_rw2 as sums of f^2 over the distinct triples (the reference adds f once per occurrence);
  * q = float(f) * F_r / F_w1r / F_rw2 in Python doubles, the three operations in that order -- what the reference computes
    and what the device is specified to compute bit for bit; a feature (r, w2) belongs to T(w1) iff q > 1.0;
  * I = ln(q), the row sums, the numerators and the similarities in `decimal` at 50 digits (q, a double, converts
    exactly); ONE rounding to double at the end of each.  The model's I and similarity are the correctly rounded values
    of the exact ones unless those lie within 1e-48 of a rounding boundary.

What a double implementation may differ by: each log by an ulp or so of a value of at most ln(2^64 * 2^30) < 66, the sums
of n such terms by n roundings, one division -- a few hundred ulp of values in [0, 1] for rows of a few hundred terms,
that is 1e-13 at the outside, under the 1e-12 the tests ask for.
"""
import collections
import decimal
import random

CTX = decimal.Context(prec=50)
ABS_TOL = 1e-12


def inverse_relation(relation):
    return relation[:-3] if relation.endswith("_of") else relation + "_of"


class Model(object):
    """words, relations: sorted lists (the relations with every inverse); rows[w] = [((r, w2), I as Decimal)] in
    ascending (r, w2) order; q[(w1, r, w2)] for every distinct triple."""

    def __init__(self, triples):
        doubled = []
        for w1, r, w2 in triples:
            doubled.append((w1, r, w2))
            doubled.append((w2, inverse_relation(r), w1))
        self.f = collections.Counter(doubled)
        self.words = sorted(set(t[0] for t in doubled))
        self.relations = sorted(set(t[1] for t in doubled))
        F_r, F_w1r, F_rw2 = collections.Counter(), collections.Counter(), collections.Counter()
        for (w1, r, w2), f in self.f.items():
            F_r[r] += f * f
            F_w1r[(w1, r)] += f * f
            F_rw2[(r, w2)] += f * f
        self.F_r, self.F_w1r, self.F_rw2 = F_r, F_w1r, F_rw2
        self.q = {}
        rows = collections.defaultdict(list)
        for (w1, r, w2), f in self.f.items():
            q = float(f) * F_r[r] / F_w1r[(w1, r)] / F_rw2[(r, w2)]
            self.q[(w1, r, w2)] = q
            if q > 1.0:
                rows[w1].append(((r, w2), CTX.ln(decimal.Decimal(q))))
        self.rows = {w: sorted(rows[w]) for w in self.words}
        self.row_sum = {w: sum((v for _, v in self.rows[w]), decimal.Decimal(0)) for w in self.words}
        self._dict = {w: dict(self.rows[w]) for w in self.words}

    def I(self, w1, r, w2):
        return float(self._dict.get(w1, {}).get((r, w2), 0.0))

    def shared(self, a, b):
        return set(self._dict[a]) & set(self._dict[b])

    def similarity(self, a, b):
        den = self.row_sum[a] + self.row_sum[b]
        if not den:
            return 0.0
        da, db = self._dict[a], self._dict[b]
        num = sum((CTX.add(da[k], db[k]) for k in self.shared(a, b)), decimal.Decimal(0))
        return float(CTX.divide(num, den))

    def sharing_pairs(self, candidates):
        """The pairs (a in front of b in `candidates`) whose rows have a feature in common, in pair order -- found
        through the features, not by trying every pair."""
        position = {w: i for i, w in enumerate(candidates)}
        by_feature = collections.defaultdict(list)
        for w in candidates:
            for k in self._dict[w]:
                by_feature[k].append(position[w])
        found = set()
        for members in by_feature.values():
            for x in range(len(members)):
                for y in range(x + 1, len(members)):
                    found.add((members[x], members[y]))
        return [(candidates[i], candidates[j]) for i, j in sorted(found)]

    def pairs(self, candidates, threshold):
        """[(a, b, similarity)] for a in front of b in `candidates`, similarity > threshold >= 0, in pair order (a pair
        without a common feature has similarity 0.0)."""
        assert threshold >= 0.0
        out = []
        for a, b in self.sharing_pairs(candidates):
            s = self.similarity(a, b)
            if s > threshold:
                out.append((a, b, s))
        return out


def candidate_words(words, word_frequencies, number_of_texts):
    floor = number_of_texts // 50
    return [w for w in sorted(words) if len(w) > 2 and word_frequencies.get(w, 0) > floor]


def synonyms_of(pairs):
    """{word: [synonyms]} in the order the pairs come in."""
    out = collections.defaultdict(list)
    for a, b, _ in pairs:
        out[a].append(b)
        out[b].append(a)
    return dict(out)


# ---- generated triples -------------------------------------------------------------------------------------------------
def word_name(i):
    return "W%05d" % i


def zipf_triples(seed, n_words, n_relations, n_triples, exponent=1.0):
    """Seeded triples whose words follow a Zipf-like law; relations r0 .. , some of them given as `r_of`."""
    rng = random.Random(seed)
    weights = [1.0 / (k + 1) ** exponent for k in range(n_words)]
    names = [word_name(i) for i in range(n_words)]
    rng.shuffle(names)
    rels = ["r%d" % i for i in range(n_relations)]
    rels = [r + "_of" if i % 3 == 2 else r for i, r in enumerate(rels)]
    a = rng.choices(names, weights, k=n_triples)
    b = rng.choices(names, weights, k=n_triples)
    return [(a[i], rng.choice(rels), b[i]) for i in range(n_triples)]


def row_length_triples(lengths, seed=0, shared_pool=24, max_shared=4):
    """One word (word_name(i)) per entry of `lengths` whose row has exactly that many features: up to `max_shared` of
    them are words of a small pool under relation `has` (so that rows intersect; `has` sorts behind `big`, so they are the
    LAST columns of the row), the rest the word's own under relation `big`.  Every triple occurs once, so
    q = F_r / (F_w1r * F_rw2) > 1 as long as no row is all of its relation; Model(...).rows says what came out, and the
    tests assert the lengths they rely on.  The feature words get short rows of their own (has_of, big_of)."""
    rng = random.Random(seed)
    triples = []
    pool = ["P%02d" % i for i in range(shared_pool)]
    for i, n in enumerate(lengths):
        w = word_name(i)
        take = rng.sample(pool, min(n, rng.randint(1, max_shared))) if n else []
        for t in take:
            triples.append((w, "has", t))
        for k in range(n - len(take)):
            triples.append((w, "big", "F%d_%d" % (i, k)))
    return triples
