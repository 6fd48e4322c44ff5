#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE ONLY -- record tests/golden/synonyms.json from the reference's SynonymExtractor.

    PYTHONHASHSEED=0 PYTHONUTF8=1 python tools/gen_synonyms_golden.py

Runs where the reference is importable through oracle/ref_shim.py, as tools/gen_cosine_golden.py does.  The reference gets
its dependency triples from the closed Tomita parser; here the parser process is the one thing that is replaced: the
reference's own `_retrieve_dependency_triples` runs, and the `subprocess.Popen` it starts is a stand-in whose output is
the case's triples as Tomita-shaped XML (for the hand-written XML case: that string as it stands), so the reference's own
XML reading and its own doubling of every triple with its inverse (synonyms.py:67-86) are part of what is recorded.  The
check for the parser's binary (`_get_tomita_path`) is answered with a dummy path.  Nothing else of the reference is
touched: the texts are real files in a temporary directory (number_of_texts of them), and I, T, similarity and
get_synonyms are the reference's.

Recorded per case: the triples (or the XML), the text and the number of texts, the words, every I > 0, the similarity of
every pair of candidate words (a flat list in the order of itertools.combinations(candidates, 2)), get_synonyms at 0.3 and at 0.0 (each word's list sorted: the reference's order is Python's
set order).  The script asserts for every case that no candidate pair's similarity lies within 1e-9 of 0.3, and that none
lies in (0, 1e-9]: the tests never have to leave a pair out.  A drawn case that violates it gets another seed, not
another margin.
"""
import itertools
import json
import os
import random
import sys
import tempfile
import types
from xml.sax.saxutils import quoteattr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "synonyms.json")
MARGIN = 1e-9


def triples_xml(triples):
    """The shape of Tomita's output the reference reads: <Relation><NAME val="w1 w2"/></Relation>, no white space in
    front of the child (synonyms.py:71 takes childNodes[0])."""
    body = "".join("<Relation><%s val=%s/></Relation>" % (r, quoteattr("%s %s" % (w1, w2))) for w1, r, w2 in triples)
    return '<?xml version="1.0" encoding="utf-8"?><fdo_objects><document>%s</document></fdo_objects>' % body


HAND_XML = ('<?xml version="1.0" encoding="utf-8"?>\n<fdo_objects>\n  <document url="" di="1" bi="-1" date="2014-01-01">\n'
            '    <facts>\n'
            '      <Relation><amod val="RED APPLE"/></Relation>\n'
            '      <Relation><amod val="RED CHERRY"/></Relation>\n'
            '      <Relation><amod val="SWEET APPLE"/></Relation>\n'
            '      <Relation><amod val="SWEET CHERRY"/></Relation>\n'
            '      <Relation><amod val="SWEET PLUM"/></Relation>\n'
            '      <Relation><amod val="SOUR PLUM"/></Relation>\n'
            '      <Relation><dobj val="EAT APPLE"/></Relation>\n'
            '      <Relation><dobj val="EAT CHERRY"/></Relation>\n'
            '      <Relation><dobj val="EAT APPLE"/></Relation>\n'
            '      <Relation><dobj val="PICK PLUM"/></Relation>\n'
            '      <Relation><dobj val="PICK CHERRY"/></Relation>\n'
            '      <Relation><nsubj_of val="TREE GROW"/></Relation>\n'
            '      <Relation><nsubj val="GROW APPLE"/></Relation>\n'
            '      <Relation><nsubj val="GROW PLUM"/></Relation>\n'
            '      <Relation><dobj val="SEE RED CHERRY"/></Relation>\n'
            '    </facts>\n  </document>\n</fdo_objects>\n')


def words_text(words, times=2):
    return " ".join(w for w in words for _ in range(times)) + "\n"


def zipf_case(name, seed, n_words, n_relations, n_triples):
    rng = random.Random(seed)
    words = ["W%02d" % i for i in range(n_words)]
    weights = [1.0 / (k + 1) for k in range(n_words)]
    rels = ["rel%d" % i for i in range(n_relations)]
    triples = [(rng.choices(words, weights)[0], rng.choice(rels), rng.choices(words, weights)[0]) for _ in range(n_triples)]
    return {"name": name, "triples": triples, "text": words_text(words), "number_of_texts": 1}


def all_words(triples):
    return sorted(set(t[0] for t in triples) | set(t[2] for t in triples))


def frequency_case(n_texts):
    """CAT and DOG have the same contexts; DOG occurs exactly n_texts // 50 times in the text: it fails the frequency
    filter and nothing else.  Every other word occurs once more than that."""
    floor = n_texts // 50
    triples = [("CAT", "subj", "RUN"), ("DOG", "subj", "RUN"), ("CAT", "subj", "EAT"), ("DOG", "subj", "EAT"),
               ("COW", "subj", "EAT"), ("COW", "subj", "MOO"), ("CAT", "amod", "SMALL"), ("DOG", "amod", "SMALL"),
               ("COW", "amod", "LARGE"), ("PIG", "amod", "LARGE"), ("PIG", "subj", "EAT"), ("PIG", "subj", "RUN")]
    words = all_words(triples)
    text = " ".join(" ".join([w] * (floor if w == "DOG" else floor + 1)) for w in words) + "\n"
    return {"name": "frequency_filter_%d_texts" % n_texts, "triples": triples, "text": text, "number_of_texts": n_texts}


def cases():
    out = [zipf_case("zipf_36_words", 11, 36, 6, 260), zipf_case("zipf_50_words", 5, 50, 4, 380)]

    rng = random.Random(3)
    words = ["ALPHA", "BRAVO", "CHARLIE", "DELTA", "ECHO", "FOXTROT", "GOLF", "HOTEL"]
    base = [(rng.choice(words), rng.choice(["mod", "obj"]), rng.choice(words)) for _ in range(24)]
    triples = []
    for i, t in enumerate(base):                            # triples occurring 1, 2 and 5 times: the squares matter
        triples += [t] * (1, 2, 5)[i % 3]
    out.append({"name": "multiplicities_1_2_5", "triples": triples, "text": words_text(words), "number_of_texts": 1})

    # raw relations that already end in _of, and a relation that occurs both plain and with _of
    triples = [("KING", "ruler_of", "LAND"), ("QUEEN", "ruler_of", "LAND"), ("KING", "ruler_of", "CASTLE"),
               ("QUEEN", "ruler_of", "CASTLE"), ("DUKE", "ruler_of", "TOWN"), ("LAND", "ruler", "EMPEROR"),
               ("TOWN", "ruler", "MAYOR"), ("MAYOR", "ruler_of", "VILLAGE"), ("KING", "owner", "CROWN"),
               ("QUEEN", "owner", "CROWN"), ("CROWN", "owner_of", "DUKE"), ("EMPEROR", "owner", "LAND"),
               ("DUKE", "owner", "TOWN"), ("KING", "ruler_of", "TOWN")]
    out.append({"name": "relations_with_of", "triples": triples, "text": words_text(all_words(triples)), "number_of_texts": 1})

    # w1 == w2
    triples = [("ECHO", "conj", "ECHO"), ("ECHO", "conj", "SOUND"), ("SOUND", "conj", "SOUND"), ("NOISE", "conj", "SOUND"),
               ("NOISE", "conj", "ECHO"), ("NOISE", "conj", "NOISE"), ("HUSH", "conj", "HUSH"), ("ECHO", "conj", "ECHO"),
               ("HUSH", "mod", "ECHO"), ("SOUND", "mod", "ECHO"), ("SOUND", "mod", "NOISE"), ("HUSH", "mod", "NOISE")]
    out.append({"name": "self_pairs", "triples": triples, "text": words_text(all_words(triples)), "number_of_texts": 1})

    # two words with identical rows (TWINA, TWINB), among others
    contexts = [("mod", "BRIGHT"), ("mod", "TALL"), ("obj_of", "BUILD"), ("obj_of", "PAINT")]
    triples = [(w, r, c) for w in ("TWINA", "TWINB") for r, c in contexts]
    triples += [("OTHER", "mod", "BRIGHT"), ("OTHER", "obj_of", "SELL"), ("FOURTH", "mod", "DARK"), ("FOURTH", "obj_of", "SELL"),
                ("FOURTH", "obj_of", "PAINT")]
    out.append({"name": "identical_rows", "triples": triples, "text": words_text(all_words(triples)), "number_of_texts": 1})

    # words all of whose q <= 1: a complete bipartite block under a relation of its own has q == 1 everywhere
    left, right = ["LEFTA", "LEFTB", "LEFTC"], ["RIGHTA", "RIGHTB"]
    triples = [(a, "full", b) for a in left for b in right]
    triples += [("SUN", "mod", "HOT"), ("FIRE", "mod", "HOT"), ("SUN", "mod", "BRIGHT"), ("FIRE", "mod", "RED"),
                ("ICE", "mod", "COLD"), ("SNOW", "mod", "COLD"), ("SNOW", "mod", "WHITE"), ("ICE", "mod", "BRIGHT")]
    out.append({"name": "no_positive_feature", "triples": triples, "text": words_text(all_words(triples)), "number_of_texts": 1})

    # OX has the contexts of COW and fails the length filter only
    triples = [("OX", "subj", "PULL"), ("COW", "subj", "PULL"), ("OX", "subj", "GRAZE"), ("COW", "subj", "GRAZE"),
               ("HORSE", "subj", "PULL"), ("HORSE", "subj", "RUN"), ("GOAT", "subj", "GRAZE"), ("GOAT", "subj", "CLIMB"),
               ("OX", "amod", "STRONG"), ("HORSE", "amod", "STRONG"), ("COW", "amod", "BROWN"), ("GOAT", "amod", "BROWN")]
    out.append({"name": "length_filter", "triples": triples, "text": words_text(all_words(triples), 3), "number_of_texts": 1})

    out += [frequency_case(n) for n in (1, 49, 50, 120)]

    # non-ASCII words (upper case as prepare_text leaves them)
    triples = [("КОШКА", "subj", "БЕЖАТЬ"), ("СОБАКА", "subj", "БЕЖАТЬ"), ("КОШКА", "subj", "СПАТЬ"), ("СОБАКА", "subj", "ЛАЯТЬ"),
               ("ΓΑΤΑ", "subj", "СПАТЬ"), ("ΓΑΤΑ", "subj", "БЕЖАТЬ"), ("КОШКА", "amod", "МАЛЕНЬКАЯ"), ("ΓΑΤΑ", "amod", "МАЛЕНЬКАЯ"),
               ("СОБАКА", "amod", "БОЛЬШАЯ"), ("ÉLÉPHANT", "amod", "БОЛЬШАЯ"), ("ÉLÉPHANT", "subj", "СПАТЬ"), ("東京", "subj", "СПАТЬ"),
               ("東京タワー", "amod", "БОЛЬШАЯ"), ("東京タワー", "subj", "ЛАЯТЬ")]
    out.append({"name": "non_ascii", "triples": triples, "text": words_text(all_words(triples)), "number_of_texts": 1})

    out.append({"name": "tomita_xml", "xml": HAND_XML, "number_of_texts": 1,
                "text": words_text(["RED", "SWEET", "SOUR", "APPLE", "CHERRY", "PLUM", "EAT", "PICK", "TREE", "GROW", "SEE"])})
    return out


class FakeParser(object):
    """What the reference starts in place of the Tomita binary: a process that prints the XML of the case."""
    xml = ""

    def __init__(self, *args, **kwargs):
        pass

    def communicate(self, input=None):
        return FakeParser.xml.encode("utf-8"), b""


def record(case, ref_synonyms, ref_utils):
    FakeParser.xml = case["xml"] if "xml" in case else triples_xml(case["triples"])
    with tempfile.TemporaryDirectory() as tmp:
        n = case["number_of_texts"]
        if n == 1:
            path = os.path.join(tmp, "text.txt")
        else:
            path = tmp
        for i in range(n):                                  # the text in the first file, the others empty
            with open(os.path.join(tmp, "text.txt" if n == 1 else "t%03d.txt" % i), "w", encoding="utf-8") as f:
                f.write(case["text"] if i == 0 else "")
        ex = ref_synonyms.SynonymExtractor(path)
    assert ex.number_of_texts == n
    words = sorted(ex.words)
    case["words"] = words
    case["relations"] = sorted(ex.relations)
    case["I"] = sorted([w, r, w2, ex.I(w, r, w2)] for w in words for (r, w2) in ex.T(w))
    candidates = sorted(w for w in ex.words if len(w) > 2 and ex.word_frequencies[w] > n // 50)
    case["candidates"] = candidates
    sims = [[a, b, ex.similarity(a, b)] for a, b in itertools.combinations(candidates, 2)]
    for a, b, s in sims:
        assert abs(s - 0.3) > MARGIN and (s == 0.0 or s > MARGIN), (case["name"], a, b, s)
    case["similarity"] = [s for _, _, s in sims]            # in the order of itertools.combinations(candidates, 2)
    for key, threshold in (("synonyms_0.3", 0.3), ("synonyms_0.0", 0.0)):
        got = ex.get_synonyms(threshold)
        case[key] = {w: sorted(got[w]) for w in sorted(got) if got[w]}
        assert set(case[key]) <= set(candidates)
    with_measure = ex.get_synonyms(0.3, True)
    for w, lst in with_measure.items():
        for other, s in lst:
            assert s == ex.similarity(*sorted((w, other))) or s == ex.similarity(w, other)
    return case


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        sys.exit("run as: PYTHONHASHSEED=0 PYTHONUTF8=1 python tools/gen_synonyms_golden.py")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shim
    ref_shim.install()
    from east.synonyms import synonyms as ref_synonyms
    from east import utils as ref_utils

    # (the module's own name `subprocess`, not the real module: platform.architecture() starts processes too)
    ref_synonyms.subprocess = types.SimpleNamespace(Popen=FakeParser, PIPE=-1)
    ref_synonyms.SynonymExtractor._get_tomita_path = lambda self: ("", "tomita")
    out = {"cases": [record(c, ref_synonyms, ref_utils) for c in cases()]}
    for c in out["cases"]:
        if "triples" in c:
            c["triples"] = [list(t) for t in c["triples"]]
    assert any(not any(i[0] == w for i in c["I"]) for c in out["cases"] if c["name"] == "no_positive_feature" for w in c["words"])
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    for c in out["cases"]:
        near = min((abs(s - 0.3) for s in c["similarity"]), default=1.0)
        print("%-28s words %3d  I>0 %4d  candidates %3d  pairs>0.3 %3d  >0 %4d  nearest to 0.3: %.2e" % (
            c["name"], len(c["words"]), len(c["I"]), len(c["candidates"]), sum(len(v) for v in c["synonyms_0.3"].values()) // 2,
            sum(len(v) for v in c["synonyms_0.0"].values()) // 2, near))


if __name__ == "__main__":
    main()
