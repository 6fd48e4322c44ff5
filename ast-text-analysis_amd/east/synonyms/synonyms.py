# -*- coding: utf-8 -*-
"""SynonymExtractor (reference east/synonyms/synonyms.py): words are similar when they occur with the same dependency
relations to the same words (Lin's measure).

The reference gets its dependency triples from the closed Tomita parser (synonyms.py:52-88).  This class takes them from
the caller instead -- Tomita's XML output made elsewhere, or any parser's output as lines of `w1<TAB>relation<TAB>w2` -- and
does everything behind them (synonyms.py:116-169) on the device: csrc/synonyms.h through hip_backend.HipSynonyms.  Parsing,
interning and the word frequencies are host work; there is no CPU fallback for the rest: without a device I, T, similarity
and get_synonyms raise HipBackendError.

Departures from the reference, none of which a score depends on (easa.py:27-33 takes a maximum over the variants):
candidates are taken in code-point order and pairs (a, b) in a < b order of that list, so every word's synonyms come in
that order (the reference's follow Python 2's set order); get_synonyms keeps its result per (threshold,
return_similarity_measure) (the reference recomputes it on every call: easa.py:28); a directory's texts are joined in
sorted file order (the reference's os.listdir order is arbitrary); a negative threshold is refused.
"""
import collections
import os
from xml.dom import minidom

import numpy as np

from east import exceptions
from east import utils as common_utils


def inverse_relation(relation):
    """synonyms.py:81 -- an involution of the strings."""
    return relation[:-3] if relation.endswith("_of") else relation + "_of"


def parse_tomita_xml(data):
    """synonyms.py:67-72: every Relation element; its first element child's name is the relation, that child's `val`
    attribute "w1 w2", split at the first space."""
    try:
        doc = minidom.parseString(data)
    except Exception as e:
        raise exceptions.TriplesFormatException(message="Malformed dependency triples: not well-formed XML (%s)." % e)
    triples = []
    for n, rel in enumerate(doc.getElementsByTagName("Relation")):
        child = next((c for c in rel.childNodes if c.nodeType == c.ELEMENT_NODE), None)
        value = child.getAttribute("val") if child is not None else ""
        if " " not in value:
            raise exceptions.TriplesFormatException(
                message="Malformed dependency triple: Relation element number %d has no child with val=\"w1 w2\"." % (n + 1))
        w1, w2 = value.split(" ", 1)
        triples.append((w1, child.nodeName, w2))
    return triples


def parse_triple_lines(text, source="<triples>"):
    """Lines of w1<TAB>relation<TAB>w2; blank lines are skipped, anything else malformed names its line."""
    triples = []
    for n, line in enumerate(text.split("\n")):
        line = line.rstrip("\r")
        if not line.strip():
            continue
        fields = line.split("\t")
        if len(fields) != 3 or not all(fields):
            raise exceptions.TriplesFormatException(line=n + 1, source=source)
        triples.append(tuple(fields))
    return triples


def read_triples(path):
    """A file whose first non-blank character is `<` is Tomita's XML, anything else UTF-8 lines of triples."""
    with open(path, "rb") as f:
        data = f.read()
    if data.lstrip()[:1] == b"<":
        return parse_tomita_xml(data)
    return parse_triple_lines(data.decode("utf-8", errors="replace"), source=path)


def intern_triples(triples):
    """-> (words sorted, relations sorted with every inverse, w1 ids, relation ids, w2 ids, inverse-relation ids)."""
    words = sorted(set(t[0] for t in triples) | set(t[2] for t in triples))
    relations = set(t[1] for t in triples)
    for r in sorted(relations):
        if inverse_relation(inverse_relation(r)) != r:
            # (x_of_of -> x_of -> x: the marginals rest on f(t) == f(inverse t))
            raise exceptions.TriplesFormatException(
                message="Relation `%s`: its inverse's inverse is `%s`, so a triple and its inverse cannot be counted "
                        "together; rename the relation." % (r, inverse_relation(inverse_relation(r))))
    relations = sorted(relations | set(inverse_relation(r) for r in relations))
    word_id = {w: i for i, w in enumerate(words)}
    relation_id = {r: i for i, r in enumerate(relations)}
    w1 = np.array([word_id[t[0]] for t in triples], dtype=np.int32)
    rel = np.array([relation_id[t[1]] for t in triples], dtype=np.int32)
    w2 = np.array([word_id[t[2]] for t in triples], dtype=np.int32)
    inverse = np.array([relation_id[inverse_relation(r)] for r in relations], dtype=np.int32)
    return words, relations, w1, rel, w2, inverse


def candidate_words(words, word_frequencies, number_of_texts):
    """synonyms.py:156-158 (Python 2: `/` on ints floors), in code-point order."""
    floor = number_of_texts // 50
    return [w for w in sorted(words) if len(w) > 2 and word_frequencies.get(w, 0) > floor]


class SynonymExtractor(object):

    def __init__(self, input_path, triples=None, device=None):
        """input_path: a directory of .txt files or a single file (synonyms.py:37-50); triples: a path (read_triples) or
        an iterable of (w1, relation, w2) strings."""
        if triples is None:
            raise exceptions.TomitaNotInstalledException()
        text, number_of_texts = self._retrieve_text(input_path)
        self._init(text, number_of_texts, triples, device)

    @classmethod
    def from_texts(cls, texts, triples, device=None):
        """The same without paths: texts = the collection (bytes or str)."""
        if triples is None:
            raise exceptions.TomitaNotInstalledException()
        self = cls.__new__(cls)
        texts = [t.decode("utf-8", errors="replace") if isinstance(t, bytes) else t for t in texts]
        self._init("".join(texts), len(texts), triples, device)
        return self

    def _init(self, text, number_of_texts, triples, device):
        self.text, self.number_of_texts = text, number_of_texts
        if isinstance(triples, (str, bytes, os.PathLike)):
            triples = read_triples(triples)
        else:
            triples = [tuple(t) for t in triples]
            for n, t in enumerate(triples):
                if len(t) != 3 or not all(isinstance(x, str) for x in t):
                    raise exceptions.TriplesFormatException(line=n + 1, source="the given triples")
        self.word_frequencies = self._calculate_word_frequencies(text)
        self._words, self._relations, self._w1, self._rel, self._w2, self._inverse = intern_triples(triples)
        self.words, self.relations = set(self._words), set(self._relations)
        self._word_id = {w: i for i, w in enumerate(self._words)}
        self._relation_id = {r: i for i, r in enumerate(self._relations)}
        self._device = device
        self._dev = None
        self._rows = None
        self.synonyms_memoized = {}

    def _retrieve_text(self, input_path):
        if os.path.isdir(input_path):
            parts = []
            for file_name in sorted(os.listdir(input_path)):
                if file_name.endswith(".txt"):
                    with open(os.path.join(os.path.abspath(input_path), file_name), "rb") as f:
                        parts.append(f.read())
            return b"".join(parts).decode("utf-8", errors="replace"), len(parts)
        with open(input_path, "rb") as f:
            return f.read().decode("utf-8", errors="replace"), 1

    def _calculate_word_frequencies(self, text):
        res = collections.defaultdict(int)
        for word in common_utils.tokenize(common_utils.prepare_text(text)):
            res[word] += 1
        return res

    # -- the device ---------------------------------------------------------------------------------------------------
    def _built(self):
        """The feature rows on the device, built on first use (HipBackendError without one)."""
        if self._dev is None:
            from east import hip_backend
            dev = hip_backend.HipSynonyms(self._device)
            try:
                dev.build(self._w1, self._rel, self._w2, self._inverse, len(self._words))
            except Exception:
                dev.close()
                raise
            self._dev = dev
        return self._dev

    def close(self):
        if getattr(self, "_dev", None) is not None:
            self._dev.close()
            self._dev = None

    __del__ = close

    def _fetched_rows(self):
        if self._rows is None:
            offsets, relation, word, value, _ = self._built().rows()
            self._rows = (offsets, (relation.astype(np.int64) << 32) | word.astype(np.int64), relation, word, value)
        return self._rows

    def I(self, w1, r, w2):
        """synonyms.py:122-134."""
        if not self._w1.size or w1 not in self._word_id or w2 not in self._word_id or r not in self._relation_id:
            return 0.0
        offsets, keys, _, _, value = self._fetched_rows()
        b, e = int(offsets[self._word_id[w1]]), int(offsets[self._word_id[w1] + 1])
        key = (self._relation_id[r] << 32) | self._word_id[w2]
        p = b + int(np.searchsorted(keys[b:e], key))
        return float(value[p]) if p < e and keys[p] == key else 0.0

    def T(self, w):
        """synonyms.py:136-142: the features (r, w') with I(w, r, w') > 0."""
        if not self._w1.size or w not in self._word_id:
            return set()
        offsets, _, relation, word, _ = self._fetched_rows()
        b, e = int(offsets[self._word_id[w]]), int(offsets[self._word_id[w] + 1])
        return set((self._relations[relation[p]], self._words[word[p]]) for p in range(b, e))

    def similarity(self, w1, w2):
        """synonyms.py:144-152."""
        if not self._w1.size or w1 not in self._word_id or w2 not in self._word_id:
            return 0.0
        return float(self._built().similarity([self._word_id[w1]], [self._word_id[w2]])[0])

    def get_synonyms(self, threshold=0.3, return_similarity_measure=False):
        """synonyms.py:154-169."""
        memo = (float(threshold), bool(return_similarity_measure))
        if memo in self.synonyms_memoized:
            return self.synonyms_memoized[memo]
        synonyms = collections.defaultdict(list)
        candidates = candidate_words(self.words, self.word_frequencies, self.number_of_texts)
        if len(candidates) >= 2:
            ids = np.array([self._word_id[w] for w in candidates], dtype=np.int32)
            a, b, sim = self._built().pairs(ids, threshold)
            for x, y, s in zip(a.tolist(), b.tolist(), sim.tolist()):
                w1, w2 = self._words[x], self._words[y]
                if return_similarity_measure:
                    synonyms[w1].append((w2, s))
                    synonyms[w2].append((w1, s))
                else:
                    synonyms[w1].append(w2)
                    synonyms[w2].append(w1)
        self.synonyms_memoized[memo] = synonyms
        return synonyms
