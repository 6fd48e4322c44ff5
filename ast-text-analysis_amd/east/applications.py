# -*- coding: utf-8 -*-
"""keyphrases_table / keyphrases_graph (reference east/applications.py:11-149), keyphrases_top and keyphrases_similar;
texts_related, texts_similar, texts_overlap, texts_passages, the clusters, keyphrases_extract and texts_terms."""

import inspect
import os
from collections import namedtuple
from collections.abc import Mapping

import numpy as np

from east import consts
from east import logging
from east import relevance
from east import utils


class _ScoreRow(Mapping):
    """One keyphrase's row of a ScoreTable: {text name: score}, read off the K x D array."""

    __slots__ = ("_table", "_k")

    def __init__(self, table, k):
        self._table, self._k = table, k

    def __getitem__(self, title):
        return float(self._table.scores[self._k, self._table._column[title]])

    def __iter__(self):
        return iter(self._table.text_titles)

    def __len__(self):
        return len(self._table.text_titles)


class ScoreTable(Mapping):
    """What keyphrases_table returns on the batched path: {raw keyphrase: {text name: score}} (applications.py:46-52) as a
    read-only mapping over the K x D score array itself.  At BASELINE configs[2] the table holds 2.56 M scores: a dict of
    dicts of Python floats costs seconds to make and a gigabyte to keep, the device fills the array in a millisecond.
    Compares equal to the dict of dicts with the same content; `scores`, `keyphrases` (row order) and `text_titles`
    (column order) are there for consumers that work on the array (east/formatting.py, keyphrases_graph)."""

    def __init__(self, keyphrases, text_titles, scores):
        self.keyphrases, self.text_titles, self.scores = list(keyphrases), list(text_titles), scores
        self._row = {kp: k for k, kp in enumerate(self.keyphrases)}
        self._column = {}
        for d, title in enumerate(self.text_titles):         # (as dict(zip(titles, row)): a repeated title keeps its last column)
            self._column[title] = d

    def __getitem__(self, keyphrase):
        return _ScoreRow(self, self._row[keyphrase])

    def __iter__(self):
        return iter(self.keyphrases)

    def __len__(self):
        return len(self.keyphrases)

    def to_dict(self):
        """The reference's own return type: a plain, mutable, JSON-serialisable dict of dicts of Python floats."""
        titles = self.text_titles
        return {kp: dict(zip(titles, row)) for kp, row in zip(self.keyphrases, np.asarray(self.scores, dtype=np.float64).tolist())}


# Tables below this many scores come back as the reference's plain dict of dicts (json.dumps, item assignment and
# isinstance(table, dict) work as they do there; 65 536 scores cost about 10 ms to box).  From here on the table is a
# ScoreTable over the array (to_dict() gives the plain form): at configs[2], 2.56 M scores, the dict costs 0.4 s and the
# device fills the array in a millisecond.
ARRAY_TABLE_MIN_SCORES = 1 << 16


def keyphrases_table(keyphrases, texts, similarity_measure=None, synonimizer=None,
                     language=consts.Language.ENGLISH):
    """Matching score of every keyphrase in every text (reference east/applications.py:11-56).

    :param keyphrases: raw keyphrase strings (empty ones are skipped, duplicates collapse)
    :param texts: {text name: text}
    :param similarity_measure: defaults to ASTRelevanceMeasure() (easa, normalized)
    :returns: {raw keyphrase: {text name: score}} -- a plain dict as in the reference; from ARRAY_TABLE_MIN_SCORES scores
              on, a ScoreTable (a read-only mapping over the score array that compares equal to that dict; `.to_dict()`)
    """
    similarity_measure = similarity_measure or relevance.ASTRelevanceMeasure()

    text_titles = list(texts.keys())
    text_collection = list(texts.values())
    similarity_measure.set_text_collection(text_collection, language)

    keyphrases_prepared = {keyphrase: utils.prepare_text(keyphrase) for keyphrase in keyphrases}
    res = {}

    # batched path: one score call for the whole table
    if hasattr(similarity_measure, "relevance_table"):
        wanted = [kp for kp in dict.fromkeys(keyphrases) if kp]          # applications.py:44-45
        if wanted:
            prepared = [keyphrases_prepared[kp] for kp in wanted]
            scores = (similarity_measure.relevance_table(prepared, synonimizer) if synonimizer
                      else similarity_measure.relevance_table(prepared))
            # (a mapping over the array: no K x D Python floats.  A rank of a multi-process run that is not the one to
            # print gets a K x 0 array -- east/parallel.py, table_rank --: rows without entries, as zip() made them)
            table = ScoreTable(wanted, text_titles[:scores.shape[1]], scores)
            return table if scores.size >= ARRAY_TABLE_MIN_SCORES else table.to_dict()
        return res

    i = 0
    total_scores = len(text_collection) * len(keyphrases)
    for keyphrase in keyphrases:
        if not keyphrase:
            continue
        res[keyphrase] = {}
        for j in range(len(text_collection)):
            i += 1
            logging.progress("Calculating matching scores", i, total_scores)
            res[keyphrase][text_titles[j]] = similarity_measure.relevance(
                keyphrases_prepared[keyphrase], text=j, synonimizer=synonimizer)
    logging.clear()
    return res


class KeyphraseGraph(object):
    """The keyphrase graph (applications.py:59-149) as arrays, the way ScoreTable is the table as an array: at BASELINE
    configs[2] a graph holds 10^5 .. 10^7 edges, the device writes them in well under a millisecond and a dict per edge
    costs seconds.  `keyphrases` is the input list (a node's id is its position in it); `support[p]` the number of texts
    position p occurs in (-1 for a position that is not a node where the graph was taken from a dict, which does not say);
    `node_ids` the positions that are nodes, in order; per edge, in the reference's order (sources in list order, a source's
    targets in list order), `edge_source` and `edge_target` (positions) and `edge_confidence` (float64).  Compares equal
    to the reference's dict with the same content; `.to_dict()` gives that dict."""

    __hash__ = None

    def __init__(self, keyphrases, support, node_ids, edge_source, edge_target, edge_confidence, referral_confidence,
                 relevance_threshold, support_threshold):
        self.keyphrases = list(keyphrases)
        self.support = np.asarray(support)
        self.node_ids = np.asarray(node_ids)
        self.edge_source, self.edge_target = np.asarray(edge_source), np.asarray(edge_target)
        self.edge_confidence = np.asarray(edge_confidence, dtype=np.float64)
        self.referral_confidence, self.relevance_threshold = referral_confidence, relevance_threshold
        self.support_threshold = support_threshold

    @classmethod
    def from_dict(cls, keyphrases, graph):
        """The reference's dict (what keyphrases_graph returns) as arrays."""
        support = np.full(len(keyphrases), -1, dtype=np.int64)
        node_ids = np.array([node["id"] for node in graph["nodes"]], dtype=np.int64)
        support[node_ids] = [node["support"] for node in graph["nodes"]]
        edges = graph["edges"]
        return cls(keyphrases, support, node_ids, np.array([e["source"] for e in edges], dtype=np.int64),
                   np.array([e["target"] for e in edges], dtype=np.int64),
                   np.array([e["confidence"] for e in edges], dtype=np.float64), graph["referral_confidence"],
                   graph["relevance_threshold"], graph["support_threshold"])

    @classmethod
    def from_device(cls, keyphrases, found, referral_confidence, relevance_threshold, support_threshold):
        """The arrays the device built (hip_backend.GraphArrays) as a graph over the keyphrase list.  The confidence is
        float(shared) / max(len(source_texts), 1) (applications.py:137), the same correctly rounded division, once per edge."""
        confidence = found.edge_shared.astype(np.float64) / np.maximum(found.support[found.edge_source], 1).astype(np.float64)
        return cls(keyphrases, found.support, found.kept, found.edge_source, found.edge_target, confidence,
                   referral_confidence, relevance_threshold, support_threshold)

    def to_dict(self):
        """The reference's own return type: {"nodes": [...], "edges": [...], the three thresholds}, plain Python values."""
        nodes = [{"id": position, "label": self.keyphrases[position], "support": support}
                 for position, support in zip(self.node_ids.tolist(), self.support[self.node_ids].tolist())]
        edges = [{"source": source, "target": target, "confidence": confidence}
                 for source, target, confidence in zip(self.edge_source.tolist(), self.edge_target.tolist(),
                                                       self.edge_confidence.tolist())]
        return {"nodes": nodes, "edges": edges, "referral_confidence": self.referral_confidence,
                "relevance_threshold": self.relevance_threshold, "support_threshold": self.support_threshold}

    def __eq__(self, other):
        if isinstance(other, KeyphraseGraph):
            other = other.to_dict()
        if not isinstance(other, dict):
            return NotImplemented
        return self.to_dict() == other

    def __ne__(self, other):
        result = self.__eq__(other)
        return result if result is NotImplemented else not result


def _device_applies(measure, texts, synonimizer, method, env):
    """Whether an application runs its main loop on the device: the measure scores into a table that stays there (it has
    `method`: relevance_graph, relevance_top or relevance_similar; None counts as absent: the measures over several
    devices or ranks), no synonimizer, distinct text titles, and the environment variable `env` (EAST_HIP_GRAPH,
    EAST_HIP_TOP, EAST_HIP_SIMILAR) is not `host` (the precedent: EAST_HIP_TEXT_PREP=host)."""
    titles = list(texts.keys())
    return (getattr(measure, method, None) is not None and not synonimizer
            and len(set(titles)) == len(titles) and os.environ.get(env, "device") != "host")


def _graph_on_device(keyphrases, texts, referral_confidence, relevance_threshold, support_threshold, measure, language):
    """keyphrases_graph with its main loop on the device: the keyphrases are scored as keyphrases_table scores them
    (empty ones skipped, duplicates collapsed: a keyphrase listed twice is two nodes over one row), the K x D table stays
    where the device wrote it, and the nodes and edges come back as arrays (csrc/graph.h).  None: no keyphrase to score
    (the host path says what the reference says then)."""
    keyphrases = list(keyphrases)
    wanted = [kp for kp in dict.fromkeys(keyphrases) if kp]              # applications.py:44-45
    if not wanted:
        return None
    measure.set_text_collection(list(texts.values()), language)
    row_of = {kp: k for k, kp in enumerate(wanted)}
    rows = np.array([row_of[kp] for kp in keyphrases], dtype=np.int32)   # (an empty keyphrase: KeyError, as table[""] raises)
    found = measure.relevance_graph([utils.prepare_text(kp) for kp in wanted], rows, referral_confidence,
                                    relevance_threshold, support_threshold)
    return KeyphraseGraph.from_device(keyphrases, found, referral_confidence, relevance_threshold, support_threshold)


def keyphrases_graph_arrays(keyphrases, texts, referral_confidence=0.6, relevance_threshold=0.25,
                            support_threshold=1, similarity_measure=None, synonimizer=None,
                            language=consts.Language.ENGLISH):
    """keyphrases_graph with the graph as arrays: a KeyphraseGraph (`.to_dict()` gives what keyphrases_graph returns; the
    formatters take it as it is).  Built on the device where keyphrases_graph builds it there; elsewhere the host path's
    dict, wrapped, so that a caller gets one type."""
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    if _device_applies(measure, texts, synonimizer, "relevance_graph", "EAST_HIP_GRAPH"):
        graph = _graph_on_device(keyphrases, texts, referral_confidence, relevance_threshold, support_threshold, measure,
                                 language)
        if graph is not None:
            return graph
    return KeyphraseGraph.from_dict(keyphrases, keyphrases_graph(keyphrases, texts, referral_confidence, relevance_threshold,
                                                                 support_threshold, measure, synonimizer, language))


def keyphrases_graph(keyphrases, texts, referral_confidence=0.6, relevance_threshold=0.25,
                     support_threshold=1, similarity_measure=None, synonimizer=None,
                     language=consts.Language.ENGLISH):
    """Keyphrase implication graph over a text corpus (reference east/applications.py:59-149).

    A keyphrase *occurs* in a text when its matching score reaches `relevance_threshold`; its
    *support* is the number of such texts.  Keyphrases with support below `support_threshold` are
    dropped; for every ordered pair (A, B) of the remaining ones an edge A -> B is drawn when at
    least `referral_confidence` of the texts containing A also contain B.

    :returns: {"nodes": [{"id", "label", "support"}], "edges": [{"source", "target", "confidence"}],
               "referral_confidence", "relevance_threshold", "support_threshold"}; node ids are the
               positions of the keyphrases in the input list.

    The main loop runs on the device, from the score table where the score call left it (_graph_on_device), when the
    measure has `relevance_graph`, no synonimizer is given, the text titles are distinct and EAST_HIP_GRAPH is not `host`;
    in every other case on the host, below.  The graph is the same either way.
    """
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    if _device_applies(measure, texts, synonimizer, "relevance_graph", "EAST_HIP_GRAPH"):
        graph = _graph_on_device(keyphrases, texts, referral_confidence, relevance_threshold, support_threshold, measure,
                                 language)
        if graph is not None:
            return graph.to_dict()
    table = keyphrases_table(keyphrases, texts, measure, synonimizer, language)

    if isinstance(table, ScoreTable) and len(set(table.text_titles)) == len(table.text_titles):
        return _graph_from_array(keyphrases, table, referral_confidence, relevance_threshold, support_threshold)

    occurs_in = {}
    if isinstance(table, ScoreTable):                        # (one comparison over the array instead of K x D look-ups)
        hits = table.scores >= relevance_threshold
        for keyphrase in keyphrases:
            found = set(table.text_titles[d] for d in np.flatnonzero(hits[table._row[keyphrase]]).tolist())
            occurs_in[keyphrase] = set(name for name in texts if name in found)
    else:
        for keyphrase in keyphrases:
            row = table[keyphrase]
            occurs_in[keyphrase] = set(name for name in texts if row[name] >= relevance_threshold)

    nodes = [{"id": position, "label": keyphrase, "support": len(occurs_in[keyphrase])}
             for position, keyphrase in enumerate(keyphrases)
             if len(occurs_in[keyphrase]) >= support_threshold]

    edges = []
    for source in nodes:
        source_texts = occurs_in[source["label"]]
        for target in nodes:
            if target is source:
                continue
            shared = len(source_texts & occurs_in[target["label"]])
            confidence = float(shared) / max(len(source_texts), 1)
            if confidence >= referral_confidence:
                edges.append({"source": source["id"], "target": target["id"], "confidence": confidence})

    return {"nodes": nodes, "edges": edges, "referral_confidence": referral_confidence,
            "relevance_threshold": relevance_threshold, "support_threshold": support_threshold}


def _graph_from_array(keyphrases, table, referral_confidence, relevance_threshold, support_threshold):
    """keyphrases_graph on the K x D score array: the same nodes and edges in the same order as the loops above (sources in
    the order of the keyphrase list, a source's targets in that order too), the pair counts by matrix products over
    blocks of sources instead of K^2 set intersections in Python (10 000 keyphrases: 10^8 of them)."""
    rows = np.array([table._row[kp] for kp in keyphrases], dtype=np.int64)            # (a repeated keyphrase: the same row twice)
    hits = table.scores[rows] >= relevance_threshold                                   # [n, D]
    support = hits.sum(axis=1)
    kept = np.flatnonzero(support >= support_threshold)
    nodes = [{"id": int(position), "label": keyphrases[position], "support": int(support[position])} for position in kept]
    edges = []
    h = hits[kept].astype(np.float32)                                                  # (counts up to D are exact in float32 below 2^24)
    sup = support[kept].astype(np.float64)
    block = max(1, (1 << 24) // max(len(kept), 1))
    for b in range(0, len(kept), block):
        shared = (h[b:b + block] @ h.T).astype(np.float64)                             # texts that hold source AND target
        confidence = shared / np.maximum(sup[b:b + block, None], 1.0)                  # float(shared) / max(len(source_texts), 1)
        src, dst = np.nonzero(confidence >= referral_confidence)
        off = src + b != dst                                                           # (no edge from a node to itself)
        for i, j, c in zip((src[off] + b).tolist(), dst[off].tolist(), confidence[src[off], dst[off]].tolist()):
            edges.append({"source": int(kept[i]), "target": int(kept[j]), "confidence": c})
    return {"nodes": nodes, "edges": edges, "referral_confidence": referral_confidence,
            "relevance_threshold": relevance_threshold, "support_threshold": support_threshold}


# ---- ranked keyphrases ---------------------------------------------------------------------------------------------------
TOP_MAX_N = 1024
_TOP_AXES = ("text", "keyphrase")


def _ranking_arguments(who, by, n, threshold, what):
    """The (by, n, threshold) of keyphrases_top and keyphrases_similar, checked: `who` is the caller's name in the messages,
    `what` its name for the threshold.  -> (axis, n, threshold)"""
    if by not in _TOP_AXES:
        raise ValueError("%s: by must be 'text' or 'keyphrase', not %r" % (who, by))
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= TOP_MAX_N:
        raise ValueError("%s: n must be an integer from 1 to %d, not %r" % (who, TOP_MAX_N, n))
    threshold = -np.inf if threshold is None else float(threshold)
    if threshold != threshold:
        raise ValueError("%s: the %s threshold is not a number" % (who, what))
    return _TOP_AXES.index(by), int(n), threshold


def _score_array(table, wanted, titles):
    """What keyphrases_table returned, a ScoreTable or a plain dict, as (the K x D array of the `wanted` keyphrases, the
    titles of its columns).  A plain dict: a repeated title holds its last column; a rank that does not print has none."""
    if isinstance(table, ScoreTable):
        scores = np.asarray(table.scores, dtype=np.float64)
    else:
        titles = [title for title in titles if title in table[wanted[0]]]
        scores = np.array([[table[kp][title] for title in titles] for kp in wanted], dtype=np.float64).reshape(len(wanted), -1)
    return scores, titles[:scores.shape[1]]


def _top_lists(found):
    """hip_backend.TopArrays -> per segment a list of (member, score), as _top_select gives it."""
    return [list(zip(index[:count], score[:count]))
            for count, index, score in zip(found.count.tolist(), found.index.tolist(), found.score.tolist())]


def _top_select(scores, axis, n, threshold):
    """The contract of include/east_hip.h ("Ranked keyphrases") in numpy: per segment (a column for axis 0, a row for
    axis 1) the eligible members (score >= threshold; a NaN never is) by score descending, member index ascending among
    equal scores (-0.0 == +0.0), the first n of them.  -> per segment a list of (member, score)."""
    scores = np.asarray(scores, dtype=np.float64)
    segments = scores.T if axis == 0 else scores
    found = []
    for values in segments:
        eligible = np.flatnonzero(values >= threshold)
        order = eligible[np.lexsort((eligible, -values[eligible]))][:n]      # (-(-0.0) == -(0.0) in the comparison: a tie)
        found.append(list(zip(order.tolist(), values[order].tolist())))
    return found


def _top_named(found, segment_names, member_names):
    return {segment: [(member_names[m], score) for m, score in entries] for segment, entries in zip(segment_names, found)}


def keyphrases_top(keyphrases, texts, n=10, by="text", relevance_threshold=None, similarity_measure=None, synonimizer=None,
                   language=consts.Language.ENGLISH):
    """The best-matching keyphrases of every text, or the best-matching texts of every keyphrase.

    :param keyphrases: raw keyphrase strings, taken as keyphrases_table takes them (empty ones are skipped, duplicates
                       collapse)
    :param texts: {text name: text}
    :param n: entries per text / keyphrase at most, 1 .. 1024
    :param by: "text" -- {text name: [(keyphrase, score), ...]}; "keyphrase" -- {keyphrase: [(text name, score), ...]}
    :param relevance_threshold: only scores >= it are listed (None: every score that is a number)
    :returns: the dict, its entries best first: by score descending and, among equal scores, in the order of the keyphrase
              list / of `texts`; plain Python values

    The selection runs on the device, on the score table where the score call left it (csrc/top.h), when the measure has
    `relevance_top`, no synonimizer is given, the text titles are distinct and EAST_HIP_TOP is not `host`; in every other
    case on the host, from keyphrases_table's array.  The result is the same either way.
    """
    axis, n, threshold = _ranking_arguments("keyphrases_top", by, n, relevance_threshold, "relevance")
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    titles = list(texts.keys())
    wanted = [kp for kp in dict.fromkeys(keyphrases) if kp]              # applications.py:44-45
    if not wanted:
        return {title: [] for title in titles} if axis == 0 else {}

    if _device_applies(measure, texts, synonimizer, "relevance_top", "EAST_HIP_TOP"):
        measure.set_text_collection(list(texts.values()), language)
        lists = _top_lists(measure.relevance_top([utils.prepare_text(kp) for kp in wanted], axis, n, threshold))
    else:
        scores, titles = _score_array(keyphrases_table(wanted, texts, measure, synonimizer, language), wanted, titles)
        lists = _top_select(scores, axis, n, threshold)
    return _top_named(lists, titles, wanted) if axis == 0 else _top_named(lists, wanted, titles)


# ---- similar texts and keyphrases ----------------------------------------------------------------------------------------
def _similarity_matrix(scores, axis):
    """The contract of include/east_hip.h ("Similar texts and keyphrases") in numpy: the profiles are the columns (axis 0)
    or the rows (axis 1) of the K x D array; S[a][b] = G_ab / (sqrt(q_a) * sqrt(q_b)), +0.0 where a q is zero, NaN on the
    diagonal.  -> the M x M array."""
    profiles = np.asarray(scores, dtype=np.float64)
    profiles = np.ascontiguousarray(profiles.T if axis == 0 else profiles)
    q = np.einsum("ml,ml->m", profiles, profiles)
    root = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        matrix = (profiles @ profiles.T) / (root[:, None] * root[None, :])
    matrix[(q == 0.0)[:, None] | (q == 0.0)[None, :]] = 0.0
    np.fill_diagonal(matrix, np.nan)
    return matrix


def keyphrases_similar(keyphrases, texts, n=10, by="text", similarity_threshold=None, similarity_measure=None, synonimizer=None,
                       language=consts.Language.ENGLISH):
    """The texts most like every text, or the keyphrases most like every keyphrase.  A text is its column of the
    keyphrase x text score table (its keyphrase profile), a keyphrase its row (its text profile); alike means the cosine
    of two profiles (+0.0 where a profile is all zeros).

    :param keyphrases: raw keyphrase strings, taken as keyphrases_table takes them (empty ones are skipped, duplicates
                       collapse)
    :param texts: {text name: text}
    :param n: entries per text / keyphrase at most, 1 .. 1024
    :param by: "text" -- {text name: [(other text name, similarity), ...]}; "keyphrase" -- {keyphrase: [(other keyphrase,
               similarity), ...]}
    :param similarity_threshold: only similarities >= it are listed (None: every similarity that is a number)
    :returns: the dict, its entries best first: by similarity descending and, among equal similarities, in the order of
              `texts` / of the keyphrase list; a member never lists itself; plain Python values

    The matrix and its ranking are made on the device, from the score table where the score call left it
    (csrc/similarity.h, csrc/top.h), when the measure has `relevance_similar`, no synonimizer is given, the text titles are
    distinct and EAST_HIP_SIMILAR is not `host`; in every other case on the host, from keyphrases_table's array.  The two
    paths sum in different orders: their similarities agree to (2 L + 16) * 2^-53 (L = the length of a profile) and they
    name the same members in the same order wherever neighbouring similarities lie further apart than twice that -- they
    are NOT promised to be the same bytes.
    """
    axis, n, threshold = _ranking_arguments("keyphrases_similar", by, n, similarity_threshold, "similarity")
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    titles = list(texts.keys())
    wanted = [kp for kp in dict.fromkeys(keyphrases) if kp]              # applications.py:44-45
    if not wanted:
        return {title: [] for title in titles} if axis == 0 else {}

    if _device_applies(measure, texts, synonimizer, "relevance_similar", "EAST_HIP_SIMILAR"):
        measure.set_text_collection(list(texts.values()), language)
        lists = _top_lists(measure.relevance_similar([utils.prepare_text(kp) for kp in wanted], axis, n, threshold))
    else:
        scores, titles = _score_array(keyphrases_table(wanted, texts, measure, synonimizer, language), wanted, titles)
        lists = _top_select(_similarity_matrix(scores, axis), 1, n, threshold)
    names = titles if axis == 0 else wanted
    return _top_named(lists, names, names)


# ---- text-to-text relatedness --------------------------------------------------------------------------------------------
_RELATED_ORIENTATIONS = ("directed", "symmetric")
_RELATED_HOST_CHUNK = 4096                  # strings a relevance_table call of the host path scores at a time


def _related_matrix(collections, score_rows, orientation):
    """The contract of include/east_hip.h ("Text-to-text relatedness") in numpy: collections[A] = the scored strings of
    text A, score_rows(strings) = their len(strings) x D scores.  F[A] = the mean of A's rows (+0.0 for a text without
    one), summed in numpy's order.  -> (R[D, D] with NaN on the diagonal, self[D], scored[D])."""
    D = len(collections)
    forward = np.zeros((D, D), dtype=np.float64)
    scored = np.array([len(strings) for strings in collections], dtype=np.int32)
    flat = [(a, s) for a, strings in enumerate(collections) for s in strings]
    for b in range(0, len(flat), _RELATED_HOST_CHUNK):
        part = flat[b:b + _RELATED_HOST_CHUNK]
        rows = np.asarray(score_rows([s for _, s in part]), dtype=np.float64).reshape(len(part), D)
        owner = np.array([a for a, _ in part], dtype=np.int64)
        for a in np.unique(owner).tolist():
            forward[a] += rows[owner == a].sum(axis=0)
    has = scored > 0
    forward[has] /= scored[has, None].astype(np.float64)
    own = forward.diagonal().copy()
    matrix = (forward + forward.T) * 0.5 if orientation == 1 else forward
    np.fill_diagonal(matrix, np.nan)
    return matrix, own, scored


def _related_on_host(texts, orientation, measure, language):
    """texts_related's matrix on the host: the strings of utils.text_to_strings_collection per text (the " " placeholder
    of a text without a kept token dropped), scored as keyphrases through relevance_table."""
    collections = [[s for s in utils.text_to_strings_collection(text) if s.replace(" ", "")] for text in texts.values()]
    measure.set_text_collection(list(texts.values()), language)
    return _related_matrix(collections, measure.relevance_table, orientation)


def texts_related(texts, n=10, orientation="symmetric", relatedness_threshold=None, similarity_measure=None,
                  language=consts.Language.ENGLISH):
    """The texts most related to every text, from the texts alone: no keyphrase file.  Every string of text A (its groups
    of three kept tokens, as the index holds them) is scored against the annotated suffix tree of text B as a keyphrase
    is; F[A][B] = the mean of those scores says how much of A's wording is found in B.

    :param texts: {text name: text}
    :param n: entries per text at most, 1 .. 1024
    :param orientation: "directed" -- F[A][B] as it is; "symmetric" -- (F[A][B] + F[B][A]) / 2
    :param relatedness_threshold: only values >= it are listed (None: every value that is a number)
    :returns: {text name: [(other text name, relatedness), ...]}, best first: by relatedness descending and, among equal
              values, in the order of `texts`; a text never lists itself; plain Python values

    The strings are scored out of the index, summed and ranked on the device (csrc/related.h, csrc/top.h) when the measure
    has `relevance_related`, the text titles are distinct and EAST_HIP_RELATED is not `host`; in every other case on the
    host: the strings go through relevance_table in chunks and the formula runs in numpy.  The two paths sum in different
    orders: their values agree to (max(c_A, c_B) + 4) * 2^-53 relative (c = a text's strings) and they name the same texts
    in the same order wherever neighbouring values lie further apart than twice that -- they are NOT promised to be the
    same bytes.
    """
    if orientation not in _RELATED_ORIENTATIONS:
        raise ValueError("texts_related: orientation must be 'symmetric' or 'directed', not %r" % (orientation,))
    _, n, threshold = _ranking_arguments("texts_related", "text", n, relatedness_threshold, "relatedness")
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    titles = list(texts.keys())
    if not titles:
        return {}
    code = _RELATED_ORIENTATIONS.index(orientation)
    if _device_applies(measure, texts, None, "relevance_related", "EAST_HIP_RELATED"):
        measure.set_text_collection(list(texts.values()), language)
        lists = _top_lists(measure.relevance_related(code, n, threshold))
    else:
        lists = _top_select(_related_on_host(texts, code, measure, language)[0], 1, n, threshold)
    return _top_named(lists, titles, titles)


# ---- text-to-text cosine similarity --------------------------------------------------------------------------------------
_TEXTS_SIMILAR_HOST_BLOCK = 4096            # units of the vector space a dense D x block array of the host path holds at a time


def _texts_cosine_matrix(doc_units, n_units, tfidf):
    """The contract of include/east_hip.h ("Text-to-text cosine similarity") in numpy: doc_units[d] = the units of text d's
    kept tokens, one entry a token, units numbered 0 .. n_units - 1.  x = count / max(n_d, 1), times 1 + ln(D / df) under
    tf-idf; norm = the root of the sum of the squares, 1.0 for a text without a posting; the products over the unit axis in
    column blocks of _TEXTS_SIMILAR_HOST_BLOCK.  -> (C[D, D] with NaN on the diagonal, self[D], postings[D])."""
    D = len(doc_units)
    doc, unit, weight = [], [], []
    df = np.zeros(n_units, dtype=np.int64)
    postings = np.zeros(D, dtype=np.int32)
    for d, ids in enumerate(doc_units):
        u, count = np.unique(np.asarray(ids, dtype=np.int64), return_counts=True)
        df[u] += 1
        postings[d] = u.size
        doc.append(np.full(u.size, d, dtype=np.int64))
        unit.append(u)
        weight.append(count.astype(np.float64) / float(max(len(ids), 1)))
    doc = np.concatenate(doc) if doc else np.zeros(0, np.int64)
    unit = np.concatenate(unit) if unit else np.zeros(0, np.int64)
    weight = np.concatenate(weight) if weight else np.zeros(0, np.float64)
    if tfidf and unit.size:
        weight = weight * (1.0 + np.log(float(D) / df[unit].astype(np.float64)))
    order = np.argsort(unit, kind="stable")
    doc, unit, weight = doc[order], unit[order], weight[order]
    gram = np.zeros((D, D), dtype=np.float64)
    square = np.zeros(D, dtype=np.float64)
    for lo in range(0, n_units, _TEXTS_SIMILAR_HOST_BLOCK):
        a, e = np.searchsorted(unit, [lo, lo + _TEXTS_SIMILAR_HOST_BLOCK])
        if a == e:
            continue
        block = np.zeros((D, min(_TEXTS_SIMILAR_HOST_BLOCK, n_units - lo)), dtype=np.float64)
        block[doc[a:e], unit[a:e] - lo] = weight[a:e]
        gram += block @ block.T
        square += np.einsum("du,du->d", block, block)
    norm = np.where(postings > 0, np.sqrt(square), 1.0)
    matrix = gram / (norm[:, None] * norm[None, :])
    own = matrix.diagonal().copy()
    np.fill_diagonal(matrix, np.nan)
    return matrix, own, postings


def _refuse_bm25(who, measure):
    """BM25 scores keyphrases against texts: the questions asked of the texts alone are the cosine measure's (the isinstance
    checks below would let its subclass through)."""
    if isinstance(measure, relevance.BM25RelevanceMeasure):
        raise ValueError("%s: BM25 scores keyphrases against texts; the texts alone are compared by the cosine measure "
                         "(use a CosineRelevanceMeasure), not by %s" % (who, type(measure).__name__))


def _texts_similar_on_host(texts, measure, language):
    """texts_similar's matrix on the host, without a device: the tokens of utils.tokenize(utils.prepare_text(text)) through
    the measure's own filter (at least 3 code points, not a stopword) and, in the stems space, its stemmer; the units
    numbered by first occurrence."""
    doc_units, number, _ = relevance.host_doc_units(texts.values(), measure, language)
    return _texts_cosine_matrix(doc_units, len(number), measure.term_weighting == consts.TermWeighting.TF_IDF)


def texts_similar(texts, n=10, similarity_threshold=None, similarity_measure=None, language=consts.Language.ENGLISH):
    """The texts most like every text, from the texts alone: no keyphrase file.  Alike means the cosine of two texts' term
    vectors -- tf or tf-idf weights over the words or the stems, as the cosine measure is set up (+0.0 for two texts without
    a common term).

    :param texts: {text name: text}
    :param n: entries per text at most, 1 .. 1024
    :param similarity_threshold: only cosines >= it are listed (None: every cosine that is a number)
    :param similarity_measure: a relevance.CosineRelevanceMeasure (None: CosineRelevanceMeasure()); any other measure raises
                               ValueError -- the AST measure's answer to the same question is texts_related
    :returns: {text name: [(other text name, cosine), ...]}, best first: by cosine descending and, among equal cosines, in
              the order of `texts`; a text never lists itself; plain Python values

    The matrix and its ranking are made on the device, straight out of the term index (csrc/cosine_texts.h, csrc/top.h),
    when the text titles are distinct and EAST_HIP_TEXTS_SIMILAR is not `host`; in every other case on the host, which then
    touches no device at all: the same tokens, the formula in numpy over column blocks of the term axis.  The two paths sum in
    different orders: their cosines agree to (t_ab + ceil(p_a / 64) + ceil(p_b / 64) + 176) * 2^-52 relative (t_ab = the
    common terms of two texts, p = a text's distinct terms) and they name the same texts in the same order wherever
    neighbouring cosines lie further apart than twice that -- they are NOT promised to be the same bytes.  (Python's
    upper() and the device's 1:1 upper-casing agree on every character but a few such as U+00DF.)
    """
    _, n, threshold = _ranking_arguments("texts_similar", "text", n, similarity_threshold, "similarity")
    measure = relevance.CosineRelevanceMeasure() if similarity_measure is None else similarity_measure
    if not isinstance(measure, relevance.CosineRelevanceMeasure):
        raise ValueError("texts_similar: the cosine of term vectors needs a CosineRelevanceMeasure, not %s (texts_related "
                         "answers with the AST measure)" % type(measure).__name__)
    _refuse_bm25("texts_similar", measure)
    titles = list(texts.keys())
    if not titles:
        return {}
    if _device_applies(measure, texts, None, "relevance_texts_similar", "EAST_HIP_TEXTS_SIMILAR"):
        measure.set_text_collection(list(texts.values()), language)
        lists = _top_lists(measure.relevance_texts_similar(n, threshold))
    else:
        lists = _top_select(_texts_similar_on_host(texts, measure, language)[0], 1, n, threshold)
    return _top_named(lists, titles, titles)


# ---- shingle overlap -----------------------------------------------------------------------------------------------------
_OVERLAP_ORIENTATIONS = ("directed", "symmetric")
OVERLAP_MAX_WORDS = 8


def _overlap_matrix(doc_sets, symmetric):
    """The contract of include/east_hip.h ("Shingle overlap") in plain Python: doc_sets[a] = the set of text a's shingles.
    Every entry is Python's int / int, the correctly rounded quotient.  -> (M[D, D] with NaN on the diagonal, self[D],
    shingles[D])."""
    D = len(doc_sets)
    size = [len(s) for s in doc_sets]
    matrix = np.zeros((D, D), dtype=np.float64)
    holders = {}
    for a, shingles in enumerate(doc_sets):
        for g in shingles:
            holders.setdefault(g, []).append(a)
    shared = np.zeros((D, D), dtype=np.int64)
    for texts in holders.values():
        if len(texts) > 1:
            at = np.asarray(texts, dtype=np.int64)
            shared[at[:, None], at[None, :]] += 1
    for a in range(D):
        for b in np.flatnonzero(shared[a]).tolist():
            i = int(shared[a, b])
            den = size[a] + size[b] - i if symmetric else size[a]
            matrix[a, b] = i / den if den else 0.0
    np.fill_diagonal(matrix, np.nan)
    return matrix, np.array([1.0 if n else 0.0 for n in size], dtype=np.float64), np.array(size, dtype=np.int32)


def _overlap_on_host(texts, stopwords, words, symmetric):
    """texts_overlap's matrix on the host, without a device: the tokens of utils.tokenize(utils.prepare_text(text)) with at
    least 3 code points, the stopwords as breaks; per text the set of its tuples of `words` consecutive words."""
    doc_sets = []
    for text in texts:
        tokens = [None if token in stopwords else token for token in utils.tokenize(utils.prepare_text(text)) if len(token) >= 3]
        doc_sets.append({tuple(tokens[j:j + words]) for j in range(len(tokens) - words + 1) if None not in tokens[j:j + words]})
    return _overlap_matrix(doc_sets, symmetric)


def _overlap_arguments(who, words, orientation, similarity_measure):
    if isinstance(words, bool) or int(words) != words or not 1 <= words <= OVERLAP_MAX_WORDS:
        raise ValueError("%s: words must be an integer in 1 .. %d, not %r" % (who, OVERLAP_MAX_WORDS, words))
    if orientation not in _OVERLAP_ORIENTATIONS:
        raise ValueError("%s: orientation must be 'symmetric' or 'directed', not %r" % (who, orientation))
    measure = relevance.CosineRelevanceMeasure(consts.VectorSpace.WORDS) if similarity_measure is None else similarity_measure
    if not isinstance(measure, relevance.CosineRelevanceMeasure):
        raise ValueError("%s: the shingles come from the term index of a CosineRelevanceMeasure, not %s" % (who, type(measure).__name__))
    _refuse_bm25(who, measure)
    return int(words), measure


def texts_overlap(texts, n=10, words=4, orientation="symmetric", overlap_threshold=None, similarity_measure=None,
                  language=consts.Language.ENGLISH):
    """The texts that contain the same WORDING as every text -- near-duplicates, lifted passages, one text quoted in a longer
    one --, from the texts alone.  A text is the set of its shingles, the phrases of `words` consecutive words (no stopword
    inside, as keyphrases_extract sees phrases; include/east_hip.h, "Shingle overlap").

    :param texts: {text name: text}
    :param n: entries per text at most, 1 .. 1024
    :param words: the words of a shingle, 1 .. 8
    :param orientation: "symmetric" -- the resemblance |A n B| / |A u B|; "directed" -- the containment |A n B| / |A| of
                        the listing text A in the listed text B
    :param overlap_threshold: only values >= it are listed (None: every value that is a number)
    :param similarity_measure: a relevance.CosineRelevanceMeasure, whose stopwords are the breaks (None:
                               CosineRelevanceMeasure("words")); any other raises ValueError
    :returns: {text name: [(other text name, value), ...]}, best first: by value descending and, among equal values, in the
              order of `texts`; a text never lists itself; plain Python values

    The matrix and its ranking are made on the device, from the token sequence the term index keeps (csrc/overlap.h,
    csrc/top.h), when the text titles are distinct and EAST_HIP_OVERLAP is not `host`; in every other case on the host,
    which then touches no device: sets of word tuples from the same tokens and the same one division of two integers.  The
    two paths give the SAME BYTES.
    """
    words, measure = _overlap_arguments("texts_overlap", words, orientation, similarity_measure)
    _, n, threshold = _ranking_arguments("texts_overlap", "text", n, overlap_threshold, "overlap")
    titles = list(texts.keys())
    if not titles:
        return {}
    if _device_applies(measure, texts, None, "relevance_texts_overlap", "EAST_HIP_OVERLAP"):
        measure.set_text_collection(list(texts.values()), language)
        lists = _top_lists(measure.relevance_texts_overlap(n, threshold, words, orientation))
    else:
        lists = _top_select(_overlap_on_host(texts.values(), measure.stopwords, words, orientation == "symmetric")[0], 1, n, threshold)
    return _top_named(lists, titles, titles)


# ---- shared passages -----------------------------------------------------------------------------------------------------
Passage = namedtuple("Passage", ("start", "words", "at", "text"))
PassagePair = namedtuple("PassagePair", ("other", "value", "starts", "covered", "found", "passages"))


def _passage_tokens(texts, stopwords):
    """Per text its positions: the tokens of utils.tokenize(utils.prepare_text(text)) with at least 3 code points -> (the
    words as they are, the same with None where the word is a stopword: a break)."""
    kept = [[token for token in utils.tokenize(utils.prepare_text(text)) if len(token) >= 3] for text in texts]
    return kept, [[None if token in stopwords else token for token in tokens] for tokens in kept]


def _passages_of_pair(ta, tb, words, min_words, per_pair):
    """The contract of include/east_hip.h ("Shared passages") in plain Python for one ordered pair: ta, tb = the positions
    of a and of b (None: a break).  -> (starts, covered, found, [(start, words, at), ...]), positions relative to their text."""
    first = {}
    for j in range(len(tb) - words + 1):
        g = tuple(tb[j:j + words])
        if None not in g:
            first.setdefault(g, j)
    shared = [j for j in range(len(ta) - words + 1) if None not in ta[j:j + words] and tuple(ta[j:j + words]) in first]
    covered, runs = set(), []
    for j in shared:
        covered.update(range(j, j + words))
        if runs and runs[-1][1] == j:
            runs[-1][1] = j + 1
        else:
            runs.append([j, j + 1])
    found = sorted(((e - j + words - 1, j) for j, e in runs if e - j + words - 1 >= min_words), key=lambda p: (-p[0], p[1]))
    kept = found[:per_pair] if per_pair else found
    return len(shared), len(covered), len(found), [(j, n, first[tuple(ta[j:j + words])]) for n, j in kept]


def _passages_arguments(words, min_words, per_pair):
    min_words = words if min_words is None else min_words
    if isinstance(min_words, bool) or int(min_words) != min_words or min_words < words:
        raise ValueError("texts_passages: min_words must be an integer that is at least words (%d), not %r" % (words, min_words))
    if isinstance(per_pair, bool) or int(per_pair) != per_pair or per_pair < 0:
        raise ValueError("texts_passages: per_pair must be an integer that is not negative (0 keeps every passage), not %r" % (per_pair,))
    return int(min_words), int(per_pair)


def texts_passages(texts, n=10, words=4, min_words=None, per_pair=5, orientation="symmetric", overlap_threshold=None, pairs=None,
                   similarity_measure=None, language=consts.Language.ENGLISH):
    """The passages two texts share, WHICH words: for a text a and another text b the maximal stretches of a in which every
    `words` consecutive words occur, in this order, somewhere in b (include/east_hip.h, "Shared passages").

    :param texts: {text name: text}
    :param n: by default every text is paired with the n others texts_overlap ranks for it -- with the same `words`,
              `orientation`, `overlap_threshold`, measure and language, in the same order
    :param words: the words of a shingle, 1 .. 8: the shortest stretch that counts as shared wording
    :param min_words: only passages of at least this many words are listed (None: `words`)
    :param per_pair: passages per pair at most, the longest first; 0 keeps all
    :param pairs: [(name of a, name of b), ...] replaces the ranking: these pairs, in this order; a pair may repeat
    :param similarity_measure: a relevance.CosineRelevanceMeasure, whose stopwords are the breaks (None:
                               CosineRelevanceMeasure("words")); any other raises ValueError
    :returns: {text name: [PassagePair(other, value, starts, covered, found, [Passage(start, words, at, text), ...]), ...]}:
              `value` the overlap value of the ranking (None under `pairs=`); `starts` the positions of the text at which a
              shingle of the other starts, `covered` the words of the text inside shared wording, `found` the passages of
              min_words words or more; per passage `start` and `at` = where it starts in the text and where its first shingle
              first starts in the other, both counted in the text's own kept tokens (at least 3 code points) from 0,
              `words` its length and `text` its words joined by one space; longest first, then by start

    Made on the device from the token sequence the term index keeps (csrc/passages.h) when the text titles are distinct and
    EAST_HIP_PASSAGES is not `host`; in every other case on the host in plain Python from the same tokens, which then
    touches no device.  The two paths give the SAME result.
    """
    words, measure = _overlap_arguments("texts_passages", words, orientation, similarity_measure)
    min_words, per_pair = _passages_arguments(words, min_words, per_pair)
    titles = list(texts.keys())
    number = {title: d for d, title in enumerate(titles)}
    if pairs is None:
        _, n, threshold = _ranking_arguments("texts_passages", "text", n, overlap_threshold, "overlap")
    else:
        pairs = [tuple(pair) for pair in pairs]
        for pair in pairs:
            if len(pair) != 2 or pair[0] not in number or pair[1] not in number or pair[0] == pair[1]:
                raise ValueError("texts_passages: a pair names two different texts of the collection, not %r" % (pair,))
    if not titles:
        return {}
    on_device = _device_applies(measure, texts, None, "shared_passages", "EAST_HIP_PASSAGES")
    if on_device:
        measure.set_text_collection(list(texts.values()), language)
    if pairs is None:
        if on_device:
            lists = _top_lists(measure.relevance_texts_overlap(n, threshold, words, orientation))
        else:
            lists = _top_select(_overlap_on_host(texts.values(), measure.stopwords, words, orientation == "symmetric")[0], 1, n, threshold)
        numbered = [(a, b, value) for a, entries in enumerate(lists) for b, value in entries]
        result = {title: [] for title in titles}
    else:
        numbered = [(number[a], number[b], None) for a, b in pairs]
        result = {}
    kept, positions = _passage_tokens(texts.values(), measure.stopwords)
    if on_device:
        found = measure.shared_passages([(a, b) for a, b, _ in numbered], words, min_words, per_pair)
        base, off = found.text_start.tolist(), found.pair_off.tolist()
        rows = list(zip(found.start.tolist(), found.words.tolist(), found.at.tolist()))
        per_pair_rows = [(s, c, f, [(j - base[a], m, at - base[b]) for j, m, at in rows[off[i]:off[i + 1]]])
                         for i, ((a, b, _), s, c, f) in enumerate(zip(numbered, found.starts.tolist(), found.covered.tolist(), found.found.tolist()))]
    else:
        per_pair_rows = [_passages_of_pair(positions[a], positions[b], words, min_words, per_pair) for a, b, _ in numbered]
    for (a, b, value), (starts, covered, count, passages) in zip(numbered, per_pair_rows):
        result.setdefault(titles[a], []).append(PassagePair(titles[b], value, starts, covered, count, [
            Passage(j, m, at, " ".join(kept[a][j:j + m])) for j, m, at in passages]))
    return result


# ---- clusters ------------------------------------------------------------------------------------------------------------
def _strongest_first(matrix):
    """The pairs a < b of a symmetric M x M array that are not NaN in the order of include/east_hip.h ("Clusters"): by
    weight descending (-0.0 == +0.0), then a, then b ascending.  -> (a, b, w); w is the upper triangle's own bytes."""
    a, b = np.triu_indices(matrix.shape[0], 1)
    w = matrix[a, b]
    edge = ~np.isnan(w)
    a, b, w = a[edge], b[edge], w[edge]
    order = np.lexsort((b, a, -(w + 0.0)))                  # (-0.0 + 0.0 is +0.0: the zeros tie)
    return a[order], b[order], w[order]


class _Sets(object):
    """Disjoint sets of 0 .. M - 1; the root of a set is its smallest member."""

    def __init__(self, M):
        self.parent = list(range(M))

    def find(self, v):
        parent = self.parent
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    def union(self, a, b):
        """-> (the root that stays, the root that went), or None when a and b are in one set already."""
        a, b = self.find(a), self.find(b)
        if a == b:
            return None
        a, b = min(a, b), max(a, b)
        self.parent[b] = a
        return a, b


def _roots(M, merge_a, merge_b, n):
    """labels[v] = the smallest member of v's cluster after the first n merges."""
    sets = _Sets(M)
    for i in range(n):
        sets.union(int(merge_a[i]), int(merge_b[i]))
    return [sets.find(v) for v in range(M)]


def _single_linkage(matrix):
    """The contract of include/east_hip.h ("Clusters") in plain Python: Kruskal's algorithm over the edges strongest
    first.  -> (merge_a, merge_b, merge_w), the forest's edges in that order."""
    matrix = np.asarray(matrix, dtype=np.float64)
    M = matrix.shape[0]
    a, b, w = _strongest_first(matrix)
    sets, took = _Sets(M), []
    for i in range(a.size):
        if len(took) == M - 1:
            break                                           # (a spanning tree: every later edge closes a cycle)
        if sets.union(int(a[i]), int(b[i])):
            took.append(i)
    took = np.asarray(took, dtype=np.int64)
    return a[took].astype(np.int32), b[took].astype(np.int32), w[took]


LINKAGES = ("single", "complete", "average")


class RefusedSimilarity(ValueError):
    """A matrix holds a similarity that complete or average linkage does not take (the host path's EAST_HIP_ERR_INVALID)."""


def _linkage_argument(who, linkage):
    if linkage not in LINKAGES:
        raise ValueError("%s: linkage must be 'single', 'complete' or 'average', not %r" % (who, linkage))
    return linkage


def _lance_williams(average, x, y, n, n2):
    """LW of include/east_hip.h ("Clusters"), elementwise: x the representative's values, y its partner's, n and n2 their
    sizes before the round as doubles."""
    lo = np.where(y < x, y, x)
    if not average:
        return lo
    hi = np.where(y < x, x, y)
    r = (n * x + n2 * y) / (n + n2)
    return np.where(r < lo, lo, np.where(r > hi, hi, r))


def _linkage_rounds(matrix, linkage, floor=None):
    """Complete or average linkage by the contract of include/east_hip.h ("Clusters"): rounds of reciprocal strongest
    pairs on a working copy, the contract's operations in the contract's order, whole arrays at a time.
    -> (merge_a, merge_b, merge_w, rounds); ValueError for a similarity the linkage does not take."""
    average = _linkage_argument("_linkage_rounds", linkage) == "average"
    if linkage == "single":
        raise ValueError("_linkage_rounds: single linkage is _single_linkage's")
    S = np.asarray(matrix, dtype=np.float64)
    M = S.shape[0]
    floor = -np.inf if floor is None or floor != floor else float(floor)
    rows, cols = np.triu_indices(M, 1)
    upper = S[rows, cols]
    refused = ~np.isfinite(upper) if average else np.isnan(upper)
    if refused.any():
        at = int(np.flatnonzero(refused)[0])
        raise RefusedSimilarity("clusters: S[%d][%d] is %s: %s linkage takes no such similarity"
                         % (rows[at], cols[at], "not finite" if average else "a NaN", linkage))
    W = np.zeros((M, M), dtype=np.float64)
    W[rows, cols] = upper
    W[cols, rows] = upper
    alive = np.arange(M)                                    # the representatives, ascending
    size = np.ones(M, dtype=np.float64)
    found, rounds = [], 0
    with np.errstate(all="ignore"):
        while alive.size > 1:
            A = alive.size
            sub = W[np.ix_(alive, alive)]
            own = np.arange(A)
            masked = sub.copy()
            masked[own, own] = -np.inf
            pick = np.argmax(masked, axis=1)                # (the first of equal weights: the smallest other end; -0.0 == +0.0)
            alone = pick == own                             # (every weight is minus infinity: the diagonal came first)
            pick[alone] = np.where(own[alone] == 0, 1, 0)
            reciprocal = (pick[pick] == own) & (own < pick)
            weight = sub[own, pick]
            merged = reciprocal & (weight >= floor)
            if not merged.any():
                break
            u, v = own[merged], pick[merged]                # positions in alive: the ends that stay, the ends that die
            found.extend(zip(weight[merged].tolist(), [rounds] * u.size, alive[u].tolist(), alive[v].tolist()))
            partner = own.copy()
            partner[u] = v
            has = partner != own
            stay = np.ones(A, dtype=bool)
            stay[v] = False
            keep = own[stay]
            kp, kh = partner[keep], has[keep]
            n, n2 = size[alive[keep]], size[alive[kp]]
            # rows u (and u') against columns v (and v'), every value in the orientation of the pair with u < v
            a, b = sub[np.ix_(keep, keep)], sub[np.ix_(keep, kp)]
            c, d = sub[np.ix_(kp, keep)], sub[np.ix_(kp, kp)]
            cu = np.where(kh[None, :], _lance_williams(average, a, b, n[None, :], n2[None, :]), a)
            cu2 = np.where(kh[None, :], _lance_williams(average, c, d, n[None, :], n2[None, :]), c)
            new = np.where(kh[:, None], _lance_williams(average, cu, cu2, n[:, None], n2[:, None]), cu)
            K = keep.size
            is_upper = np.arange(K)[:, None] < np.arange(K)[None, :]
            new = np.where(is_upper, new, new.T)
            changed = kh[:, None] | kh[None, :]
            block = W[np.ix_(alive[keep], alive[keep])]
            W[np.ix_(alive[keep], alive[keep])] = np.where(changed, new, block)
            size[alive[u]] += size[alive[v]]
            alive = alive[keep]
            rounds += 1
    found.sort(key=lambda m: (-(m[0] + 0.0), m[1], m[2]))
    return (np.asarray([m[2] for m in found], dtype=np.int32), np.asarray([m[3] for m in found], dtype=np.int32),
            np.asarray([m[0] for m in found], dtype=np.float64), rounds)


class Clustering(object):
    """Clusters of named members (single linkage unless `linkage` says otherwise).

    names     the members, in index order
    linkage   "single", "complete" or "average"
    merges    the dendrogram, [(name_a, name_b, similarity)], strongest merge first (index of a < index of b);
              merge_a, merge_b (int32), merge_w (float64) hold the same as arrays of member indexes
    labels    per member the smallest member index of its cluster -- None when neither a threshold nor k was given
    clusters  lists of names: the clusters ordered by their smallest member, the members in index order -- or None
    """

    def __init__(self, names, merge_a, merge_b, merge_w, labels=None, linkage="single"):
        self.names = list(names)
        self.linkage = linkage
        self.merge_a = np.asarray(merge_a, dtype=np.int32)
        self.merge_b = np.asarray(merge_b, dtype=np.int32)
        self.merge_w = np.asarray(merge_w, dtype=np.float64)
        self.merges = [(self.names[a], self.names[b], w) for a, b, w in
                       zip(self.merge_a.tolist(), self.merge_b.tolist(), self.merge_w.tolist())]
        self.labels = None if labels is None else [int(x) for x in labels]
        self.clusters = None
        if self.labels is not None:
            members = {}
            for v, root in enumerate(self.labels):
                members.setdefault(root, []).append(self.names[v])
            self.clusters = [members[root] for root in sorted(members)]

    def to_linkage(self):
        """The (M - 1) x 4 array of scipy.cluster.hierarchy: per merge the two clusters joined (a member is its index,
        the cluster merge i made is M + i; the smaller id first), the SIMILARITY in the distance column -- it falls where
        SciPy's distances rise -- and the size of the new cluster.  Defined when the dendrogram is one tree."""
        M = len(self.names)
        if len(self.merge_a) != M - 1 or M < 1:
            raise ValueError("to_linkage: the dendrogram is not one tree (%d merges of %d members)" % (len(self.merge_a), M))
        sets, cluster, size = _Sets(M), list(range(M)), [1] * M
        Z = np.zeros((M - 1, 4), dtype=np.float64)
        for i in range(M - 1):
            a, b = sets.find(int(self.merge_a[i])), sets.find(int(self.merge_b[i]))
            ids = sorted((cluster[a], cluster[b]))
            kept, gone = sets.union(a, b)
            size[kept] += size[gone]
            cluster[kept] = M + i
            Z[i] = (ids[0], ids[1], self.merge_w[i], size[kept])
        return Z


def _cut_arguments(who, threshold, k):
    if threshold is not None and k is not None:
        raise ValueError("%s: give a threshold or a number of clusters k, not both" % who)
    if threshold is not None:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("%s: the threshold is not a number" % who)
    if k is not None:
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError("%s: k must be an integer of at least 1, not %r" % (who, k))
        k = int(k)
    return threshold, k


def _clustering_of_index(names, index, threshold, k, linkage="single"):
    """The Clustering of the clusters `index` (a hip_backend index) has just built."""
    merge_a, merge_b, merge_w = index.clusters_merges()
    labels = None
    if threshold is not None or k is not None:
        labels = index.clusters_cut(threshold, k)[0]
    return Clustering(names, merge_a, merge_b, merge_w, labels, linkage)


def _clustering_of_matrix(names, matrix, threshold, k, linkage="single"):
    """The same on the host, from an M x M array."""
    if linkage == "single":
        merge_a, merge_b, merge_w = _single_linkage(matrix)
    else:
        merge_a, merge_b, merge_w = _linkage_rounds(matrix, linkage, threshold)[:3]
    M, F = len(names), len(merge_a)
    labels = None
    if threshold is not None:
        n = 0
        while n < F and merge_w[n] >= threshold:
            n += 1
        labels = _roots(M, merge_a, merge_b, n)
    elif k is not None:
        labels = _roots(M, merge_a, merge_b, max(0, min(F, M - k)))
    return Clustering(names, merge_a, merge_b, merge_w, labels, linkage)


def _clusters_on_device(measure, linkage, threshold, *arguments):
    """measure.relevance_clusters: as ever for single linkage; complete and average take the threshold as their floor."""
    if linkage == "single":
        return measure.relevance_clusters(*arguments)
    try:
        parameters = inspect.signature(measure.relevance_clusters).parameters
    except (TypeError, ValueError):                         # (no signature to read: the call itself will tell)
        parameters = None
    if parameters is not None and not any(p.kind == p.VAR_KEYWORD for p in parameters.values()) \
            and not ("linkage" in parameters and "floor" in parameters):
        raise ValueError("%s.relevance_clusters takes no linkage and floor: it serves single linkage only, not linkage=%r"
                         % (type(measure).__name__, linkage))
    return measure.relevance_clusters(*arguments, linkage=linkage, floor=threshold)


def texts_clusters(texts, threshold=None, k=None, similarity_measure=None, language=consts.Language.ENGLISH, linkage="single"):
    """The groups the texts fall into, from the texts alone: agglomerative clustering -- single linkage, or with
    linkage="complete" / "average" those linkages (include/east_hip.h, "Clusters"; a threshold is then also the floor
    below which no merge is made, so the dendrogram ends there) -- of the matrix texts_related (an AST measure: the
    symmetric relatedness) or texts_similar (a CosineRelevanceMeasure: the cosine of the term vectors) ranks.

    :param texts: {text name: text}
    :param threshold: flat clusters = the connected components of "similarity >= threshold"
    :param k: flat clusters by number: the strongest merges are applied until k clusters are left (there are never fewer
              than the matrix has connected components); at most one of threshold and k -- with neither, only the
              dendrogram is filled
    :param similarity_measure: None: relevance.ASTRelevanceMeasure()
    :returns: a Clustering

    The matrix is built and clustered on the device (csrc/clusters.h) when the measure has `relevance_clusters`, the text
    titles are distinct and EAST_HIP_CLUSTERS is not `host`; in every other case the matrix comes from the host paths of
    texts_related / texts_similar and Kruskal's algorithm runs here.  The two matrices differ in their last bits by their
    own contracts, so a near-tie may merge differently; on ONE matrix both give the same bytes.
    """
    threshold, k = _cut_arguments("texts_clusters", threshold, k)
    linkage = _linkage_argument("texts_clusters", linkage)
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    _refuse_bm25("texts_clusters", measure)
    titles = list(texts.keys())
    if not titles:
        return Clustering([], [], [], [], None if threshold is None and k is None else [], linkage)
    if _device_applies(measure, texts, None, "relevance_clusters", "EAST_HIP_CLUSTERS"):
        measure.set_text_collection(list(texts.values()), language)
        return _clustering_of_index(titles, _clusters_on_device(measure, linkage, threshold), threshold, k, linkage)
    if isinstance(measure, relevance.CosineRelevanceMeasure):
        matrix = _texts_similar_on_host(texts, measure, language)[0]
    else:
        matrix = _related_on_host(texts, 1, measure, language)[0]
    return _clustering_of_matrix(titles, matrix, threshold, k, linkage)


def texts_overlap_clusters(texts, words=4, threshold=None, k=None, linkage="single", similarity_measure=None,
                           language=consts.Language.ENGLISH):
    """The groups the texts fall into by their shared wording: agglomerative clustering (texts_clusters' linkages, cuts and
    result) of the symmetric matrix texts_overlap ranks, the resemblance of the texts' sets of `words`-word shingles.  Single
    linkage at a resemblance threshold gives the near-duplicate groups.

    :param texts: {text name: text}
    :param words: the words of a shingle, 1 .. 8
    :param threshold, k, linkage: as texts_clusters takes them
    :param similarity_measure: a relevance.CosineRelevanceMeasure (None: CosineRelevanceMeasure("words")); any other raises ValueError
    :returns: a Clustering

    On the device (csrc/overlap.h, csrc/clusters.h, csrc/linkage.h) when the text titles are distinct and EAST_HIP_OVERLAP is
    not `host`; in every other case the host path's matrix and the host clustering, no device touched.  The two matrices are
    the same bytes.
    """
    words, measure = _overlap_arguments("texts_overlap_clusters", words, "symmetric", similarity_measure)
    threshold, k = _cut_arguments("texts_overlap_clusters", threshold, k)
    linkage = _linkage_argument("texts_overlap_clusters", linkage)
    titles = list(texts.keys())
    if not titles:
        return Clustering([], [], [], [], None if threshold is None and k is None else [], linkage)
    if _device_applies(measure, texts, None, "relevance_overlap_clusters", "EAST_HIP_OVERLAP"):
        measure.set_text_collection(list(texts.values()), language)
        index = measure.relevance_overlap_clusters(words, linkage, None if linkage == "single" else threshold)
        return _clustering_of_index(titles, index, threshold, k, linkage)
    matrix = _overlap_on_host(texts.values(), measure.stopwords, words, True)[0]
    return _clustering_of_matrix(titles, matrix, threshold, k, linkage)


def keyphrases_clusters(keyphrases, texts, by="text", threshold=None, k=None, similarity_measure=None, synonimizer=None,
                        language=consts.Language.ENGLISH, linkage="single"):
    """The groups the texts (by="text") or the keyphrases (by="keyphrase") fall into by their profiles in the keyphrase x
    text score table: agglomerative clustering (single linkage, or linkage="complete" / "average" as texts_clusters takes
    it) of the cosine matrix keyphrases_similar ranks.

    :param keyphrases: raw keyphrase strings, taken as keyphrases_table takes them (empty ones are skipped, duplicates
                       collapse)
    :param texts: {text name: text}
    :param threshold, k: as texts_clusters takes them
    :returns: a Clustering of the text names or of the keyphrases

    On the device (csrc/similarity.h, csrc/clusters.h) when the measure has `relevance_clusters`, no synonimizer is given,
    the text titles are distinct and EAST_HIP_CLUSTERS is not `host`; in every other case on the host, from
    keyphrases_table's array.
    """
    if by not in _TOP_AXES:
        raise ValueError("keyphrases_clusters: by must be 'text' or 'keyphrase', not %r" % (by,))
    axis = _TOP_AXES.index(by)
    threshold, k = _cut_arguments("keyphrases_clusters", threshold, k)
    linkage = _linkage_argument("keyphrases_clusters", linkage)
    measure = similarity_measure or relevance.ASTRelevanceMeasure()
    titles = list(texts.keys())
    wanted = [kp for kp in dict.fromkeys(keyphrases) if kp]              # applications.py:44-45
    if not wanted or not titles:
        return Clustering([], [], [], [], None if threshold is None and k is None else [], linkage)
    if _device_applies(measure, texts, synonimizer, "relevance_clusters", "EAST_HIP_CLUSTERS"):
        measure.set_text_collection(list(texts.values()), language)
        index = _clusters_on_device(measure, linkage, threshold, [utils.prepare_text(kp) for kp in wanted], axis)
        return _clustering_of_index(titles if axis == 0 else wanted, index, threshold, k, linkage)
    scores, titles = _score_array(keyphrases_table(wanted, texts, measure, synonimizer, language), wanted, titles)
    return _clustering_of_matrix(titles if axis == 0 else wanted, _similarity_matrix(scores, axis), threshold, k, linkage)


# ---- phrase extraction -----------------------------------------------------------------------------------------------------
Phrase = namedtuple("Phrase", ("text", "words", "count", "texts", "score"))
EXTRACT_MAX_WORDS = 8


def _extract_arguments(n, max_words, min_words, min_count, min_texts):
    """The arguments of keyphrases_extract as integers, or ValueError with the line that names the one that is wrong."""
    values = []
    for name, value in (("n", n), ("max_words", max_words), ("min_words", min_words), ("min_count", min_count),
                        ("min_texts", min_texts)):
        if isinstance(value, bool) or int(value) != value:
            raise ValueError("keyphrases_extract: %s must be an integer, not %r" % (name, value))
        values.append(int(value))
    n, max_words, min_words, min_count, min_texts = values
    if n < 0:
        raise ValueError("keyphrases_extract: n must not be negative (0 keeps every candidate), not %d" % n)
    if not 1 <= max_words <= EXTRACT_MAX_WORDS:
        raise ValueError("keyphrases_extract: max_words must lie in 1 .. %d, not %d" % (EXTRACT_MAX_WORDS, max_words))
    if not 1 <= min_words <= max_words:
        raise ValueError("keyphrases_extract: min_words must lie in 1 .. max_words, not %d" % min_words)
    if min_count < 1:
        raise ValueError("keyphrases_extract: min_count must be at least 1, not %d" % min_count)
    if min_texts < 1:
        raise ValueError("keyphrases_extract: min_texts must be at least 1, not %d" % min_texts)
    return values


def _phrases_on_host(texts, stopwords, n, max_words, min_words, min_count, min_texts):
    """The contract of include/east_hip.h ("Phrase extraction") in plain Python, without a device: the tokens of
    utils.tokenize(utils.prepare_text(text)) with at least 3 code points, the stopwords as breaks; the n-grams named level
    by level through dicts.  -> ([(text, words, count, texts, first, first_text, term ids)], best first and cut by n; the
    candidates before the cut)."""
    term, doc, words, number = [], [], [], {}
    for d, text in enumerate(texts):
        for token in utils.tokenize(utils.prepare_text(text)):
            if len(token) < 3:
                continue
            term.append(-1 if token in stopwords else number.setdefault(token, len(number)))
            doc.append(d)
            words.append(token)
    T = len(term)
    candidates = []
    below = None                                        # (ids per position, count per id, open per id, the level's survivors)
    for level in range(1, max_words + 1):
        groups = {}
        if level == 1:
            for j in range(T):
                if term[j] >= 0:
                    groups.setdefault(term[j], []).append(j)
        else:
            ids = below[0]
            for j in range(T - level + 1):
                e = j + level - 1
                if ids[j] >= 0 and doc[e] == doc[j] and term[e] >= 0:
                    groups.setdefault((ids[j], term[e]), []).append(j)
        ids, count, is_open, found = [-1] * T, [], [], []
        for positions in groups.values():
            if len(positions) < min_count:
                continue
            for j in positions:
                ids[j] = len(count)
            n_texts = 1 + sum(1 for a, b in zip(positions, positions[1:]) if doc[a] != doc[b])
            found.append((level, len(positions), n_texts, positions[0]))
            count.append(len(positions))
            is_open.append(False)
            if below is not None:
                for j in (positions[0], positions[0] + 1):
                    if below[1][below[0][j]] == len(positions):
                        below[2][below[0][j]] = True
        if below is not None:
            candidates += [c for c, o in zip(below[3], below[2]) if not o]
        below = (ids, count, is_open, found)
        if not found:
            break
    candidates += [c for c, o in zip(below[3], below[2]) if not o]
    candidates = sorted((c for c in candidates if c[0] >= min_words and c[2] >= min_texts), key=lambda c: (c[0], c[3]))
    candidates.sort(key=lambda c: -c[0] * c[1])         # (stable: words, then first, among equal scores)
    kept = candidates[:n] if n else candidates
    return [(" ".join(words[first:first + w]), w, c, t, first, doc[first], term[first:first + w])
            for w, c, t, first in kept], len(candidates)


def keyphrases_extract(texts, n=100, max_words=3, min_words=1, min_count=2, min_texts=1, similarity_measure=None,
                       language=consts.Language.ENGLISH):
    """Keyphrase candidates out of the texts themselves: the repeated phrases of min_words to max_words words, counted
    exactly, without those that only ever occur inside one longer phrase of the same count, best first (the contract:
    include/east_hip.h, "Phrase extraction").

    :param texts: {text name: text} or a sequence of texts (bytes or str), in the order that numbers the positions
    :param n: phrases at most; 0 = every candidate
    :param max_words: the longest phrase, 1 .. 8; min_words: the shortest, 1 .. max_words
    :param min_count: occurrences a phrase needs; min_texts: texts it must occur in
    :param similarity_measure: a relevance.CosineRelevanceMeasure in the `words` space, whose stopwords are the breaks
                               (None: CosineRelevanceMeasure("words") with the default stopwords); any other raises ValueError
    :returns: [Phrase(text, words, count, texts, score)], score = count * words, by score descending, then words
              ascending, then first occurrence; `text` is the upper-cased words joined by one space -- a line of a keyphrase
              file

    The phrases are extracted on the device from the measure's term index (csrc/phrases.h) unless EAST_HIP_EXTRACT is
    `host`; then plain Python computes the same contract from the same tokens and touches no device.  Nothing in it is
    floating point: the two give the same bytes.
    """
    n, max_words, min_words, min_count, min_texts = _extract_arguments(n, max_words, min_words, min_count, min_texts)
    measure = relevance.CosineRelevanceMeasure(consts.VectorSpace.WORDS) if similarity_measure is None else similarity_measure
    if not isinstance(measure, relevance.CosineRelevanceMeasure) or measure.vector_space != consts.VectorSpace.WORDS:
        raise ValueError("keyphrases_extract: phrases are extracted from the term index of a CosineRelevanceMeasure in the "
                         "'words' space, not %s" % (type(measure).__name__ if not isinstance(measure, relevance.CosineRelevanceMeasure)
                                                    else "the '%s' space" % measure.vector_space))
    _refuse_bm25("keyphrases_extract", measure)
    texts = list(texts.values()) if isinstance(texts, Mapping) else list(texts)
    if os.environ.get("EAST_HIP_EXTRACT", "device") == "host":
        rows = _phrases_on_host(texts, measure.stopwords, n, max_words, min_words, min_count, min_texts)[0]
        return [Phrase(text, w, c, t, c * w) for text, w, c, t, _, _, _ in rows]
    measure.set_text_collection(texts, language)
    found = measure.extract_phrases(n, max_words, min_words, min_count, min_texts)
    return [Phrase(text, w, c, t, c * w) for text, w, c, t in
            zip(found.strings(), found.words.tolist(), found.count.tolist(), found.texts.tolist())]


# ---- characteristic terms --------------------------------------------------------------------------------------------------
Term = namedtuple("Term", ("text", "value", "texts", "df"))
TermGroup = namedtuple("TermGroup", ("names", "terms"))


def _terms_arguments(n, min_texts):
    for name, value in (("n", n), ("min_texts", min_texts)):
        if isinstance(value, bool) or int(value) != value:
            raise ValueError("texts_terms: %s must be an integer, not %r" % (name, value))
    if not 1 <= n <= TOP_MAX_N:
        raise ValueError("texts_terms: n must lie in 1 .. %d, not %d" % (TOP_MAX_N, n))
    if min_texts < 1:
        raise ValueError("texts_terms: min_texts must be at least 1, not %d" % min_texts)
    return int(n), int(min_texts)


def _terms_vectors(doc_units, n_units, tfidf, group, n_groups):
    """The contract of include/east_hip.h ("Characteristic terms") in numpy: doc_units[d] = the units of text d's kept
    tokens, one entry a token; group[d] in 0 .. n_groups - 1.  x = count / max(n_d, 1), times 1 + ln(D / df) under tf-idf;
    norm = the root of the sum of the squares, 1.0 for a text without a posting; q = x / norm; per (group, unit) the sum of
    q over the group's texts in ascending order, divided by the group's members.
    -> (members[G], offsets[G + 1], unit, value, texts per entry in (group, unit) order, df[n_units])."""
    D = len(doc_units)
    group = np.asarray(group, dtype=np.int64)
    members = np.bincount(group, minlength=n_groups).astype(np.int32)
    df = np.zeros(n_units, dtype=np.int64)
    doc, unit, q = [], [], []
    for d, ids in enumerate(doc_units):
        u, count = np.unique(np.asarray(ids, dtype=np.int64), return_counts=True)
        df[u] += 1
        doc.append(np.full(u.size, d, dtype=np.int64))
        unit.append(u)
        q.append(count.astype(np.float64) / float(max(len(ids), 1)))
    if tfidf:
        q = [x * (1.0 + np.log(float(D) / df[u].astype(np.float64))) for x, u in zip(q, unit)]
    q = [x / (np.sqrt(np.sum(x * x)) if x.size else 1.0) for x in q]
    doc = np.concatenate(doc) if doc else np.zeros(0, np.int64)
    unit = np.concatenate(unit) if unit else np.zeros(0, np.int64)
    q = np.concatenate(q) if q else np.zeros(0, np.float64)
    key = group[doc] * max(n_units, 1) + unit
    order = np.argsort(key, kind="stable")                  # (the texts ascend inside a (group, unit) run)
    key, q = key[order], q[order]
    heads = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if key.size else np.zeros(0, np.int64)
    e_group, e_unit = key[heads] // max(n_units, 1), key[heads] % max(n_units, 1)
    texts = np.diff(np.concatenate((heads, [key.size]))).astype(np.int32)
    value = np.add.reduceat(q, heads) / members[e_group].astype(np.float64) if key.size else np.zeros(0, np.float64)
    offsets = np.searchsorted(e_group, np.arange(n_groups + 1)).astype(np.int64)
    return members, offsets, e_unit.astype(np.int32), value, texts, df.astype(np.int32)


def _terms_ranked(unit, value, texts, min_texts, n):
    """The contract's order of one group's entries: those with texts >= min_texts by value descending, then unit ascending;
    the first n -> indexes into the arrays."""
    keep = np.flatnonzero(texts >= min_texts)
    return keep[np.lexsort((unit[keep], -value[keep]))][:n]


def _terms_on_host(doc_units, n_units, tfidf, group, n_groups, n, min_texts):
    """-> (members[G], per group [(unit, value, texts, df)], best first)."""
    members, offsets, unit, value, texts, df = _terms_vectors(doc_units, n_units, tfidf, group, n_groups)
    lists = []
    for g in range(n_groups):
        a, e = offsets[g], offsets[g + 1]
        best = a + _terms_ranked(unit[a:e], value[a:e], texts[a:e], min_texts, n)
        lists.append([(int(unit[i]), float(value[i]), int(texts[i]), int(df[unit[i]])) for i in best])
    return members, lists


def _groups_of_labels(labels):
    """Clustering.labels (per member the smallest member of its cluster) -> (group[d], the groups ordered by their smallest member)."""
    roots = sorted(set(labels))
    number = {root: g for g, root in enumerate(roots)}
    return [number[root] for root in labels], len(roots)


def texts_terms(texts, n=10, min_texts=1, similarity_measure=None, language=consts.Language.ENGLISH, threshold=None, k=None,
                linkage="single"):
    """What every text -- or, with a threshold or k, every cluster of texts -- is about: its characteristic terms, the units
    of the cosine measure's vector space (words or stems) with the largest mean normalised tf or tf-idf weight (the
    contract: include/east_hip.h, "Characteristic terms").

    :param texts: {text name: text}
    :param n: terms per group at most, 1 .. 1024
    :param min_texts: a term is listed when that many texts of its group hold it
    :param similarity_measure: a relevance.CosineRelevanceMeasure (None: CosineRelevanceMeasure()); any other raises ValueError
    :param threshold, k, linkage: with one of threshold and k the texts are clustered exactly as texts_clusters clusters them
                                  with the same measure, linkage and cut, on the same index, and the groups are the clusters,
                                  ordered by their smallest member; with neither, every text is a group of its own
    :returns: [TermGroup(names=[text names], terms=[Term(text, value, texts, df), ...])]: value = the mean over the group's
              texts of weight / norm, texts = the group's texts that hold the term, df = the collection's; by value
              descending, then in the order the terms first occur in the collection

    The sums and the ranking are made on the device (csrc/terms.h) when the text titles are distinct and EAST_HIP_TERMS is not
    `host`; in every other case on the host, which then touches no device at all: the same tokens, the contract in numpy, the
    clusters through the host clustering.  The two paths agree to (texts + max ceil(p_d / 64) / 2 + 48) * 2^-53 relative each of the exact value and name
    the same terms in the same order wherever neighbouring values lie further apart than twice that -- they are NOT promised
    to be the same bytes.
    """
    n, min_texts = _terms_arguments(n, min_texts)
    threshold, k = _cut_arguments("texts_terms", threshold, k)
    linkage = _linkage_argument("texts_terms", linkage)
    measure = relevance.CosineRelevanceMeasure() if similarity_measure is None else similarity_measure
    if not isinstance(measure, relevance.CosineRelevanceMeasure):
        raise ValueError("texts_terms: characteristic terms are read off the term index of a CosineRelevanceMeasure, not %s"
                         % type(measure).__name__)
    _refuse_bm25("texts_terms", measure)
    titles = list(texts.keys())
    if not titles:
        return []
    clustered = threshold is not None or k is not None
    tfidf = measure.term_weighting == consts.TermWeighting.TF_IDF
    if _device_applies(measure, texts, None, "relevance_terms", "EAST_HIP_TERMS"):
        measure.set_text_collection(list(texts.values()), language)
        group, n_groups = None, len(titles)
        if clustered:
            found = _clustering_of_index(titles, _clusters_on_device(measure, linkage, threshold), threshold, k, linkage)
            group, n_groups = _groups_of_labels(found.labels)
        arrays = measure.relevance_terms(n, min_texts, group)
        names = measure.unit_names()
        lists = [[(names[u], v, t, f) for u, v, t, f in zip(arrays.unit[g, :c].tolist(), arrays.value[g, :c].tolist(),
                                                           arrays.texts[g, :c].tolist(), arrays.df[g, :c].tolist())]
                 for g, c in enumerate(arrays.count.tolist())]
    else:
        doc_units, number, _ = relevance.host_doc_units(texts.values(), measure, language)
        group, n_groups = list(range(len(titles))), len(titles)
        if clustered:
            matrix = _texts_cosine_matrix(doc_units, len(number), tfidf)[0]
            group, n_groups = _groups_of_labels(_clustering_of_matrix(titles, matrix, threshold, k, linkage).labels)
        names = list(number)                                # (numbered by first occurrence: the dict's own order)
        lists = [[(names[u], v, t, f) for u, v, t, f in found]
                 for found in _terms_on_host(doc_units, len(number), tfidf, group, n_groups, n, min_texts)[1]]
    group = list(range(len(titles))) if group is None else group
    members = [[] for _ in range(n_groups)]
    for d, g in enumerate(group):
        members[g].append(titles[d])
    return [TermGroup(members[g], [Term(*t) for t in lists[g]]) for g in range(n_groups)]
