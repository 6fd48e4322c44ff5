# -*- coding: utf-8 -*-
"""Relevance measures (reference east/relevance.py:16-168).

Both keep the reference surface (set_text_collection / relevance) and add the batched path the GPU needs: ONE build
call for the whole text collection and `relevance_table`, ONE score call for all keyphrases.
ASTRelevanceMeasure: the documents become one device-resident shard of annotated suffix arrays.
CosineRelevanceMeasure (`-s cosine`): the documents become one device-resident term index -- postings (term, document,
count) -- and a keyphrase is scored against every document by walking the posting lists of its terms.
BM25RelevanceMeasure (`-s bm25`): Okapi BM25 as a second score call of that term index.
"""
import itertools
import os

import numpy as np

from east import consts
from east import exceptions
from east import hip_backend
from east import utils
from east.asts import utils as ast_utils


class RelevanceMeasure(object):

    relevance_texts_similar = None      # (the cosine of two texts' term vectors: the cosine measure alone)
    text_similarity_matrix = None
    relevance_clusters = None           # (single-linkage clusters on the device: the single-device measures)

    def set_text_collection(self, texts, language=consts.Language.ENGLISH):
        raise NotImplementedError()

    def relevance(self, keyphrase, text, synonimizer=None):
        # text is the index of the text to measure the relevance to
        raise NotImplementedError()


def synonym_variants(query, synonimizer):
    """The queries easa.py:27-33 scores for a keyphrase under a synonimizer: every word of the
    (prepared) keyphrase may be replaced by one of its synonyms -- the product of the per-word
    alternatives, synonyms first, each variant the concatenation of its words.  `synonimizer`
    is anything with get_synonyms() -> {word: [synonyms]}; a word missing from the mapping
    raises KeyError exactly as the reference's dictionary look-up does."""
    alternatives = synonym_alternatives(query, synonimizer)
    if has_empty_variant(alternatives):
        raise ZeroDivisionError("float division by zero")              # easa.py:134 on an empty variant
    return ["".join(words) for words in itertools.product(*alternatives)]


def has_empty_variant(alternatives):
    """Whether the product of the per-word alternatives holds an empty string: no words at all, or an empty
    alternative for every word."""
    return all("" in alts for alts in alternatives)


def synonym_alternatives(query, synonimizer):
    """Per word of the prepared keyphrase: its synonyms followed by the word itself (what synonym_variants forms the
    product of).  Linear in the number of words: this is what the row cache is keyed by and what the multi-rank path
    validates on every rank.  Raises KeyError for a word missing from the mapping."""
    synonyms = synonimizer.get_synonyms()
    return tuple(tuple(synonyms[word]) + (word,) for word in utils.tokenize(query))


class _Shard(object):
    """The device index of a measure plus a one-row score cache.  Shared by the measure and its
    per-document views without a reference back to either, so that dropping the measure releases
    the device handle at once (no reference cycle waiting for the garbage collector)."""

    def __init__(self):
        self.index = None
        self.row_cache = (None, None, None)
        self.host_symbols = None

    def row(self, query, normalized, synonimizer=None):
        q = query.replace(" ", "")
        # (the synonym row is keyed by the per-word alternatives -- linear in the words, the product is only formed on a
        # miss: a synonimizer whose mapping changes, or a new one at a collected one's address, must not get a stale row)
        key = (q, bool(normalized)) if synonimizer is None else ("synonyms", synonym_alternatives(query, synonimizer))
        if self.row_cache[0] != key:
            if synonimizer is not None:
                # easa.py:27-34: max over the variants, scored with normalized=True whatever was asked for
                variants = synonym_variants(query, synonimizer)
                qs, qo = hip_backend.pack_queries(variants, keep_spaces=True)
                row = self.index.score_table_grouped(qs, qo, [0, len(variants)], True)[0]
            else:
                if not q:
                    raise ZeroDivisionError("float division by zero")          # easa.py:134
                qs, qo = hip_backend.pack_queries([q])
                row = self.index.score_table(qs, qo, normalized)[0]
            self.row_cache = (key, None, row)
        return self.row_cache[2]

    def symbols(self, doc):
        """The EASA string of one document as code points (host copy, fetched once per build)."""
        if self.host_symbols is None:
            self.host_symbols = ast_utils.reference_code_points(self.index.symbols())
        off = self.index.doc_offsets
        return self.host_symbols[int(off[doc]):int(off[doc + 1])]

    def suffix_scores(self, query, normalized, doc):
        q = query.replace(" ", "")
        if not q:
            raise ZeroDivisionError("float division by zero")                  # easa.py:134
        qs, qo = hip_backend.pack_queries([q])
        table, suf = self.index.score_table(qs, qo, normalized, want_suffix=True)
        return float(table[0, doc]), {q[i:]: float(suf[doc, i]) for i in range(len(q))}


class _DocumentAST(object):
    """What `measure.asts[i]` is in the reference: something with .score()."""

    def __init__(self, shard, doc):
        self._shard, self._doc = shard, doc

    def score(self, query, normalized=True, synonimizer=None, return_suffix_scores=False):
        if synonimizer:                                                         # easa.py:27-34
            return float(self._shard.row(query, normalized, synonimizer)[self._doc])
        if return_suffix_scores:                                                # easa.py:132-137
            return self._shard.suffix_scores(query, normalized, self._doc)
        return self._shard.row(query, normalized)[self._doc]

    # the rest of the AST surface (base.py:28-34), from this document's tables in the shard
    def traverse(self, callback, order=consts.TraversalOrder.DEPTH_FIRST_PRE_ORDER):
        from east.asts import intervals
        index, d = self._shard.index, self._doc
        t = index.tables(d, names=("suftab", "lcptab", "anntab", "childtab_down"))
        left = index.lcp_interval_lefts(d)
        if order == consts.TraversalOrder.DEPTH_FIRST_POST_ORDER:
            visits = intervals.post_order(t["lcptab"], t["anntab"], left)
        elif order == consts.TraversalOrder.DEPTH_FIRST_PRE_ORDER:
            visits = intervals.pre_order(t["lcptab"], t["anntab"], left, t["childtab_down"], t["suftab"],
                                         self._shard.symbols(d))
        else:
            raise NotImplementedError                                           # easa.py:87-89
        for visit in visits:
            callback(visit)


class ASTRelevanceMeasure(RelevanceMeasure):

    def __init__(self, ast_algorithm=consts.ASTAlgorithm.EASA, normalized=True, device=None):
        super(ASTRelevanceMeasure, self).__init__()
        if ast_algorithm not in list(consts.ASTAlgorithm):
            from east import exceptions
            raise exceptions.NoSuchASTAlgorithm(name=ast_algorithm)
        self.ast_algorithm = ast_algorithm
        self.normalized = normalized
        self.device = device
        self._shard = _Shard()

    @property
    def index(self):
        return self._shard.index

    @index.setter
    def index(self, value):
        self._shard.index = value

    # HOT LOOP A (relevance.py:34-49) as one batched build
    def set_text_collection(self, texts, language=consts.Language.ENGLISH):
        texts = list(texts)
        self.texts = texts
        self.language = language
        if os.environ.get("EAST_HIP_TEXT_PREP", "device") == "device":
            # utils.text_to_strings_collection + make_unique_endings (relevance.py:44-45) on the device
            if self.index is None:
                self.index = hip_backend.HipIndex(self.device)
            self.index.build_texts(list(texts))
            self.asts = [_DocumentAST(self._shard, d) for d in range(len(texts))]
            self._shard.row_cache = (None, None, None)
            self._shard.host_symbols = None
            return
        collections = [utils.text_to_strings_collection(text) for text in texts]   # relevance.py:44-45
        self.set_strings_collections(collections)

    def set_strings_collections(self, collections):
        """collections[d] = the strings collection of document d (one AST each)."""
        parts = [ast_utils.strings_to_symbols(sc) for sc in collections]
        if any(ast_utils.is_tagged(p) for p in parts):       # text at or above U+0A00 somewhere: one encoding for the shard
            parts = [ast_utils.tag_terminators(p) for p in parts]
        self._build_from_parts(parts, collections)

    def _build_from_parts(self, parts, collections):
        doc_offsets = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([p.size for p in parts], out=doc_offsets[1:])
        n_strings = np.array([len(sc) for sc in collections], dtype=np.int32)
        symbols = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        if self.index is None:
            self.index = hip_backend.HipIndex(self.device)
        self.index.build(symbols, doc_offsets, n_strings)
        self.asts = [_DocumentAST(self._shard, d) for d in range(len(parts))]
        self._shard.row_cache = (None, None, None)
        self._shard.host_symbols = ast_utils.reference_code_points(symbols)

    def relevance(self, keyphrase, text, synonimizer=None):
        """relevance.py:51-53: the score of a prepared keyphrase in text number `text`."""
        return float(self._shard.row(keyphrase, self.normalized, synonimizer or None)[text])

    # HOT LOOP B (applications.py:43-52) as one batched call
    def relevance_table(self, prepared_keyphrases, synonimizer=None):
        """K prepared keyphrases -> K x D float64 array of scores.  With a synonimizer every
        keyphrase is expanded into its variants (synonym_variants), all variants of all keyphrases
        are scored in the one call and a segmented max on the device folds them back (easa.py:27-34)."""
        if synonimizer:
            groups = [synonym_variants(kp, synonimizer) for kp in prepared_keyphrases]
            offsets = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([len(g) for g in groups], out=offsets[1:])
            qs, qo = hip_backend.pack_queries([v for g in groups for v in g], keep_spaces=True)
            return self.index.score_table_grouped(qs, qo, offsets, True)
        queries = [kp.replace(" ", "") for kp in prepared_keyphrases]
        if not all(queries):
            raise ZeroDivisionError("float division by zero")
        qs, qo = hip_backend.pack_queries(queries)
        return self.index.score_table(qs, qo, self.normalized)

    def _score_resident(self, prepared_keyphrases):
        """Scores K prepared keyphrases as relevance_table does and leaves the K x D table on the device."""
        queries = [kp.replace(" ", "") for kp in prepared_keyphrases]
        if not all(queries):
            raise ZeroDivisionError("float division by zero")
        qs, qo = hip_backend.pack_queries(queries)
        self.index.set_keyphrases(qs, qo)
        self.index.score_resident(self.normalized)

    # HOT LOOP C (applications.py:59-149) on the device, from the table the score call leaves there
    def relevance_graph(self, prepared_keyphrases, rows, referral_confidence, relevance_threshold, support_threshold):
        """The keyphrase graph of K prepared keyphrases: they are scored as relevance_table scores them, the K x D table
        stays on the device and the graph is built from it there.  rows[p] = the keyphrase (0 .. K - 1) of node position
        p.  -> hip_backend.GraphArrays."""
        self._score_resident(prepared_keyphrases)
        return self.index.graph(rows, relevance_threshold, support_threshold, referral_confidence)

    def relevance_top(self, prepared_keyphrases, axis, n, threshold=-np.inf):
        """The n best keyphrases of every text (axis hip_backend.TOP_BY_TEXT) or the n best texts of every keyphrase
        (TOP_BY_KEYPHRASE): the keyphrases are scored as relevance_graph scores them, the K x D table stays on the device
        and the selection runs on it there.  -> hip_backend.TopArrays."""
        self._score_resident(prepared_keyphrases)
        return self.index.top(axis, n, threshold)

    def relevance_similar(self, prepared_keyphrases, axis, n, threshold=-np.inf):
        """The n most similar other texts of every text (axis hip_backend.TOP_BY_TEXT: the cosine of two columns of the
        score table) or the n most similar other keyphrases of every keyphrase (TOP_BY_KEYPHRASE: of two rows).  The
        keyphrases are scored exactly as relevance_top scores them; the table, the M x M similarity matrix and its ranking
        stay on the device (csrc/similarity.h).  -> hip_backend.TopArrays."""
        self._score_resident(prepared_keyphrases)
        return self.index.similar(axis, n, threshold)

    def relevance_related(self, orientation, n, threshold=-np.inf):
        """The n most related other texts of every text of the collection: every string of text A is scored against the
        tree of text B as a keyphrase is, straight out of the index (csrc/related.h); orientation
        hip_backend.RELATED_DIRECTED or RELATED_SYMMETRIC.  -> hip_backend.TopArrays."""
        return self.index.related(self.normalized, orientation, n, threshold)

    def relatedness_matrix(self, orientation):
        """The D x D matrix relevance_related ranks -> (matrix, self, scored) of HipIndex.related_matrix."""
        self.index.related_build(self.normalized, orientation)
        return self.index.related_matrix()

    def relevance_clusters(self, prepared_keyphrases=None, axis=None, linkage="single", floor=None):
        """Clusters of a matrix of this measure, built and clustered where it lies (csrc/clusters.h, csrc/linkage.h).
        Without keyphrases: the texts, by their symmetric relatedness (relatedness_matrix).  With keyphrases: the texts
        (axis hip_backend.TOP_BY_TEXT) or the keyphrases (TOP_BY_KEYPHRASE) by the cosine of their score profiles, the
        matrix relevance_similar ranks.  linkage: "single", "complete" or "average"; floor: only merges of at least this
        similarity are made (None: all).  -> the index: its clusters_merges(), clusters_cut(), similarity_matrix() /
        related_matrix() speak of what was built."""
        if prepared_keyphrases is None:
            self.index.related_build(self.normalized, hip_backend.RELATED_SYMMETRIC)
            self.index.clusters_build(hip_backend.GRAPH_SOURCE_RELATED, linkage, floor)
        else:
            self._score_resident(prepared_keyphrases)
            self.index.similarity(axis)
            self.index.clusters_build(hip_backend.GRAPH_SOURCE_SIMILARITY, linkage, floor)
        return self.index


class MultiDeviceASTRelevanceMeasure(ASTRelevanceMeasure):
    """ASTRelevanceMeasure over several GPUs of this process (`east -g N`): the documents are sharded over the devices --
    contiguous blocks balanced by size, one AST shard per device, no collective on the build path --, every shard scores
    its own documents and the K x D_local blocks are assembled by one all-gather (hip_backend.HipGroup ->
    east_hip_score_table_multi: RCCL between distinct devices).  Same surface and same numbers as the single-device
    measure (relevance.py:27-53); no torch, no child processes.  `devices`: a count or a list of device ordinals."""

    def __init__(self, ast_algorithm=consts.ASTAlgorithm.EASA, normalized=True, devices=1):
        super(MultiDeviceASTRelevanceMeasure, self).__init__(ast_algorithm, normalized, None)
        # (EAST_HIP_GROUP_DEVICES=0,0,1: the shards' device ordinals spelled out -- logical shards on one device, the tests)
        spelled = os.environ.get("EAST_HIP_GROUP_DEVICES", "")
        self.devices = [int(d) for d in spelled.split(",")] if spelled and isinstance(devices, int) else devices
        self.group = None
        self._shards = []

    relevance_graph = None       # (the table is spread over the devices: keyphrases_graph keeps its host path)
    relevance_top = None         # (... and so does keyphrases_top)
    relevance_similar = None     # (... and keyphrases_similar)
    relevance_related = None     # (every shard holds its own documents' trees only: texts_related keeps its host path)
    relatedness_matrix = None
    relevance_clusters = None    # (no device holds a whole matrix: the clusters keep their host path)

    def _after_build(self, n_docs):
        self._shards = []
        for view in self.group.shards:
            shard = _Shard()
            shard.index = view
            self._shards.append(shard)
        self.asts = []
        for d in range(n_docs):
            s = int(np.searchsorted(self.group.first_doc, d, side="right")) - 1
            self.asts.append(_DocumentAST(self._shards[s], int(d - self.group.first_doc[s])))
        self._row = (None, None)

    def set_text_collection(self, texts, language=consts.Language.ENGLISH):
        texts = list(texts)
        self.texts = texts
        self.language = language
        if self.group is None:
            self.group = hip_backend.HipGroup(self.devices)
        if os.environ.get("EAST_HIP_TEXT_PREP", "device") == "device":
            self.group.build_texts(texts)
            self._after_build(len(texts))
            return
        self.set_strings_collections([utils.text_to_strings_collection(text) for text in texts])

    def _build_from_parts(self, parts, collections):
        doc_offsets = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([p.size for p in parts], out=doc_offsets[1:])
        n_strings = np.array([len(sc) for sc in collections], dtype=np.int32)
        if self.group is None:
            self.group = hip_backend.HipGroup(self.devices)
        self.group.build(np.concatenate(parts), doc_offsets, n_strings)
        self._after_build(len(parts))                        # (the shard views keep their slices of the symbols)

    def relevance(self, keyphrase, text, synonimizer=None):
        key = (keyphrase, bool(self.normalized), None if not synonimizer else synonym_alternatives(keyphrase, synonimizer))
        if self._row[0] != key:
            self._row = (key, self.relevance_table([keyphrase], synonimizer or None)[0])
        return float(self._row[1][text])

    def relevance_table(self, prepared_keyphrases, synonimizer=None):
        if synonimizer:
            # (the segmented max over the variants runs per shard: the blocks side by side are the table)
            groups = [synonym_variants(kp, synonimizer) for kp in prepared_keyphrases]
            offsets = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([len(g) for g in groups], out=offsets[1:])
            qs, qo = hip_backend.pack_queries([v for g in groups for v in g], keep_spaces=True)
            blocks = [view.score_table_grouped(qs, qo, offsets, True) for view in self.group.shards if view.n_docs]
            return np.concatenate(blocks, axis=1)
        queries = [kp.replace(" ", "") for kp in prepared_keyphrases]
        if not all(queries):
            raise ZeroDivisionError("float division by zero")
        qs, qo = hip_backend.pack_queries(queries)
        return self.group.score_table(qs, qo, self.normalized)


def default_stopwords():
    """nltk's English stopword list, upper-cased (utils.py:41-46), or None where nltk or its corpus is not there."""
    try:
        from nltk.corpus import stopwords
        return frozenset(utils.prepare_text(word) for word in stopwords.words("english"))
    except (ImportError, LookupError):
        return None


class CosineRelevanceMeasure(RelevanceMeasure):
    """relevance.py:56-168: the cosine between a document's and a keyphrase's term vectors.

    Tokens are tokenize_and_filter's (utils.py:41-46): [\\w']+ over the prepared text, at least 3 code points, not a
    stopword.  The terms are the tokens (`words`) or their stems (`stems`); a document's weights are
    tf = count / max(n_d, 1), times idf = 1 + ln(D / df) under `tf-idf`; the keyphrase's are count / max(its kept
    tokens, 1) over the terms of the collection.  The index is built on the device (hip_backend.HipCosineIndex); the
    keyphrases' few tokens are prepared here.

    stopwords: None = nltk's English list where nltk is installed, else none (`stopwords_source` says which: "nltk",
    "none", "given"); or any words, upper-cased here.  `stopwords` holds the set that is used.
    stemmer: anything with .stem(str) -> str; None = nltk's SnowballStemmer(language) for `stems` -- without nltk
    StemmerUnavailableException, at once, before any device work.
    """

    def __init__(self, vector_space=consts.VectorSpace.STEMS, term_weighting=consts.TermWeighting.TF_IDF, device=None,
                 stopwords=None, stemmer=None):
        super(CosineRelevanceMeasure, self).__init__()
        if vector_space == consts.VectorSpace.LEMMATA:
            raise exceptions.LemmataUnavailableException()
        if vector_space not in consts.VectorSpace:
            raise exceptions.NoSuchVectorSpace(name=vector_space)
        if term_weighting not in consts.TermWeighting:
            raise exceptions.NoSuchTermWeighting(name=term_weighting)
        self._snowball = None
        if vector_space == consts.VectorSpace.STEMS and stemmer is None:
            try:
                from nltk.stem import snowball
            except ImportError:
                raise exceptions.StemmerUnavailableException()
            self._snowball = snowball
        self.vector_space = vector_space
        self.term_weighting = term_weighting
        self.device = device
        self.stemmer = stemmer
        if stopwords is None:
            found = default_stopwords()
            self.stopwords = found if found is not None else frozenset()
            self.stopwords_source = "nltk" if found is not None else "none"
        else:
            self.stopwords = frozenset(utils.prepare_text(word) for word in stopwords)
            self.stopwords_source = "given"
        self.index = None
        self._stem_class = None
        self._row = (None, None)

    def set_text_collection(self, texts, language=consts.Language.ENGLISH):
        texts = list(texts)
        self.texts = texts
        self.language = language
        if self._snowball is not None:
            self.stemmer = self._snowball.SnowballStemmer(language)
        if self.index is None:
            self.index = hip_backend.HipCosineIndex(self.device)
        self.index.build_texts(texts, sorted(self.stopwords))
        self._stem_class = None
        if self.vector_space == consts.VectorSpace.STEMS:
            # every distinct term stemmed once; a class per stem, numbered by its smallest term id
            classes = {}
            term_class = [classes.setdefault(self.stemmer.stem(term), len(classes)) for term in self.index.terms()]
            self.index.set_classes(term_class, len(classes))
            self._stem_class = classes
        self._row = (None, None)

    def _query_terms(self, query):
        """The kept tokens of a prepared keyphrase (tokenize_and_filter), stemmed in the `stems` space."""
        tokens = [t for t in utils.tokenize(query) if len(t) >= 3 and t not in self.stopwords]
        if self.vector_space == consts.VectorSpace.STEMS:
            return [self.stemmer.stem(t) for t in tokens]
        return tokens

    def relevance_table(self, prepared_keyphrases, synonimizer=None):
        """K prepared keyphrases -> K x D float64 array of scores (relevance.py:150-168 for every pair).  The synonimizer
        is accepted and ignored, as the reference does."""
        return self._score(prepared_keyphrases, True)

    def relevance_graph(self, prepared_keyphrases, rows, referral_confidence, relevance_threshold, support_threshold):
        """The keyphrase graph of K prepared keyphrases (ASTRelevanceMeasure.relevance_graph): the query ids are prepared
        as relevance_table prepares them, the table stays on the device."""
        self._score(prepared_keyphrases, False)
        return self.index.graph(rows, relevance_threshold, support_threshold, referral_confidence)

    def relevance_top(self, prepared_keyphrases, axis, n, threshold=-np.inf):
        """The n best members of every text or keyphrase (ASTRelevanceMeasure.relevance_top); the table stays on the device."""
        self._score(prepared_keyphrases, False)
        return self.index.top(axis, n, threshold)

    def relevance_similar(self, prepared_keyphrases, axis, n, threshold=-np.inf):
        """The n most similar other members of every text or keyphrase (ASTRelevanceMeasure.relevance_similar)."""
        self._score(prepared_keyphrases, False)
        return self.index.similar(axis, n, threshold)

    def relevance_texts_similar(self, n, threshold=-np.inf):
        """The n most similar other texts of every text of the collection: the cosine of their term vectors in this
        measure's vector space and weighting, straight out of the term index (csrc/cosine_texts.h); after
        set_text_collection.  -> hip_backend.TopArrays."""
        return self.index.texts_similar(self.term_weighting == consts.TermWeighting.TF_IDF, n, threshold)

    def text_similarity_matrix(self):
        """The D x D matrix relevance_texts_similar ranks -> (matrix, self, postings) of HipCosineIndex.texts_matrix."""
        self.index.texts_build(self.term_weighting == consts.TermWeighting.TF_IDF)
        return self.index.texts_matrix()

    def relevance_clusters(self, prepared_keyphrases=None, axis=None, linkage="single", floor=None):
        """Clusters of a matrix of this measure, built and clustered where it lies
        (ASTRelevanceMeasure.relevance_clusters).  Without keyphrases: the texts, by the cosine of their term vectors
        (text_similarity_matrix).  With keyphrases: the texts or the keyphrases by the cosine of their score profiles.
        -> the index."""
        if prepared_keyphrases is None:
            self.index.texts_build(self.term_weighting == consts.TermWeighting.TF_IDF)
            self.index.clusters_build(hip_backend.GRAPH_SOURCE_COSINE_TEXTS, linkage, floor)
        else:
            self._score(prepared_keyphrases, False)
            self.index.similarity(axis)
            self.index.clusters_build(hip_backend.GRAPH_SOURCE_SIMILARITY, linkage, floor)
        return self.index

    def text_overlap_matrix(self, words=4, orientation="symmetric"):
        """The D x D matrix of shared w-word shingles of the indexed collection: the resemblance |A n B| / |A u B|
        ("symmetric") or the containment |A n B| / |A| of the row's text in the column's ("directed"; include/east_hip.h,
        "Shingle overlap"; csrc/overlap.h); after set_text_collection.  Shingles are made of words whatever the vector space.
        -> (matrix, self, shingles) of HipCosineIndex.overlap_matrix."""
        self.index.overlap_build(words, hip_backend.OVERLAP_ORIENTATIONS.index(orientation))
        return self.index.overlap_matrix()

    def relevance_texts_overlap(self, n, threshold=-np.inf, words=4, orientation="symmetric"):
        """The n other texts every text of the collection shares most w-word shingles with (text_overlap_matrix, ranked
        where it lies).  -> hip_backend.TopArrays."""
        return self.index.texts_overlap(words, hip_backend.OVERLAP_ORIENTATIONS.index(orientation), n, threshold)

    def relevance_overlap_clusters(self, words=4, linkage="single", floor=None):
        """Clusters of the symmetric overlap matrix, built and clustered where it lies.  -> the index."""
        self.index.overlap_build(words, hip_backend.OVERLAP_SYMMETRIC)
        self.index.clusters_build(hip_backend.GRAPH_SOURCE_OVERLAP, linkage, floor)
        return self.index

    def shared_passages(self, pairs, words=4, min_words=None, per_pair=5):
        """For every (a, b) of `pairs` (text numbers of the indexed collection) the passages of a whose every `words`
        consecutive words occur in b, longest first (include/east_hip.h, "Shared passages"; csrc/passages.h); after
        set_text_collection.  Passages are made of words whatever the vector space.  -> hip_backend.PassageArrays."""
        pairs = list(pairs)
        return self.index.passages([a for a, _ in pairs], [b for _, b in pairs], words, min_words, per_pair)

    def extract_phrases(self, n=0, max_words=3, min_words=1, min_count=2, min_texts=1):
        """The repeated phrases of the indexed collection as keyphrase candidates, best first (include/east_hip.h, "Phrase
        extraction"; csrc/phrases.h); after set_text_collection, in the `words` space: a phrase is made of words, not of
        stems.  n = 0: every candidate.  -> hip_backend.PhraseArrays."""
        if self.vector_space != consts.VectorSpace.WORDS:
            raise ValueError("extract_phrases: phrases are made of words, not of %s (use vector_space='words')" % self.vector_space)
        return self.index.phrases(n, max_words, min_words, min_count, min_texts)

    def relevance_terms(self, n, min_texts=1, groups=None):
        """The characteristic terms of every text of the collection (groups None) or of every group of texts (groups[d] =
        the group of text d): per group the n units of this measure's vector space with the largest mean normalised
        weight among those that min_texts of its texts hold (include/east_hip.h, "Characteristic terms"; csrc/terms.h);
        after set_text_collection.  -> hip_backend.TermArrays; unit_names() names the units."""
        return self.index.terms(self.term_weighting == consts.TermWeighting.TF_IDF, n, min_texts, groups)

    def unit_names(self):
        """The units of the vector space in id order: the words, or in the stems space the stem of every class."""
        if self._stem_class is None:
            return self.index.terms()
        names = [None] * len(self._stem_class)
        for stem, number in self._stem_class.items():
            names[number] = stem
        return names

    def _query_ids(self, prepared_keyphrases):
        """(ids int32, offsets int64) of a score call: the kept tokens of every keyphrase as units of the index's vector
        space, -1 outside it."""
        per_query = [self._query_terms(q) for q in prepared_keyphrases]
        offsets = np.zeros(len(per_query) + 1, dtype=np.int64)
        np.cumsum([len(q) for q in per_query], out=offsets[1:])
        flat = [t for q in per_query for t in q]
        if self._stem_class is not None:
            ids = [self._stem_class.get(t, -1) for t in flat]
        else:
            distinct = list(dict.fromkeys(flat))
            where = dict(zip(distinct, self.index.lookup(distinct).tolist()))
            ids = [where[t] for t in flat]
        return np.array(ids, dtype=np.int32), offsets

    def _score(self, prepared_keyphrases, fetch):
        ids, offsets = self._query_ids(prepared_keyphrases)
        return self.index.score_table(ids, offsets, self.term_weighting == consts.TermWeighting.TF_IDF, fetch)

    def relevance(self, keyphrase, text, synonimizer=None):
        """relevance.py:150-168: the score of a prepared keyphrase in text number `text` (one row is cached)."""
        if self._row[0] != keyphrase:
            self._row = (keyphrase, self.relevance_table([keyphrase])[0])
        return float(self._row[1][text])


def host_doc_units(texts, measure, language):
    """The token loop of the host paths, without a device: per text the units of its kept tokens -- utils.tokenize(
    utils.prepare_text(text)) through the measure's own filter (at least 3 code points, not a stopword) and, in the stems
    space, its stemmer -- one entry a token, the units numbered by first occurrence.
    -> (doc_units, {unit's word or stem: its number}, the stemmer or None)."""
    stems = measure.vector_space == consts.VectorSpace.STEMS
    stemmer = None
    if stems:
        stemmer = measure.stemmer if measure._snowball is None else measure._snowball.SnowballStemmer(language)
    number, stem_of, doc_units = {}, {}, []
    for text in texts:
        ids = []
        for token in utils.tokenize(utils.prepare_text(text)):
            if len(token) < 3 or token in measure.stopwords:
                continue
            if stems:
                if token not in stem_of:
                    stem_of[token] = stemmer.stem(token)
                token = stem_of[token]
            ids.append(number.setdefault(token, len(number)))
        doc_units.append(ids)
    return doc_units, number, stemmer


BM25_K1, BM25_B = 1.2, 0.75


def bm25_parameters(k1, b):
    """(k1, b) as floats; ValueError unless k1 is finite and >= 0 and 0 <= b <= 1 (NaN is neither)."""
    try:
        k1, b = float(k1), float(b)
    except (TypeError, ValueError):
        raise ValueError("BM25: k1 and b must be numbers, not %r and %r" % (k1, b))
    if not (0.0 <= k1 < float("inf")) or not (0.0 <= b <= 1.0):
        raise ValueError("BM25: k1 must be finite and >= 0 and b between 0 and 1, not k1 = %r, b = %r" % (k1, b))
    return k1, b


def bm25_host_table(doc_units, n_units, q_ids, k1, b):
    """The contract of include/east_hip.h ("BM25") in numpy: doc_units[d] = the units of text d's kept tokens, one entry a
    token; q_ids[k] = the units of keyphrase k's kept tokens, -1 outside the vector space.  Every operation in the order
    the device takes it.  -> K x D float64."""
    D = len(doc_units)
    out = np.zeros((len(q_ids), D), dtype=np.float64)
    if not D:
        return out
    n_d = np.array([len(ids) for ids in doc_units], dtype=np.float64)
    avgdl = float(sum(len(ids) for ids in doc_units)) / float(D)
    doc, unit, count = [], [], []
    for d, ids in enumerate(doc_units):
        u, c = np.unique(np.asarray(ids, dtype=np.int64), return_counts=True)
        doc.append(np.full(u.size, d, dtype=np.int64))
        unit.append(u)
        count.append(c.astype(np.float64))
    doc, unit, count = np.concatenate(doc), np.concatenate(unit), np.concatenate(count)
    order = np.argsort(unit, kind="stable")                  # (unit, document) order: the documents ascend inside a unit
    doc, unit, count = doc[order], unit[order], count[order]
    unit_off = np.searchsorted(unit, np.arange(n_units + 1))
    w = np.zeros(0, dtype=np.float64)
    if unit.size:
        df = (unit_off[1:] - unit_off[:-1]).astype(np.float64)[unit]
        idf = np.log1p((float(D) - df + 0.5) / (df + 0.5))
        w = idf * (count * (k1 + 1.0)) / (count + k1 * ((1.0 - b) + b * (n_d[doc] / avgdl)))
    for k, ids in enumerate(q_ids):
        qtf = {}
        for u in ids:
            if 0 <= u < n_units:
                qtf[u] = qtf.get(u, 0) + 1
        for u, c in qtf.items():                             # (a dict keeps the order of the first occurrences)
            a, e = unit_off[u], unit_off[u + 1]
            out[k, doc[a:e]] += float(c) * w[a:e]
    return out


class BM25RelevanceMeasure(CosineRelevanceMeasure):
    """Okapi BM25 (`-s bm25`; include/east_hip.h, "BM25") over the cosine measure's term index: the same tokens, stopwords,
    stemmer, set_text_collection and query preparation; the score call is the index's second one (csrc/bm25.h), whose table
    the graph, the ranking, the similarity and the clusters read as they read a cosine table.

    score(k, d) = the sum over the keyphrase's distinct units u with a posting in d of
                  qtf_ku * log1p((D - df_u + 0.5) / (df_u + 0.5)) * c_ud (k1 + 1) / (c_ud + k1 (1 - b + b n_d / avgdl)).

    k1 finite and >= 0, 0 <= b <= 1: anything else raises ValueError here, before any device work.  BM25 scores keyphrases
    against texts: the text-to-text questions and the phrase extraction are the cosine measure's and raise ValueError.

    EAST_HIP_BM25=host (read here): the measure touches no device -- relevance_table computes the formula in numpy from
    the tokens of host_doc_units, and relevance_graph / relevance_top / relevance_similar / relevance_clusters are None, so
    the applications take their host loops.  Device and host agree to (t + 24) * 2^-53 relative each of the exact value
    (t = the contributing units of a score); they are not promised to be the same bytes (log1p is two libraries' code)."""

    def __init__(self, vector_space=consts.VectorSpace.STEMS, k1=BM25_K1, b=BM25_B, device=None, stopwords=None, stemmer=None):
        self.k1, self.b = bm25_parameters(k1, b)
        super(BM25RelevanceMeasure, self).__init__(vector_space, consts.TermWeighting.TF_IDF, device, stopwords, stemmer)
        self.on_host = os.environ.get("EAST_HIP_BM25", "device") == "host"
        if self.on_host:
            self.relevance_graph = self.relevance_top = self.relevance_similar = self.relevance_clusters = None
            self._doc_units, self._number = [], {}

    def set_text_collection(self, texts, language=consts.Language.ENGLISH):
        if not self.on_host:
            return super(BM25RelevanceMeasure, self).set_text_collection(texts, language)
        self.texts = list(texts)
        self.language = language
        self._doc_units, self._number, stemmer = host_doc_units(self.texts, self, language)
        if stemmer is not None:
            self.stemmer = stemmer
        self._row = (None, None)

    def _score(self, prepared_keyphrases, fetch):
        if self.on_host:
            q_ids = [[self._number.get(t, -1) for t in self._query_terms(q)] for q in prepared_keyphrases]
            return bm25_host_table(self._doc_units, len(self._number), q_ids, self.k1, self.b)
        ids, offsets = self._query_ids(prepared_keyphrases)
        return self.index.bm25_table(ids, offsets, self.k1, self.b, fetch)

    def _cosine_only(self, what):
        raise ValueError("%s: BM25 scores keyphrases against texts; this is the cosine measure's (use a CosineRelevanceMeasure)" % what)

    def relevance_texts_similar(self, n, threshold=-np.inf):
        self._cosine_only("relevance_texts_similar")

    def text_similarity_matrix(self):
        self._cosine_only("text_similarity_matrix")

    def extract_phrases(self, n=0, max_words=3, min_words=1, min_count=2, min_texts=1):
        self._cosine_only("extract_phrases")

    def relevance_terms(self, n, min_texts=1, groups=None):
        self._cosine_only("relevance_terms")

    def text_overlap_matrix(self, words=4, orientation="symmetric"):
        self._cosine_only("text_overlap_matrix")

    def relevance_texts_overlap(self, n, threshold=-np.inf, words=4, orientation="symmetric"):
        self._cosine_only("relevance_texts_overlap")

    def relevance_overlap_clusters(self, words=4, linkage="single", floor=None):
        self._cosine_only("relevance_overlap_clusters")

    def shared_passages(self, pairs, words=4, min_words=None, per_pair=5):
        self._cosine_only("shared_passages")

    def unit_names(self):
        self._cosine_only("unit_names")

    def relevance_clusters(self, prepared_keyphrases=None, axis=None, linkage="single", floor=None):
        if prepared_keyphrases is None:
            self._cosine_only("relevance_clusters without keyphrases")
        return super(BM25RelevanceMeasure, self).relevance_clusters(prepared_keyphrases, axis, linkage, floor)
