# -*- coding: utf-8 -*-
"""GPU tier: phrase extraction on the device (csrc/phrases.h; include/east_hip.h, "Phrase extraction").  Every case builds the
cosine term index of a collection, extracts, fetches, and compares every fetched array byte for byte with
tests/phrases_exact.py -- the dict of word tuples that tests/test_phrases_host.py pins by hand.  Nothing is floating point:
there is no tolerance.  Every shape is the smallest at which the step it names can go wrong."""
import ctypes
import functools

import numpy as np
import pytest

import cosine_exact
import phrases_exact as model

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
NO_INDEX = "phrases: no cosine index has been built on this handle"
NO_PHRASES = "no phrases have been extracted on this handle"


def _index(hip, texts, stop=()):
    index = hip.HipCosineIndex()
    index.build_texts(list(texts), sorted(cosine_exact.prepared_stopwords(stop)))
    return index


def _check(index, m, what="", **params):
    args = dict(n=0, max_words=3, min_words=1, min_count=2, min_texts=1)
    args.update(params)
    found = index.phrases(**args)
    expected = m.extract(**args)
    model.check(found, expected, (what, params))
    assert index.last_phrases_ms > 0.0
    return found


def _whole(hip, texts, stop=(), what="", longest=model.MAX_WORDS + 1, sweeps=({},)):
    index = _index(hip, texts, stop)
    m = model.PhraseModel(texts, stop, longest)
    assert index.info()["kept_tokens"] == m.kept_tokens
    found = [_check(index, m, what, **params) for params in sweeps]
    index.close()
    return found


# ---- hand-made cases -----------------------------------------------------------------------------------------------------------
def test_header_example(hip):
    found, = _whole(hip, model.HEADER_EXAMPLE)
    got = list(zip(found.strings(), found.words.tolist(), found.count.tolist(), found.texts.tolist(), found.first.tolist()))
    assert got == model.HEADER_EXPECTED
    assert (found.candidates, found.levels) == (4, 3)


@pytest.mark.parametrize("times", model.REPEATS)
def test_one_word_repeated(hip, times):
    """Runs across a workgroup (256, 257) and across a scan tile (4 097); overlapping occurrences all count."""
    all_levels, three = _whole(hip, model.one_word(times), sweeps=({"max_words": 8, "min_count": 1}, {}))
    assert sorted(all_levels.count.tolist()) == list(range(max(1, times - 7), times + 1))      # (every length has a count of its own)
    assert three.count.tolist() == [times - 2, times - 1, times]              # (scores 3 (t - 2) > 2 (t - 1) > t from t = 5 on)


def test_two_word_period(hip):
    found, _ = _whole(hip, model.two_word_period(), sweeps=({}, {"max_words": 8}))
    assert found.strings()[:2] == ["TICK TOCK TICK", "TOCK TICK TOCK"]


# ---- text boundaries, breaks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(model.boundary_collections()))
def test_text_boundaries(hip, name):
    texts, stop = model.boundary_collections()[name]
    found = _whole(hip, texts, stop, name, sweeps=({}, {"max_words": 8, "min_count": 1}, {"min_texts": 2}, {"min_texts": len(texts)}))
    by_text = dict(zip(found[0].strings(), zip(found[0].count.tolist(), found[0].texts.tolist())))
    if name == "last and first token of neighbours":
        assert "EDGE NEXT" not in found[1].strings() and by_text["NEXT"] == (2, 2)
    if name == "seventy texts beside three hundred in one":
        assert by_text["HERE SHARED PHRASE"] == (70, 70) and by_text["INNER LOOP INNER"] == (299, 1)
    if name == "a word over three texts":
        assert by_text["WWW"] == (4097, 3) and by_text["WWW WWW"] == (4094, 3)


@pytest.mark.parametrize("name", sorted(model.break_collections()))
def test_breaks(hip, name):
    texts, stop = model.break_collections()[name]
    found = _whole(hip, texts, stop, name, sweeps=({}, {"max_words": 8, "min_count": 1}))
    if name != "stopwords inside, in front and behind":
        # zero candidates is a result that can be built and fetched
        assert all(f.candidates == 0 and f.words.size == 0 and f.text_off.tolist() == [0] and f.levels == 1 for f in found)
    else:
        assert found[0].strings() == ["QUICK FOX", "QUICK", "FOX"]


# ---- parameters -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zipf_model():
    return model.PhraseModel(*model.zipf_collection())


@pytest.fixture(scope="module")
def zipf_index(hip):
    index = _index(hip, *model.zipf_collection())
    yield index
    index.close()


@pytest.mark.parametrize("max_words", range(1, 9))
def test_parameters_words_and_counts(zipf_index, max_words):
    m = _zipf_model()
    for min_count in (1, 2, 3, 50):
        found = _check(zipf_index, m, max_words=max_words, min_count=min_count)
        if min_count == 1:
            # the domain never shrinks but by the phrases that meet a break or the end of their text
            assert found.levels == max_words and (found.survivors[:max_words] > 0).all()
        if min_count == 50 and max_words == 8:
            # the early end: a level without a survivor is the last, the levels behind it are not run
            assert found.levels < 8 and found.survivors[found.levels - 1] == 0
            assert (found.domain[found.levels:] == 0).all() and (found.survivors[found.levels:] == 0).all()
    for min_words in (1, 2, max_words):
        if min_words <= max_words:
            _check(zipf_index, m, max_words=max_words, min_words=min_words)


def test_parameters_texts_and_cut(zipf_index):
    m = _zipf_model()
    D = len(model.zipf_collection()[0])
    for min_texts in (1, 2, D):
        for min_words in (1, 2, 3):
            _check(zipf_index, m, min_texts=min_texts, min_words=min_words)
    C = m.extract().candidates
    assert C > 5
    for n in (0, 1, 5, C - 1, C, C + 1):
        found = _check(zipf_index, m, n=n)
        assert found.candidates == C and found.words.size == (min(n, C) if n else C)


def test_ties_keep_words_then_first(hip):
    texts, stop = model.ties_collection()
    found, = _whole(hip, texts, stop)
    six = [(w, f) for w, c, f in zip(found.words.tolist(), found.count.tolist(), found.first.tolist()) if w * c == 6]
    assert len(six) == 36 and six == sorted(six) and {w for w, _ in six} == {1, 2, 3}


def test_wide_ids(hip):
    """70 000 distinct words: term ids of 17 bits, packed keys of level 2 of 34."""
    texts, stop = model.wide_collection()
    found, = _whole(hip, texts, stop, longest=3, sweeps=({"max_words": 2},))
    assert found.candidates == 69999 and int(found.term_ids.max()) == 69999 and found.survivors[1] == 69999


# ---- text ------------------------------------------------------------------------------------------------------------------------
def test_text_of_the_fuzz_documents(hip):
    """ß, İ, final sigma, junk bytes and high planes: phrase text and term ids are the model's."""
    index = hip.HipCosineIndex()
    for it, rnd in enumerate(cosine_exact.fuzz_rounds()):
        index.build_texts(list(rnd["texts"]), sorted(cosine_exact.prepared_stopwords(rnd["stopwords"])))
        m = model.PhraseModel(rnd["texts"], rnd["stopwords"], longest=5)
        _check(index, m, it, max_words=4, min_count=1)
    index.close()


def test_hash_independence(hip):
    """With 8 hash bits the first seed collides and the index takes a second: the phrases are the same bytes."""
    lib = hip.load()
    texts, stop = model.zipf_collection()
    texts = list(texts[:4])
    m = model.PhraseModel(texts, stop, longest=4)
    assert lib.east_hip_debug_set_term_hash_bits(8) == OK
    try:
        index = _index(hip, texts, stop)
        assert index.info()["hash_attempts"] >= 2
        _check(index, m)
        index.close()
    finally:
        assert lib.east_hip_debug_set_term_hash_bits(0) == OK


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------
def _raw(found):
    return [getattr(found, name).tobytes() for name in ("words", "count", "texts", "first", "first_text", "term_ids", "text_off", "text")]


def test_lifecycle(hip):
    lib = hip.load()
    index = hip.HipCosineIndex()
    h = index._h
    out = (ctypes.c_int64 * 4)()
    levels = (ctypes.c_int64 * 8)()
    none = [None] * 8
    error = lambda: lib.east_hip_last_error().decode()
    assert lib.east_hip_phrases_fetch(h, *none) == ERR_NOT_BUILT and error() == NO_PHRASES
    assert lib.east_hip_phrases_levels(h, levels, levels) == ERR_NOT_BUILT and error() == NO_PHRASES
    assert lib.east_hip_phrases_build(h, 1, 3, 2, 1, 0, out) == ERR_NOT_BUILT and error() == NO_INDEX
    assert lib.east_hip_last_phrases_ms(h) == -1.0
    index.build_texts(model.HEADER_EXAMPLE, ())
    assert lib.east_hip_phrases_fetch(h, *none) == ERR_NOT_BUILT and error() == NO_PHRASES
    m = model.PhraseModel(model.HEADER_EXAMPLE)
    first = _check(index, m)
    # every refusal names its argument and leaves the earlier result fetchable
    for args, word in (((1, 0, 2, 1, 0), "max_words"), ((1, 9, 2, 1, 0), "max_words"), ((0, 3, 2, 1, 0), "min_words"),
                       ((4, 3, 2, 1, 0), "min_words"), ((1, 3, 0, 1, 0), "min_count"), ((1, 3, 2, 0, 0), "min_texts"),
                       ((1, 3, 2, 1, -1), "N")):
        assert lib.east_hip_phrases_build(h, *(args + (out,))) == ERR_INVALID
        assert error().startswith("phrases: " + word) and "\n" not in error()
        assert lib.east_hip_phrases_fetch(h, *none) == OK
    assert lib.east_hip_phrases_build(h, 1, 3, 2, 1, 0, None) == ERR_INVALID and error().startswith("phrases: out")
    words = np.zeros(4, dtype=np.int32)
    assert lib.east_hip_phrases_fetch(h, words.ctypes.data_as(hip._c_i32p), *none[1:]) == OK and words.tolist() == [3, 3, 3, 2]
    # two builds give the same bytes; score calls and set_classes leave a later build alone
    assert _raw(_check(index, m)) == _raw(first)
    index.score_table(np.array([0, 1], dtype=np.int32), np.array([0, 2], dtype=np.int64))
    index.set_classes([0, 0, 1], 2)
    assert lib.east_hip_phrases_fetch(h, *none) == OK
    assert _raw(_check(index, m)) == _raw(first)
    index.set_classes([], 0)
    # a new cosine build withdraws the result
    index.build_texts(model.one_word(5), ())
    assert lib.east_hip_phrases_fetch(h, *none) == ERR_NOT_BUILT and error() == NO_PHRASES
    assert lib.east_hip_last_phrases_ms(h) == -1.0
    _check(index, model.PhraseModel(model.one_word(5)))
    # east_hip_reset drops it, with the index
    assert lib.east_hip_reset(h) == OK
    assert lib.east_hip_phrases_fetch(h, *none) == ERR_NOT_BUILT and error() == NO_PHRASES
    assert lib.east_hip_phrases_build(h, 1, 3, 2, 1, 0, out) == ERR_NOT_BUILT and error() == NO_INDEX
    index.close()


def test_keyphrases_extract_device_and_host_agree(hip, monkeypatch):
    from east import applications, relevance
    texts, stop = model.zipf_collection()
    named = {"t%02d" % d: t for d, t in enumerate(texts)}
    measure = relevance.CosineRelevanceMeasure("words", stopwords=stop)
    monkeypatch.delenv("EAST_HIP_EXTRACT", raising=False)
    on_device = applications.keyphrases_extract(named, n=50, similarity_measure=measure)
    measure.index.close()
    monkeypatch.setenv("EAST_HIP_EXTRACT", "host")
    on_host = applications.keyphrases_extract(named, n=50, similarity_measure=relevance.CosineRelevanceMeasure("words", stopwords=stop))
    assert len(on_device) == 50 and on_device == on_host
    assert [repr(p) for p in on_device] == [repr(p) for p in on_host]
