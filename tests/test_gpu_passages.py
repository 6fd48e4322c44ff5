"""GPU tier: the shared passages on the device (csrc/passages.h; include/east_hip.h, "Shared passages").  Every case compares
every fetched array with the model of tests/passages_exact.py -- Python sets of word tuples and a plain loop over the
positions -- with ==, under route 1 (b in the shingle's text list), route 2 (the shingle in b's list) and from a second
build.  Nothing here has a tolerance."""
import numpy as np
import pytest

import cosine_exact
import overlap_exact
import passages_exact as model

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
FIELDS = ("pair_off", "starts", "covered", "found", "start", "words", "at", "text_start")


def _index(hip, texts, stop=model.STOP):
    index = hip.HipCosineIndex()
    index.build_texts(list(texts), sorted(cosine_exact.prepared_stopwords(stop)))
    return index


def _lists(found):
    return {name: getattr(found, name).tolist() for name in FIELDS}


def _check(hip, index, texts, stop, pairs, w, min_words=None, per_pair=0, want=None):
    """The three builds of a case against the model -> (the last build's PassageArrays, the model's dict)."""
    lib = hip.load()
    want = want or model.exact(texts, stop, pairs, w, min_words, per_pair)
    found = None
    try:
        for route in (1, 2, 0):                                       # (0: the default, the second build of its route)
            assert lib.east_hip_debug_set_passages_route(route) == OK
            found = index.passages([a for a, _ in pairs], [b for _, b in pairs], w, min_words, per_pair)
            assert found.info["route"] == (route or found.info["route"]) and found.info["route"] in (1, 2)
            got = _lists(found)
            for name in FIELDS:
                assert got[name] == want[name], (name, "route", route, "w", w, "min_words", min_words, "per_pair", per_pair)
    finally:
        lib.east_hip_debug_set_passages_route(0)
    info = found.info
    assert info["n_docs"] == len(texts) and info["pairs"] == len(pairs) and info["returned"] == len(want["start"])
    assert info["shared_starts"] == sum(want["starts"]) and index.last_passages_ms() > 0.0
    assert abs(sum(index.passages_phases_ms()) - index.last_passages_ms()) < 0.01      # (three stretches of one time line)
    return found, want


def test_worked_case(hip):
    index = _index(hip, model.WORKED, ())
    found, _ = _check(hip, index, model.WORKED, (), [(0, 1), (1, 0)], 2)
    got = _lists(found)
    assert got["pair_off"] == [0, 2, 3] and got["starts"] == [3, 2] and got["covered"] == [5, 3] and got["found"] == [2, 1]
    assert list(zip(got["start"], got["words"], got["at"])) == [(1, 3, 8), (5, 2, 8), (8, 3, 1)]
    assert got["text_start"] == [0, 7, 12]
    index.close()


def test_text_lengths_around_the_word(hip):
    """Texts of 63, 64, 65, 127, 128 and 129 shingle positions: rows of one, two and three words, full and one bit short or over."""
    texts = model.length_texts()
    index = _index(hip, texts, ())
    pairs = model.all_pairs(len(texts))
    found, want = _check(hip, index, texts, (), pairs, 2)
    lengths = np.diff(found.text_start)
    assert lengths.tolist() == [64, 65, 66, 128, 129, 130]
    assert found.info["bit_words"] == sum((int(lengths[a]) + 63) // 64 for a, _ in pairs)
    assert max(want["words"]) >= 120
    _check(hip, index, texts, (), pairs, 1)
    _check(hip, index, texts, (), pairs, 3, 10, 1)
    index.close()


def test_runs_at_the_word_edges(hip):
    texts, cases = model.bit_edge_texts()
    index = _index(hip, texts, ())
    pairs = [(0, partner) for partner, _ in cases.values()]
    found, want = _check(hip, index, texts, (), pairs, 2)
    for i, (name, (partner, (lo, hi))) in enumerate(cases.items()):
        assert pairs[i] == (0, partner)
        p0, p1 = want["pair_off"][i], want["pair_off"][i + 1]
        assert p1 - p0 == 1 and (want["start"][p0], want["words"][p0]) == (lo, hi - lo + 2), name
        assert want["starts"][i] == hi - lo + 1 and want["covered"][i] == hi - lo + 2, name
    # the mirrored pairs, and all edges at once in one list with the others
    _check(hip, index, texts, (), [(b, a) for a, b in pairs] + pairs, 2)
    index.close()


def test_a_run_over_three_whole_words(hip):
    """Identical texts of 200 words: one passage of 200 words over a row of four words, three of them full."""
    text = " ".join(model.fresh(200, "i"))
    texts = (text, text, "unrelated words only here")
    index = _index(hip, texts, ())
    for w in (1, 2, 8):
        found, want = _check(hip, index, texts, (), [(0, 1), (1, 0), (0, 2), (2, 1)], w)
        assert list(zip(want["start"], want["words"], want["at"])) == [(0, 200, 200), (200, 200, 0)]
        assert want["starts"][:2] == [201 - w] * 2 and want["covered"][:2] == [200, 200]
    index.close()


def test_no_carry_between_rows(hip):
    texts = model.row_border_texts()
    index = _index(hip, texts, ())
    for w in (1, 2):
        found, want = _check(hip, index, texts, (), [(0, 2), (1, 2)], w)
        assert list(zip(want["start"], want["words"])) == [(62, 2), (64, 2)] and found.info["bit_words"] == 2
        assert want["starts"] == [3 - w, 3 - w]
        _check(hip, index, texts, (), [(1, 2), (0, 2), (0, 2), (1, 2), (2, 0), (2, 1)], w)
    index.close()


def test_adjacent_positions_in_neighbouring_texts(hip):
    texts = model.neighbours_texts()
    index = _index(hip, texts, ())
    pairs = model.all_pairs(len(texts))
    found, want = _check(hip, index, texts, (), pairs, 1)
    i = pairs.index((0, 3))
    assert want["starts"][i] == 2 and want["found"][i] == 2         # aaa and ccc, bbb between them
    # positions 2 (ccc, the end of text 0) and 3 (ddd, the start of text 1) are both held by text 3 and are two passages
    assert (want["start"][want["pair_off"][pairs.index((1, 3))]], want["words"][want["pair_off"][pairs.index((1, 3))]]) == (3, 1)
    index.close()


def test_pair_lists_and_collection_sizes(hip):
    # D = 2; 0 pairs; duplicate pairs; (a, b) with (b, a)
    index = _index(hip, model.WORKED, ())
    found, _ = _check(hip, index, model.WORKED, (), [], 2)
    assert found.pair_off.tolist() == [0] and found.info["bit_words"] == 0 and found.info["returned"] == 0
    found, want = _check(hip, index, model.WORKED, (), [(0, 1), (0, 1), (1, 0), (0, 1)], 2)
    assert want["start"][0:2] == want["start"][2:4] == want["start"][5:7]
    index.close()
    # D = 65
    texts = overlap_exact.tile_edge_texts(65)
    index = _index(hip, texts)
    for w in (1, 2, 3):
        _check(hip, index, texts, model.STOP, model.some_pairs(65, 120), w)
    index.close()


def test_shingle_cases(hip):
    # no shared shingle; w larger than every text; stopword-only and empty texts
    texts = model.content_texts()
    index = _index(hip, texts)
    pairs = model.all_pairs(len(texts))
    for w in (1, 2, 4, 8):
        found, want = _check(hip, index, texts, model.STOP, pairs, w)
    assert found.info["levels"] == 8
    index.close()
    nothing = ("aaa bbb ccc ddd", "eee fff ggg hhh", "", "the the")
    index = _index(hip, nothing)
    found, want = _check(hip, index, nothing, model.STOP, model.all_pairs(4), 2)
    assert found.info["shared_shingles"] == 0 and found.info["passages"] == 0 and want["starts"] == [0] * 12
    short = ("aaa bbb ccc", "aaa bbb ccc", "ddd")
    index.close()
    index = _index(hip, short)
    found, want = _check(hip, index, short, model.STOP, model.all_pairs(3), 4)
    assert found.info["shared_shingles"] == 0 and want["found"] == [0] * 6
    index.close()
    # a stopword splits a passage
    split = ("aaa bbb the ccc ddd", "aaa bbb ccc ddd the aaa bbb")
    index = _index(hip, split)
    found, want = _check(hip, index, split, model.STOP, [(0, 1), (1, 0)], 2)
    assert list(zip(want["start"], want["words"], want["at"]))[:2] == [(0, 2, 5), (3, 2, 7)]
    index.close()


def test_at_is_the_smallest_position(hip):
    texts = ("xxx one two three yyy", "one two zzz one two three www one two three")
    index = _index(hip, texts, ())
    found, want = _check(hip, index, texts, (), [(0, 1), (1, 0)], 2)
    assert (want["start"][0], want["words"][0], want["at"][0]) == (1, 3, 5)
    index.close()


def test_a_unit_held_by_300_texts(hip):
    texts = model.held_by_many_texts(300)
    index = _index(hip, texts, ())
    pairs = [(0, 299), (299, 0), (150, 151), (298, 1), (1, 298), (299, 298)] + [(d, (d * 7 + 1) % 300) for d in range(0, 300, 11) if d != (d * 7 + 1) % 300]
    found, want = _check(hip, index, texts, (), pairs, 2)
    assert found.info["shared_shingles"] == 1 and found.info["postings"] == 300
    assert (want["starts"][1], want["found"][1], want["at"][want["pair_off"][1]]) == (3, 3, 1)
    index.close()


def test_filter_order_and_cut(hip):
    texts = model.order_texts()
    index = _index(hip, texts, ())
    found, want = _check(hip, index, texts, (), [(0, 1)], 2)
    assert want["words"] == [5, 5, 3, 3, 3, 2] and want["start"] == sorted(want["start"][:2]) + sorted(want["start"][2:5]) + want["start"][5:]
    for min_words, per_pair in ((None, 1), (None, 6), (None, 7), (3, 0), (3, 5), (3, 2), (5, 0), (6, 0), (40, 3)):
        found, want = _check(hip, index, texts, (), [(0, 1), (1, 0), (0, 1)], 2, min_words, per_pair)
    assert want["found"] == [0, 0, 0] and want["starts"][0] == 15 and found.info["passages"] == 18
    index.close()


def test_zipf_collection_every_width(hip):
    texts = overlap_exact.zipf_texts()
    index = _index(hip, texts)
    pairs = model.all_pairs(len(texts))
    assert len(pairs) == 240
    tokens = model.token_lists(texts, model.STOP)
    I = {w: overlap_exact.exact(texts, model.STOP, w)[3] for w in (2, 4)}
    longest = []
    for w in range(1, model.MAX_WORDS + 1):
        found, want = _check(hip, index, texts, model.STOP, pairs, w, None, 0 if w % 2 else 3)
        longest.append(max(want["words"]))
        assert found.info["kept_tokens"] >= 19000 and found.info["levels"] == w
        if w in I:      # the distinct shingles at the shared starts are the overlap's intersection
            for a, b in pairs[::7]:
                assert len(model.pair_exact(tokens, a, b, w)[4]) == I[w][a, b]
    assert longest[7] >= 12
    index.close()


def test_fuzz_documents(hip):
    for i, r in enumerate(cosine_exact.fuzz_rounds()[:40]):
        index = _index(hip, r["texts"], r["stopwords"])
        D = len(r["texts"])
        if D > 1:
            _check(hip, index, r["texts"], r["stopwords"], model.some_pairs(D, 30), 1 + i % 3, None if i % 2 else 2 + i % 3, i % 4)
        index.close()


def test_lifecycle(hip):
    lib = hip.load()
    index = hip.HipCosineIndex()
    h = index._h
    out = np.zeros(12, dtype=np.int64)
    p_out = out.ctypes.data_as(hip._c_i64p)
    pa, pb = np.array([0, 1, 5], dtype=np.int32), np.array([1, 0, 7], dtype=np.int32)
    as_p = lambda x: x.ctypes.data_as(hip._c_i32p)

    def build(words=2, min_words=2, per_pair=0, a=pa, b=pb, n=3, handle=h, out=p_out):
        rc = lib.east_hip_passages_build(handle, words, min_words, per_pair, None if a is None else as_p(a), None if b is None else as_p(b), n, out)
        return rc, lib.east_hip_last_error().decode()

    def fetch():
        return lib.east_hip_passages_fetch(h, *[None] * 8)

    assert build() == (ERR_NOT_BUILT, "passages: no cosine index has been built on this handle")
    assert fetch() == ERR_NOT_BUILT and lib.east_hip_last_error().decode() == "no passages have been built on this handle"
    assert lib.east_hip_last_passages_ms(h) == -1.0
    assert build(handle=None)[0] == ERR_INVALID
    assert lib.east_hip_debug_set_passages_route(3) == ERR_INVALID and lib.east_hip_debug_set_passages_route(-1) == ERR_INVALID
    texts = overlap_exact.tile_edge_texts(65)
    stop = sorted(cosine_exact.prepared_stopwords(model.STOP))
    index.build_texts(list(texts), stop)
    assert fetch() == ERR_NOT_BUILT
    pairs = list(zip(pa.tolist(), pb.tolist()))
    want = model.exact(texts, model.STOP, pairs, 2)
    assert _lists(index.passages(pa, pb, 2, None, 0)) == want and fetch() == OK

    def fetched():
        found = hip.PassageArrays()
        found.pair_off = np.zeros(4, np.int64)
        found.starts, found.covered, found.found = (np.zeros(3, np.int32) for _ in range(3))
        found.start, found.words, found.at = (np.zeros(want["pair_off"][-1], np.int32) for _ in range(3))
        found.text_start = np.zeros(66, np.int32)
        assert lib.east_hip_passages_fetch(h, found.pair_off.ctypes.data_as(hip._c_i64p), *[as_p(x) for x in (
            found.starts, found.covered, found.found, found.start, found.words, found.at, found.text_start)]) == OK
        return _lists(found)

    # every refusal names what is wrong and leaves the earlier result fetchable
    same_a, same_b = np.array([0, 1, 4], np.int32), np.array([1, 0, 4], np.int32)
    far, low = np.array([0, 1, 65], np.int32), np.array([1, -1, 2], np.int32)
    for arguments, said in ((dict(words=0, min_words=0), "words must lie in 1 .. 8"), (dict(words=9, min_words=9), "words must lie in 1 .. 8"),
                            (dict(min_words=1), "min_words must not be below words"), (dict(per_pair=-1), "per_pair must not be negative"),
                            (dict(n=-1), "the number of pairs"), (dict(n=(1 << 24) + 1), "the number of pairs"),
                            (dict(a=None), "the pairs are null"), (dict(b=None), "the pairs are null"), (dict(out=None), "out is null"),
                            (dict(a=same_a, b=same_b), "pair 2 pairs text 4 with itself"), (dict(a=far), "pair 2 names a text outside 0 .. 64"),
                            (dict(b=low), "pair 1 names a text outside 0 .. 64")):
        rc, message = build(**arguments)
        assert rc == ERR_INVALID and said in message and message.startswith("passages: "), (arguments, message)
        assert fetched() == want and index.last_passages_ms() > 0.0
    assert build(a=None, b=None, n=0)[0] == OK and fetch() == OK          # (no pair: a result)
    assert _lists(index.passages(pa, pb, 2, None, 0)) == want

    # the overlap matrix and the extracted phrases are untouched by a passages build, and the passages by theirs
    index.overlap_build(2, 1)
    matrix = tuple(a.tobytes() for a in index.overlap_matrix())
    phrases = index.phrases(0, 3, 1, 2, 1)
    before = (phrases.words.tobytes(), phrases.count.tobytes())
    assert fetched() == want
    every = model.all_pairs(65)[::9]
    assert _lists(index.passages([a for a, _ in every], [b for _, b in every], 3, None, 2)) == model.exact(texts, model.STOP, every, 3, None, 2)
    assert tuple(a.tobytes() for a in index.overlap_matrix()) == matrix
    assert matrix == tuple(a.tobytes() for a in overlap_exact.exact(texts, model.STOP, 2, True)[:3])
    R = len(phrases.words)
    words, count = np.empty(R, np.int32), np.empty(R, np.int32)
    assert lib.east_hip_phrases_fetch(h, as_p(words), as_p(count), *[None] * 6) == OK
    assert (words.tobytes(), count.tobytes()) == before and R > 0
    assert _lists(index.passages(pa, pb, 2, None, 0)) == want

    # score calls and the classes leave it alone; a cosine build withdraws it, and so does a reset
    index.score_table(np.array([0, 1, 2], dtype=np.int32), np.array([0, 2, 3], dtype=np.int64), True)
    V = index.n_terms
    index.set_classes(np.arange(V, dtype=np.int32) // 2, (V + 1) // 2)
    assert fetched() == want
    assert _lists(index.passages(pa, pb, 2, None, 0)) == want           # (passages are made of words whatever the vector space)
    index.set_classes([], 0)
    index.build_texts(list(texts), stop)
    assert fetch() == ERR_NOT_BUILT and lib.east_hip_last_passages_ms(h) == -1.0
    assert _lists(index.passages(pa, pb, 2, None, 0)) == want
    # the consumer offers no matrix: source 7 stays unknown
    top = np.zeros(4, dtype=np.int64)
    assert lib.east_hip_top_build_resident(h, 7, hip.TOP_BY_KEYPHRASE, 3, 0.0, top.ctypes.data_as(hip._c_i64p)) == ERR_INVALID
    assert "unknown table source" in lib.east_hip_last_error().decode()
    assert lib.east_hip_reset(h) == OK
    assert fetch() == ERR_NOT_BUILT and build()[0] == ERR_NOT_BUILT and lib.east_hip_last_passages_ms(h) == -1.0
    index.close()


def test_applications_device_against_host(hip, monkeypatch):
    from east import applications, relevance
    texts = {"t%02d" % d: text for d, text in enumerate(overlap_exact.zipf_texts(3000, 9))}
    texts.update({"c%d" % d: text for d, text in enumerate(model.content_texts())})
    make = lambda: relevance.CosineRelevanceMeasure("words", stopwords=model.STOP)
    named = [("c0", "c3"), ("c3", "c0"), ("t00", "t05"), ("c2", "c1"), ("c0", "c3"), ("c4", "c0")]
    for arguments in (dict(n=4, words=2), dict(n=3, words=4, orientation="directed", overlap_threshold=0.01, per_pair=0),
                      dict(n=17, words=1, min_words=3, per_pair=2), dict(words=2, pairs=named), dict(words=3, pairs=named, per_pair=1)):
        monkeypatch.delenv("EAST_HIP_PASSAGES", raising=False)
        device = applications.texts_passages(texts, similarity_measure=make(), **arguments)
        monkeypatch.setenv("EAST_HIP_PASSAGES", "host")
        host = applications.texts_passages(texts, similarity_measure=make(), **arguments)
        assert device == host and any(device.values()), arguments
        if "pairs" not in arguments:
            assert list(device) == list(texts)
    c0 = device["c0"][0]
    assert c0.other == "c3" and c0.value is None and c0.passages[0] == applications.Passage(0, 10, 3, model.content_texts()[0].upper())
