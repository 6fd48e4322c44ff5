"""gpu tier: text-to-text relatedness on the device (csrc/related.h through include/east_hip.h, "Text-to-text
relatedness").  The yardstick is tests/related_exact.py and never the project's host path: the string lists come from
utils.text_to_strings_collection on the host (from index.prepared() for tagged text), the per-string scores from
HipIndex.score_table on those strings -- existing code, pinned elsewhere; on the two smallest cases from
tests/score_exact.py as well --, and the matrix, self and scored are compared with the model in exact arithmetic: every value
within (max(c_A, c_B) + 4) * 2^-53 * exact.  The SELECTION is the ranking's contract (applications._top_select) applied to
the device's own fetched matrix."""
import ctypes
import random

import numpy as np
import pytest

import related_exact as model
import score_exact

pytestmark = pytest.mark.gpu

INF = float("inf")
OK, ERR_INVALID, ERR_NOT_BUILT = 0, -2, -6
TILE = 256                      # csrc/related.h: REL_TILE
BLOCK = 256                     # csrc/common.h: suffixes of a workgroup of the score walk

LATIN = "abcdefghijklmnopqrstuvwxyz"


def _word(rng, alphabet=LATIN, lo=3, hi=8):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


def _text(seed, n_strings, alphabet=LATIN, vocabulary=60):
    """A text of exactly n_strings strings (three kept tokens each) over a small seeded vocabulary."""
    rng = random.Random(seed)
    words = [_word(rng, alphabet) for _ in range(vocabulary)]
    return " ".join(rng.choice(words) for _ in range(3 * n_strings)).encode("utf-8")


def _wide_alphabet():
    """More than 254 letters below U+0A00 that upper-casing leaves alone: the index takes the 32-bit code stream."""
    letters = [chr(c) for c in range(0xC0, 0x0A00) if chr(c).isalpha() and chr(c).upper() == chr(c) and len(chr(c).upper()) == 1]
    assert len(letters) > 300
    return "".join(letters[:300])


def _cases():
    wide = _wide_alphabet()
    cjk = "".join(chr(c) for c in range(0x4E00, 0x4E40))
    long_words = " ".join(c * 100 for c in "xyz")                             # one string of 300 symbols: longer than BLOCK
    return {
        "one": [_text(1, 4, vocabulary=6)],
        "empty": [_text(2, 5, vocabulary=6), b"a 12 to 7 it"],
        "twins": [_text(3, 7), _text(4, 9), _text(3, 7)],
        "tiles": [_text(5, 1), _text(6, TILE), _text(7, TILE + 1), _text(8, 3 * TILE - 1)],
        "wide": [_text(100 + d, 1 + d % 5, vocabulary=12) for d in range(65)],
        "long": [_text(9, 6), (long_words + " " + _text(10, 3).decode()).encode(), _text(11, 2)],
        "u32": [_text(12, 40, alphabet=wide, vocabulary=200), _text(13, 30, alphabet=wide, vocabulary=200), _text(14, 5)],
        "cjk": [_text(15, 6, alphabet=cjk), (_text(16, 4).decode() + " " + _text(17, 5, alphabet=cjk).decode()).encode("utf-8"),
                _text(18, 3)],
    }


def _strings_of_prepared(index):
    """The strings as the index holds them, decoded from the prepared symbols (either encoding)."""
    from east.asts import utils as ast_utils
    symbols, doc_offsets, n_strings = index.prepared()
    tagged = ast_utils.is_tagged(symbols)
    out = []
    for d in range(len(n_strings)):
        doc = symbols[int(doc_offsets[d]):int(doc_offsets[d + 1])]
        strings, cur = [], []
        for c in doc.tolist():
            if (c >= ast_utils.TERMINATOR_TAG) if tagged else (c >= 0x0A00):
                strings.append("".join(map(chr, cur)))
                cur = []
            else:
                cur.append(c)
        assert not cur and len(strings) == int(n_strings[d])
        out.append(strings)
    return out, tagged


class _Case(object):
    """One collection: built once, its strings scored once by HipIndex.score_table (normalized and not), the models made on
    demand and shared among the tests."""

    def __init__(self, hip, name):
        from east import utils
        self.hip, self.name, self.texts = hip, name, _cases()[name]
        self.index = hip.HipIndex()
        self.index.build_texts(self.texts)
        self.D = len(self.texts)
        self.collections, self.tagged = _strings_of_prepared(self.index)
        if not self.tagged:
            assert self.collections == [utils.text_to_strings_collection(t) for t in self.texts]
        self.flat = sorted({s for strings in self.collections for s in model.scored_strings(strings)})
        self.row = {s: i for i, s in enumerate(self.flat)}
        self._scores, self._exact = {}, {}

    def scores(self, normalized):
        if normalized not in self._scores:
            qs, qo = self.hip.pack_queries(self.flat)
            self._scores[normalized] = self.index.score_table(qs, qo, bool(normalized)) if self.flat else np.zeros((0, self.D))
        return self._scores[normalized]

    def exact(self, normalized, orientation):
        key = (normalized, orientation)
        if key not in self._exact:
            table = self.scores(normalized)
            self._exact[key] = model.exact(self.collections, lambda s, b: table[self.row[s], b], orientation)
        return self._exact[key]


_made = {}


@pytest.fixture
def case(hip, request):
    name = request.param
    if name not in _made:
        _made[name] = _Case(hip, name)
    return _made[name]


def _ranking_agrees(found, matrix, n, threshold):
    from east import applications
    want = applications._top_select(matrix, 1, n, threshold)
    assert found.count.tolist() == [len(entries) for entries in want]
    for s, entries in enumerate(want):
        assert found.index[s, :len(entries)].tolist() == [i for i, _ in entries], s
        assert found.score[s, :len(entries)].tobytes() == np.array([v for _, v in entries], dtype=np.float64).tobytes(), s
        assert (found.index[s, len(entries):] == -1).all() and not found.score[s, len(entries):].any()


@pytest.mark.parametrize("case", ["one", "empty", "twins", "tiles", "wide", "long", "u32", "cjk"], indirect=True)
def test_matrix_self_and_scored_are_the_contract(hip, case):
    """Every case, both orientations, normalized and not: values within the per-entry bound, scored equal, the NaN diagonal,
    the symmetric form byte-symmetric, the ranking = _top_select of the fetched matrix, two builds the same bytes."""
    index, D = case.index, case.D
    if case.name == "u32":
        assert index.info()["sigma_text"] > 254
    if case.name == "cjk":
        assert case.tagged
    if case.name == "long":
        assert max(len(s) for s in case.flat) > BLOCK
    if case.name == "tiles":
        assert [len(c) for c in case.collections] == [1, TILE, TILE + 1, 3 * TILE - 1]
    for normalized in (1, 0):
        case.scores(normalized)
        for orientation in (model.DIRECTED, model.SYMMETRIC):
            want = case.exact(normalized, orientation)
            d, n_scored, launches = index.related_build(normalized, orientation)
            assert (d, n_scored) == (D, int(want.scored.sum())) and launches == (1 if n_scored else 0)
            matrix, own, scored = index.related_matrix()
            assert matrix.dtype == np.float64 and scored.dtype == np.int32
            worst = model.check(matrix, own, scored, want)
            print("%s normalized=%d orientation=%d: worst error / bound = %.3f" % (case.name, normalized, orientation, worst))
            if orientation == model.SYMMETRIC:
                assert matrix.tobytes() == matrix.T.copy().tobytes()
            for n, threshold in ((1, -INF), (3, -INF), (64, 0.0), (65, -INF), (1024, float(np.nanmedian(matrix)) if D > 1 else 0.5)):
                _ranking_agrees(index.rank_related(n, threshold), matrix, n, threshold)
            again = index.related(normalized, orientation, 2)
            _ranking_agrees(again, matrix, 2, -INF)
            m2, o2, s2 = index.related_matrix()
            assert m2.tobytes() == matrix.tobytes() and o2.tobytes() == own.tobytes() and s2.tobytes() == scored.tobytes()
    assert 0.0 < index.last_related_ms() < 10000.0


def test_shapes_of_the_smallest_cases(hip):
    one, empty, twins = (_made.get(name) or _made.setdefault(name, _Case(hip, name)) for name in ("one", "empty", "twins"))
    one.index.related_build(1, model.SYMMETRIC)
    matrix, own, scored = one.index.related_matrix()
    assert matrix.shape == (1, 1) and np.isnan(matrix[0, 0]) and own[0] > 0.0 and scored.tolist() == [4]
    found = one.index.rank_related(5)
    assert found.count.tolist() == [0] and found.index.tolist() == [[-1] * 5]
    empty.index.related_build(1, model.DIRECTED)
    matrix, own, scored = empty.index.related_matrix()
    assert scored.tolist() == [5, 0] and matrix[1, 0].tobytes() == np.float64(0.0).tobytes() and own[1].tobytes() == np.float64(0.0).tobytes()
    assert matrix[0, 1] >= 0.0                                               # (still a column)
    assert empty.index.rank_related(5).count.tolist() == [1, 1]
    for orientation in (model.DIRECTED, model.SYMMETRIC):
        twins.index.related_build(1, orientation)
        matrix, own, _ = twins.index.related_matrix()
        assert matrix[0, 1].tobytes() == matrix[2, 1].tobytes() and matrix[1, 0].tobytes() == matrix[1, 2].tobytes()
        assert own[0].tobytes() == own[2].tobytes() and matrix[0, 2].tobytes() == matrix[2, 0].tobytes()


@pytest.mark.parametrize("name", ["one", "empty"])
def test_scores_of_the_exact_model(hip, name):
    """The two smallest cases once more with per-string scores that come from tests/score_exact.py, not from the device."""
    case = _made.get(name) or _made.setdefault(name, _Case(hip, name))
    L = max(len(s) for strings in case.collections for s in strings)
    docs = [score_exact.Document([[ord(c) for c in s] for s in strings], L) for strings in case.collections]
    for normalized in (1, 0):
        score = lambda s, b: docs[b].score([ord(c) for c in s], bool(normalized))[0]
        table = case.scores(normalized)
        for s in case.flat:
            assert [score(s, b) for b in range(case.D)] == table[case.row[s]].tolist()
        for orientation in (model.DIRECTED, model.SYMMETRIC):
            case.index.related_build(normalized, orientation)
            model.check(*case.index.related_matrix(), model.exact(case.collections, score, orientation))


@pytest.mark.parametrize("case", ["tiles", "long", "u32"], indirect=True)
def test_the_chunk_setting_does_not_show(hip, case):
    """A build under a chunk of one tile, and one of three tiles, gives the bytes of the default: the tile tree does not know
    of score launches."""
    lib, index = hip.load(), case.index
    results = {}
    try:
        for strings in (0, TILE, 3 * TILE, 1):
            assert lib.east_hip_debug_set_related_chunk(strings) == OK
            for orientation in (model.DIRECTED, model.SYMMETRIC):
                _, n_scored, launches = index.related_build(1, orientation)
                tiles = sum(-(-int(c) // TILE) for c in case.exact(1, orientation).scored)
                per = {0: tiles, 1: 1}.get(strings, strings // TILE)
                assert launches == -(-tiles // per), (strings, launches, tiles)
                results.setdefault(orientation, []).append(tuple(a.tobytes() for a in index.related_matrix()))
    finally:
        lib.east_hip_debug_set_related_chunk(0)
    for orientation, found in results.items():
        assert all(f == found[0] for f in found[1:]), orientation
    if case.name == "tiles":
        model.check(*index.related_matrix(), case.exact(1, model.SYMMETRIC))


def test_the_handle_afterwards(hip):
    """The related build replaces the resident keyphrases: score_resident is refused until new ones are set; a ranking of
    keyphrases set again gives what it gave before; a later score call leaves the finished matrix valid; the reset call
    releases it."""
    lib = hip.load()
    texts = _cases()["twins"]
    index = hip.HipIndex()
    nothing = np.zeros(3, dtype=np.int64)
    assert lib.east_hip_related_build(index._h, 1, 1, nothing.ctypes.data_as(hip._c_i64p)) == ERR_NOT_BUILT
    index.build_texts(texts)
    assert lib.east_hip_related_fetch(index._h, None, None, None) == ERR_NOT_BUILT
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_RELATED, hip.TOP_BY_KEYPHRASE, 3, -INF, None) == ERR_NOT_BUILT
    assert lib.east_hip_related_build(index._h, 1, 2, None) == ERR_INVALID
    assert lib.east_hip_related_build(index._h, 1, -1, None) == ERR_INVALID
    qs, qo = hip.pack_queries(["ABC", "XYZQ", "EEE"])
    index.set_keyphrases(qs, qo)
    index.score_resident(True)
    before = index.top(hip.TOP_BY_TEXT, 3)
    index.related_build(1, model.SYMMETRIC)
    matrix = index.related_matrix()
    with pytest.raises(Exception) as refused:
        index.score_resident(True)
    assert "no keyphrases set" in str(refused.value) and "(code %d)" % ERR_INVALID in str(refused.value)
    assert lib.east_hip_top_build_resident(index._h, hip.GRAPH_SOURCE_AST, hip.TOP_BY_TEXT, 3, -INF, None) == ERR_NOT_BUILT
    index.set_keyphrases(qs, qo)
    index.score_resident(True)
    after = index.top(hip.TOP_BY_TEXT, 3)
    assert all(getattr(after, f).tobytes() == getattr(before, f).tobytes() for f in ("count", "index", "score"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(index.related_matrix(), matrix))      # (still valid)
    _ranking_agrees(index.rank_related(2), matrix[0], 2, -INF)
    assert lib.east_hip_reset(index._h) == OK
    assert lib.east_hip_related_fetch(index._h, None, None, None) == ERR_NOT_BUILT
    assert lib.east_hip_last_related_ms(index._h) == -1.0
    index.close()


def test_texts_related_on_the_device_and_on_the_host(hip, monkeypatch):
    """applications.texts_related on the device against EAST_HIP_RELATED=host: the values agree within twice the bound; the
    names are compared only through each path's own matrix.  keyphrases_top afterwards gives what it gave before."""
    from east import applications, relevance, utils
    raw = _cases()["twins"] + [b"no 1 of it", _text(20, 30)]
    texts = {"t%d" % d: t for d, t in enumerate(raw)}
    names = list(texts)
    D = len(names)
    kps = ["abc def", "xyz", "ghi"]
    monkeypatch.delenv("EAST_HIP_RELATED", raising=False)
    monkeypatch.delenv("EAST_HIP_TOP", raising=False)
    measure = relevance.ASTRelevanceMeasure()
    top_before = applications.keyphrases_top(kps, texts, 2, "text", None, measure)
    for orientation, code in (("directed", model.DIRECTED), ("symmetric", model.SYMMETRIC)):
        on_device = applications.texts_related(texts, 3, orientation, None, measure)
        device_matrix, _, scored = measure.index.related_matrix()
        assert on_device == {names[s]: [(names[i], v) for i, v in entries]
                             for s, entries in enumerate(applications._top_select(device_matrix, 1, 3, -INF))}
        monkeypatch.setenv("EAST_HIP_RELATED", "host")
        full = applications.texts_related(texts, 1024, orientation, None, measure)
        host_matrix = np.full((D, D), np.nan)
        for a, entries in enumerate(full.values()):
            for other, v in entries:
                host_matrix[a, names.index(other)] = v
        on_host = applications.texts_related(texts, 3, orientation, None, measure)
        monkeypatch.delenv("EAST_HIP_RELATED")
        assert on_host == {names[s]: [(names[i], v) for i, v in entries]
                           for s, entries in enumerate(applications._top_select(host_matrix, 1, 3, -INF))}
        collections = [utils.text_to_strings_collection(t) for t in raw]
        flat = sorted({s for strings in collections for s in model.scored_strings(strings)})
        table = measure.relevance_table(flat)
        row = {s: i for i, s in enumerate(flat)}
        want = model.exact(collections, lambda s, b: table[row[s], b], code)
        assert scored.tolist() == want.scored.tolist()
        for a in range(D):
            for b in range(D):
                if a != b:
                    assert abs(device_matrix[a, b] - host_matrix[a, b]) <= 2.0 * float(want.allowed(a, b)), (a, b)
        assert applications.keyphrases_top(kps, texts, 2, "text", None, measure) == top_before
