"""The five entry points that take raw texts (east_hip_build_texts[_v], east_hip_cosine_build_texts[_v],
east_hip_group_build_texts_v) share one input type, one set of checks, one upload and one tokenizer (csrc/textfront.h):
what they reject, they reject alike and before they touch the handle; joined and separate texts are the same input; a
shard of a group sees its own texts and no others."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -2                                            # EAST_HIP_ERR_INVALID

# the messages as csrc/textfront.h, csrc/cosine.h and the _v entry points spelled them before the checks became one
NULL_ARG = "null argument or no documents"
NEGATIVE = "negative text length"
RANGE = "total bytes out of range"
ENDS = "text_offsets must start at 0 and end at the total"
INCREASE = "text_offsets must increase"
SEPARATOR = "every text must be followed by one 0xFF separator byte"
NULL_TEXT = "null text"

TEXTS = [b"alpha beta gamma alpha", b"beta delta"]
HUGE = 0x7FFFFFF0

SIX = [b"",
       b"token",
       b"alpha beta gamma",
       "éclair дом — \U0001F600 Ωmega ‰ café".encode("utf-8"),      # 2-, 3- and 4-byte units
       b"abc\xc3 def\xe2\x82 ghi\xffjkl mno \xc3",                                                          # malformed
       "中文中 kept 한국어 words กขก".encode("utf-8")]                  # word characters at or above U+0A00


def _i64(values):
    return np.array(values, dtype=np.int64)


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _bad_inputs(hip):
    """[(name, message, raised inside a shard of a group, joined arguments or None, separate arguments or None)]: the
    arguments behind the handle, in front of the stopwords."""
    tables = hip._table_args()
    blob, offsets = hip._joined(TEXTS)
    ptrs, lengths = hip._separate(TEXTS)
    D, n = len(TEXTS), len(blob)
    assert tables[6] > 0                               # (there are upper-case mappings from below U+0A00 to above it)

    def joined(bytes_=blob, n_bytes=n, off=offsets, n_docs=D, t=tables):
        return (bytes_, n_bytes, None if off is None else _p(off), n_docs) + tuple(t), off

    def separate(p=ptrs, ln=lengths, n_docs=D, t=tables):
        return (p, None if ln is None else _p(ln), n_docs) + tuple(t), (p, ln)

    def with_table(i, value):
        return tables[:i] + (value,) + tables[i + 1:]

    cases = [
        ("null text_offsets", NULL_ARG, False, joined(off=None), None),
        ("null texts", NULL_ARG, False, None, separate(p=None)),
        ("null lengths", NULL_ARG, False, None, separate(ln=None)),
        ("no documents", NULL_ARG, False, joined(n_docs=0), separate(n_docs=0)),
        ("null Unicode table", NULL_ARG, True, joined(t=with_table(1, None)), separate(t=with_table(1, None))),
        ("null class table", NULL_ARG, True, joined(t=with_table(0, None)), separate(t=with_table(0, None))),
        ("n_hi_upper = -1", NULL_ARG, True, joined(t=with_table(6, -1)), separate(t=with_table(6, -1))),
        ("null hi_upper_from", NULL_ARG, True, joined(t=with_table(4, None)), separate(t=with_table(4, None))),
        ("negative length", NEGATIVE, False, None, separate(ln=_i64([len(TEXTS[0]), -1]))),
        ("offsets start at 1", ENDS, False, joined(off=_i64([1, offsets[1], n])), None),
        ("offsets do not increase", INCREASE, False, joined(off=_i64([0, n, n])), None),
        ("offsets end short of the total", ENDS, False, joined(off=_i64([0, offsets[1], n - 1])), None),
        ("a text without its 0xFF", SEPARATOR, False, joined(bytes_=blob[:-1] + b" "), None),
        ("a first text without its 0xFF", SEPARATOR, False, joined(bytes_=blob[:offsets[1] - 1] + b" " + blob[offsets[1]:]), None),
        ("null text of positive length", NULL_TEXT, True, None,
         separate(p=(ctypes.c_char_p * D)(TEXTS[0], None), ln=_i64([len(TEXTS[0]), 5]))),
        # rejected on the range, before a byte is read: there is no such buffer
        ("total out of range", RANGE, True, joined(n_bytes=HUGE, off=_i64([0, HUGE]), n_docs=1),
         separate(ln=_i64([HUGE - 1]), n_docs=1)),
    ]
    return cases


def test_rejection_is_the_same_at_every_entry_point(hip):
    from east import utils
    lib = hip.load()
    sw_cps, sw_off = hip.pack_words(["GAMMA"])
    stop = (sw_cps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _p(sw_off), 1)
    index = hip.HipIndex()
    cosine = hip.HipCosineIndex(index=index)
    group = hip.HipGroup([0, 0])
    try:
        index.build_texts(TEXTS)
        cosine.build_texts(TEXTS, stopwords=["GAMMA"])
        qs, qo = hip.pack_queries([utils.prepare_text(k) for k in ("alpha beta", "delta")])
        before = index.prepared(), index.score_table(qs, qo), cosine.terms()
        assert "ALPHA" in before[2] and "DELTA" in before[2] and before[1][0, 0] > 0 and before[1][1, 1] > 0

        def untouched():
            now = index.prepared(), index.score_table(qs, qo), cosine.terms()
            return all(np.array_equal(a, b) for a, b in zip(now[0], before[0])) and np.array_equal(now[1], before[1]) and \
                now[2] == before[2]

        def rejected(rc, want, where):
            got = lib.east_hip_last_error().decode()
            assert rc == INVALID and got == want, (where, rc, got, want)

        for name, message, in_shard, joined, separate in _bad_inputs(hip):
            if joined is not None:
                args, _keep = joined
                rejected(lib.east_hip_build_texts(index._h, *args), message, (name, "build_texts"))
                assert untouched(), name
                rejected(lib.east_hip_cosine_build_texts(index._h, *(args + stop)), message, (name, "cosine_build_texts"))
                assert untouched(), name
            if separate is not None:
                args, (_p_keep, ln) = separate
                rejected(lib.east_hip_build_texts_v(index._h, *args), message, (name, "build_texts_v"))
                assert untouched(), name
                rejected(lib.east_hip_cosine_build_texts_v(index._h, *(args + stop)), message, (name, "cosine_build_texts_v"))
                assert untouched(), name
                # (a group hands its shards their texts: what only a shard sees -- the tables, its texts, their total -- the
                # first shard that fails reports with its name in front)
                prefix = ""
                if in_shard:
                    doc = 1 if name == "null text of positive length" else 0
                    first = hip.shard_documents(ln[:args[2]], 2)
                    prefix = "shard %d (device 0): " % (int(np.searchsorted(first, doc, side="right")) - 1)
                rejected(lib.east_hip_group_build_texts_v(group._g, *args), prefix + message, (name, "group_build_texts_v"))
        # and the handle goes on working
        index.build_texts(TEXTS[::-1])
        assert np.array_equal(np.diff(index.prepared()[1]), np.diff(before[0][1])[::-1])
    finally:
        group.close()
        index.close()


def _build_joined(hip, index, raw):
    blob, offsets = hip._joined(raw)
    rc = hip.load().east_hip_build_texts(index._h, blob, len(blob), _p(offsets), len(raw), *hip._table_args())
    assert rc == 0, hip.load().east_hip_last_error()
    index.n_docs = len(raw)
    return index.prepared()


def _build_separate(hip, index, raw):
    ptrs, lengths = hip._separate(raw)
    rc = hip.load().east_hip_build_texts_v(index._h, ptrs, _p(lengths), len(raw), *hip._table_args())
    assert rc == 0, hip.load().east_hip_last_error()
    index.n_docs = len(raw)
    return index.prepared()


def _cosine(hip, cos, raw, separate):
    lib = hip.load()
    sw_cps, sw_off = hip.pack_words([])
    args = hip._table_args() + (sw_cps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _p(sw_off), 0)
    if separate:
        ptrs, lengths = hip._separate(raw)
        rc = lib.east_hip_cosine_build_texts_v(cos._h, ptrs, _p(lengths), len(raw), *args)
    else:
        blob, offsets = hip._joined(raw)
        rc = lib.east_hip_cosine_build_texts(cos._h, blob, len(blob), _p(offsets), len(raw), *args)
    assert rc == 0, lib.east_hip_last_error()
    cos.n_docs = len(raw)
    info = cos.info()
    cos.n_terms = V = info["terms"]
    table = cos.score_table([0, 1, 2, V - 1, -1], [0, 1, 3, 5], True)
    assert table.shape == (3, len(raw)) and np.count_nonzero(table) >= 3
    return cos.terms(), {k: v for k, v in info.items() if k not in ("build_us", "score_us")}, table


@pytest.mark.parametrize("raw", [SIX, SIX[:5]], ids=["with_high_text", "streamed_to_the_end"])
def test_joined_and_separate_texts_are_the_same_input(hip, raw):
    """(Without the text at or above U+0A00 the streamed preparation finishes on its own; with it, the preparation in one
    piece takes over behind it.)"""
    from east import utils
    from east.asts import utils as ast_utils
    lib = hip.load()
    assert all(len(t) < 1024 for t in raw)
    index = hip.HipIndex()
    cos = hip.HipCosineIndex()
    try:
        for chunk in (0, 23):
            assert lib.east_hip_debug_set_text_stream(chunk) == 0
            joined = _build_joined(hip, index, raw)
            separate = _build_separate(hip, index, raw)
            assert lib.east_hip_debug_set_text_ring(1, 64) == 0
            ring = _build_separate(hip, index, raw)
            assert lib.east_hip_debug_set_text_ring(-1, 0) == 0
            for other in (separate, ring):
                assert all(np.array_equal(a, b) for a, b in zip(joined, other)), chunk
            # (... and what they agree on is the host chain's, document by document, where the symbols are the reference's)
            sym, off, ms = joined
            assert ast_utils.is_tagged(sym) == (len(raw) == 6)
            for d, t in enumerate(raw if len(raw) == 5 else []):
                want = ast_utils.strings_to_symbols(utils.text_to_strings_collection(t))
                assert np.array_equal(sym[off[d]:off[d + 1]], want), (chunk, d)
            a, b = _cosine(hip, cos, raw, False), _cosine(hip, cos, raw, True)
            assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), chunk
    finally:
        assert lib.east_hip_debug_set_text_stream(-1) == 0
        assert lib.east_hip_debug_set_text_ring(-1, 0) == 0
        index.close()
        cos.close()


def test_a_shard_of_a_group_prepares_its_own_texts(hip):
    """Offsets that were not rebased to the shard's first text, or texts taken from one place too far, would show here."""
    group = hip.HipGroup([0, 0])
    single = hip.HipIndex()
    try:
        group.build_texts(SIX)
        first = group.first_doc.tolist()
        assert first[0] == 0 and first[-1] == len(SIX) and 0 < first[1] < len(SIX)
        for s, shard in enumerate(group.shards):
            single.build_texts(SIX[first[s]:first[s + 1]])
            for a, b in zip(shard.prepared(), single.prepared()):
                assert np.array_equal(a, b), s
    finally:
        single.close()
        group.close()
