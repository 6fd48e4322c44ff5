"""gpu tier: the first radix pass's histogram counted by the remap pass of a speculative build
(csrc/radix_sort.h: presence_remap_hist_kernel).

Kernel level: the fused kernel against remap_bytes_kernel + presence_kernel + radix_hist_kernel<gen> through the same
code map (east_hip_debug_first_pass_hist runs both) -- byte stream, presence words, per-tile running sums, group sums and
sharded digit totals array_equal, whatever the bytes are: the first scatter takes its destinations from these counts.  For
the small sizes a numpy model of the window keys is a second witness.

Build level: builds on one handle with and without the fused histogram (east_hip_debug_set_speculation(2)) against the
oracle and against each other.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLES = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")
TILE, GROUP, BINS, SHARDS, TEXT_SYMBOLS, PRESENT_WORDS = 4096, 8, 256, 8, 0x0A00, 80
TERM = 0x0A00


# ---- the plan of the first level, as csrc/window_sort.h makes it (lvl0_window, lvl0_spare_bits) -------------------

def _spare_bits(used, key_bits, bt, w):
    total = min(-(-used // 8) * 8, key_bits)
    return min(total - used, bt - 1) if w < 12 else 0


def _window(n, bt, tf):
    w, w_max, reach = 3, min(64 // bt, 12), float(tf) ** 3
    while w < w_max and reach < 64.0 * n:
        reach *= tf
        w += 1
    w32 = 32 // bt
    if 3 <= w32 < w:
        spare32 = _spare_bits(w32 * bt, 32, bt, w32)
        buckets = float((tf >> (bt - spare32)) + 1) if spare32 > 0 else 1.0
        if float(tf) ** w32 * buckets >= 4.0 * n:
            w = w32
    return w


def _plans(n, sigma):
    """(key_bytes, w, bt, spare, term_first, shift, mask): the narrow and the wide window the build would take for n
    symbols over sigma text symbols, first digit above the fused finish's low bits where it would run, else bit 0."""
    tf = sigma + 1
    bt = tf.bit_length()
    out = []
    w = _window(n, bt, tf)
    for wide in (False, True):
        ww = max(w, min(12, 64 // bt)) if wide else w
        key_bytes = 8 if wide or ww * bt > 32 else 4
        spare = _spare_bits(ww * bt, key_bytes * 8, bt, ww)
        total = ww * bt + spare
        shift = 8 if total >= 16 else 0
        out.append((key_bytes, ww, bt, spare, tf, shift, (1 << min(8, total - shift)) - 1))
    return out


def _run(hip, sym, code_map, plan):
    key_bytes, w, bt, spare, tf, shift, mask = plan
    n = int(sym.size)
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    s8 = np.zeros(2 * (n + 16), dtype=np.uint8)
    present = np.zeros(2 * PRESENT_WORDS, dtype=np.uint32)
    hist = np.zeros(2 * BINS * tiles, dtype=np.uint32)
    gsum = np.zeros(2 * BINS * groups, dtype=np.uint32)
    total = np.zeros(2 * SHARDS * BINS, dtype=np.uint32)
    u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    sym = np.ascontiguousarray(sym, dtype=np.uint32)
    code_map = np.ascontiguousarray(code_map, dtype=np.uint32)
    rc = hip.load().east_hip_debug_first_pass_hist(
        0, sym.ctypes.data_as(u32p), n, code_map.ctypes.data_as(u32p), key_bytes, w, bt, spare, tf, shift, mask,
        s8.ctypes.data_as(u8p), present.ctypes.data_as(u32p), hist.ctypes.data_as(u32p), gsum.ctypes.data_as(u32p),
        total.ctypes.data_as(u32p))
    assert rc == 0, (rc, plan, n)
    return {"s8": s8.reshape(2, n + 16), "present": present.reshape(2, PRESENT_WORDS), "hist": hist.reshape(2, tiles, BINS),
            "group_sum": gsum.reshape(2, groups, BINS), "digit_total": total.reshape(2, SHARDS, BINS)}


def _model(s8, n, plan):
    """hist / group_sum / digit_total from the byte stream in numpy: the window keys as csrc/window_sort.h defines them."""
    key_bytes, w, bt, spare, tf, shift, mask = plan
    b = np.concatenate([s8[:n + 16].astype(np.uint64), np.zeros(16, dtype=np.uint64)])
    key = np.zeros(n, dtype=np.uint64)
    ended = np.zeros(n, dtype=bool)
    pos = np.arange(n)
    for i in range(w):
        x = np.where(ended, 0, b[pos + i])
        term = x == 0xFF
        ended |= term
        key = (key << np.uint64(bt)) | np.where(term, np.uint64(tf), x)
    if spare:
        x = b[pos + w]
        x = np.where(ended, 0, np.where(x == 0xFF, np.uint64(tf), x))
        key = (key << np.uint64(spare)) | (x >> np.uint64(bt - spare))
    digit = ((key >> np.uint64(shift)) & np.uint64(mask)).astype(np.int64)
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    per_tile = np.zeros((groups * GROUP, BINS), dtype=np.int64)
    np.add.at(per_tile, (pos // TILE, digit), 1)
    per_group = per_tile.reshape(groups, GROUP, BINS)
    running = (np.cumsum(per_group, axis=1) - per_group).reshape(groups * GROUP, BINS)[:tiles]
    gsum = per_group.sum(axis=1)
    total = np.zeros((SHARDS, BINS), dtype=np.int64)
    np.add.at(total, np.arange(groups) % SHARDS, gsum)
    return running, gsum, total


def _check(hip, sym, code_map, plan, model=True, what=""):
    out = _run(hip, sym, code_map, plan)
    n = int(sym.size)
    for name, v in out.items():
        assert np.array_equal(v[0], v[1]), (name, what, plan, n)
    want = np.where(sym < TEXT_SYMBOLS, code_map[np.minimum(sym, TEXT_SYMBOLS - 1)] & 0xFF, 0xFF).astype(np.uint8)
    assert np.array_equal(out["s8"][0][:n], want) and not out["s8"][0][n:].any(), (what, plan, n)
    bits = np.zeros(PRESENT_WORDS, dtype=np.uint32)
    for c in np.unique(sym[sym < TEXT_SYMBOLS]):
        bits[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    assert np.array_equal(out["present"][0], bits), (what, plan, n)
    assert int(out["digit_total"][0].sum()) == n
    if model:
        running, gsum, total = _model(out["s8"][0], n, plan)
        assert np.array_equal(out["hist"][0], running), (what, plan, n)
        assert np.array_equal(out["group_sum"][0], gsum), (what, plan, n)
        assert np.array_equal(out["digit_total"][0], total), (what, plan, n)


def _alphabet(rng, sigma):
    cps = np.sort(rng.choice(np.arange(32, TEXT_SYMBOLS), size=sigma, replace=False)).astype(np.uint32)
    code_map = np.zeros(TEXT_SYMBOLS, dtype=np.uint32)
    code_map[cps] = np.arange(1, sigma + 1, dtype=np.uint32)
    return cps, code_map


def _text(rng, cps, n, term_every=40):
    sym = cps[rng.integers(0, cps.size, size=n)]
    t = rng.random(n) < 1.0 / term_every
    sym[t] = TERM + (np.cumsum(t)[t] - 1).astype(np.uint32) % 1000
    return sym


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 32767, 32768, 32769, 100003, (1 << 22) + 77])
def test_fused_kernel_equals_remap_then_histogram(hip, n):
    """Every size at which the kernel takes another path: below one 16-byte group, n % 4 != 0, one symbol either side of
    a tile and of a histogram group, several groups, more groups than digit-total shards; three alphabets, the narrow and
    the wide window of the plan each (32- and 64-bit keys); text that ends in a terminator and text that does not."""
    rng = np.random.default_rng(1000 + n)
    for sigma in (2, 27, 200):
        cps, code_map = _alphabet(rng, sigma)
        for plan in _plans(n, sigma):
            sym = _text(rng, cps, n)
            if sigma != 27:
                sym[-1] = TERM
            _check(hip, sym, code_map, plan, model=n <= 100003, what="sigma %d" % sigma)
    # the first digit at bit 0 (no fused finish behind the sort)
    cps, code_map = _alphabet(rng, 27)
    key_bytes, w, bt, spare, tf, _, _ = _plans(n, 27)[0]
    _check(hip, _text(rng, cps, n), code_map, (key_bytes, w, bt, spare, tf, 0, 255), model=n <= 100003, what="shift 0")


def test_terminators_at_the_seams(hip):
    """A terminator at every offset -8 .. +1 around a tile seam and around a group seam (a key reaches up to 12 symbols
    to its right: the truncation behind a terminator crosses the seam), runs of terminators, terminators only."""
    rng = np.random.default_rng(7)
    cps, code_map = _alphabet(rng, 27)
    n = GROUP * TILE + TILE + 500
    plans = _plans(n, 27)
    for seam in (TILE, GROUP * TILE):
        for off in range(-8, 2):
            sym = cps[rng.integers(0, cps.size, size=n)]
            sym[seam + off] = TERM
            for plan in plans:
                _check(hip, sym, code_map, plan, what="seam %d%+d" % (seam, off))
        sym = cps[rng.integers(0, cps.size, size=n)]
        sym[seam - 5:seam + 3] = TERM + np.arange(8, dtype=np.uint32)
        sym[-1] = TERM + 8
        for plan in plans:
            _check(hip, sym, code_map, plan, what="run over seam %d" % seam)
    for m in (7, TILE + 1, n):
        sym = (TERM + np.arange(m, dtype=np.uint32) % 1000).astype(np.uint32)
        for plan in plans:
            _check(hip, sym, code_map, plan, what="terminators only")


def test_wrong_code_map_still_counts_what_it_wrote(hip):
    """A map that is wrong for the text (a speculative build finds out at its end): symbols absent from it become byte 0,
    others the byte of another alphabet -- the counts must still be those of the bytes written."""
    rng = np.random.default_rng(11)
    for n in (5, 4097, 3 * GROUP * TILE + 123):
        cps_text, _ = _alphabet(rng, 60)
        cps_map, code_map = _alphabet(rng, 27)
        code_map[cps_text[:20]] = np.arange(1, 21, dtype=np.uint32)      # a third of the text is known to the map
        for plan in _plans(n, 27):
            sym = _text(rng, cps_text, n)
            _check(hip, sym, code_map, plan, what="wrong guess")
        # a map of wide codes (the handle's last alphabet was larger than a byte's worth is never guessed; the low byte counts)
        wide_map = (np.arange(TEXT_SYMBOLS, dtype=np.uint32) * 7 + 1) % 254
        _check(hip, _text(rng, cps_text, n), wide_map, _plans(n, 27)[0], what="any bytes")


# ---- build level ---------------------------------------------------------------------------------------------------

def _sequence():
    from east import synthetic
    rng = np.random.default_rng(77)
    vocab = synthetic.zipf_vocabulary(rng, size=200, exponent=1.0)
    one = lambda sym_m: ([sym_m[0]], [sym_m[1]])
    seq = []
    seq.append(("first", one(synthetic.word_stream_document(rng, 300000, want_text=False)[1:])))
    seq.append(("right guess", one(synthetic.word_stream_document(rng, 300000, want_text=False)[1:])))
    seq.append(("zipf: rounds", one(synthetic.zipf_document(rng, 300000, vocab))))
    seq.append(("after rounds", one(synthetic.word_stream_document(rng, 200000, want_text=False)[1:])))
    sym5 = rng.integers(65, 70, size=150001, dtype=np.uint32)
    sym5[-1] = TERM
    seq.append(("5-letter alphabet", one((sym5, 1))))
    seq.append(("back to words", one(synthetic.word_stream_document(rng, 100000, want_text=False)[1:])))
    rep = np.tile(np.array([65, 66, 67], dtype=np.uint32), 40000)
    seq.append(("long repeats", one((np.concatenate([rep, [TERM]]).astype(np.uint32), 1))))
    # the size varies from build to build: other tile counts, below one tile, several documents, one again
    seq.append(("words 100000", one(synthetic.word_stream_document(rng, 100000, want_text=False)[1:])))
    seq.append(("words 113000", one(synthetic.word_stream_document(rng, 113000, want_text=False)[1:])))
    seq.append(("words 113000 again", one(synthetic.word_stream_document(rng, 113000, want_text=False)[1:])))
    seq.append(("below one tile", one(synthetic.word_stream_document(rng, 3000, want_text=False)[1:])))
    seq.append(("below one tile again", one(synthetic.word_stream_document(rng, 3100, want_text=False)[1:])))
    two = [synthetic.word_stream_document(rng, 60000, want_text=False)[1:] for _ in range(2)]
    seq.append(("two documents", ([d[0] for d in two], [d[1] for d in two])))
    seq.append(("one document again", one(synthetic.word_stream_document(rng, 120000, want_text=False)[1:])))
    seq.append(("and again", one(synthetic.word_stream_document(rng, 120000, want_text=False)[1:])))
    return seq


def _build_all(hip_backend, seq):
    index = hip_backend.HipIndex()
    tables, fused = [], []
    for _, (syms, ms) in seq:
        sym = np.concatenate(syms)
        off = np.concatenate([[0], np.cumsum([s.size for s in syms])]).astype(np.int64)
        index.build(sym, off, np.array(ms, dtype=np.int32))
        fused.append(index.info()["first_hist_fused"])
        tables.append([index.tables(d) for d in range(len(syms))])
    return tables, fused


def test_builds_on_one_handle_with_and_without_the_fused_histogram(hip, oracle):
    """One handle, word-stream documents: the first build counts the first histogram in a launch of its own, the second
    in the remap pass; then every kind of wrong guess, sizes that change from build to build (tile count, below one
    tile) and a build of two documents, which takes the old path.  All six tables equal the oracle's every time, and the
    same sequence with east_hip_debug_set_speculation(2) gives the same tables without the fused kernel."""
    lib = hip.load()
    seq = _sequence()
    tables, fused = _build_all(hip, seq)
    for (what, (syms, ms)), per_doc in zip(seq, tables):
        for sym, m, t in zip(syms, ms, per_doc):
            o = oracle.OracleEASA(symbols=sym, n_strings=m)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (what, name)
    names = [what for what, _ in seq]
    assert fused[0] == 0 and fused[1] == 1, list(zip(names, fused))
    assert fused[names.index("two documents")] == 0
    assert fused[names.index("words 113000 again")] == 1 and fused[names.index("below one tile again")] == 1
    assert fused[names.index("and again")] == 1, list(zip(names, fused))
    assert lib.east_hip_debug_set_speculation(2) == 0
    try:
        tables2, fused2 = _build_all(hip, seq)
    finally:
        assert lib.east_hip_debug_set_speculation(1) == 0
    assert not any(fused2), list(zip(names, fused2))
    for what, a, b in zip(names, tables, tables2):
        for ta, tb in zip(a, b):
            for name in TABLES:
                assert np.array_equal(ta[name], tb[name]), (what, name)
