"""gpu tier: the small launches at the end of a build and in a score call.

  * ann_wide_kernel's block order (slice-major inside groups of 8 runs): tables of 1 to 513 tiles -- one run, a group that is
    not full, a full one and one more --, every rank listed and next to none;
  * level 2 of the min pyramid, written by ann_stream_kernel: every level of a built handle against the minimum over
    aligned blocks of 16^l ranks of its LCP table, padding included;
  * the flags of a speculative build (something was kept / the alphabet differs / nothing) set by the placement pass's own
    workgroups, and the check of the documents' last symbols in the code map's launch;
  * q_code made once per code map and set of keyphrases;
  * the score walk's second output.

Every table and score is compared with a handle of its own that has built nothing else (reserve_symbols: none out of the
pool), the annotation tables with the stack pass of tests/test_gpu_annotation_search.py and with the oracle.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_annotation_search import _check, geometry  # noqa: F401  (geometry: a fixture)

pytestmark = pytest.mark.gpu

TABLES = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")
TERM = 0x0A00
NONE = 0xFFFFFFFF
_u32p, _i64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)


# ---- block order of ann_wide_kernel ----------------------------------------------------------------------------------

def _ramp(n):
    """lcp[0] = 0, then descending: every PSV is rank 0, every rank beyond the first window is listed."""
    return np.concatenate([[0], np.arange(n - 1, 0, -1)]).astype(np.uint32)


def _sparse(rng, n, tile):
    """Equal fillers (each finds its answer in its left neighbour) and one or two ranks per tile with a smaller value: those
    find their equal a tile away, and the filler behind each is the first l-index of an interval that ends at the next of
    them -- a handful of listed ranks per tile, never more than the first slice of a run takes."""
    lcp = np.full(n, 9, dtype=np.uint32)
    lcp[0] = 0
    for t in range(1, -(-n // tile)):
        lo, hi = t * tile, min((t + 1) * tile, n)
        k = int(rng.integers(1, 3))
        at = rng.choice(np.arange(lo, hi), size=min(k, hi - lo), replace=False)
        lcp[at] = 5
    return lcp


@pytest.mark.parametrize("t", [1, 63, 64, 65, 513])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("kind", ["ramp", "sparse"])
def test_wide_block_order(hip, geometry, t, delta, kind):
    tile = geometry[0]
    n = tile * t + delta
    if kind == "ramp":
        listed = _check(hip, _ramp(n), what="ramp, %d tiles %+d" % (t, delta))
        if n > 2 * tile:
            assert listed >= n - 2 * tile               # every slice of every run had work
    else:
        rng = np.random.default_rng(100 * t + delta + 1)
        listed = _check(hip, _sparse(rng, n, tile), what="sparse, %d tiles %+d" % (t, delta))
        assert listed <= 4 * t + 4                      # (the placed ranks and the filler behind each): only the first slice


def test_wide_block_order_documents_inside_a_run(hip, geometry):
    """Several documents whose seams fall inside runs of 64 tiles (and inside tiles): each seam's zero bounds the searches."""
    tile = geometry[0]
    n = 130 * tile + 7
    starts = [3 * tile + 5, 40 * tile, 64 * tile - 1, 64 * tile + 1, 100 * tile + tile // 2]
    doc_off = [0] + starts + [n]
    rng = np.random.default_rng(7)
    for kind in ("ramp", "sparse"):
        lcp = _ramp(n) if kind == "ramp" else _sparse(rng, n, tile)
        lcp[lcp == 0] = 1
        lcp[doc_off[:-1]] = 0
        _check(hip, lcp, doc_off, [int(rng.integers(1, 4)) for _ in doc_off[:-1]], what="%s, documents at %s" % (kind, starts))


# ---- the pyramid ---------------------------------------------------------------------------------------------------------

def _fresh(hip, sym):
    return hip.HipIndex(reserve_symbols=int(sym.size))


def _one_document(rng, n, letters):
    sym = rng.integers(65, 65 + letters, size=n).astype(np.uint32)
    sym[-1] = TERM
    return sym


def _pyramid_level(hip, index, level):
    """(number of levels, length, the level with its padding) of a built handle."""
    lib = hip.load()
    geo = np.zeros(3, dtype=np.int64)
    assert lib.east_hip_debug_pyramid_level(index._h, level, None, 0, geo.ctypes.data_as(_i64p)) == 0
    out = np.full(int(geo[2]), 0xDEADBEEF, dtype=np.uint32)
    if out.size:
        rc = lib.east_hip_debug_pyramid_level(index._h, level, out.ctypes.data_as(_u32p), out.size, geo.ctypes.data_as(_i64p))
        assert rc == 0, lib.east_hip_last_error()
    return int(geo[0]), int(geo[1]), out


def _level_model(lcp, level):
    """min over aligned blocks of 16^level ranks; the padding up to a multiple of 16 entries holds NONE."""
    n, width = lcp.size, 16 ** level
    length = -(-n // width)
    want = np.full(-(-length // 16) * 16, NONE, dtype=np.uint32)
    want[:length] = np.minimum.reduceat(lcp, np.arange(0, n, width))
    return length, want


@pytest.mark.parametrize("n", [255 * 16, 256 * 16, 256 * 16 + 1, 257 * 16, 1001 * 16 - 11, 4096 * 16 - 1, 4096 * 16, 4096 * 16 + 1])
def test_pyramid_levels_of_a_built_handle(hip, n):
    """255, 256, 257 level-1 entries (16, 16 and 17 level-2 entries: no third level / the first one), a level 1 that is no
    multiple of 16 long, and one rank to either side of 4 096 x 16 (level 3 gets its second entry)."""
    rng = np.random.default_rng(n)
    sym = _one_document(rng, n, 4)
    index = _fresh(hip, sym)
    index.build(sym, [0, n], [1])
    lcp = index.tables(0, names=("lcptab",))["lcptab"].astype(np.uint32)
    levels = _pyramid_level(hip, index, 0)[0]
    want_levels = 1
    while -(-n // 16 ** (want_levels - 1)) > 16:
        want_levels += 1
    assert levels == want_levels, (n, levels, want_levels)
    assert levels >= 3
    for level in range(1, levels):
        _, length, got = _pyramid_level(hip, index, level)
        want_length, want = _level_model(lcp, level)
        assert length == want_length, (n, level, length, want_length)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (n, "level", level, "first differing entries", bad[:8], got[bad[:8]], want[bad[:8]])
    assert _pyramid_level(hip, index, levels)[1:2] == (0,)             # (a level the pyramid does not have)
    index.close()


@pytest.mark.parametrize("n", [3 * 2048 + 5, 70001])
def test_wide_intervals_across_tile_seams_against_the_oracle(hip, oracle, geometry, n):
    """Two letters: the intervals of the prefixes A, AA, AAA, ... are n / 2, n / 4, ... ranks wide -- wider than 4 096, than
    256 and than a tile, across every tile seam.  Annotation and child tables against the oracle."""
    assert n > 2 * geometry[0]
    rng = np.random.default_rng(n)
    sym = _one_document(rng, n, 2)
    index = _fresh(hip, sym)
    index.build(sym, [0, n], [1])
    got = index.tables(0)
    o = oracle.OracleEASA(symbols=sym, n_strings=1)
    ann = np.asarray(o.anntab)
    assert ((ann > 256) & (ann <= 4096)).sum() >= 4 and (n < 8192 or (ann > 4096).sum() >= 3)
    for name in TABLES:
        assert np.array_equal(got[name], getattr(o, name)), (n, name)
    index.close()


# ---- the flags of a speculative build ------------------------------------------------------------------------------------

N_FLAGS = 65536 + 1000          # (just above REFINE_SMALL_INPUT, csrc/window_sort.h)


def _texts_for_flags():
    rng = np.random.default_rng(11)
    random_upper = _one_document(rng, N_FLAGS, 26)
    random_upper_2 = _one_document(rng, N_FLAGS, 26)
    random_lower = _one_document(rng, N_FLAGS, 26)
    random_lower[:-1] += 32
    period3 = np.tile(np.array([65, 66, 67], dtype=np.uint32), N_FLAGS // 3 + 1)[:N_FLAGS].copy()
    period3[-1] = TERM
    return random_upper, random_upper_2, random_lower, period3


@pytest.mark.parametrize("pair", ["large tie groups", "another alphabet", "random twice"])
def test_speculative_build_flags(hip, pair):
    """The second build of each pair is speculative (no refinement rounds expected, the alphabet of the first).  A guess that
    does not hold repeats the build: two launches of the code map's kernel, and the placement's counts read back
    (build_info: first_n, first_kept); one that holds does neither."""
    upper, upper_2, lower, period3 = _texts_for_flags()
    second = {"large tie groups": period3, "another alphabet": lower, "random twice": upper_2}[pair]
    index = _fresh(hip, upper)
    index.build(upper, [0, N_FLAGS], [1])
    first = index.info()
    assert first["window_sorted"] == 1 and first["refine_rounds"] == 0, first        # (what the next build's guesses rest on)
    index.profile_enable(True)
    index.build(second, [0, N_FLAGS], [1])
    report = index.profile_report()
    index.profile_enable(False)
    info = index.info()
    print(pair, info, {k: v[0] for k, v in report.items()})
    assert "spec_counts_kernel" not in report and "validate_last_symbol_kernel" not in report and "codemap_kernel" not in report
    if pair == "random twice":
        assert report["validate_codemap_kernel"][0] == 1, report
        assert info["first_n"] == 0, info                   # (nothing read back: the build went through on its guesses)
    else:
        assert report["validate_codemap_kernel"][0] == 2, report
        assert info["first_n"] > 0, info
        if pair == "large tie groups":
            assert info["first_kept"] > 0 and info["refine_rounds"] + info["persist_rounds"] > 0, info
    got = index.tables(0)
    fresh = _fresh(hip, second)
    fresh.build(second, [0, N_FLAGS], [1])
    want = fresh.tables(0)
    for name in TABLES:
        assert np.array_equal(got[name], want[name]), (pair, name)
    index.close()
    fresh.close()


# ---- the documents' last symbols -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_docs", [1, 255, 256, 257])
@pytest.mark.parametrize("faulty", ["first", "last"])
def test_document_without_a_terminator(hip, n_docs, faulty):
    from east import exceptions
    rng = np.random.default_rng(n_docs)
    doc_len = 40
    sym = rng.integers(65, 91, size=n_docs * doc_len).astype(np.uint32)
    sym[doc_len - 1::doc_len] = TERM
    off = np.arange(n_docs + 1, dtype=np.int64) * doc_len
    ms = np.ones(n_docs, dtype=np.int32)
    bad = sym.copy()
    bad[doc_len - 1 if faulty == "first" else n_docs * doc_len - 1] = 65
    index = _fresh(hip, sym)
    with pytest.raises(exceptions.HipBackendError, match="does not end in a string terminator"):       # a first build
        index.build(bad, off, ms)
    index.build(sym, off, ms)
    want = index.tables(n_docs - 1)
    index.profile_enable(True)
    with pytest.raises(exceptions.HipBackendError, match="does not end in a string terminator"):       # a speculative build
        index.build(bad, off, ms)
    report = index.profile_report()
    index.profile_enable(False)
    # ... which it was: queued once on the guesses of the build before, bytes and bitmap in one pass, no sample, no second attempt
    assert report["validate_codemap_kernel"][0] == 1, report
    assert "presence_kernel" not in report and "sample_prefix_kernel" not in report, report
    assert "presence_remap_kernel" in report or "presence_remap_hist_kernel" in report, report
    index.build(sym, off, ms)
    got = index.tables(n_docs - 1)
    for name in TABLES:
        assert np.array_equal(got[name], want[name]), name
    index.close()


# ---- q_code ---------------------------------------------------------------------------------------------------------------

def _scores_of_a_fresh_handle(hip, sym, off, ms, qs, qo, tagged=False):
    from east.asts import utils as ast_utils
    fresh = _fresh(hip, sym)
    fresh.build(ast_utils.tag_terminators(sym) if tagged else sym, off, ms)
    table = fresh.score_table(qs, qo, True)
    fresh.close()
    return table


def _resident(index, n_kp, normalized=True):
    import torch
    out = torch.full((n_kp, index.n_docs), -7.0, dtype=torch.float64, device="cuda:%d" % index.device)
    index.score_resident(normalized, out.data_ptr())
    return out.cpu().numpy()


def test_query_map_follows_the_code_map_and_the_keyphrases(hip):
    from east import synthetic
    from east.asts import utils as ast_utils
    rng = np.random.default_rng(21)
    n = N_FLAGS
    upper = _one_document(rng, n, 26)
    lower = upper.copy()
    lower[:-1] += 32
    off, ms = [0, n], [1]
    # keyphrases with symbols of both alphabets: half of each matches nothing in the other text
    qa, oa = synthetic.keyphrases(rng, upper, 40)
    qb, ob = synthetic.keyphrases(rng, lower, 40)
    qs, qo = np.concatenate([qa, qb]), np.concatenate([oa, ob[1:] + oa[-1]])
    qs2, qo2 = synthetic.keyphrases(rng, np.concatenate([upper[:-1], lower]), 50)
    index = _fresh(hip, upper)
    index.profile_enable(True)

    def launches():
        return index.profile_report().get("query_map_kernel", (0, 0.0))[0]

    # 1. build, set_keyphrases, score
    index.build(upper, off, ms)
    index.set_keyphrases(qs, qo)
    k = qo.size - 1
    want_upper = _scores_of_a_fresh_handle(hip, upper, off, ms, qs, qo)
    assert np.array_equal(_resident(index, k), want_upper)
    assert launches() == 1
    # 2. score again: the same keyphrases under the same code map
    assert np.array_equal(_resident(index, k), want_upper)
    assert launches() == 1
    # 3. the same text again: a speculative build that confirms the code map
    index.build(upper, off, ms)
    assert np.array_equal(_resident(index, k), want_upper)
    assert launches() == 1
    # 4. another alphabet
    index.build(lower, off, ms)
    want_lower = _scores_of_a_fresh_handle(hip, lower, off, ms, qs, qo)
    assert not np.array_equal(want_lower, want_upper)
    assert np.array_equal(_resident(index, k), want_lower)
    assert launches() == 2
    # 5. other keyphrases
    index.set_keyphrases(qs2, qo2)
    k = qo2.size - 1
    assert np.array_equal(_resident(index, k), _scores_of_a_fresh_handle(hip, lower, off, ms, qs2, qo2))
    assert launches() == 3
    # 6. a tagged build (of the first text: the code map changes back)
    index.build(ast_utils.tag_terminators(upper), off, ms)
    assert np.array_equal(_resident(index, k), _scores_of_a_fresh_handle(hip, upper, off, ms, qs2, qo2, tagged=True))
    assert launches() == 4
    index.close()


def test_query_map_after_a_build_that_did_not_compare_the_bitmaps(hip):
    """A speculative build from a device pointer that is not 16-byte aligned takes the symbol-by-symbol alphabet pass and only
    has its alphabet SIZE checked: A-Z then a-z goes through without a repeat on a NEW code map, and q_code is made again."""
    import torch
    from east import synthetic
    rng = np.random.default_rng(23)
    n = N_FLAGS
    upper = _one_document(rng, n, 26)
    lower = upper.copy()
    lower[:-1] += 32
    off, ms = [0, n], [1]
    qa, oa = synthetic.keyphrases(rng, upper, 40)
    qb, ob = synthetic.keyphrases(rng, lower, 40)
    qs, qo = np.concatenate([qa, qb]), np.concatenate([oa, ob[1:] + oa[-1]])
    k = qo.size - 1

    def shifted(sym):                                   # (a view one element into an allocation: 4 bytes past a 16-byte boundary)
        t = torch.from_numpy(np.concatenate([[0], sym]).astype(np.uint32).view(np.int32)).to("cuda:0")
        assert (t.data_ptr() + 4) % 16 == 4
        return t, t.data_ptr() + 4

    index = _fresh(hip, upper)
    index.profile_enable(True)
    keep_u, ptr_u = shifted(upper)
    keep_l, ptr_l = shifted(lower)
    index.build_device(ptr_u, n, off, ms)
    index.set_keyphrases(qs, qo)
    want_upper = _scores_of_a_fresh_handle(hip, upper, off, ms, qs, qo)
    want_lower = _scores_of_a_fresh_handle(hip, lower, off, ms, qs, qo)
    assert not np.array_equal(want_lower, want_upper)
    assert np.array_equal(_resident(index, k), want_upper)
    index.build_device(ptr_l, n, off, ms)
    report = index.profile_report()
    assert report["validate_codemap_kernel"][0] == 2, report          # (one per build: the second was not repeated)
    assert np.array_equal(_resident(index, k), want_lower)
    assert index.profile_report()["query_map_kernel"][0] == 2
    # the same text again from an aligned pointer: the bitmaps are compared and agree, q_code stands
    aligned = torch.from_numpy(lower.view(np.int32)).to("cuda:0")
    index.build_device(aligned.data_ptr(), n, off, ms)
    assert np.array_equal(_resident(index, k), want_lower)
    assert index.profile_report()["query_map_kernel"][0] == 2
    # ... and once more unaligned: not compared, so not taken for confirmed
    index.build_device(ptr_l, n, off, ms)
    assert np.array_equal(_resident(index, k), want_lower)
    assert index.profile_report()["query_map_kernel"][0] == 3
    del keep_u, keep_l
    index.close()


# ---- the score walk's second output ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_docs", [1, 9])
@pytest.mark.parametrize("path", ["fused", "reduce", "fused, large table", "reduce, large table"])
def test_score_resident_into_the_callers_block(hip, n_docs, path):
    """The kernels' second output (a table of at most 2^18 scores) and the copy behind the walk (a larger one)."""
    from east import synthetic
    rng = np.random.default_rng(31 + n_docs)
    n_kp = 60 if "large" not in path else (1 << 18) // n_docs + 1
    lens = rng.integers(3000, 5000, size=n_docs)
    docs = [_one_document(rng, int(m), 4) for m in lens]
    sym = np.concatenate(docs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ms = np.ones(n_docs, dtype=np.int32)
    qs, qo = synthetic.keyphrases(rng, sym, min(n_kp, 30000), off)
    if n_kp > 30000:                                     # (one document: the same keyphrases several times over)
        reps = -(-n_kp // 30000)
        qo = np.concatenate([[0], np.cumsum(np.tile(np.diff(qo), reps))]).astype(np.int64)
        qs = np.tile(qs, reps)
    if path.startswith("reduce"):
        # one keyphrase longer than a workgroup: per-suffix results and the reduction kernel
        long_kp = docs[-1][100:100 + 300]
        assert long_kp.size > 256 and (long_kp < TERM).all()
        qs, qo = np.concatenate([qs, long_kp]), np.concatenate([qo, [qo[-1] + long_kp.size]])
    index = _fresh(hip, sym)
    index.build(sym, off, ms)
    for normalized in (True, False):
        want = index.score_table(qs, qo, normalized)
        assert (want > 0).any()
        assert np.array_equal(_resident(index, qo.size - 1, normalized), want), (path, n_docs, normalized)
    index.close()
