"""gpu tier: what a build leaves queued and remembered for the call behind it.

  * ann_wide_kernel's two block orders (grouped / slice-major over the whole grid), each forced by the knob, on the
    tables of tests/test_gpu_step_tail.py and with document seams inside runs and tiles;
  * the order a build takes from the count of the build before on its handle (east_hip_build_info [28]);
  * the k-gram tables finished behind the build's flags read-back (east_hip_build_info [29]): the scores of every call
    sequence with the knob on equal those with the knob off, on handles of their own;
  * the caller's symbol buffer overwritten as soon as east_hip_build_device has returned;
  * the pinned block the flags come back into and the document table goes up from: errors found by the read-back, the
    handle's recovery, two handles side by side, a handle closed right behind a build.

Every knob is process-wide and goes back to its default in a finalizer.
"""
import numpy as np
import pytest

from test_gpu_annotation_search import _check, geometry  # noqa: F401  (geometry: a fixture)
from test_gpu_step_tail import _ramp, _sparse

pytestmark = pytest.mark.gpu

TABLES = ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index")
TERM = 0x0A00
N_MARKED = 65536 + 1000         # (just above REFINE_SMALL_INPUT, csrc/window_sort.h: the build marks the k-gram tables)
GROUPED, WHOLE_GRID = 1, 2


@pytest.fixture
def knobs(hip, request):
    """Setters by name; every knob a test touched is put back when it ends."""
    lib = hip.load()
    defaults = {"ann_wide_order": 0, "eager_kgram": 1, "window_sort": 1, "speculation": 1, "segmented_sort": -1}

    def restore():
        for name, value in defaults.items():
            assert getattr(lib, "east_hip_debug_set_" + name)(value) == 0

    request.addfinalizer(restore)

    def set_knob(name, value):
        assert name in defaults
        assert getattr(lib, "east_hip_debug_set_" + name)(value) == 0

    return set_knob


def _fresh(hip, n):
    return hip.HipIndex(reserve_symbols=int(n))          # (never a recycled handle)


def _random_document(rng, n, letters=26, base=65):
    sym = rng.integers(base, base + letters, size=n).astype(np.uint32)
    sym[-1] = TERM
    return sym


def _collection(rng, lens, letters=26, base=65):
    docs = [_random_document(rng, int(m), letters, base) for m in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(docs), off, np.ones(len(docs), dtype=np.int32)


def _all_tables(index):
    return [index.tables(d) for d in range(index.n_docs)]


def _assert_tables_equal(got, want, what):
    assert len(got) == len(want), what
    for d, (g, w) in enumerate(zip(got, want)):
        for name in TABLES:
            assert np.array_equal(g[name], w[name]), (what, "document", d, name)


def _tables_of_a_fresh_handle(hip, sym, off, ms):
    fresh = _fresh(hip, sym.size)
    fresh.build(sym, off, ms)
    out = _all_tables(fresh)
    fresh.close()
    return out


def _resident(index, n_kp, normalized=True):
    import torch
    out = torch.full((n_kp, index.n_docs), -7.0, dtype=torch.float64, device="cuda:%d" % index.device)
    index.score_resident(normalized, out.data_ptr())
    return out.cpu().numpy()


# ---- the two block orders of ann_wide_kernel -------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [GROUPED, WHOLE_GRID])
@pytest.mark.parametrize("t", [1, 63, 64, 65, 513])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("kind", ["ramp", "sparse"])
def test_both_block_orders(hip, geometry, knobs, order, t, delta, kind):
    tile = geometry[0]
    n = tile * t + delta
    knobs("ann_wide_order", order)
    if kind == "ramp":
        listed = _check(hip, _ramp(n), what="ramp, %d tiles %+d, order %d" % (t, delta, order))
        if n > 2 * tile:
            assert listed >= n - 2 * tile               # every slice of every run had work
    else:
        rng = np.random.default_rng(100 * t + delta + 1)
        listed = _check(hip, _sparse(rng, n, tile), what="sparse, %d tiles %+d, order %d" % (t, delta, order))
        assert listed <= 4 * t + 4                      # only the first slice of a run


@pytest.mark.parametrize("order", [GROUPED, WHOLE_GRID])
def test_both_block_orders_with_documents_inside_a_run(hip, geometry, knobs, order):
    tile = geometry[0]
    n = 130 * tile + 7
    starts = [3 * tile + 5, 40 * tile, 64 * tile - 1, 64 * tile + 1, 100 * tile + tile // 2]
    doc_off = [0] + starts + [n]
    rng = np.random.default_rng(7)
    knobs("ann_wide_order", order)
    for kind in ("ramp", "sparse"):
        lcp = _ramp(n) if kind == "ramp" else _sparse(rng, n, tile)
        lcp[lcp == 0] = 1
        lcp[doc_off[:-1]] = 0
        _check(hip, lcp, doc_off, [int(rng.integers(1, 4)) for _ in doc_off[:-1]],
               what="%s, documents at %s, order %d" % (kind, starts, order))


def test_unknown_block_order_is_refused(hip, knobs):
    lib = hip.load()
    assert lib.east_hip_debug_set_ann_wide_order(3) != 0 and lib.east_hip_debug_set_ann_wide_order(-1) != 0
    knobs("ann_wide_order", 0)


# ---- the order a build takes from the build before -------------------------------------------------------------------------

def test_block_order_follows_the_count_of_the_build_before(hip, geometry, knobs):
    tile = geometry[0]
    rng = np.random.default_rng(3)
    n_small, n_large = 3 * tile + 5, (2 * 64 + 1) * tile
    random_a, random_b = _random_document(rng, n_small), _random_document(rng, n_small)
    one_letter = np.full(n_large, 65, dtype=np.uint32)
    one_letter[-1] = TERM
    # the reference: a handle of its own with the order pinned to grouped (the handle under test runs on the default)
    knobs("ann_wide_order", GROUPED)
    want_one_letter = _tables_of_a_fresh_handle(hip, one_letter, np.array([0, n_large]), np.array([1]))
    knobs("ann_wide_order", 0)
    index = _fresh(hip, n_large)

    def build(sym):
        index.build(sym, [0, sym.size], [1])
        return index.info()["ann_wide_order"]

    assert build(random_a) == GROUPED                   # a first build: no count
    assert build(random_b) == WHOLE_GRID                # random text lists next to nothing
    assert build(one_letter) == WHOLE_GRID              # on the stale hint ...
    _assert_tables_equal(_all_tables(index), want_one_letter, "one letter in the whole-grid order")
    assert build(one_letter) == GROUPED                 # ... which this build has replaced: every rank is listed
    _assert_tables_equal(_all_tables(index), want_one_letter, "one letter in the grouped order")
    assert build(random_a) == GROUPED                   # (still on the one-letter count; leaves a short one)
    assert hip.load().east_hip_reset(index._h) == 0
    assert build(random_b) == GROUPED                   # the reset forgot it
    index.close()


# ---- k-gram tables queued behind the flags read-back -----------------------------------------------------------------------

def _case_one_small(rng):
    return _collection(rng, [5000])


def _case_three(rng):
    return _collection(rng, [N_MARKED // 3 + 7, N_MARKED // 3, N_MARKED // 3 + 100])


def _case_257(rng):
    return _collection(rng, rng.integers(200, 400, size=257))


def _case_one_marked(rng):
    return _collection(rng, [N_MARKED])


def _play(hip, eager, knobs, inp, steps, n_kp=40, seed=5, other=None):
    """The call sequence `steps` on a handle of its own: every score table it produced, and kgram_queued after every build."""
    from east import synthetic
    knobs("eager_kgram", int(eager))
    sym, off, ms = inp
    qs, qo = synthetic.keyphrases(np.random.default_rng(seed), sym, n_kp, off)
    index = _fresh(hip, sym.size)
    scores, queued = [], []
    _play.infos = []                                     # (for the message of a failed assertion)
    try:
        for step in steps:
            if step == "build":
                index.build(sym, off, ms)
                _play.infos.append(index.info())
                queued.append(_play.infos[-1]["kgram_queued"])
            elif step == "build other":
                index.build(other[0], other[1], other[2])
                _play.infos.append(index.info())
                queued.append(_play.infos[-1]["kgram_queued"])
            elif step == "keyphrases":
                index.set_keyphrases(qs, qo)
            elif step == "score":
                scores.append(_resident(index, qo.size - 1))
                scores.append(_resident(index, qo.size - 1, normalized=False))
            elif step == "tables":
                scores.append(np.concatenate([t["anntab"] for t in _all_tables(index)]))
            else:
                raise AssertionError(step)
    finally:
        index.close()
    return scores, queued


def _both(hip, knobs, inp, steps, **kw):
    on, queued_on = _play(hip, True, knobs, inp, steps, **kw)
    _both.infos = _play.infos
    off, queued_off = _play(hip, False, knobs, inp, steps, **kw)
    assert len(on) == len(off) and len(on) > 0
    for i, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b), (steps, "result", i)
    assert (on[0] > 0).any()
    assert queued_off == [0] * len(queued_off), queued_off
    return queued_on


STEADY = ["build", "keyphrases", "score", "build", "score"]


@pytest.mark.parametrize("case", [_case_one_small, _case_three, _case_257, _case_one_marked], ids=lambda f: f.__name__)
def test_eager_kgram_tables_give_the_same_scores(hip, knobs, case):
    inp = case(np.random.default_rng(41))
    queued = _both(hip, knobs, inp, STEADY)
    assert queued[0] == 0                               # no keyphrases yet
    if case is not _case_one_small:
        assert queued[1] == 1, queued                   # marks written, keyphrases resident: queued, and they stood


def test_eager_kgram_tables_on_incomplete_marks(hip, knobs):
    """FLAG_KG_BAD: the fused finish (forced: window sort 6) hands a bucket to the rounds while the k-gram code reaches
    below the top part of the key -- 9 documents (4 key bits, kept in the keys: no segmented sort) of 145 000 symbols over
    64 letters (7 bits): 4 symbols in a 32-bit key with no spare bit, 3 levels of k-gram tables (66^3 bins), so the third
    symbol's field reaches into the low 8 bits; mildly skewed letters (a steeper skew takes 64-bit keys) and a planted
    period of three, the bucket that is handed over.  What the build queued is discarded (kgram_queued == 2) and the score
    side builds the tables.  Without speculation: the build behind set_keyphrases runs as the first one did."""
    rng = np.random.default_rng(8800)
    p = 1.0 / np.sqrt(np.arange(64) + 1.0)
    lens = [145000] * 9
    docs = []
    for m in lens:
        d = (40 + rng.choice(64, size=m, p=p / p.sum())).astype(np.uint32)
        d[1000:4000] = np.tile(d[:3], 1000)
        d[-1] = TERM
        docs.append(d)
    inp = (np.concatenate(docs), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.ones(9, dtype=np.int32))
    knobs("window_sort", 6)
    knobs("segmented_sort", 0)
    knobs("speculation", 0)
    queued = _both(hip, knobs, inp, STEADY)
    assert queued == [0, 2], (queued, _both.infos)


def test_eager_kgram_tables_behind_a_wrong_alphabet_guess(hip, knobs):
    rng = np.random.default_rng(43)
    upper = _collection(rng, [N_MARKED])
    lower = (upper[0].copy(), upper[1], upper[2])
    lower[0][:-1] += 32
    queued = _both(hip, knobs, upper, ["build", "keyphrases", "score", "build other", "score"], other=lower)
    assert queued == [0, 1], queued                     # (the repeat's tables: the first attempt's were marked over)


@pytest.mark.parametrize("steps", [["build", "keyphrases", "build", "build", "score"],
                                   ["build", "keyphrases", "build", "tables", "score"],
                                   ["build", "keyphrases", "build", "score", "score"]],
                         ids=["build build score", "build tables score", "score score"])
def test_eager_kgram_tables_in_other_call_orders(hip, knobs, steps):
    queued = _both(hip, knobs, _case_one_marked(np.random.default_rng(47)), steps)
    assert queued[0] == 0 and set(queued[1:]) == {1}, queued


def test_keyphrases_set_behind_the_build_queue_nothing(hip, knobs):
    queued = _both(hip, knobs, _case_one_marked(np.random.default_rng(53)), ["build", "keyphrases", "score"])
    assert queued == [0]


# ---- the caller's symbols ------------------------------------------------------------------------------------------------

def test_symbol_buffer_overwritten_behind_build_device(hip, knobs):
    import torch
    from east import synthetic
    rng = np.random.default_rng(59)
    sym, off, ms = _case_one_marked(rng)
    qs, qo = synthetic.keyphrases(rng, sym, 40, off)
    want_index = _fresh(hip, sym.size)
    knobs("eager_kgram", 0)
    want_index.build(sym, off, ms)
    want_index.set_keyphrases(qs, qo)
    want_scores, want_tables = _resident(want_index, qo.size - 1), _all_tables(want_index)
    want_index.close()
    knobs("eager_kgram", 1)
    d_sym = torch.from_numpy(sym.view(np.int32)).to("cuda:0")
    index = _fresh(hip, sym.size)
    index.build_device(d_sym.data_ptr(), sym.size, off, ms)
    index.set_keyphrases(qs, qo)
    index.build_device(d_sym.data_ptr(), sym.size, off, ms)
    d_sym.fill_(0x41)                                    # the call has returned: the buffer is the caller's again
    torch.cuda.synchronize()
    assert index.info()["kgram_queued"] == 1
    assert np.array_equal(_resident(index, qo.size - 1), want_scores)
    _assert_tables_equal(_all_tables(index), want_tables, "symbols overwritten behind the build")
    index.close()


# ---- the pinned block ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_docs", [1, 2, 257])
@pytest.mark.parametrize("fault", ["no terminator", "n_strings"])
def test_errors_found_by_the_read_back_and_recovery(hip, n_docs, fault):
    from east import exceptions
    rng = np.random.default_rng(61 + n_docs)
    sym, off, ms = _collection(rng, rng.integers(60, 90, size=n_docs))
    bad_sym, bad_ms = sym.copy(), ms.copy()
    if fault == "no terminator":
        bad_sym[int(off[n_docs // 2 + 1]) - 1] = 65
    else:
        bad_ms[n_docs // 2] = 2
    want = _tables_of_a_fresh_handle(hip, sym, off, ms)
    index = _fresh(hip, sym.size)
    for _ in range(2):                                  # a first build, then a speculative one
        with pytest.raises(exceptions.HipBackendError, match=r"\(code -5\)"):
            index.build(bad_sym, off, bad_ms)
        index.build(sym, off, ms)
        _assert_tables_equal(_all_tables(index), want, "%s among %d documents" % (fault, n_docs))
    index.close()


def test_two_handles_with_interleaved_builds(hip):
    rng = np.random.default_rng(67)
    a1, a2 = _collection(rng, [3000, 2000, 4100]), _collection(rng, [3000, 2000, 4100])
    b1, b2 = _collection(rng, rng.integers(100, 200, size=40)), _collection(rng, rng.integers(100, 200, size=300))
    ha, hb = _fresh(hip, 1 << 16), _fresh(hip, 1 << 16)
    ha.build(*a1)
    hb.build(*b1)
    ha.build(*a2)
    hb.build(*b2)
    _assert_tables_equal(_all_tables(ha), _tables_of_a_fresh_handle(hip, *a2), "handle a")
    _assert_tables_equal(_all_tables(hb), _tables_of_a_fresh_handle(hip, *b2), "handle b")
    ha.build(*a1)
    _assert_tables_equal(_all_tables(hb), _tables_of_a_fresh_handle(hip, *b2), "handle b behind a's build")
    _assert_tables_equal(_all_tables(ha), _tables_of_a_fresh_handle(hip, *a1), "handle a, third build")
    ha.close()
    hb.close()


def test_handle_closed_right_behind_build_device(hip, knobs):
    import torch
    from east import synthetic
    rng = np.random.default_rng(71)
    sym, off, ms = _case_one_marked(rng)
    qs, qo = synthetic.keyphrases(rng, sym, 40, off)
    d_sym = torch.from_numpy(sym.view(np.int32)).to("cuda:0")
    want = _tables_of_a_fresh_handle(hip, sym, off, ms)
    for destroy in (False, True):
        index = _fresh(hip, sym.size)
        index.build_device(d_sym.data_ptr(), sym.size, off, ms)
        index.set_keyphrases(qs, qo)
        index.build_device(d_sym.data_ptr(), sym.size, off, ms)     # (leaves the k-gram launches queued)
        assert index.info()["kgram_queued"] == 1
        if destroy:
            h, index._h = index._h, None
            hip.load().east_hip_destroy(h)
        else:
            index.close()
    again = _fresh(hip, sym.size)
    again.build_device(d_sym.data_ptr(), sym.size, off, ms)
    _assert_tables_equal(_all_tables(again), want, "a handle made behind the closed ones")
    again.close()
