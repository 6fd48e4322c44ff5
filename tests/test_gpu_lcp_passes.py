"""gpu tier: the two passes that make the LCP table, at kernel level (csrc/build.h: direct_lcp -- lcp_kernel, lcp8_kernel,
lcp_doc_starts_kernel --, finish_capped_lcp -- inverse_sa_kernel, lcp_phi_classify / compare / long_kernel in both
instantiations, the anchors' scan, lcp_phi_anchors_kernel, lcp_phi_fill_kernel).

Everything goes through east_hip_debug_lcp, which runs the functions the build calls on a caller's text and suffix array
and returns the table behind each pass.  The witness is tests/lcp_exact.py (pinned to brute force by
tests/test_lcp_exact_host.py, which also shows that every case reaches what it claims): the direct table is held to its
contract against the exact table, the final table is array_equal to Kasai's, and the two list counters equal the
witness's count for the very direct table the device returned.  The thresholds come from the library (geometry_out);
the cases are made for lcp_exact.GEOMETRY, and the first test fails if the two differ.
"""
import ctypes

import numpy as np
import pytest

import lcp_exact as L

pytestmark = pytest.mark.gpu

_u32p, _i64p, _i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
ERR_INVALID = -2
CASES = {t.what: t for t in L.cases()}
MODE_B = {t.what: t for t in L.mode_b_texts()}


def _lcp(hip, width, stream, term_first, sa, doc_off, n_strings, budget=-1, table=None, fill=0x5A, expect=0):
    stream = np.ascontiguousarray(stream, dtype=np.uint8 if width == 1 else np.uint32)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    n_strings = np.ascontiguousarray(n_strings, dtype=np.int32)
    n = int(sa.size)
    padded = L.pyr_padded(n)
    direct, final = np.full(padded, 0xEEEEEEEE, dtype=np.uint32), np.full(padded, 0xEEEEEEEE, dtype=np.uint32)
    capped, counts = np.full(1, 0xEEEEEEEE, dtype=np.uint32), np.full(2, 0xEEEEEEEE, dtype=np.uint32)
    ann, geo = np.full(n, 0xEEEEEEEE, dtype=np.uint32), np.zeros(6, dtype=np.uint32)
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.uint32)
    rc = hip.load().east_hip_debug_lcp(0, width, stream.ctypes.data_as(ctypes.c_void_p), n, term_first, sa.ctypes.data_as(_u32p),
                                       doc_off.ctypes.data_as(_i64p), doc_off.size - 1, n_strings.ctypes.data_as(_i32p), budget,
                                       table.ctypes.data_as(_u32p) if table is not None else None, fill,
                                       direct.ctypes.data_as(_u32p), capped.ctypes.data_as(_u32p), final.ctypes.data_as(_u32p),
                                       counts.ctypes.data_as(_u32p), ann.ctypes.data_as(_u32p), geo.ctypes.data_as(_u32p))
    assert rc == expect, (rc, hip.last_error() if hasattr(hip, "last_error") else "")
    if expect != 0:                                       # (nothing was launched, nothing was written)
        assert np.all(direct == 0xEEEEEEEE) and np.all(final == 0xEEEEEEEE) and np.all(ann == 0xEEEEEEEE) and capped[0] == 0xEEEEEEEE
        return None
    return direct, int(capped[0]), final, (int(counts[0]), int(counts[1])), ann, tuple(int(g) for g in geo)


def _run(hip, text, width, budget=-1, table=None, fill=0x5A):
    return _lcp(hip, width, text.stream(width), text.term_first, text.sa(), text.doc_off, text.n_strings, budget, table, fill)


def _check_final(text, width, direct, final, counts, geo):
    exact = text.exact(width)
    assert not np.any(final[:text.n] & L.PARTIAL), "an unfinished entry is left"
    if not np.array_equal(final[:text.n], exact):
        bad = int(np.flatnonzero(final[:text.n] != exact)[0])
        raise AssertionError("%s, width %d: the final table differs at rank %d: %d, want %d (direct %#x)"
                             % (text.what, width, bad, final[bad], exact[bad], direct[bad]))
    assert np.all(final[text.n:] == L.NONE), "the padding of the final table"
    assert counts == L.counters(direct, exact, text.sa(), text.reducible(width), width, geo)


def test_geometry(hip):
    t = L.random_text("tiny", 40, 3, 1)
    geo = _run(hip, t, 4)[5]
    assert geo == L.GEOMETRY, "tests/lcp_exact.py states the caps and strides its cases are made for: restate them"


@pytest.mark.parametrize("budget", ["none", "zero", "build"])
@pytest.mark.parametrize("name", list(CASES))
def test_direct_and_finishing_pass(hip, name, budget):
    text = CASES[name]
    b = {"none": -1, "zero": 0, "build": L.build_budget(text.n)}[budget]
    for width in text.widths():
        direct, capped, final, counts, ann, geo = _run(hip, text, width, b)
        L.check_direct(direct, capped, text.exact(width), text.doc_off, width, b, geo)
        if b <= 0:                                        # (where the cuts are determined, so is the whole table)
            assert np.array_equal(direct, L.model_direct(text.exact(width), text.n, width, b, geo))
        _check_final(text, width, direct, final, counts, geo)
        if not capped:
            assert counts == (0, 0) and np.array_equal(direct, final)
        assert not np.any(ann == 0xEEEEEEEE)


@pytest.mark.parametrize("subset", ["1%", "50%", "all", "all_k0"])
@pytest.mark.parametrize("name", list(MODE_B) + ["ladder_u32", "ladder_residues", "run_one_letter_300", "run_period3_200",
                                                 "two_copies_200", "identical_strings_200", "documents_300_+63", "documents_200"])
def test_finishing_pass_on_given_tables(hip, name, subset):
    text = MODE_B[name] if name in MODE_B else CASES[name]
    fraction = {"1%": 0.01, "50%": 0.5}.get(subset, 1.0)
    for width in text.widths():
        table = L.partial_table(text, width, fraction, 77, zero=subset == "all_k0")
        direct, capped, final, counts, ann, geo = _run(hip, text, width, table=table)
        assert np.array_equal(direct[:text.n], table) and np.all(direct[text.n:] == L.NONE)
        assert capped == int(np.any(table & L.PARTIAL))
        _check_final(text, width, direct, final, counts, geo)
        if name == "random_300_long_list" and subset.startswith("all"):
            assert counts[0] > 4 * 8192                   # (more than one grid-stride round of the compare kernel)


@pytest.mark.parametrize("name", ["ladder_bytes_long_5", "run_one_letter_200", "documents_200"])
def test_nothing_depends_on_what_lies_behind_the_pad(hip, name):
    """The comparisons read far past the stream's end (the long kernel 8 192 bytes / 1 024 words past a position); what
    they find there -- the scope starts out as the fill byte -- decides nothing."""
    text = CASES[name]
    for width in text.widths():
        for b in (0, -1):
            a, z = _run(hip, text, width, b, fill=0x00), _run(hip, text, width, b, fill=0xFF)
            for x, y in zip(a, z):
                assert np.array_equal(x, y)
            _check_final(text, width, a[0], a[2], a[3], a[5])
        # the same with every rank handed to the finishing pass
        table = L.partial_table(text, width, 1.0, 5, zero=True)
        a, z = _run(hip, text, width, table=table, fill=0x01), _run(hip, text, width, table=table, fill=0xFF)
        for x, y in zip(a, z):
            assert np.array_equal(x, y)
        _check_final(text, width, a[0], a[2], a[3], a[5])


def test_rejections(hip):
    """Every argument check answers EAST_HIP_ERR_INVALID before anything is launched; the outputs stay untouched."""
    t = L.Text("two_documents", [[np.array([1, 2, 1, 2, 3]), np.array([2, 1])], [np.array([3, 3, 1])]])
    sa, off, m = t.sa(), t.doc_off, t.n_strings
    exact = t.exact(4)

    def run(width=4, stream=None, term_first=None, sa_=sa, off_=off, m_=m, budget=-1, table=None, fill=0, expect=ERR_INVALID):
        return _lcp(hip, width, t.stream(width) if stream is None else stream, t.term_first if term_first is None else term_first,
                    sa_, off_, m_, budget, table, fill, expect)
    assert run(expect=0) is not None and run(width=1, expect=0) is not None
    run(width=2)
    run(budget=-2)
    run(fill=256)
    run(off_=[1, 9, t.n]), run(off_=[0, 9, 9]), run(off_=[0, 9, t.n - 1]), run(off_=[0, 9, t.n + 1]), run(off_=[0, t.n, 9])
    swapped = sa.copy(); swapped[[8, 9]] = swapped[[9, 8]]           # a suffix of the other document
    run(sa_=swapped)
    twice = sa.copy(); twice[1] = twice[2]
    run(sa_=twice)
    beyond = sa.copy(); beyond[-1] = t.n
    run(sa_=beyond)
    run(off_=[0, 8, t.n])                                            # the first document then ends in text
    run(m_=[2, 2]), run(m_=[0, 1])
    for width in (1, 4):
        s = t.stream(width).copy(); s[0] = 0
        run(width=width, stream=s)
    s = t.codes.copy(); s[0] = t.term_first + t.n
    run(stream=s)
    s = t.codes.copy(); s[5], s[8] = s[8], s[5]                      # terminators out of order
    run(stream=s)
    s = t.codes.copy(); s[8] = s[5]                                  # a terminator twice
    run(stream=s)
    run(term_first=1), run(term_first=0x7FFFFFF0)
    # mode B
    assert run(table=exact, expect=0) is not None
    for r in (0, 9):
        bad = exact.astype(np.uint32); bad[r] = L.PARTIAL
        run(table=bad)
    r = 3
    room = t.n - int(max(sa[r], sa[r - 1]))
    ok = exact.astype(np.uint32); ok[r] = L.PARTIAL | min(room, int(exact[r]))
    assert run(table=ok, expect=0) is not None
    bad = exact.astype(np.uint32); bad[r] = L.PARTIAL | (room + 1)
    run(table=bad)
