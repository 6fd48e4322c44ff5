"""gpu tier: long repeats in text of more than 254 symbols, through whole builds.  Such text is held as dense u32 codes:
DC3 sorts it (to the bottom of its recursion on a run), lcp_kernel compares neighbours and cuts, the `<false>`
instantiations of the finishing pass complete the table, the score walk ends its matches on u32 codes, and the arena has
to hold the finishing pass behind a wide build.  An article that appears twice in a Chinese or Korean collection takes
this path.

The texts are those of tests/lcp_exact.py (shown on the CPU to reach what they claim by tests/test_lcp_exact_host.py),
spelled in 300 letters below U+0A00 or, tagged, in 300 code points from U+4E00 and U+AC00.  The eight sort paths of
tests/test_gpu_parity.py do not apply: more than 254 symbols always takes DC3.
"""
import numpy as np
import pytest

import lcp_exact as L
from test_gpu_parity import _check_index, _repeat_keyphrases

pytestmark = pytest.mark.gpu

LOW = np.arange(0x0100, 0x0100 + 300, dtype=np.uint32)
HIGH = np.concatenate([np.arange(0x4E00, 0x4E00 + 150), np.arange(0xAC00, 0xAC00 + 150)]).astype(np.uint32)
CASES = {t.what: t for t in L.cases()}
KERNELS = ("lcp_kernel", "lcp_phi_classify_kernel<false>", "lcp_phi_compare_kernel<false>", "lcp_phi_long_kernel<false>",
           "lcp_phi_fill_kernel")


def _shard():
    """Identical and near-identical strings of 18 000 symbols; a one-letter run behind fillers; short ordinary text."""
    rng = np.random.default_rng(60)
    s = rng.integers(1, 301, size=18000)
    near = s.copy()
    near[12345] = near[12345] % 300 + 1
    run = np.concatenate([np.arange(1, 301), np.full(8000, 17)])
    words = [rng.integers(1, 301, size=int(rng.integers(1, 12))) for _ in range(40)]
    return L.Text("shard_of_three", [[s, s, near], [run], words])


def _texts():
    return [CASES["run_one_letter_300"], CASES["run_period3_300"], CASES["two_copies_300"], CASES["ladder_u32"], _shard()]


def _tagged_text():
    rng = np.random.default_rng(61)
    body = rng.integers(1, 301, size=12000)
    return L.Text("two_copies_and_a_run", [[np.concatenate([np.arange(1, 301), [1], body, [2], body, np.full(17000, 150)])]])


def _check_build(hip, oracle, text, letters, tagged):
    index = hip.HipIndex()
    index.profile_enable()
    sym = text.symbols(letters, tagged=tagged)
    low = text.symbols(LOW)                                  # what the oracle reads: the same text below U+0A00
    off, ms = text.doc_off, text.n_strings
    index.build(sym, off, ms)
    info = index.info()
    assert info["sigma_text"] == 300 and info["sigma_text"] > 254 and info["window_sorted"] == 0 and info["dc3_levels"] >= 1
    report = index.profile_report()
    for kernel in KERNELS:
        assert report.get(kernel, (0, 0.0))[0] >= 1, (kernel, sorted(report))
    assert not any(k.startswith("lcp8_kernel") or k.endswith("<true>") for k in report if k.startswith("lcp")), sorted(report)
    index.profile_enable(False)
    # the table itself against the witness, then all six tables and the lefts in full, and the keyphrases
    exact = text.exact(4)
    for d in range(len(ms)):
        assert np.array_equal(index.tables(d, names=("lcptab",))["lcptab"], exact[off[d]:off[d + 1]]), d
    body = sym[:off[1]]
    body = body[(body >> 31) == 0] if tagged else body[body < 0x0A00]
    qs, qo = _repeat_keyphrases(body)
    assert qo.size - 1 >= 45
    qs_low = np.where(np.isin(qs, letters), LOW[np.minimum(np.searchsorted(letters, qs), 299)], qs).astype(np.uint32)
    assert not np.isin(0x05D0, letters) and not np.isin(0x05D0, LOW)
    tables = {norm: index.score_table(qs, qo, norm, want_suffix=True) for norm in (True, False)}
    assert (tables[True][0][:, 0] > 0).any()
    _check_index(oracle, index, low, off, ms, scores=(qs_low, qo, tables))
    # other text on the same handle
    rng = np.random.default_rng(62)
    other = L.Text("other", [[rng.integers(1, 281, size=int(rng.integers(1, 40))) for _ in range(5)], [np.arange(1, 281)]])
    index.build(other.symbols(letters, tagged=tagged), other.doc_off, other.n_strings)
    assert index.info()["sigma_text"] == 280
    for d in range(2):
        a, b = int(other.doc_off[d]), int(other.doc_off[d + 1])
        o = oracle.OracleEASA(symbols=other.symbols(LOW)[a:b], n_strings=int(other.n_strings[d]))
        t = index.tables(d)
        for name in ("suftab", "lcptab", "anntab", "childtab_up", "childtab_down", "childtab_next_l_index"):
            assert np.array_equal(t[name], getattr(o, name)), (name, d)


@pytest.mark.parametrize("text", _texts(), ids=lambda t: t.what)
def test_wide_alphabet_repeats_below_the_terminator_base(hip, oracle, text):
    _check_build(hip, oracle, text, LOW, False)


def test_wide_alphabet_repeats_in_han_and_hangul(hip, oracle):
    _check_build(hip, oracle, _tagged_text(), HIGH, True)
