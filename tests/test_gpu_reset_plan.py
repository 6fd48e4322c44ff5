"""gpu tier: what east_hip_reset forgets of the build's plan (csrc/handle.h, csrc/build.h: next_plan).

One handle builds two word-stream documents of 120 000 symbols one after the other, is reset, and builds two more.  The
second build is speculative and counts its first radix histogram in the remap pass, from the first-pass plan the first
build left (tests/test_gpu_first_pass_hist.py establishes that for this shape).  The reset keeps the build hints -- the
third build is speculative as well -- but forgets the plan, the first-pass plan with it, and without one build_impl does
not launch the fused kernel.  What the fourth build does depends on what the window sort plans without a sample: not
asserted.  All six tables of all four builds equal the oracle's.
"""
import numpy as np
import pytest

from test_gpu_first_pass_hist import TABLES

pytestmark = pytest.mark.gpu


def test_reset_forgets_the_first_pass_plan_and_keeps_the_tables_right(hip, oracle):
    from east import synthetic
    rng = np.random.default_rng(2024)
    docs = [synthetic.word_stream_document(rng, 120000, want_text=False)[1:] for _ in range(4)]
    lib = hip.load()
    index = hip.HipIndex()
    fused = []
    try:
        for i, (sym, m) in enumerate(docs):
            if i == 2:
                assert lib.east_hip_reset(index._h) == 0
            index.build(sym, np.array([0, sym.size], dtype=np.int64), np.array([m], dtype=np.int32))
            fused.append(index.info()["first_hist_fused"])
            t = index.tables(0)
            o = oracle.OracleEASA(symbols=sym, n_strings=m)
            for name in TABLES:
                assert np.array_equal(t[name], getattr(o, name)), (i, name)
    finally:
        index.close()
    print("first_hist_fused per build:", fused)
    assert fused[0] == 0 and fused[1] == 1, fused
    assert fused[2] == 0, fused
