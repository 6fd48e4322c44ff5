"""CPU tier: the oracle against the reference's own outputs on a differential fuzz.

The reference's tables and scores for 595 random small collections are stored in tests/golden/reference_fuzz.json.gz
(oracle/gen_golden.py records them from the imported reference); the oracle must reproduce every one of them."""
import gzip
import json
import os

import numpy as np

from conftest import GOLDEN

TABLES = ["suftab", "lcptab", "childtab_up", "childtab_down", "childtab_next_l_index", "anntab"]


def test_oracle_equals_reference_on_fuzz(oracle):
    with gzip.open(os.path.join(GOLDEN, "reference_fuzz.json.gz"), "rt", encoding="utf-8") as f:
        fuzz = json.load(f)
    assert fuzz["seed"] == 77 and fuzz["iters"] == 120
    n = 0
    for case in fuzz["cases"]:
        strings = case["strings"]
        orc = oracle.OracleEASA(strings)
        assert case["string"] == orc.symbols.tolist(), strings
        for name in TABLES:
            assert np.array_equal(np.asarray(case[name]), getattr(orc, name)), (name, strings)
        for rec in case["queries"]:
            q = rec["query"]
            qq = q.replace(" ", "")
            for i, norm in enumerate((True, False)):
                want = rec["score"][i]
                assert rec["linear"][i] == want, (strings, q, norm)          # the reference's ast_linear agrees with its easa
                suffix = {qq[j:]: v for j, v in enumerate(rec["suffix"][i])}
                for fast in (False, True):
                    o = orc.score(q, normalized=norm, return_suffix_scores=True, fast=fast)
                    assert want == o[0], (strings, q, norm, fast)
                    assert suffix == o[1], (strings, q, norm, fast)
        n += 1
    assert n == len(fuzz["cases"]) == 595
