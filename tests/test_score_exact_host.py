"""CPU tier: pin the exact model of the score walk (tests/score_exact.py) before anything on the device is compared with
it -- to the reference's recorded scores, to the oracle's two walks, and every generated case to what it is there for."""
import numpy as np
import pytest

import score_exact as sx
from conftest import load_golden


def _golden_cases():
    yield load_golden("readme_example.json")
    yield load_golden("test_base_case.json")
    for case in load_golden("fuzz_small.json")["cases"]:
        yield case


def test_model_equals_the_reference_fixtures():
    """Scores and per-suffix scores as the reference itself recorded them (oracle/gen_golden.py), bit for bit."""
    n = 0
    for case in _golden_cases():
        longest = max(len(q["query"]) for q in case["queries"])
        doc = sx.Document([[ord(c) for c in s] for s in case["strings"]], longest + 1)
        for q in case["queries"]:
            qs = [ord(c) for c in q["query"].replace(" ", "")]
            for mode, norm in (("normalized", True), ("denormalized", False)):
                total, suf = doc.score(qs, norm)
                assert total == q[mode], (case["strings"], q["query"], mode)
                assert suf == q["suffix_" + mode], (case["strings"], q["query"], mode)
            n += 1
    assert n >= 300


@pytest.mark.parametrize("fixture", ["sample_table.json", "hse_config1.json", "zipf_docs.json", "prose_like_docs.json"])
def test_model_equals_the_reference_table_fixtures(fixture):
    """The recorded keyphrase x text tables (scores only: these fixtures carry no per-suffix scores), through the product's
    text preparation, bit for bit."""
    from east import utils
    g = load_golden(fixture)
    kps = {kp: [ord(c) for c in utils.prepare_text(kp).replace(" ", "")] for kp in g["keyphrases"]}
    longest = max(len(q) for q in kps.values())
    for name, text in g["texts"].items():
        strings = utils.text_to_strings_collection(text.encode("utf-8"))
        doc = sx.Document([[ord(c) for c in s] for s in strings], longest + 1)
        for mode, norm in (("normalized", True), ("denormalized", False)):
            for kp, q in kps.items():
                assert doc.score(q, norm)[0] == g[mode][kp][name], (fixture, name, kp, mode)


def test_model_on_text_above_the_terminator_base():
    """high_text.json records ast_naive, the method as defined, for text at or above U+0A00 (where easa.py itself goes
    wrong).  ast_naive adds the same terms in another order, so the fixture is met to 1e-12 -- the oracle's own bound in
    test_oracle_golden.py -- and not bit for bit; the symbols need no renaming here: the model does not order them."""
    n = 0
    for case in load_golden("high_text.json")["cases"]:
        longest = max(len(q["query"]) for q in case["queries"])
        doc = sx.Document([[ord(c) for c in s] for s in case["strings"]], longest + 1)
        for q in case["queries"]:
            qs = [ord(c) for c in q["query"].replace(" ", "")]
            for mode, norm in (("normalized", True), ("denormalized", False)):
                total, suf = doc.score(qs, norm)
                assert abs(total - q[mode]) <= 1e-12, (case["strings"], q["query"], mode)
                assert np.allclose(suf, q["suffix_" + mode], rtol=0, atol=1e-12)
            n += 1
    assert n >= 150


def _assert_equal(got, want, what):
    if not np.array_equal(got, want):
        at = tuple(np.argwhere(got != want)[0])
        raise AssertionError("%s differs at %s: %r, want %r" % (what, at, got[at], want[at]))


@pytest.mark.parametrize("case", sx.small_cases(), ids=repr)
def test_model_equals_the_oracle(oracle, case):
    """Whole tables and whole per-suffix arrays, both normalizations: the model against the oracle's faithful port of the
    reference walk, against its interval walk, and against the batched interval walk."""
    sym, off, ms, rename = case.oracle_input()
    kps = case.keyphrases()
    renamed = [np.array(rename(q), dtype=np.uint32) for q in kps]
    qs, qo = sx.pack(renamed)
    asts = [oracle.OracleEASA(symbols=sym[off[d]:off[d + 1]], n_strings=int(ms[d])) for d in range(ms.size)]
    sa = np.concatenate([a.suftab for a in asts])
    for norm in (True, False):
        table, suf = case.tables(norm)
        assert table.shape == (len(kps), ms.size) and suf.shape == (ms.size, qo[-1])
        want, want_suf = oracle.score_table_fast(sym, off, ms, sa, qs, qo, norm, want_suffix=True)
        _assert_equal(table, want, "%s: table (%s)" % (case, norm))
        _assert_equal(suf, want_suf, "%s: per-suffix results (%s)" % (case, norm))
        for fast in (False, True):
            for d, ast in enumerate(asts):
                for k, q in enumerate(renamed):
                    total, s = ast.score_symbols(q, norm, fast=fast, want_suffix=True)
                    assert total == table[k, d] and np.array_equal(s, suf[d, qo[k]:qo[k + 1]]), (case, d, kps[k], norm, fast)


def _assert_facts(case):
    for plan in case.plans:
        facts = case.facts(*plan)
        for name, want in case.expected(plan).items():
            got = facts[name]
            ok = got >= want if not isinstance(want, bool) else got == want
            assert ok, "%s, tables of depth %d%s: %s is %r, wanted %r" % (case, plan[0], " (pairs)" if plan[1] else "", name,
                                                                        got, want)


@pytest.mark.parametrize("case", sx.small_cases(), ids=repr)
def test_small_case_shows_what_it_is_for(case):
    _assert_facts(case)
    n = sum(len(s) + 1 for doc in case.docs for s in doc)
    assert n <= 65536                                    # (the score side builds the tables itself)
    if case.marked:
        assert case.plans == [(sx.marked_k(case.sigma_t, n, len(case.docs)), False), (sx.marked_k(case.sigma_t, n, len(case.docs)), True)]
    else:
        assert case.plans == [(sx.small_k(case.sigma_t, n, len(case.docs)), False)]


def test_alphabets_and_table_rows_of_the_small_cases():
    """sigma_t in {1, 2, 3, 4, 6, 14}: A = 3 .. 16, k = 3, 3, 3, 3, 2, 2, rows of 27, 64, 125, 216, 64, 256 entries -- on
    both sides of a wavefront and of a workgroup for the fill kernel."""
    mixed = [c for c in sx.small_cases() if c.name.startswith("mixed_sigma")]
    assert [c.sigma_t for c in mixed] == [1, 2, 3, 4, 6, 14]
    assert [c.A ** c.plans[0][0] for c in mixed] == [27, 64, 125, 216, 64, 256]
    by_name = {c.name: c for c in sx.small_cases()}
    assert len(by_name["random_alone"].docs) == 1 and len(by_name["seventy_documents"].docs) == 70
    n = sum(len(s) + 1 for s in by_name["search_kernel"].docs[0])
    assert n >= 256 * by_name["search_kernel"].A ** 3             # (score_host.h: the table entries by binary search)
    assert by_name["u32_symbols"].sigma_t > 254
    assert sorted(doc_n for doc_n in (sum(len(s) + 1 for s in doc) for doc in sx.tiny_documents([2, 3]))) == [2, 3, 4, 4, 5]


def test_packing_case_packs_as_meant():
    """Consecutive keyphrases that sum to 255, 256 and 257 suffixes, one of exactly 256, a last one of 1; with the
    keyphrase of 257 the sums cannot run inside the walk."""
    case = [c for c in sx.small_cases() if c.name == "packing"][0]
    lengths = [len(q) for q in case.keyphrases()]
    blocks = sx.packing_blocks(lengths)
    assert blocks == [255, 256, 200, 57, 256, 256, 1 + 254, 2, 255 + 1], blocks
    assert max(lengths) == sx.PACK_BLOCK and lengths[-1] == 1
    long_lengths = [len(q) for q in case.with_long]
    assert sx.packing_blocks(long_lengths) is None and max(long_lengths) == sx.PACK_BLOCK + 1 and long_lengths[-1] == 1


@pytest.mark.parametrize("which", ["pairs", "pairs_runs", "chunks"])
def test_marked_case_shows_what_it_is_for(which):
    case = sx.marked_cases()[which]
    n = sum(len(s) + 1 for doc in case.docs for s in doc)
    assert n > 65536
    assert case.plans[0][0] == sx.marked_k(case.sigma_t, n, len(case.docs)) == 4 and case.A == 8
    assert (sx.small_k(case.sigma_t, n, len(case.docs)), False) in case.plans      # (behind DC3: the score side's own tables)
    if which == "chunks":
        assert (4, True) in case.plans                   # (score path 4 forces the pair layout on it)
    _assert_facts(case)


@pytest.mark.parametrize("which", ["chunks_274", "bins_limit"])
def test_large_case_shows_what_it_is_for(which):
    case = sx.large_case(which)
    n = sum(len(s) + 1 for doc in case.docs for s in doc)
    k = sx.marked_k(case.sigma_t, n, 1)
    bins = case.A ** k
    if which == "chunks_274":
        assert (case.A, k, bins, -(-bins // 1024)) == (23, 4, 279841, 274)
    else:
        assert (case.A, k, bins) == (32, 4, 1048576)                 # KGRAM_KEYS_MAX_BINS exactly
        assert case.A + 1 + case.A ** 2 + 1 == 1058 > 1024              # the upper tables do not fit KG_UP_LDS_WORDS
    assert len(case.keyphrases()) > 20000
    _assert_facts(case)
