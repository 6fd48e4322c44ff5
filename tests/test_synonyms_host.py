# -*- coding: utf-8 -*-
"""CPU tier of synonym extraction: the exact host model (tests/synonyms_exact.py) against the reference's recorded results
(tests/golden/synonyms.json, tools/gen_synonyms_golden.py), and the host half of east.synonyms -- the two file formats,
interning, the candidate filter, the command line's refusals, the binding.  Nothing here needs a device."""
import io
import itertools
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import synonyms_exact
from conftest import ROOT, load_golden

GOLDEN = load_golden("synonyms.json")["cases"]
CASES = {c["name"]: c for c in GOLDEN}


def case_triples(case):
    """The raw triples of a fixture case (the XML case through the product's own reader)."""
    if "xml" in case:
        from east.synonyms import synonyms
        return synonyms.parse_tomita_xml(case["xml"].encode("utf-8"))
    return [tuple(t) for t in case["triples"]]


def case_similarities(case):
    """[(a, b, similarity)] of every pair of candidates: the fixture holds the values in combinations order."""
    pairs = list(itertools.combinations(case["candidates"], 2))
    assert len(pairs) == len(case["similarity"])
    return [(a, b, s) for (a, b), s in zip(pairs, case["similarity"])]


def test_the_fixture_holds_the_cases_it_was_made_for():
    assert len(GOLDEN) >= 12
    names = set(CASES)
    assert {"zipf_36_words", "zipf_50_words", "multiplicities_1_2_5", "relations_with_of", "self_pairs", "identical_rows", "no_positive_feature",
            "length_filter", "non_ascii", "tomita_xml"} <= names
    assert {"frequency_filter_%d_texts" % n for n in (1, 49, 50, 120)} <= names
    assert all(len(c["words"]) <= 60 for c in GOLDEN)
    for c in GOLDEN:                                    # the margin the generator asserts, checked again on what it wrote
        assert all(abs(s - 0.3) > 1e-9 and (s == 0.0 or s > 1e-9) for s in c["similarity"]), c["name"]
    c = CASES["no_positive_feature"]
    assert [w for w in c["words"] if not any(i[0] == w for i in c["I"])]
    assert "OX" in CASES["length_filter"]["words"] and "OX" not in CASES["length_filter"]["candidates"]
    for n in (1, 49, 50, 120):
        c = CASES["frequency_filter_%d_texts" % n]
        assert c["number_of_texts"] == n and "DOG" in c["words"] and "DOG" not in c["candidates"] and "CAT" in c["candidates"]
    c = CASES["identical_rows"]
    assert [s for a, b, s in case_similarities(c) if (a, b) == ("TWINA", "TWINB")] == [1.0]
    assert any(t[0] == t[2] for t in CASES["self_pairs"]["triples"])
    rels = set(t[1] for t in CASES["relations_with_of"]["triples"])
    assert {"ruler", "ruler_of"} <= rels
    assert any(ord(ch) > 127 for w in CASES["non_ascii"]["words"] for ch in w)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_model_against_the_reference(case):
    """Words, relations, the set of positive features (decided by q, exactly), I and every candidate pair's similarity to
    1e-12, the synonym sets at 0.3 and 0.0 equal."""
    from east import utils
    model = synonyms_exact.Model(case_triples(case))
    assert model.words == case["words"]
    assert model.relations == case["relations"]
    got_I = sorted([w, r, w2, float(v)] for w in model.words for (r, w2), v in model.rows[w])
    assert [i[:3] for i in got_I] == [i[:3] for i in case["I"]]
    worst = max([abs(a[3] - b[3]) for a, b in zip(got_I, case["I"])] or [0.0])
    assert worst <= synonyms_exact.ABS_TOL, worst
    freq = {}
    for tok in utils.tokenize(utils.prepare_text(case["text"])):
        freq[tok] = freq.get(tok, 0) + 1
    candidates = synonyms_exact.candidate_words(model.words, freq, case["number_of_texts"])
    assert candidates == case["candidates"]
    want = {(a, b): s for a, b, s in case_similarities(case)}
    assert len(want) == len(candidates) * (len(candidates) - 1) // 2
    for i, a in enumerate(candidates):
        for b in candidates[i + 1:]:
            assert abs(model.similarity(a, b) - want[(a, b)]) <= synonyms_exact.ABS_TOL, (a, b)
    for key, threshold in (("synonyms_0.3", 0.3), ("synonyms_0.0", 0.0)):
        got = synonyms_exact.synonyms_of(model.pairs(candidates, threshold))
        assert {w: sorted(v) for w, v in got.items()} == case[key]
    assert sorted(model.sharing_pairs(candidates)) == sorted((a, b) for a, b, s in case_similarities(case) if s > 0.0)


def test_marginals_are_sums_of_squares():
    """A triple that occurs f times counts f times f (synonyms.py:129-131 sum the frequency over a list with one entry per
    occurrence), and F_rw2(r, w2) == F_w1r(w2, r')."""
    model = synonyms_exact.Model([("A", "r", "B")] * 5 + [("A", "r", "C")] * 2 + [("D", "r", "B")])
    assert model.f[("A", "r", "B")] == 5 and model.f[("B", "r_of", "A")] == 5
    assert model.F_w1r[("A", "r")] == 25 + 4 and model.F_rw2[("r", "B")] == 25 + 1 and model.F_r["r"] == 30
    for (r, w2), v in model.F_rw2.items():
        assert model.F_w1r[(w2, synonyms_exact.inverse_relation(r))] == v
    assert model.q[("A", "r", "B")] == 5.0 * 30 / 29 / 26


# ---- the host half of east.synonyms -------------------------------------------------------------------------------------
def test_interning_and_the_inverse_relation_table():
    from east.synonyms import synonyms
    triples = [("B", "mod", "A"), ("C", "obj_of", "A"), ("A", "_of", "C"), ("Я", "mod", "B")]
    words, relations, w1, rel, w2, inverse = synonyms.intern_triples(triples)
    assert words == ["A", "B", "C", "Я"]                               # code-point order
    assert relations == ["", "_of", "mod", "mod_of", "obj", "obj_of"]   # every inverse is there
    assert [relations[i] for i in inverse] == ["_of", "", "mod_of", "mod", "obj_of", "obj"]
    assert inverse[inverse].tolist() == list(range(len(relations)))     # an involution
    assert [(words[a], relations[r], words[b]) for a, r, b in zip(w1, rel, w2)] == triples
    assert all(x.dtype == np.int32 for x in (w1, rel, w2, inverse))
    for r in ("x", "x_of", "_of", "", "of"):
        assert synonyms.inverse_relation(synonyms.inverse_relation(r)) == r
    # the one kind of name on which synonyms.py:81 is no involution (a_of_of -> a_of -> a): refused, not miscounted
    from east import exceptions
    with pytest.raises(exceptions.EastException) as e:
        synonyms.intern_triples([("A", "a_of_of", "B")])
    assert "a_of_of" in str(e.value)
    model = synonyms_exact.Model(triples)
    assert model.words == words and model.relations == relations


def test_candidate_filter_floors_the_division():
    from east.synonyms import synonyms
    freq = {"ONE": 1, "TWO": 2, "THREE": 3, "AB": 9, "ZERO": 0}
    words = ["ONE", "TWO", "THREE", "AB", "ZERO", "ABSENT"]
    assert synonyms.candidate_words(words, freq, 1) == ["ONE", "THREE", "TWO"]
    assert synonyms.candidate_words(words, freq, 49) == ["ONE", "THREE", "TWO"]          # 49 // 50 == 0
    assert synonyms.candidate_words(words, freq, 50) == ["THREE", "TWO"]
    assert synonyms.candidate_words(words, freq, 99) == ["THREE", "TWO"]                 # 99 // 50 == 1, not 1.98
    assert synonyms.candidate_words(words, freq, 120) == ["THREE"]
    assert synonyms.candidate_words(words, freq, 150) == []
    assert synonyms.candidate_words(words, freq, 1) == synonyms_exact.candidate_words(words, freq, 1)


def test_the_two_file_formats_and_their_errors(tmp_path):
    from east import exceptions
    from east.synonyms import synonyms
    case = CASES["tomita_xml"]
    xml = tmp_path / "triples.xml"
    xml.write_bytes(("\n  " + case["xml"].split("?>", 1)[1]).encode("utf-8"))     # leading white space, no declaration
    triples = synonyms.read_triples(str(xml))
    assert ("SEE", "dobj", "RED CHERRY") in triples                    # split at the FIRST space (synonyms.py:72)
    assert ("TREE", "nsubj_of", "GROW") in triples and len(triples) == 15
    tsv = tmp_path / "triples.tsv"
    tsv.write_bytes("".join("%s\t%s\t%s\r\n" % t for t in triples).encode("utf-8") + "\n".encode("utf-8") + "КОТ\tmod\tЯ\n".encode("utf-8"))
    assert synonyms.read_triples(str(tsv)) == triples + [("КОТ", "mod", "Я")]
    bad = tmp_path / "bad.tsv"
    bad.write_text("A\tr\tB\n\nA\tr\n", encoding="utf-8")
    with pytest.raises(exceptions.EastException) as e:
        synonyms.read_triples(str(bad))
    assert "line 3" in str(e.value)
    bad.write_text("A\tr\tB\tC\n", encoding="utf-8")
    with pytest.raises(exceptions.EastException) as e:
        synonyms.read_triples(str(bad))
    assert "line 1" in str(e.value)
    bad.write_text("A\t\tB\n", encoding="utf-8")
    with pytest.raises(exceptions.EastException):
        synonyms.read_triples(str(bad))
    bad.write_text("<a><Relation><mod/></Relation></a>", encoding="utf-8")
    with pytest.raises(exceptions.EastException):
        synonyms.read_triples(str(bad))
    bad.write_text("<a><Relation>", encoding="utf-8")
    with pytest.raises(exceptions.EastException):
        synonyms.read_triples(str(bad))


def test_extractor_host_attributes(tmp_path):
    """words, relations, word_frequencies, number_of_texts as the reference's; no device is touched by the constructor."""
    from east import exceptions, synonyms
    case = CASES["frequency_filter_120_texts"]
    d = tmp_path / "texts"
    d.mkdir()
    for i in range(120):
        (d / ("t%03d.txt" % i)).write_text(case["text"] if i == 7 else "", encoding="utf-8")
    (d / "notes.md").write_text("DOG DOG DOG", encoding="utf-8")
    ex = synonyms.SynonymExtractor(str(d), triples=[tuple(t) for t in case["triples"]])
    assert ex.number_of_texts == 120
    assert sorted(ex.words) == case["words"] and sorted(ex.relations) == case["relations"]
    assert ex.word_frequencies["DOG"] == 2 and ex.word_frequencies["CAT"] == 3
    from east.synonyms.synonyms import candidate_words
    assert candidate_words(ex.words, ex.word_frequencies, ex.number_of_texts) == case["candidates"]
    single = synonyms.SynonymExtractor(str(d / "t007.txt"), triples=iter([("CAT", "subj", "RUN")]))
    assert single.number_of_texts == 1 and single.words == {"CAT", "RUN"} and single.relations == {"subj", "subj_of"}
    same = synonyms.SynonymExtractor.from_texts([case["text"].encode("utf-8"), "", ""], [tuple(t) for t in case["triples"]])
    assert same.number_of_texts == 3 and dict(same.word_frequencies) == dict(ex.word_frequencies)
    with pytest.raises(exceptions.TomitaNotInstalledException):
        synonyms.SynonymExtractor(str(d))
    with pytest.raises(exceptions.TomitaNotInstalledException):
        synonyms.SynonymExtractor.from_texts(["x"], None)
    with pytest.raises(exceptions.EastException):
        synonyms.SynonymExtractor.from_texts(["x"], [("A", "r")])
    empty = synonyms.SynonymExtractor.from_texts(["x"], [])
    assert empty.get_synonyms() == {} and empty.similarity("A", "B") == 0.0 and empty.T("A") == set() and empty.I("A", "r", "B") == 0.0


def test_no_cpu_fallback_for_the_compute_calls():
    from east import exceptions, hip_backend, synonyms
    if hip_backend.device_count() > 0:
        pytest.skip("a HIP device is present")
    case = CASES["identical_rows"]
    ex = synonyms.SynonymExtractor.from_texts([case["text"]], [tuple(t) for t in case["triples"]])
    for call in (lambda: ex.get_synonyms(), lambda: ex.similarity("TWINA", "TWINB"), lambda: ex.T("TWINA"),
                 lambda: ex.I("TWINA", "mod", "TALL")):
        with pytest.raises(exceptions.HipBackendError):
            call()


# ---- the command line ---------------------------------------------------------------------------------------------------
def _east(argv, env=None, monkeypatch=None):
    from east import main
    if monkeypatch is not None:
        for var in ("WORLD_SIZE", "RANK", "EAST_HIP_DEVICES", "EAST_HIP_FORCE_DIST", "EAST_HIP_MULTI"):
            monkeypatch.delenv(var, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main.main(argv)
    return rc, out.getvalue()


@pytest.fixture()
def cli_files(tmp_path):
    (tmp_path / "kp.txt").write_text("red apple\n", encoding="utf-8")
    d = tmp_path / "texts"
    d.mkdir()
    (d / "a.txt").write_text("red apple sweet cherry", encoding="utf-8")
    (d / "b.txt").write_text("sour plum", encoding="utf-8")
    (tmp_path / "triples.tsv").write_text("RED\tamod\tAPPLE\nSWEET\tamod\tAPPLE\n", encoding="utf-8")
    return tmp_path


def test_cli_refusals(cli_files, monkeypatch):
    from east import hip_backend
    kp, texts, triples = str(cli_files / "kp.txt"), str(cli_files / "texts"), str(cli_files / "triples.tsv")
    tail = ["keyphrases", "table", kp, texts]
    touched = []

    def no_device(*args, **kwargs):
        touched.append(args)
        raise AssertionError("a refused command line reached the device")
    monkeypatch.setattr(hip_backend, "HipIndex", no_device)
    # -y alone: the line it has always printed
    rc, out = _east(["-y"] + tail, monkeypatch=monkeypatch)
    assert rc == 1 and out == "Synonym extraction (-y) needs the external Tomita parser and is not available.\n"
    rc, out = _east(["-t", triples] + tail, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "-y" in out
    rc, out = _east(["-y", "-t", triples, "-g", "2"] + tail, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "one device" in out and "-g 2" in out
    rc, out = _east(["-y", "-t", triples] + tail, env={"EAST_HIP_DEVICES": "4"}, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "one device" in out
    rc, out = _east(["-y", "-t", triples] + tail, env={"WORLD_SIZE": "2", "RANK": "0"}, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "WORLD_SIZE=2" in out
    rc, out = _east(["-y", "-t", triples] + tail, env={"WORLD_SIZE": "2", "RANK": "1"}, monkeypatch=monkeypatch)
    assert rc == 1 and out == ""
    rc, out = _east(["-y", "-t", triples] + tail, env={"EAST_HIP_FORCE_DIST": "1"}, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "collective" in out
    # a triples file that cannot be read ends with one line too
    (cli_files / "bad.tsv").write_text("RED\tamod\n", encoding="utf-8")
    rc, out = _east(["-y", "-t", str(cli_files / "bad.tsv")] + tail, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1 and "line 1" in out
    rc, out = _east(["-y", "-t", str(cli_files / "missing.tsv")] + tail, monkeypatch=monkeypatch)
    assert rc == 1 and out.count("\n") == 1
    assert touched == []
    from east import main
    assert "-y -t" in main.__doc__


def test_binding_against_the_header():
    """Every synonyms entry point is declared in the header with the arguments the binding passes."""
    import ctypes
    from east import hip_backend
    with open(os.path.join(ROOT, "include", "east_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = ["east_hip_synonyms_build", "east_hip_synonyms_info", "east_hip_synonyms_get_rows", "east_hip_synonyms_similarity",
             "east_hip_synonyms_pairs", "east_hip_synonyms_fetch", "east_hip_last_synonyms_ms", "east_hip_debug_set_synonyms_chunk"]
    ctype_of = {"east_hip_handle_t": ctypes.c_void_p, "int32_t *": hip_backend._c_i32p,
                "int64_t *": hip_backend._c_i64p, "double *": hip_backend._c_dblp, "int64_t": ctypes.c_int64,
                "int32_t": ctypes.c_int32, "double": ctypes.c_double, "int": ctypes.c_int}
    for name in names:
        m = re.search(r"\b(int|double)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = hip_backend.SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "double": ctypes.c_double}[m.group(1)]
        declared = []
        for a in m.group(2).split(","):
            kind = re.match(r"^(.*?)\w+$", " ".join(a.split())).group(1).replace("const ", "").strip()
            declared.append(ctype_of[kind])
        assert declared == list(args), name
    if not os.path.exists(hip_backend.LIB_PATH):      # a fresh checkout: hipcc cross-compiles without a GPU
        import __graft_entry__
        __graft_entry__.build()
    lib = hip_backend.load()
    assert lib.east_hip_debug_set_synonyms_chunk(0) == 0
    assert lib.east_hip_last_synonyms_ms(None) == -1.0
    assert lib.east_hip_synonyms_info(None, None, 0) < 0


# ---- the model on id arrays (tests/test_gpu_synonyms_scale.py's yardstick) ------------------------------------------------
def _close(got, want, rel=1e-15):
    return abs(float(got) - float(want)) <= rel * abs(float(want))


def _array_model_against_the_decimal_model(triples, candidates=None):
    from east.synonyms import synonyms
    model = synonyms_exact.Model(triples)
    words, relations, w1, rel, w2, inverse = synonyms.intern_triples(triples)
    assert words == model.words and relations == model.relations
    am = synonyms_exact.array_model(w1, rel, w2, inverse, len(words))
    assert am.info() == {"raw_triples": len(triples), "distinct_triples": len(model.f), "words": len(words), "relations": len(relations),
                         "features": sum(len(r) for r in model.rows.values()), "longest_row": max(len(r) for r in model.rows.values())}
    # every distinct triple: f and q bit-equal, in the key's order
    names = [(words[a], relations[r], words[b]) for a, r, b in zip(am.w1.tolist(), am.rel.tolist(), am.w2.tolist())]
    assert names == sorted(model.f, key=lambda t: (words.index(t[0]), relations.index(t[1]), words.index(t[2])))
    assert am.f.tolist() == [model.f[t] for t in names]
    assert am.q.tolist() == [model.q[t] for t in names]
    # the same kept features in the same order, I and the row sums
    offsets = am.offsets()
    sums = am.sums()
    for i, w in enumerate(words):
        b, e = int(offsets[i]), int(offsets[i + 1])
        assert [(relations[r], words[x]) for r, x in zip(am.relation[b:e].tolist(), am.word[b:e].tolist())] == [k for k, _ in model.rows[w]]
        assert all(_close(v, d) for v, (_, d) in zip(am.I[b:e], model.rows[w]))
        assert _close(sums[i], model.row_sum[w])
    # every candidate pair
    cand = words if candidates is None else candidates
    ids = [words.index(w) for w in cand]
    a, b, sim, shared, n_a, n_b = synonyms_exact.pairs_model(am, ids)
    want = model.pairs(cand, 0.0)
    assert [(words[x], words[y]) for x, y in zip(a.tolist(), b.tolist())] == [(x, y) for x, y, _ in want]
    assert all(_close(s, t[2]) for s, t in zip(sim.tolist(), want))
    assert shared.tolist() == [len(model.shared(x, y)) for x, y, _ in want]
    assert n_a.tolist() == [len(model.rows[x]) for x, _, _ in want] and n_b.tolist() == [len(model.rows[y]) for _, y, _ in want]
    pa = [ids[i] for i in range(len(ids)) for _ in ids[i + 1:]]
    pb = [y for i in range(len(ids)) for y in ids[i + 1:]]
    looked_up = synonyms_exact.similarity_model(am, pa, pb)[0]
    got = {(x, y): s for x, y, s in zip(a.tolist(), b.tolist(), sim.tolist())}
    assert all(_close(s, got.get((x, y), 0.0)) for s, x, y in zip(looked_up.tolist(), pa, pb))     # (another order of the wide sum)
    return am


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_array_model_against_the_decimal_model(case):
    _array_model_against_the_decimal_model(case_triples(case), case["candidates"])


def test_array_model_against_the_decimal_model_on_zipf_triples():
    am = _array_model_against_the_decimal_model(synonyms_exact.zipf_triples(seed=77, n_words=300, n_relations=6, n_triples=3000))
    assert am.info()["features"] > 1000


def _crossed(model, multiple):
    """The multiples of `multiple`, in distinct-triple order, that a group (w1, r) lies across."""
    at = np.arange(multiple, model.key.size, multiple)
    return at[model.gid[at - 1] == model.gid[at]]


def test_the_scale_case_holds_what_it_is_for():
    (w1, rel, w2, inverse, W), m = synonyms_exact.scale_case()
    assert W == 40000 and inverse.size == 64 and np.flatnonzero(inverse == np.arange(64)).tolist() == list(synonyms_exact.SCALE_SELF_INVERSE)
    assert 480000 < w1.size < 500000
    D = m.key.size
    assert D > 524288                                                   # the marginals kernel's loop takes a second turn
    group_sizes = np.bincount(m.gid)
    assert (group_sizes > 64).any() and (group_sizes > 256).any()
    assert _crossed(m, 64).size and _crossed(m, 256).size and _crossed(m, 524288).tolist() == [524288]
    assert int(m.f.max()) ** 2 > 2 ** 32 and int(m.F_r.max()) > 2 ** 32 and int(m.F_w1r.max()) > 2 ** 32
    assert int(m.f.max()) ** 2 < 2 ** 53                                # (what stays untested: integers a double cannot hold)
    for r in synonyms_exact.SCALE_SELF_INVERSE:                         # self-inverse relations in use, kept features among them
        assert (m.relation == r).sum() > 1000
    ones = m.q == 1.0
    assert ones.sum() == 2 * sum(na * nb for _, na, nb in synonyms_exact.SCALE_BLOCKS) and not m.keep[ones].any()
    assert sorted(set(m.rel[ones].tolist())) == [56, 57, 58, 59]
    assert np.unique(m.rel).size == 64                                  # every LDS relation counter of the 64
    assert m.w1.max() == W - 1 or m.w1.max() >= 1 << 15                 # ids in the sort's highest bit


def test_the_top_case_holds_what_it_is_for():
    for n_words in (1 << 26, (1 << 25) + 3):
        w1, rel, w2, inverse, W = synonyms_exact.top_case(n_words)
        assert W == n_words and inverse.size == 4096 and 200 <= w1.size <= 400
        m = synonyms_exact.array_model(w1, rel, w2, inverse, W)
        top, half = n_words - 1, 1 << 25
        assert {0, 1, 2, half - 1, half, top - 1, top} <= set(m.row.tolist()) and {0, half - 1, half, top - 1, top} <= set(m.word.tolist())
        assert set(m.relation.tolist()) == {0, 1, 2047, 2048, 4094, 4095}
        assert ((m.row == top) & (m.relation == 4095) & (m.word >= top - 1)).any()      # every field at its top in one key
        assert m.info()["features"] > 50 and (~m.keep).sum() > 10
        # what a relation mask one bit short would do is visible: 2048 and 0, 4095 and 2047 have different marginals
        assert m.F_r[2048] != m.F_r[0] and m.F_r[4095] != m.F_r[2047] and m.F_r[4094] != m.F_r[2046]
    assert (1 << 25) + 2 < (1 << 26) and ((1 << 25) + 2).bit_length() == ((1 << 26) - 1).bit_length()    # the same sort width


@pytest.mark.parametrize("W", synonyms_exact.WORD_COUNTS)
def test_the_word_count_cases_hold_what_they_are_for(W):
    w1, rel, w2, inverse, n_words = synonyms_exact.word_count_case(W)
    assert n_words == W and w1.size == 200
    assert (w1 == W - 1).any() and (w2 == W - 1).any()
    m = synonyms_exact.array_model(w1, rel, w2, inverse, W)
    if W == 1:
        assert not w1.any() and not w2.any() and m.info()["features"] == 0         # (0, r, 0): q == 1 / f
    if W >= 255:
        assert (m.row == W - 1).any() and (m.word == W - 1).any()                   # the highest id in a kept feature, both ways
        assert m.info()["features"] > 50


@pytest.mark.parametrize("D", synonyms_exact.DISTINCT_COUNTS + synonyms_exact.SCAN_TILE_DISTINCT)
def test_the_distinct_count_cases_hold_what_they_are_for(D):
    w1, rel, w2, inverse, W = synonyms_exact.distinct_count_case(D)
    m = synonyms_exact.array_model(w1, rel, w2, inverse, W)
    assert m.key.size == D and w1.size == D // 2 + D % 2
    assert np.unique(synonyms_exact.pack_keys(w1, rel, w2)).size == w1.size        # all raw triples distinct
    assert m.f.max() == (2 if D % 2 else 1)
    assert m.info()["features"] > D // 4


def test_the_pair_case_holds_what_it_is_for():
    (w1, rel, w2, inverse, W), m = synonyms_exact.pair_case()
    assert (W, inverse.size, w1.size) == (9000, 24, 90000)
    hub = int(m.row_words[np.argmax(m.row_len)])
    assert m.row_len.max() > 16 * 128                                   # more than 16 chunks of the default length
    for C in synonyms_exact.PAIR_CANDIDATES:
        cand = synonyms_exact.pair_candidates(m, C)
        assert cand.size == C == np.unique(cand).size and hub in cand.tolist()
        assert (np.diff(cand) < 0).any() and (np.diff(cand) > 0).any()             # in no id order
        a, b, sim, shared, n_a, n_b = synonyms_exact.pairs_model(m, cand)
        assert np.abs(sim - synonyms_exact.PAIR_THRESHOLD).min() > synonyms_exact.PAIR_MARGIN
        assert (sim > synonyms_exact.PAIR_THRESHOLD).sum() > 1000 and a.size > 30000 and shared.max() > 40
    assert 1300 * -(-1300 // 256) + 1 > 4096                            # two scan tiles of pair counts
    assert -(-4097 // 256) == 17
