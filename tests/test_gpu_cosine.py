"""gpu tier: the cosine relevance measure on the device (csrc/cosine.h through include/east_hip.h) against the fixture
recorded from the reference (tests/golden/cosine.json) and against the plain restatement of test_cosine_host.py."""
import io
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

import cosine_exact as cx
from conftest import load_golden, word_stream
from test_cosine_host import ToyStemmer, assert_scores, case_texts, restate

pytestmark = pytest.mark.gpu


def _measure(space, weighting, stopwords=()):
    from east import relevance
    return relevance.CosineRelevanceMeasure(space, weighting, stopwords=list(stopwords),
                                            stemmer=ToyStemmer() if space == "stems" else None)


def _prepared(queries):
    from east import utils
    return [utils.prepare_text(q) for q in queries]


def test_fixture_cases_through_the_measure(hip):
    g = load_golden("cosine.json")
    for case in g["cases"]:
        texts = case_texts(g, case)
        prepared = _prepared(case["queries"])
        for mode in case["modes"]:
            stop = g["stopwords"] if mode["stopwords"] else ()
            m = _measure(mode["space"], mode["weighting"], stop)
            m.set_text_collection([t.encode("utf-8") for t in texts])
            table = m.relevance_table(prepared)
            assert_scores(table.tolist(), mode["scores"])
            assert_scores(table.tolist(), restate(texts, case["queries"], mode["space"], mode["weighting"], stop, ToyStemmer()))
            for k in (0, len(prepared) - 1):                         # relevance(): the one-row cache
                assert [m.relevance(prepared[k], d) for d in range(len(texts))] == table[k].tolist()


def test_keyphrases_table_and_graph(hip):
    from east import applications
    g = load_golden("cosine.json")["cli"]
    hse = load_golden("hse_config1.json")["texts"]
    texts = {name: hse[name].encode("utf-8") for name in sorted(hse)}
    table = applications.keyphrases_table(g["keyphrases"], texts, _measure("words", "tf-idf"))
    for kp in g["keyphrases"]:
        assert_scores([[table[kp][n] for n in texts]], [[g["table"][kp][n] for n in texts]])
    graph = applications.keyphrases_graph(g["keyphrases"], texts, 0.6, 0.25, 1, _measure("words", "tf-idf"))
    assert graph["nodes"] == g["graph"]["nodes"]
    assert [(e["source"], e["target"]) for e in graph["edges"]] == [(e["source"], e["target"]) for e in g["graph"]["edges"]]
    assert np.allclose([e["confidence"] for e in graph["edges"]], [e["confidence"] for e in g["graph"]["edges"]], rtol=0, atol=1e-12)


def _same_print(out, want):
    """The same text, and every printed number the same to the printed precision."""
    num = re.compile(r"\d+\.\d+")
    assert num.sub("#", out) == num.sub("#", want)
    got, exp = [float(x) for x in num.findall(out)], [float(x) for x in num.findall(want)]
    assert len(got) == len(exp) and all(abs(a - b) <= 1.01e-3 for a, b in zip(got, exp))


def test_cli_cosine_table_and_graph(hip, tmp_path):
    try:
        import nltk  # noqa: F401
        pytest.skip("nltk is installed: the CLI removes its stopwords, the fixture was recorded without")
    except ImportError:
        pass
    from east import formatting, main
    g = load_golden("cosine.json")["cli"]
    tdir = tmp_path / "texts"
    tdir.mkdir()
    for name, text in load_golden("hse_config1.json")["texts"].items():
        (tdir / (name + ".txt")).write_bytes(text.encode("utf-8"))
    kp = tmp_path / "kp.txt"
    kp.write_bytes("\n".join(g["keyphrases"]).encode("utf-8"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main.main(["-s", "cosine", "-v", "words", "-w", "tf-idf", "keyphrases", "table", str(kp), str(tdir)]) == 0
    _same_print(buf.getvalue(), g["xml"] + "\n")
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main.main(["-s", "cosine", "-v", "words", "-f", "edges", "keyphrases", "graph", str(kp), str(tdir)]) == 0
    assert buf.getvalue() == formatting.graph2edges(g["graph"]) + "\n"


def test_toy_stemmer_merges_terms(hip):
    texts = [b"testing tests tested", b"runs running runner", b"nothing related here"]
    m = _measure("stems", "tf")
    m.set_text_collection(texts)
    info = m.index.info()
    assert m.index.terms() == ["TESTING", "TESTS", "TESTED", "RUNS", "RUNNING", "RUNNER", "NOTHING", "RELATED", "HERE"]
    assert info["terms"] == 9 and info["classes"] == 8 and info["postings"] == 8
    queries = ["TEST", "RUN RUNNING", "TESTS NOTHING"]
    table = m.relevance_table(queries)
    assert table[0, 0] > 0 and table[1, 1] > 0
    assert_scores(table.tolist(), restate([t.decode() for t in texts], queries, "stems", "tf", (), ToyStemmer()))


def _random_words(rng, n, lo=3, hi=9):
    lens = rng.integers(lo, hi + 1, size=n)
    letters = rng.integers(65, 91, size=int(lens.sum()), dtype=np.uint8).tobytes().decode()
    ends = np.cumsum(lens)
    return [letters[e - l:e] for e, l in zip(ends.tolist(), lens.tolist())]


def test_forced_hash_collisions_give_the_same_bits(hip):
    rng = np.random.default_rng(5)
    texts = [word_stream(rng, 100_000) for _ in range(4)]           # ~50 000 distinct words
    queries = [" ".join(w) for w in zip(_random_words(rng, 300), texts[0].decode().split()[:300])]
    m0 = _measure("words", "tf-idf")
    m0.set_text_collection(texts)
    t0 = m0.relevance_table(queries)
    lib = hip.load()
    assert lib.east_hip_debug_set_term_hash_bits(8) == 0
    try:
        m1 = _measure("words", "tf-idf")
        m1.set_text_collection(texts)
        t1 = m1.relevance_table(queries)
    finally:
        lib.east_hip_debug_set_term_hash_bits(0)
    i0, i1 = m0.index.info(), m1.index.info()
    assert i0["hash_attempts"] == 1 and i1["hash_attempts"] == 2
    assert i1["terms"] == i0["terms"] > 10 ** 4
    assert t0.tobytes() == t1.tobytes()
    assert m0.index.terms() == m1.index.terms()
    assert (t0 > 0).any()


def test_repeated_runs_are_bit_identical(hip):
    g = load_golden("cosine.json")
    case = g["cases"][0]
    texts = [t.encode("utf-8") for t in case_texts(g, case)]
    prepared = _prepared(case["queries"])
    tables = []
    for _ in range(2):
        m = _measure("words", "tf-idf")
        m.set_text_collection(texts)
        tables.append(m.relevance_table(prepared).tobytes())
        m.set_text_collection(texts)                                # the same measure, built again
        tables.append(m.relevance_table(prepared).tobytes())
        tables.append(m.relevance_table(prepared).tobytes())        # the cached weights
    assert len(set(tables)) == 1


def _word_codes(text):
    """The tokens of >= 3 letters of A-Z + space text as integers, 5 bits per letter from the top (a word of at most 12
    letters has one code and a code one word)."""
    b = np.frombuffer(text, dtype=np.uint8)
    edges = np.diff(np.concatenate([[0], (b != 32).astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
    lens = ends - starts
    starts, lens = starts[lens >= 3], lens[lens >= 3]
    assert lens.size == 0 or lens.max() <= 12
    code = np.zeros(starts.size, dtype=np.uint64)
    for j in range(12):
        m = lens > j
        code[m] |= (b[starts[m] + j].astype(np.uint64) - np.uint64(64)) << np.uint64(5 * (11 - j))
    return code


def _member(sorted_keys, x):
    """(x is in sorted_keys, its place there)."""
    pos = np.searchsorted(sorted_keys, x)
    found = sorted_keys[np.minimum(pos, sorted_keys.size - 1)] == x if sorted_keys.size else np.zeros(x.size, dtype=bool)
    return found & (pos < sorted_keys.size), pos


def configs2_exact(parts, n_docs, sample_docs):
    """The exact model of cosine_exact.py (integers exact, ln / sqrt / the quotient at 50 digits, one rounding) on the
    integer word codes of configs2_restatement: {d: (scores of every keyphrase in document d, its postings)}."""
    uniq, df_keys, df, per_kp = parts["uniq"], parts["df_keys"], parts["df"], parts["per_kp"]
    idf = {}
    out = {}
    for d in sample_docs:
        u, cnt = uniq[d]
        dfs = df[np.searchsorted(df_keys, u)]
        squares = np.bincount(dfs, cnt.astype(np.float64) ** 2)              # (integers below 2^53: exact)
        for f in np.flatnonzero(squares).tolist():
            idf.setdefault(f, 1 + cx.MP.log(cx.MP.mpf(n_docs) / f))
        rad = sum((int(squares[f]) * idf[f] ** 2 for f in np.flatnonzero(squares).tolist()), cx.MP.mpf(0))
        scores = np.zeros(len(per_kp))
        for k, (codes, c) in enumerate(per_kp):
            in_vocab, _ = _member(df_keys, codes)
            hit, pos = _member(u, codes)
            if hit.any():
                num = sum((int(c[i]) * int(cnt[pos[i]]) * idf[int(dfs[pos[i]])] for i in np.flatnonzero(hit).tolist()), cx.MP.mpf(0))
                q2 = int((c[in_vocab].astype(np.int64) ** 2).sum())
                scores[k] = float(num / cx.MP.sqrt(rad * q2))
        out[d] = (scores, int(u.size))
    return out


def configs2_restatement(texts, kps, sample_docs, parts=None):
    """The restatement of test_cosine_host for word-stream text, on integer word codes: (shared[k, d] = keyphrase k and
    document d share a term, {d: scores of every keyphrase in the sampled document d}).  `parts`: a dict that receives
    the integer structures (configs2_exact, the counts of east_hip_cosine_info)."""
    D, K = len(texts), len(kps)
    codes = [_word_codes(t) for t in texts]
    uniq = [np.unique(c, return_counts=True) for c in codes]
    df_keys, df = np.unique(np.concatenate([u for u, _ in uniq]), return_counts=True)
    per_kp = [np.unique(_word_codes(kp.encode()), return_counts=True) for kp in kps]
    q_len = np.array([int(c.sum()) for _, c in per_kp], dtype=np.float64)
    owner = np.repeat(np.arange(K), [u.size for u, _ in per_kp])
    distinct = np.concatenate([u for u, _ in per_kp])
    counts = np.concatenate([c for _, c in per_kp]).astype(np.float64)
    in_vocab, _ = _member(df_keys, distinct)
    qv = np.where(in_vocab, counts / np.maximum(q_len[owner], 1.0), 0.0)
    qn2 = np.bincount(owner, qv * qv, minlength=K)
    qn = np.where(np.bincount(owner, in_vocab, minlength=K) > 0, np.sqrt(qn2), 1.0)
    shared = np.zeros((K, D), dtype=bool)
    for d, (u, _) in enumerate(uniq):
        hit, _ = _member(u, distinct)
        shared[owner[hit], d] = True
    scores = {}
    for d in sample_docs:
        u, cnt = uniq[d]
        w = cnt / max(codes[d].size, 1) * (1.0 + np.log(D / df[np.searchsorted(df_keys, u)]))
        norm = np.sqrt(np.sum(w * w)) if w.size else 1.0
        hit, pos = _member(u, distinct)
        dot = np.bincount(owner, np.where(hit, w[np.minimum(pos, u.size - 1)] * qv, 0.0), minlength=K)
        scores[d] = dot / (norm * qn)
    if parts is not None:
        parts.update(uniq=uniq, df_keys=df_keys, df=df, per_kp=per_kp, q_len=q_len, kept_tokens=sum(int(c.size) for c in codes),
                     terms=int(df_keys.size), postings=sum(int(u.size) for u, _ in uniq))
    return shared, scores


def test_configs2_shape_against_the_restatement(hip):
    """BASELINE configs[2]: 256 texts of 1 MiB, 10 000 keyphrases.  All keyphrases against the restatement on a sample of
    documents; on all of them, scores in [0, 1] and a score > 0 exactly where the keyphrase and the document share a term."""
    rng = np.random.default_rng(2)
    D, K = 256, 10_000
    texts = [word_stream(rng, 1 << 20) for _ in range(D)]

    def word_at(t, p):
        a, e = t.rfind(b" ", 0, p) + 1, t.find(b" ", p)
        return t[a:e if e >= 0 else len(t)].decode()
    pool = [word_at(texts[int(d)], int(p)) for d, p in zip(rng.integers(0, D, 20_000), rng.integers(0, 1 << 20, 20_000))]
    pool = [w for w in pool if w] or ["NONE"]
    fresh = _random_words(rng, 5_000, 11, 12)                        # (no word of the texts is that long)
    kps = []
    for k in range(K):
        n = int(rng.integers(1, 4))
        kps.append(" ".join(pool[int(x)] if rng.random() < 0.8 else fresh[int(x) % len(fresh)]
                            for x in rng.integers(0, len(pool), n)))
    m = _measure("words", "tf-idf")
    m.set_text_collection(texts)
    table = m.relevance_table(kps)
    assert table.shape == (K, D)

    sample = (0, 37, 128, 255)
    parts = {}
    shared, scores = configs2_restatement(texts, kps, sample, parts)
    info = m.index.info()                                            # the counts, from the integer codes
    assert (info["n_docs"], info["kept_tokens"], info["words"], info["terms"], info["postings"], info["classes"]) == \
        (D, parts["kept_tokens"], parts["terms"], parts["terms"], parts["postings"], 0)
    assert ((table >= 0.0) & (table <= 1.0 + 1e-12)).all()
    assert np.array_equal(table > 0.0, shared)
    assert shared.any() and not shared.all()
    for d in sample:
        want = scores[d]
        assert np.abs(table[:, d] - want).max() <= 1e-12
        assert np.array_equal(table[:, d] == 0.0, want == 0.0)
    for d, (exact, p_d) in configs2_exact(parts, D, sample).items():      # ... and the relative bound of DESIGN.md 9
        cx.check_scores(table[:, [d]], exact[:, None], [p_d], parts["q_len"])


def test_one_text_of_a_single_huge_token(hip):
    rng = np.random.default_rng(7)
    big = rng.integers(65, 91, size=16 << 20, dtype=np.uint8).tobytes()
    mid = big[:5000]                                                 # three pieces of the hash
    texts = [big, b"SHORT WORDS HERE " + mid + b" " + mid, big]
    m = _measure("words", "tf-idf")
    m.set_text_collection(texts)
    info = m.index.info()
    assert info["terms"] == 5 and info["postings"] == 6 and info["hash_attempts"] == 1
    terms = m.index.terms()
    assert [len(t) for t in terms] == [16 << 20, 5, 5, 4, 5000] and terms[4] == mid.decode() and terms[0] == big.decode()
    queries = ["SHORT", mid.decode(), "SHORT " + mid.decode(), "WORDS NOPE"]
    table = m.relevance_table(queries)
    assert_scores(table.tolist(), restate([t.decode() for t in texts], queries, "words", "tf-idf"))
    assert table[1, 1] > 0 and table[1, 0] == 0.0 and table[1, 2] == 0.0


def test_easa_and_cosine_share_a_handle(hip):
    from east import exceptions, hip_backend, utils
    idx = hip_backend.HipIndex()
    a_texts = [b"The quick brown fox jumps", b"XABXAC suffix arrays of the texts"]
    idx.build_texts(a_texts)
    qs, qo = hip_backend.pack_queries([utils.prepare_text(k) for k in ("quick fox", "ABC", "suffix")])
    easa0 = idx.score_table(qs, qo)
    cos = hip_backend.HipCosineIndex(index=idx)
    c_texts = [b"alpha beta gamma", b"beta gamma delta delta"]
    cos.build_texts(c_texts)
    ids = cos.lookup(["BETA", "DELTA", "NOPE"])
    assert ids.tolist() == [1, 3, -1]
    cos0 = cos.score_table(ids, [0, 3], True)
    assert_scores(cos0.tolist(), restate([t.decode() for t in c_texts], ["BETA DELTA NOPE"], "words", "tf-idf"))
    assert np.array_equal(idx.score_table(qs, qo), easa0)              # the cosine build left the EASA index alone
    idx.build_texts([b"another collection entirely", b"of two texts"])
    assert np.array_equal(cos.score_table(ids, [0, 3], True), cos0)     # ... and the other way round
    assert hip.load().east_hip_reset(idx._h) == 0                     # reset forgets both
    assert cos.info()["built"] == 0
    with pytest.raises(exceptions.HipBackendError):
        cos.score_table(ids, [0, 3], True)
    idx.close()
