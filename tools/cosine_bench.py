#!/usr/bin/env python3
"""Timing of the cosine relevance measure (csrc/cosine.h, `east -s cosine`): the index build and the score table at
BASELINE configs[2]'s shape -- 256 texts of 1 MiB, 10 000 keyphrases -- over word-stream text (tests/conftest.py's
word_stream: uniform A-Z words of 3..10 letters) and over the Zipf stand-in (east.synthetic.zipf_vocabulary), and at the HSE
config-1 shape (30 texts x 10 keyphrases).  Device ms: the library's events around its own work (the upload of the texts
included); wall ms: the Python call; chars/s: input bytes over device time.  For comparison, the plain restatement of the
tests (tests/test_cosine_host.py) on a slice.  One JSON line per measurement.

    python tools/cosine_bench.py [--repeat 5] [--slice-docs 4] [--slice-keyphrases 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def word_stream_text(rng, n_bytes, lo=3, hi=10):
    """tests/conftest.py's word_stream (BASELINE synthetic text)."""
    n_words = n_bytes // ((lo + hi) // 2) + 16
    lens = rng.integers(lo, hi + 1, size=n_words)
    buf = rng.integers(65, 91, size=int(lens.sum() + n_words), dtype=np.uint8)
    buf[np.cumsum(lens + 1) - 1] = 32
    return buf[:n_bytes].tobytes()


def zipf_text(rng, n_bytes, vocab):
    """About n_bytes of Zipf-distributed words of the stand-in vocabulary joined by single spaces (the words of
    east.synthetic.zipf_document)."""
    mean_len = float((vocab["lens"] * np.diff(np.concatenate([[0.0], vocab["cdf"]]))).sum())
    n_words = max(1, int(n_bytes / (mean_len + 1.0)))
    ids = np.searchsorted(vocab["cdf"], rng.random(n_words), side="left").clip(0, vocab["lens"].size - 1)
    lens = vocab["lens"][ids]
    src = np.repeat(vocab["starts"][ids] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    out = np.full(int(lens.sum()) + n_words, 32, dtype=np.uint8)
    dst = np.repeat(np.cumsum(lens + 1) - (lens + 1) - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    out[dst] = vocab["letters"][src]
    return out[:n_bytes].tobytes()


def keyphrases_from(rng, texts, k):
    out = []
    for _ in range(k):
        words = []
        for _ in range(int(rng.integers(1, 4))):
            t = texts[int(rng.integers(0, len(texts)))]
            p = int(rng.integers(0, len(t)))
            a, e = t.rfind(b" ", 0, p) + 1, t.find(b" ", p)
            words.append(t[a:e if e >= 0 else len(t)].decode())
        out.append(" ".join(w for w in words if w) or "NONE")
    return out


def measure(name, texts, keyphrases, repeat, slice_docs, slice_kps):
    from east import relevance, utils
    from test_cosine_host import restate
    prepared = [utils.prepare_text(k) for k in keyphrases]
    m = relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[])
    m.set_text_collection(texts)                       # warm-up: allocations, code objects
    m.relevance_table(prepared)
    b_dev, b_wall, s_dev, s_wall = [], [], [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        m.set_text_collection(texts)
        b_wall.append((time.perf_counter() - t0) * 1e3)
        b_dev.append(m.index.info()["build_us"] / 1e3)
        t0 = time.perf_counter()
        table = m.relevance_table(prepared)
        s_wall.append((time.perf_counter() - t0) * 1e3)
        s_dev.append(m.index.info()["score_us"] / 1e3)
    info = m.index.info()
    n_bytes = sum(len(t) for t in texts)
    d = min(slice_docs, len(texts))
    kk = min(slice_kps, len(keyphrases))
    t0 = time.perf_counter()
    host = restate([t.decode("utf-8", "replace") for t in texts[:d]], keyphrases[:kk], "words", "tf-idf")
    host_ms = (time.perf_counter() - t0) * 1e3
    sub = relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[])
    sub.set_text_collection(texts[:d])
    diff = float(np.max(np.abs(sub.relevance_table(prepared[:kk]) - np.array(host)))) if kk else 0.0
    bd, sd = statistics.median(b_dev), statistics.median(s_dev)
    print(json.dumps({
        "shape": name, "docs": len(texts), "bytes": n_bytes, "keyphrases": len(keyphrases),
        "kept_tokens": info["kept_tokens"], "terms": info["terms"], "postings": info["postings"],
        "build_device_ms": round(bd, 3), "build_wall_ms": round(statistics.median(b_wall), 3),
        "build_chars_per_s": round(n_bytes / (bd / 1e3), 1) if bd > 0 else None,
        "score_device_ms": round(sd, 3), "score_wall_ms": round(statistics.median(s_wall), 3),
        "scores_per_s": round(table.size / (sd / 1e3), 1) if sd > 0 else None,
        "host_restatement": {"docs": d, "keyphrases": kk, "bytes": sum(len(t) for t in texts[:d]), "ms": round(host_ms, 1),
                             "max_abs_diff": diff},
        "repeat": repeat}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--slice-docs", type=int, default=4)
    ap.add_argument("--slice-keyphrases", type=int, default=200)
    a = ap.parse_args()
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    rng = np.random.default_rng(2)
    texts = [word_stream_text(rng, 1 << 20) for _ in range(256)]
    measure("configs2_word_stream", texts, keyphrases_from(rng, texts, 10_000), a.repeat, a.slice_docs, a.slice_keyphrases)
    vocab = synthetic.zipf_vocabulary(rng)
    texts = [zipf_text(rng, 1 << 20, vocab) for _ in range(256)]
    measure("configs2_zipf", texts, keyphrases_from(rng, texts, 10_000), a.repeat, a.slice_docs, a.slice_keyphrases)
    with open(os.path.join(ROOT, "tests", "golden", "hse_config1.json"), encoding="utf-8") as f:
        hse = json.load(f)
    texts = [hse["texts"][n].encode("utf-8") for n in sorted(hse["texts"])]
    measure("hse_config1", texts, hse["keyphrases"], a.repeat, len(texts), len(hse["keyphrases"]))


if __name__ == "__main__":
    main()
