#!/usr/bin/env python3
"""Timing of the text-to-text cosine similarity (csrc/cosine_texts.h, `east texts similar`) on the collections of
tools/cosine_bench.py, so that the numbers sit beside DESIGN.md 9's: the Zipf stand-in and word-stream text at 256 texts of
1 MiB, 4 096 texts of 16 KiB of the Zipf stand-in, and the HSE texts.  Per shape (medians of --repeat):

  matrix_ms         device time of the matrix build (east_hip_last_text_similarity_ms: the scatter into document order, the tile
                    kernel and the fold per batch of segments, the finish), the weights and norms already made
  first_matrix_ms   the same for the first build after the index build: the weights and norms are made inside it
  rank_ms           device time of the ranking (N = 10) of the matrix (east_hip_last_top_ms)
  index_build_ms    device time of the same collection's index build, for scale
  host_path_s       the shapes of at most --host-bytes only: wall time of applications.texts_similar with
                    EAST_HIP_TEXTS_SIMILAR=host

    python tools/texts_similar_bench.py [--repeat 5] [--shapes zipf,word_stream,many,hse] [--out profiles/texts_similar_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 10


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def measure(name, texts, repeat, host_bytes):
    from east import applications, hip_backend, relevance
    index = hip_backend.HipCosineIndex()
    index.build_texts(texts)                            # warm-up: allocations, code objects
    index.texts_similar(True, N)
    build, first, matrix, rank = [], [], [], []
    for _ in range(repeat):
        index.build_texts(texts)
        build.append(index.info()["build_us"] / 1e3)
        info = index.texts_build(True)
        first.append(index.last_texts_ms())
        index.texts_build(True)
        matrix.append(index.last_texts_ms())
        index.rank_texts(N)
        rank.append(float(index._lib.east_hip_last_top_ms(index._h)))
    C, own, postings = index.texts_matrix()
    n_bytes = sum(len(t) for t in texts)
    row = {"shape": name, "docs": len(texts), "bytes": n_bytes, **{k: info[k] for k in ("units", "postings", "tiles", "segments", "launches")},
           "matrix_ms": spread(matrix), "first_matrix_ms": spread(first), "rank_ms": spread(rank), "index_build_ms": spread(build),
           "matrix_over_index_build": round(statistics.median(matrix) / statistics.median(build), 3),
           "mean_cosine": round(float(np.nanmean(C)), 6) if len(texts) > 1 else None,
           "largest_self_error_ulps": round(float(np.abs(own[postings > 0] - 1.0).max() / 2.0 ** -52), 1), "repeat": repeat}
    index.close()
    if n_bytes <= host_bytes:
        os.environ["EAST_HIP_TEXTS_SIMILAR"] = "host"
        try:
            t0 = time.perf_counter()
            applications.texts_similar({str(i): t for i, t in enumerate(texts)}, N, None,
                                       relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[]))
            row["host_path_s"] = round(time.perf_counter() - t0, 3)
        finally:
            del os.environ["EAST_HIP_TEXTS_SIMILAR"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="zipf,word_stream,many,hse")
    ap.add_argument("--host-bytes", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cosine_bench import word_stream_text, zipf_text
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    wanted = a.shapes.split(",")
    rng = np.random.default_rng(2)
    rows = []
    stream = [word_stream_text(rng, 1 << 20) for _ in range(256)]      # (drawn whether wanted or not: the same texts as tools/cosine_bench.py)
    if "word_stream" in wanted:
        rows.append(measure("configs2_word_stream", stream, a.repeat, a.host_bytes))
    del stream
    vocab = synthetic.zipf_vocabulary(rng)
    if "zipf" in wanted:
        rows.append(measure("configs2_zipf", [zipf_text(rng, 1 << 20, vocab) for _ in range(256)], a.repeat, a.host_bytes))
    if "many" in wanted:
        rows.append(measure("zipf_4096x16KiB", [zipf_text(rng, 1 << 14, vocab) for _ in range(4096)], a.repeat, a.host_bytes))
    if "hse" in wanted:
        with open(os.path.join(ROOT, "tests", "golden", "hse_config1.json"), encoding="utf-8") as f:
            hse = json.load(f)
        rows.append(measure("hse_config1", [hse["texts"][n].encode("utf-8") for n in sorted(hse["texts"])], a.repeat, a.host_bytes))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/texts_similar_bench.py", "cases": rows}, f, indent=1)


if __name__ == "__main__":
    main()
