#!/usr/bin/env python3
"""Timing of synonym extraction (csrc/synonyms.h, `east -y -t`) on seeded synthetic triples whose words follow a Zipf law:
about 2 000, 20 000 and 100 000 words with 10, 20 and 50 raw triples per word on average, 24 relations, every word a
candidate, threshold 0.3.  Per size, medians of --repeat calls after one warm-up call:

  build_device_ms   the feature build between two events on the handle's stream (uploads and read-backs included)
  pairs_device_ms   the pair pass (count, scan, fill) likewise
  pairs_wall_ms     the pairs call with the fetch of the (a, b, similarity) arrays
  pairs_examined    C (C - 1) / 2; pairs_emitted: those above the threshold
  row_bytes         what the CSR rows occupy (16 bytes a feature); rows_read_bytes: what the pair kernel's two passes read
                    of them by construction -- every target row once per source block in front of it (C / 16 blocks, half of
                    them on average), every source row once per target tile behind it --; rows_read_gb_s = that over the
                    pair pass's time, pairs_per_us = pairs examined over it

The per-kernel split comes from the library's profiler (one more build and pair pass with it switched on).

--reference times the reference's own get_synonyms instead (where the reference is present: the build container, through
oracle/ref_shim.py with the parser process replaced as tools/gen_synonyms_golden.py does), on a ladder of sizes of the same
generator, 10 raw triples per word, up to the largest it finishes in about a minute, and records that under "reference" in
the same file.

    python tools/synonyms_bench.py [--sizes 2000x10,20000x20,100000x50] [--repeat 5] [--out profiles/synonyms_bench.json]
    PYTHONHASHSEED=0 PYTHONUTF8=1 python tools/synonyms_bench.py --reference --out profiles/synonyms_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((2_000, 10), (20_000, 20), (100_000, 50))
RELATIONS = 24
THRESHOLD = 0.3
SRC, TGT = 16, 256                      # csrc/synonyms.h: SY_SRC, SY_TGT


def zipf_ids(n_words, per_word, seed=1):
    """(w1, relation, w2) id arrays of n_words * per_word raw triples: both words Zipf (weight 1 / rank), the relation
    uniform.  Ids are ranks, so word 0 is the hub."""
    rng = np.random.default_rng(seed)
    n = n_words * per_word
    weights = 1.0 / np.arange(1, n_words + 1)
    cdf = np.cumsum(weights / weights.sum())
    w1 = np.minimum(np.searchsorted(cdf, rng.random(n)), n_words - 1).astype(np.int32)
    w2 = np.minimum(np.searchsorted(cdf, rng.random(n)), n_words - 1).astype(np.int32)
    rel = rng.integers(0, RELATIONS, size=n).astype(np.int32) * 2            # even ids: r, odd ids: r_of
    inverse = (np.arange(2 * RELATIONS, dtype=np.int32) ^ 1)
    return w1, rel, w2, inverse


def measure(dev, n_words, per_word, repeat):
    w1, rel, w2, inverse = zipf_ids(n_words, per_word)
    cand = np.arange(n_words, dtype=np.int32)
    dev.build(w1, rel, w2, inverse, n_words)                                   # warm-up (allocations)
    build_ms = []
    for _ in range(repeat):
        dev.build(w1, rel, w2, inverse, n_words)
        build_ms.append(dev.last_ms)
    info = dev.info()
    dev.pairs(cand, THRESHOLD)
    pairs_ms, wall_ms = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        a, b, sim = dev.pairs(cand, THRESHOLD)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        pairs_ms.append(dev.last_ms)
    dev.index.profile_enable(True)
    dev.build(w1, rel, w2, inverse, n_words)
    dev.pairs(cand, THRESHOLD, fetch=False)
    kernels = {name: round(ms, 4) for name, (count, ms) in dev.index.profile_report().items()}
    dev.index.profile_enable(False)

    C = n_words
    row_bytes = info["features"] * 16
    # per pass: a target row is read by the source blocks in front of it, a source row staged by the target tiles behind it
    rows_read = 2 * (row_bytes * (C / SRC) / 2 + row_bytes * (C / TGT) / 2)
    t = statistics.median(pairs_ms)
    return {"words": n_words, "raw_triples": int(w1.size), "triples_per_word": per_word, "relations": 2 * RELATIONS,
            "distinct_triples": info["distinct_triples"], "features": info["features"], "longest_row": info["longest_row"],
            "candidates": C, "threshold": THRESHOLD,
            "build_device_ms": round(statistics.median(build_ms), 3), "pairs_device_ms": round(t, 3),
            "pairs_wall_ms": round(statistics.median(wall_ms), 3),
            "pairs_examined": C * (C - 1) // 2, "pairs_emitted": int(a.size),
            "row_bytes": row_bytes, "rows_read_bytes": int(rows_read), "rows_read_gb_s": round(rows_read / t / 1e6, 2),
            "pairs_per_us": round(C * (C - 1) / 2 / t / 1e3, 2), "kernels_ms": kernels, "repeat": repeat}


def time_reference(budget_s=60.0):
    """The reference's get_synonyms on the ladder 25, 50, 100, ... words (10 raw triples a word): the largest size it
    finishes within the budget, a step being taken only while the last one took less than an eighth of it (the work
    grows with W^2 R look-ups per word pair, synonyms.py:136-169)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import types
    import ref_shim
    import gen_synonyms_golden as gen
    ref_shim.install()
    from east.synonyms import synonyms as ref
    ref.subprocess = types.SimpleNamespace(Popen=gen.FakeParser, PIPE=-1)
    ref.SynonymExtractor._get_tomita_path = lambda self: ("", "tomita")
    ladder = []
    n_words = 25
    while True:
        w1, rel, w2, _ = zipf_ids(n_words, 10)
        names = ["WORD%06d" % i for i in range(n_words)]
        triples = [(names[a], "rel%d" % (r // 2), names[b]) for a, r, b in zip(w1.tolist(), rel.tolist(), w2.tolist())]
        gen.FakeParser.xml = gen.triples_xml(triples)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "text.txt")
            with open(path, "w", encoding="utf-8") as f:
                f.write(" ".join(names) + "\n")
            ex = ref.SynonymExtractor(path)
        t0 = time.perf_counter()
        found = ex.get_synonyms(THRESHOLD)
        seconds = time.perf_counter() - t0
        ladder.append({"words": len(ex.words), "raw_triples": len(triples), "get_synonyms_s": round(seconds, 3),
                       "pairs_emitted": sum(len(v) for v in found.values()) // 2})
        print(json.dumps(ladder[-1]), flush=True)
        if seconds * 8 > budget_s:
            break
        n_words *= 2
    return {"what": "the reference's SynonymExtractor.get_synonyms(0.3), Python 3 through oracle/ref_shim.py, one CPU core",
            "ladder": ladder, "largest": ladder[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None, help="e.g. 2000x10,20000x20 (default: the three of the docstring)")
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    record = {"tool": "tools/synonyms_bench.py"}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            record = json.load(f)
    if a.reference:
        record["reference"] = time_reference()
    else:
        try:
            import torch  # noqa: F401  (first: torch brings its own HIP runtime)
        except ImportError:
            pass
        from east import hip_backend
        assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
        sizes = SIZES if not a.sizes else tuple(tuple(int(x) for x in s.split("x")) for s in a.sizes.split(","))
        dev = hip_backend.HipSynonyms()
        done = {(s["words"], s["triples_per_word"]): s for s in record.get("sizes", [])}
        for n_words, per_word in sizes:
            done[(n_words, per_word)] = measure(dev, n_words, per_word, a.repeat)
            print(json.dumps(done[(n_words, per_word)]), flush=True)
        dev.close()
        record["sizes"] = [done[k] for k in sorted(done)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
