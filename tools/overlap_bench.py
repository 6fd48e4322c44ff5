#!/usr/bin/env python3
"""Timing of the shingle overlap (csrc/overlap.h, `east texts overlap`) on an MI355X: per shape the cosine index build it
starts from and, at w = 4, the build under route 1 (the integer matrix-core kernel) and route 2 (the f64 tile kernel on unit
weights), alternating, in device ms, medians of --repeat runs with every run kept; the part up to the operands in text
order (the naming levels, the postings, the sizes, the sort) and the part behind it (product and quotients) separately.

Shapes: the 30 texts of tests/golden/hse_config1.json; the Zipf stand-in 256 x 1 MiB of tools/cosine_bench.py; 4 096 texts
of 16 KiB of the same; 256 x 1 MiB of a uniform word stream (almost no repeats: few shared shingles).

    python tools/overlap_bench.py [--repeat 5] [--shapes hse,zipf256,zipf4096,stream256] [--out profiles/overlap_bench.json]

One JSON line per shape on stdout; --out collects them in one file.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORDS = 4


def shapes(names):
    from cosine_bench import word_stream_text, zipf_text
    from east import synthetic
    rng = np.random.default_rng(2)
    for name in names:
        if name == "hse":
            with open(os.path.join(ROOT, "tests", "golden", "hse_config1.json"), encoding="utf-8") as f:
                hse = json.load(f)
            yield "hse_config1", [hse["texts"][n].encode("utf-8") for n in sorted(hse["texts"])]
        elif name == "zipf256":
            vocab = synthetic.zipf_vocabulary(rng)
            yield "zipf_256x1MiB", [zipf_text(rng, 1 << 20, vocab) for _ in range(256)]
        elif name == "zipf4096":
            vocab = synthetic.zipf_vocabulary(rng)
            yield "zipf_4096x16KiB", [zipf_text(rng, 16 << 10, vocab) for _ in range(4096)]
        elif name == "stream256":
            yield "word_stream_256x1MiB", [word_stream_text(rng, 1 << 20) for _ in range(256)]
        else:
            raise SystemExit("unknown shape %r" % name)


def measure(name, texts, repeat):
    from east import hip_backend
    lib = hip_backend.load()
    index = hip_backend.HipCosineIndex()
    index.build_texts(texts, ())                       # warm-up: allocations, code objects
    builds = []
    for _ in range(repeat):
        index.build_texts(texts, ())
        builds.append(index.info()["build_us"] / 1e3)
    info = index.info()
    line = {"shape": name, "docs": len(texts), "bytes": sum(len(t) for t in texts), "kept_tokens": info["kept_tokens"],
            "terms": info["terms"], "words": WORDS, "index_build_ms": round(statistics.median(builds), 3),
            "index_build_runs_ms": [round(r, 3) for r in builds], "repeat": repeat}
    runs = {1: [], 2: []}
    parts = {1: [], 2: []}
    try:
        for route in (1, 2):                            # warm-up of both
            lib.east_hip_debug_set_overlap_route(route)
            found = index.overlap_build(WORDS, hip_backend.OVERLAP_SYMMETRIC)
        for _ in range(repeat):
            for route in (1, 2):
                lib.east_hip_debug_set_overlap_route(route)
                found = index.overlap_build(WORDS, hip_backend.OVERLAP_SYMMETRIC)
                runs[route].append(index.last_overlap_ms())
                parts[route].append((found["operands_us"] / 1e3, found["product_us"] / 1e3))
    finally:
        lib.east_hip_debug_set_overlap_route(0)
    for key in ("shingle_positions", "distinct_shingles", "shared_shingles", "postings", "segments", "levels", "tiles"):
        line[key] = found[key]
    for route, tag in ((1, "route1_i8"), (2, "route2_f64")):
        line[tag] = {"build_ms": round(statistics.median(runs[route]), 3), "runs_ms": [round(r, 3) for r in runs[route]],
                     "operands_ms": round(statistics.median(p[0] for p in parts[route]), 3),
                     "product_ms": round(statistics.median(p[1] for p in parts[route]), 3),
                     "product_runs_ms": [round(p[1], 3) for p in parts[route]]}
    spread2 = max(p[1] for p in parts[2]) - min(p[1] for p in parts[2])
    line["route2_product_spread_ms"] = round(spread2, 3)
    line["i8_ahead_by_ms"] = round(line["route2_f64"]["product_ms"] - line["route1_i8"]["product_ms"], 3)
    line["ratio_to_index_build"] = round(min(line["route1_i8"]["build_ms"], line["route2_f64"]["build_ms"]) / line["index_build_ms"], 3)
    index.close()
    print(json.dumps(line, ensure_ascii=False), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="hse,zipf256,zipf4096,stream256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from east import hip_backend
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    lines = [measure(name, texts, a.repeat) for name, texts in shapes(a.shapes.split(","))]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump({"tool": "tools/overlap_bench.py", "device_ms": "the library's events around its own work",
                       "shapes": lines}, f, indent=1, ensure_ascii=False)
            f.write("\n")


if __name__ == "__main__":
    main()
