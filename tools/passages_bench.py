#!/usr/bin/env python3
"""Timing of the shared passages (csrc/passages.h, `east texts passages`) on an MI355X: per shape of tools/overlap_bench.py,
at w = 4 and with the n = 10 partners of every text that the overlap ranks, the passages build under route 1 (b in the
shingle's text list) and route 2 (the shingle in b's list), alternating, in device ms from the library's events, medians of
--repeat runs with every run kept: names and postings, the match kernel, runs + order + cut; the bit words and the match
kernel's bytes written over its time; beside the same texts' overlap build.

    python tools/passages_bench.py [--repeat 5] [--shapes hse,zipf256,zipf4096,stream256] [--out profiles/passages_bench.json]

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

WORDS, PARTNERS, PER_PAIR = 4, 10, 5


def measure(name, texts, repeat):
    from east import hip_backend
    lib = hip_backend.load()
    index = hip_backend.HipCosineIndex()
    index.build_texts(texts, ())
    index.overlap_build(WORDS, hip_backend.OVERLAP_SYMMETRIC)       # warm-up
    overlap = []
    for _ in range(repeat):
        index.overlap_build(WORDS, hip_backend.OVERLAP_SYMMETRIC)
        overlap.append(index.last_overlap_ms())
    top = index.rank_overlap(min(PARTNERS, max(len(texts) - 1, 1)))
    pa = np.repeat(np.arange(len(texts), dtype=np.int32), top.count)
    pb = np.concatenate([row[:c] for row, c in zip(top.index, top.count.tolist())]).astype(np.int32)
    line = {"shape": name, "docs": len(texts), "bytes": sum(len(t) for t in texts), "words": WORDS, "partners": PARTNERS,
            "per_pair": PER_PAIR, "repeat": repeat, "overlap_build_ms": round(statistics.median(overlap), 3),
            "overlap_build_runs_ms": [round(r, 3) for r in overlap]}
    runs, parts = {1: [], 2: []}, {1: [], 2: []}
    try:
        for route in (1, 2):                            # warm-up of both
            lib.east_hip_debug_set_passages_route(route)
            found = index.passages(pa, pb, WORDS, None, PER_PAIR)
        for _ in range(repeat):
            for route in (1, 2):
                lib.east_hip_debug_set_passages_route(route)
                found = index.passages(pa, pb, WORDS, None, PER_PAIR)
                runs[route].append(index.last_passages_ms())
                parts[route].append(index.passages_phases_ms())
    finally:
        lib.east_hip_debug_set_passages_route(0)
    line.update(found.info)
    del line["route"]
    line["longest_passage_words"] = int(found.words.max()) if found.words.size else 0
    for route, tag in ((1, "route1_text_list"), (2, "route2_unit_list")):
        match = statistics.median(p[1] for p in parts[route])
        line[tag] = {"build_ms": round(statistics.median(runs[route]), 3), "runs_ms": [round(r, 3) for r in runs[route]],
                     "names_postings_ms": round(statistics.median(p[0] for p in parts[route]), 3),
                     "match_ms": round(match, 4), "match_runs_ms": [round(p[1], 4) for p in parts[route]],
                     "runs_order_cut_ms": round(statistics.median(p[2] for p in parts[route]), 3),
                     "match_written_GBps": round(found.info["bit_words"] * 8 / (match * 1e-3) / 1e9, 3) if match > 0 else None}
    line["route1_match_spread_ms"] = round(max(p[1] for p in parts[1]) - min(p[1] for p in parts[1]), 4)
    line["route2_match_spread_ms"] = round(max(p[1] for p in parts[2]) - min(p[1] for p in parts[2]), 4)
    line["route1_ahead_by_ms"] = round(line["route2_unit_list"]["build_ms"] - line["route1_text_list"]["build_ms"], 3)
    line["ratio_to_overlap_build"] = round(min(line["route1_text_list"]["build_ms"], line["route2_unit_list"]["build_ms"]) / line["overlap_build_ms"], 3)
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
    from overlap_bench import shapes
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    lines = [measure(name, texts, a.repeat) for name, texts in shapes(a.shapes.split(","))]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump({"tool": "tools/passages_bench.py", "device_ms": "the library's events around its own work",
                       "shapes": lines}, f, indent=1, ensure_ascii=False)
            f.write("\n")


if __name__ == "__main__":
    main()
