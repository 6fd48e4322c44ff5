#!/usr/bin/env python3
"""Timing of phrase extraction (csrc/phrases.h, `east keyphrases extract`) on an MI355X: per shape the cosine index build it
starts from, the extraction at the defaults (max_words 3, min_count 2) and with eight levels, per level its domain, its
survivors and its time, the ratio to the index build, and the host path where it is short enough to wait for.

Shapes: the 30 texts of tests/golden/hse_config1.json; the Zipf stand-in 256 x 1 MiB of tools/cosine_bench.py; 4 096 texts
of 16 KiB of the same; a 64 MiB uniform word stream (almost no repeats: the domain collapses behind level 2).

Device ms: the library's events around its own work, read-backs between the levels included.  The time of level n is the
median build cut at max_words = n minus the median build cut at n - 1 (a level's emission moves with the cut: the levels
add up to the whole build, a single one is good to a few per cent).  One JSON line per shape.

    python tools/phrases_bench.py [--repeat 5] [--shapes hse,zipf256,zipf4096,stream64] [--index-only]

--index-only: the cosine index build alone (the A/B of two libraries: EAST_HIP_LIBRARY names the one to load).
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

HOST_MAX_BYTES = 8 << 20            # the host path is timed up to here (it takes minutes beyond)


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
        elif name == "stream64":
            yield "word_stream_64MiB", [word_stream_text(rng, 64 << 20)]
        else:
            raise SystemExit("unknown shape %r" % name)


def median_ms(run, repeat):
    return statistics.median(run() for _ in range(repeat))


def measure(name, texts, repeat, index_only):
    from east import applications, hip_backend
    index = hip_backend.HipCosineIndex()
    index.build_texts(texts, ())                       # warm-up: allocations, code objects

    def build():
        index.build_texts(texts, ())
        return index.info()["build_us"] / 1e3

    runs = [build() for _ in range(repeat)]
    info = index.info()
    line = {"shape": name, "docs": len(texts), "bytes": sum(len(t) for t in texts), "kept_tokens": info["kept_tokens"],
            "terms": info["terms"], "index_build_ms": round(statistics.median(runs), 3), "index_build_runs_ms": [round(r, 3) for r in runs],
            "library": os.path.basename(hip_backend.LIB_PATH), "repeat": repeat}
    if not index_only:
        index.phrases()                                # warm-up

        def extract(**params):
            def run():
                index.phrases(**params)
                return index.last_phrases_ms
            return run

        for tag, max_words in (("defaults", 3), ("eight_levels", 8)):
            whole = median_ms(extract(max_words=max_words), repeat)
            found = index.phrases(max_words=max_words)
            cuts = [median_ms(extract(max_words=n), repeat) for n in range(1, found.levels + 1)]
            line[tag] = {"max_words": max_words, "min_count": 2, "build_ms": round(whole, 3), "candidates": found.candidates,
                         "levels_run": found.levels, "ratio_to_index_build": round(whole / line["index_build_ms"], 3),
                         "levels": [{"words": n + 1, "domain": int(found.domain[n]), "survivors": int(found.survivors[n]),
                                     "ms": round(cuts[n] - (cuts[n - 1] if n else 0.0), 3)} for n in range(found.levels)]}
        line["top"] = index.phrases(n=5).strings()
        if line["bytes"] <= HOST_MAX_BYTES:
            t0 = time.perf_counter()
            rows, _ = applications._phrases_on_host(texts, frozenset(), 0, 3, 1, 2, 1)
            line["host_path_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert [r[0] for r in rows] == index.phrases().strings()
        else:
            line["host_path_ms"] = "not timed"
    index.close()
    print(json.dumps(line, ensure_ascii=False), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="hse,zipf256,zipf4096,stream64")
    ap.add_argument("--index-only", action="store_true")
    a = ap.parse_args()
    from east import hip_backend
    if a.index_only:
        # (a library from before the phrases, or before a later consumer, exports none of their entry points: the index
        # build needs none)
        import ctypes
        lib = ctypes.CDLL(hip_backend.LIB_PATH)
        for entry in [e for e in hip_backend.SIGNATURES if not hasattr(lib, e)]:
            del hip_backend.SIGNATURES[entry]
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    for name, texts in shapes(a.shapes.split(",")):
        measure(name, texts, a.repeat, a.index_only)


if __name__ == "__main__":
    main()
