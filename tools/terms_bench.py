#!/usr/bin/env python3
"""Timing of the characteristic terms (csrc/terms.h, `east texts terms`) on an MI355X: per shape the cosine index build it
starts from, the terms per text and of 12 average-linkage clusters, each with the pre-selection in front of the final sort
(east_hip_debug_set_terms_select 0) and without it (1), and the host path where it is short enough to wait for.

Shapes: the 30 texts of tests/golden/hse_config1.json; the Zipf stand-in 256 x 1 MiB of tools/cosine_bench.py; 4 096 texts
of 16 KiB of the same; the word stream 256 x 1 MiB of tools/cosine_bench.py (26.5 million distinct terms).

Device ms: the library's events around its own work, read-backs included; medians of --repeat builds with n = 10, tf-idf,
the words space.  entries / passing / sorted: out[4], out[5], out[6] of the build -- the distinct (group, unit) pairs, those
that pass min_texts = 1, those that reach the final sort.  The clusters' own build (matrix, linkage, cut) is not in the
terms' time.  One JSON line per shape on stdout, all of them as a list in --out.

    python tools/terms_bench.py [--repeat 5] [--shapes hse,zipf256,zipf4096,stream256] [--out profiles/terms_bench.json]
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
CLUSTERS = 12


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
    from east import applications, hip_backend, relevance
    lib = hip_backend.load()
    index = hip_backend.HipCosineIndex()
    index.build_texts(texts, ())                       # warm-up: allocations, code objects

    def build():
        index.build_texts(texts, ())
        return index.info()["build_us"] / 1e3

    runs = [build() for _ in range(repeat)]
    info = index.info()
    line = {"shape": name, "docs": len(texts), "bytes": sum(len(t) for t in texts), "terms": info["terms"],
            "postings": info["postings"], "index_build_ms": round(statistics.median(runs), 3), "n": 10, "repeat": repeat}
    index.texts_build(True)
    index.clusters_build(hip_backend.GRAPH_SOURCE_COSINE_TEXTS, "average")
    labels = index.clusters_cut(None, min(CLUSTERS, len(texts)))[0].tolist()
    roots = sorted(set(labels))
    groups = [roots.index(r) for r in labels]
    for tag, group, G in (("per_text", None, None), ("clusters", groups, len(roots))):
        row = {"groups": len(texts) if group is None else G}
        reference = None
        for mode, key in ((0, "select"), (1, "plain_sort")):
            assert lib.east_hip_debug_set_terms_select(mode) == 0
            try:
                index.terms(True, 10, 1, group, G)     # warm-up
                ms = []
                for _ in range(repeat):
                    found = index.terms(True, 10, 1, group, G)
                    ms.append(index.last_terms_ms())
            finally:
                lib.east_hip_debug_set_terms_select(0)
            row[key] = {"device_ms": round(statistics.median(ms), 3), "entries": found.info["entries"], "passing": found.info["passing"],
                        "sorted": found.info["sorted"], "radix_passes": found.info["radix_passes"], "launches": found.info["launches"]}
            result = (found.count.tobytes(), found.unit.tobytes(), found.value.tobytes())
            assert reference in (None, result), "the pre-selection changed the result"
            reference = result
        row["ratio_to_index_build"] = round(row["select"]["device_ms"] / line["index_build_ms"], 3)
        line[tag] = row
    if line["bytes"] <= HOST_MAX_BYTES:
        measure_ = relevance.CosineRelevanceMeasure("words", "tf-idf", stopwords=[])
        t0 = time.perf_counter()
        doc_units, number, _ = relevance.host_doc_units(texts, measure_, "english")
        applications._terms_on_host(doc_units, len(number), True, list(range(len(texts))), len(texts), 10, 1)
        line["host_path_per_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    else:
        line["host_path_per_text_ms"] = "not timed"
    index.close()
    print(json.dumps(line, ensure_ascii=False), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--shapes", default="hse,zipf256,zipf4096,stream256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_bench.json"))
    a = ap.parse_args()
    from east import hip_backend
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    lines = []
    for name, texts in shapes(a.shapes.split(",")):
        lines.append(measure(name, texts, a.repeat))
        with open(a.out, "w", encoding="utf-8") as f:      # (after every shape: a run cut short keeps what it measured)
            json.dump(lines, f, indent=1, ensure_ascii=False)
            f.write("\n")


if __name__ == "__main__":
    main()
