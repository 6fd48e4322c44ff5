#!/usr/bin/env python3
"""Timing of text-to-text relatedness (csrc/related.h, `east texts related`) on seeded prose-model texts
(east.synthetic.prose_like_texts): D texts of B bytes each, 42 x 16 KiB (the size of the reference's sample collection),
64 x 128 KiB, 256 x 128 KiB and -- with --large -- 64 x 1 MiB.  Per shape, after a warm-up build:

  related_ms        device time of the whole related build (east_hip_last_related_ms: the string directory with its one
                    read-back, every chunk's feed, walk and sums, the finish), median of --repeat builds, with min and max
  scores_per_s      scored strings x D over that time
  walk_ms           the yardstick: the SAME strings uploaded as one keyphrase list (east_hip_set_keyphrases) and scored by
                    one east_hip_score_resident (east_hip_last_score_ms, median, min, max) -- what the walk alone costs;
                    related_over_walk = related_ms / walk_ms is what the directory, the feed and the sums cost on top
  kernels_ms        one more build with the handle's per-kernel event profiler on (a pass of its own: events around every
                    launch slow the build down), summed per kernel, and the shares of the walk, the sums and the directory
  host_path_s       the smallest shape only: wall time of applications.texts_related with EAST_HIP_RELATED=host

--sweep D x B: the chunk budget swept over powers of two on that shape (east_hip_debug_set_related_chunk: strings =
budget / (8 D)), a median of --repeat builds each; the result is checked to be the same bytes under every budget.

The matrix of every shape is checked in the same run: byte-symmetric, NaN on the diagonal, values in [0, 1], and each
text's row ranked by the device = numpy's ranking of the fetched matrix.  One JSON line per case; --out writes them to a file
as well (profiles/related_bench.json).  For kernel times from the profiler of the platform, run the tool under it with
--shapes of one shape and --repeat 1.

    python tools/related_bench.py [--repeat 5] [--large] [--sweep 256x131072] [--out profiles/related_bench.json]
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

SHAPES = ((42, 16 << 10), (64, 128 << 10), (256, 128 << 10))
LARGE = (64, 1 << 20)
N = 10
DIRECTORY = ("rel_ends_kernel", "rel_lengths_kernel", "scan_reduce_kernel", "scan_apply_kernel")
SUMS = ("rel_reduce_kernel", "rel_fold_kernel", "rel_finish_kernel")
FEED = ("rel_feed_kernel",)


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def strings_of(index):
    """The scored strings of the index as one keyphrase list (q_symbols, q_offsets), out of its prepared symbols."""
    symbols, _, _ = index.prepared()
    term = symbols >= (0x80000000 if symbols.size and int(symbols[-1]) >> 31 else 0x0A00)
    kept = ~term & (symbols != 0x20)
    ends = np.flatnonzero(term)
    before = np.concatenate(([0], np.cumsum(kept)))
    offsets = np.concatenate(([0], before[ends + 1]))
    offsets = offsets[np.concatenate(([True], np.diff(offsets) > 0))]          # (a string without a symbol is not scored)
    return symbols[kept].astype(np.uint32), offsets.astype(np.int64)


def kernel_groups(kernels):
    def total(names):
        return sum(ms for name, ms in kernels.items() if any(name.startswith(n) or n in name for n in names))
    walk = total(("score_walk_kernel", "score_reduce_kernel", "kgram_", "query_map_kernel"))
    parts = {"walk": walk, "sums": total(SUMS), "directory": total(DIRECTORY), "feed": total(FEED)}
    whole = sum(kernels.values())
    return {k: round(v / whole, 4) if whole else None for k, v in parts.items()}


def check(index, D):
    matrix, own, scored = index.related_matrix()
    assert np.isnan(np.diag(matrix)).all() and matrix.tobytes() == matrix.T.copy().tobytes()
    off = matrix[~np.eye(D, dtype=bool)]
    assert (off >= 0.0).all() and (off <= 1.0).all() and (own >= 0.0).all() and (own <= 1.0 + 1e-12).all()
    found = index.rank_related(N)
    ranked = np.where(np.isnan(matrix), -np.inf, matrix)
    want = np.argsort(-ranked, axis=1, kind="stable")[:, :min(N, D - 1)]
    assert np.array_equal(found.index[:, :want.shape[1]], want)
    return matrix, own, scored


def measure(hip, D, doc_bytes, a, host_path):
    from east import synthetic
    texts = synthetic.prose_like_texts(np.random.default_rng(7), D, doc_bytes)
    index = hip.HipIndex()
    index.build_texts(texts)
    _, n_scored, launches = index.related_build(True, hip.RELATED_SYMMETRIC)        # the warm-up: the buffers are allocated here
    matrix, own, scored = check(index, D)
    related = []
    for _ in range(a.repeat):
        index.related_build(True, hip.RELATED_SYMMETRIC)
        related.append(index.last_related_ms())
    assert index.related_matrix()[0].tobytes() == matrix.tobytes()
    index.profile_enable(True)
    index.related_build(True, hip.RELATED_SYMMETRIC)
    kernels = {name: round(ms, 4) for name, (count, ms) in index.profile_report().items()}
    index.profile_enable(False)

    qs, qo = strings_of(index)
    assert qo.size - 1 == n_scored
    index.set_keyphrases(qs, qo)
    index.score_resident(True)                                                     # warm-up
    walk = []
    for _ in range(a.repeat):
        index.score_resident(True)
        walk.append(index.last_score_ms)
    r, w = statistics.median(related), statistics.median(walk)
    out = {"docs": D, "doc_bytes": doc_bytes, "symbols": int(index.info()["n_total"]), "scored_strings": n_scored,
           "score_launches": launches, "scores": n_scored * D, "related_ms": spread(related), "walk_ms": spread(walk),
           "scores_per_s": round(n_scored * D / (r * 1e-3), 1), "walk_scores_per_s": round(n_scored * D / (w * 1e-3), 1),
           "related_over_walk": round(r / w, 3), "kernels_ms": kernels, "kernel_shares": kernel_groups(kernels),
           "mean_relatedness": round(float(np.nanmean(matrix)), 6), "mean_self": round(float(own.mean()), 6), "repeat": a.repeat}
    index.close()
    if host_path:
        from east import applications, relevance
        named = {"t%d" % d: t for d, t in enumerate(texts)}
        os.environ["EAST_HIP_RELATED"] = "host"
        try:
            t0 = time.perf_counter()
            applications.texts_related(named, N, "symmetric", None, relevance.ASTRelevanceMeasure())
            out["host_path_s"] = round(time.perf_counter() - t0, 3)
        finally:
            del os.environ["EAST_HIP_RELATED"]
    return out


def sweep(hip, D, doc_bytes, a):
    from east import synthetic
    lib = hip.load()
    index = hip.HipIndex()
    index.build_texts(synthetic.prose_like_texts(np.random.default_rng(7), D, doc_bytes))
    rows, first = [], None
    try:
        for log2 in range(22, 33, 2):
            strings = max((1 << log2) // (8 * D), 1)
            lib.east_hip_debug_set_related_chunk(strings)
            _, n_scored, launches = index.related_build(True, hip.RELATED_SYMMETRIC)
            found = index.related_matrix()[0].tobytes()
            first = first or found
            assert found == first, "the matrix depends on the chunk"
            times = []
            for _ in range(a.repeat):
                index.related_build(True, hip.RELATED_SYMMETRIC)
                times.append(index.last_related_ms())
            rows.append({"chunk_table_bytes": 1 << log2, "chunk_strings": strings, "score_launches": launches, "related_ms": spread(times)})
    finally:
        lib.east_hip_debug_set_related_chunk(0)
    index.close()
    return {"sweep": True, "docs": D, "doc_bytes": doc_bytes, "scored_strings": n_scored, "budgets": rows, "repeat": a.repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="e.g. 42x16384,64x131072 (default: the three of the docstring)")
    ap.add_argument("--large", action="store_true", help="64 x 1 MiB as well")
    ap.add_argument("--sweep", default=None, help="D x bytes: sweep the chunk budget on that shape")
    ap.add_argument("--no-host-path", action="store_true")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (first: torch brings its own HIP runtime)
    except ImportError:
        pass
    from east import hip_backend
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    shapes = SHAPES + ((LARGE,) if a.large else ())
    if a.shapes:
        shapes = tuple(tuple(int(x) for x in s.split("x")) for s in a.shapes.split(","))
    smallest = min(shapes, key=lambda s: s[0] * s[1]) if shapes else None
    results = []
    for D, doc_bytes in shapes:
        results.append(measure(hip_backend, D, doc_bytes, a, (D, doc_bytes) == smallest and not a.no_host_path))
        print(json.dumps(results[-1]), flush=True)
    if a.sweep:
        D, doc_bytes = (int(x) for x in a.sweep.split("x"))
        results.append(sweep(hip_backend, D, doc_bytes, a))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/related_bench.py", "cases": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
