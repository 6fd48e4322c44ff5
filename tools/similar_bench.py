#!/usr/bin/env python3
"""Timing of similar texts / similar keyphrases (csrc/similarity.h + csrc/top.h, `east keyphrases similar`) on synthetic
score tables with topic structure (east.synthetic.topic_score_table), K x D = 10 000 x 256 (BASELINE configs[2]),
30 000 x 256 and 10 000 x 4 096, by text and by keyphrase, n = 10, medians:

  (a) what a user did before this ran on the device: the K x D table copied from the device to the host, then
      p @ p.T, the normalisation by the roots of its diagonal, and np.argsort of every row.  Every step but the copy is
      linear in the number of rows, so for M above --host-rows (default 2 048) the first --host-rows rows are timed and the
      time is scaled by M / rows ("a_rows_timed" says how many were; 30 000 rows would hold the device for minutes);
  (b) the matrix built and ranked where the table lies: device ms (the library's events: similarity + ranking) and wall ms
      of the two calls with the fetch of the M x n result.

Checked in the same run: the ranked similarities of the timed rows against numpy's values at the same places, and for
M <= --check-members (default 10 000) the whole fetched matrix against numpy's, both to (2 L + 16) * 2^-53.
matrix_write_share = the M x M x 8 bytes of the matrix over the similarity's device time as a share of the 8 TB/s the HBM3E
of an MI355X is specified for; fp64_tflops = 2 x 64 x 64 x L per computed tile (the upper triangle of tiles) over the same
time.  One JSON line per case; --out writes them to a file as well (profiles/similar_bench.json).

    python tools/similar_bench.py [--repeat 5] [--out profiles/similar_bench.json]
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

SHAPES = ((10_000, 256), (30_000, 256), (10_000, 4_096))
N = 10
HBM_PEAK_BYTES_PER_S = 8.0e12


def device_to_host_ms(scores, repeat):
    """The copy of a K x D float64 table from device memory into pageable host memory, as the score call makes it."""
    import torch
    on_device = torch.from_numpy(scores).to("cuda:0")
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        host = on_device.cpu().numpy()
        times.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(host, scores)
    return statistics.median(times)


def host_rows(profiles, rows, n):
    """(a) for the first `rows` members: their rows of the similarity matrix and their n best others -> (S, index, ms)."""
    t0 = time.perf_counter()
    q = np.einsum("ml,ml->m", profiles, profiles)
    root = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (profiles[:rows] @ profiles.T) / (root[:rows, None] * root[None, :])
    S[(q[:rows] == 0.0)[:, None] | (q == 0.0)[None, :]] = 0.0
    S[np.arange(rows), np.arange(rows)] = -np.inf              # (never first: the member itself)
    index = np.argsort(-S, axis=1, kind="stable")[:, :n] if n else None     # (n = 0: the matrix alone, for the check)
    ms = (time.perf_counter() - t0) * 1e3
    S[np.arange(rows), np.arange(rows)] = np.nan
    return S, index, ms


def measure(index, scores, copy_ms, axis, a):
    K, D = scores.shape
    M, L = (D, K) if axis == 0 else (K, D)
    bound = (2 * L + 16) * 2.0 ** -53
    profiles = np.ascontiguousarray(scores.T if axis == 0 else scores)
    rows = min(M, a.host_rows)
    S_host, _, host_ms = host_rows(profiles, rows, N)

    index.similarity_from_uploaded(axis)                            # the warm-up of (b): its buffers are allocated here
    index.rank_similarity(N)
    sim_ms, top_ms, wall_ms = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        index.similarity_from_uploaded(axis)
        found = index.rank_similarity(N)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        sim_ms.append(index.last_similarity_ms)
        top_ms.append(index.last_top_ms)
    assert found.count.tolist() == [min(N, M - 1)] * M
    listed = np.take_along_axis(S_host, found.index[:rows, :found.count[0]].astype(np.int64), axis=1)
    ranked_error = float(np.abs(found.score[:rows, :found.count[0]] - listed).max())
    assert ranked_error <= bound, (ranked_error, bound)
    matrix_error = None
    if M <= a.check_members:
        S_dev, _ = index.similarity_matrix()
        S_all = S_host if rows == M else host_rows(profiles, M, 0)[0]
        assert np.isnan(np.diag(S_dev)).all()
        matrix_error = float(np.nanmax(np.abs(S_dev - S_all)))
        assert matrix_error <= bound, (matrix_error, bound)
        del S_dev, S_all

    index.profile_enable(True)
    index.similarity_from_uploaded(axis)
    index.rank_similarity(N)
    kernels = {name: round(ms, 4) for name, (count, ms) in index.profile_report().items()}
    index.profile_enable(False)

    tiles = (M + 63) // 64
    flops = 2.0 * 64 * 64 * L * tiles * (tiles + 1) / 2
    sim = statistics.median(sim_ms)
    a_total = copy_ms + host_ms * (M / rows)
    b = statistics.median(wall_ms)
    return {"keyphrases": K, "docs": D, "by": ("text", "keyphrase")[axis], "n": N, "members": M, "profile_length": L,
            "a_copy_to_host_ms": round(copy_ms, 3), "a_rows_timed": rows, "a_gram_normalise_argsort_ms": round(host_ms * (M / rows), 1),
            "a_total_ms": round(a_total, 1),
            "b_similarity_device_ms": round(sim, 4), "b_ranking_device_ms": round(statistics.median(top_ms), 4),
            "b_wall_with_fetch_ms": round(b, 3), "a_over_b": round(a_total / b, 1),
            "matrix_bytes": M * M * 8, "matrix_write_share": round(M * M * 8 / (sim * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
            "fp64_tflops": round(flops / (sim * 1e-3) / 1e12, 3),
            "bound": bound, "ranked_error": ranked_error, "matrix_error": matrix_error,
            "kernels_ms": kernels, "host_cpus": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(), "repeat": a.repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="e.g. 10000x256,30000x256 (default: the three of the docstring)")
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--check-members", type=int, default=10_000)
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (first: torch brings its own HIP runtime)
    except ImportError:
        pass
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    shapes = SHAPES if not a.shapes else tuple(tuple(int(x) for x in s.split("x")) for s in a.shapes.split(","))
    index = hip_backend.HipIndex()
    results = []
    for K, D in shapes:
        scores = synthetic.topic_score_table(np.random.default_rng(7), K, D)
        copy_ms = device_to_host_ms(scores, a.repeat)
        index.similarity_from_table(scores, 0)                       # the upload
        for axis in (0, 1):
            results.append(measure(index, scores, copy_ms, axis, a))
            print(json.dumps(results[-1]), flush=True)
    index.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/similar_bench.py", "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "cases": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
