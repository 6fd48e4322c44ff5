#!/usr/bin/env python3
"""Timing of the single-linkage clusters (csrc/clusters.h, `east texts clusters` / `east keyphrases clusters`).  Cases:
random distinct weights at M = 256, 4 096, 10 000 and -- where the device and the host hold 7.2 GB -- 30 000; the all-equal
and the hierarchy family (tests/clusters_exact.py) at 4 096; the profile cosines of the keyphrases of a 10 000 x 256 score
table with topic structure (east.synthetic.topic_score_table, as tools/similar_bench.py).  Per case, medians of --repeat after
a warm-up, with min and max:

  rounds, launches      of a build from the matrix where it lies (no symmetry check)
  build_ms              east_hip_last_clusters_ms of that build: the rounds, their read-backs, the ranking of the merges
  round_ms              build_ms / rounds
  row_read_ms           east_hip_last_top_ms of east_hip_top_build_resident by row (n = 10) on the same matrix: one
                        coalesced read of M^2 doubles, the yardstick of "a round is about one read of the matrix"
  round_over_row_read   round_ms / row_read_ms
  kernels_ms            the handle's event profiler over one more build: per kernel (launches, total ms)
  host_route_s          fetching the matrix (uploaded cases: nothing to fetch) and numpy's sort plus Kruskal as
                        east.applications runs it; measured where M <= --host-members, else scaled from the largest measured
                        case by M^2 log M and marked "scaled"

    python tools/clusters_bench.py [--repeat 5] [--sizes 256,4096,10000,30000] [--out profiles/clusters_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def random_distinct(rng, M):
    """Symmetric, NaN on the diagonal, (almost surely) distinct weights; mirrored block by block, without a second M x M
    temporary."""
    S = rng.random((M, M))
    B = 2048
    for i in range(0, M, B):
        S[i:i + B, i + B:] = S[i + B:, i:i + B].T
        S[i:i + B, i:i + B] = np.maximum(S[i:i + B, i:i + B], S[i:i + B, i:i + B].T)
    np.fill_diagonal(S, np.nan)
    return S


def measure(name, index, source, M, repeat, host_matrix, host_members, last_host):
    from east import applications, hip_backend
    index.clusters_build(source)                                      # warm-up
    if source == hip_backend.GRAPH_SOURCE_UPLOADED:                   # (the ranking reads an uploaded copy of its OWN)
        index.top_from_table(host_matrix(), hip_backend.TOP_BY_KEYPHRASE, 10)
    build, row = [], []
    for _ in range(repeat):
        info = index.clusters_build(source)
        build.append(index.last_clusters_ms)
        hip_backend._top_build(index._lib, index._h, source, None, hip_backend.TOP_BY_KEYPHRASE, 10, -np.inf)
        row.append(index.last_top_ms)
    index.profile_enable(True)
    index.clusters_build(source)
    kernels = {k: (c, round(ms, 4)) for k, (c, ms) in index.profile_report().items() if k.startswith("clu_")}
    index.profile_enable(False)
    rounds = max(info["rounds"], 1)
    case = {"case": name, "members": M, "merges": info["merges"], "rounds": info["rounds"], "launches": info["launches"],
            "build_ms": spread(build), "round_ms": spread([b / rounds for b in build]), "row_read_ms": spread(row),
            "round_over_row_read": round(statistics.median(build) / rounds / statistics.median(row), 3), "kernels_ms": kernels,
            "repeat": repeat}
    if M <= host_members:
        t0 = time.perf_counter()
        S = host_matrix()
        merges = applications._single_linkage(S)
        case["host_route_s"] = round(time.perf_counter() - t0, 3)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(merges, index.clusters_merges())), name
        last_host[:] = [M, case["host_route_s"]]
    elif last_host:
        m0, s0 = last_host
        case["host_route_s"] = round(s0 * (M * M * math.log(M)) / (m0 * m0 * math.log(m0)), 1)
        case["host_route_scaled_from"] = m0
    print(json.dumps(case), flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sizes", default="256,4096,10000,30000")
    ap.add_argument("--host-members", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import clusters_exact
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    rng = np.random.default_rng(16)
    index = hip_backend.HipIndex()
    cases, last_host = [], []
    for M in sorted(int(x) for x in a.sizes.split(",")):
        try:
            S = random_distinct(rng, M)
            index.clusters_build_host(S)
        except (MemoryError, hip_backend.exceptions.HipBackendError) as e:
            print(json.dumps({"case": "distinct_%d" % M, "skipped": str(e)}), flush=True)
            continue
        cases.append(measure("distinct_%d" % M, index, hip_backend.GRAPH_SOURCE_UPLOADED, M, a.repeat, lambda: S, a.host_members, last_host))
        del S
    for family in ("equal", "hierarchy"):
        S = clusters_exact.family(family, 4096)
        index.clusters_build_host(S)
        cases.append(measure("%s_4096" % family, index, hip_backend.GRAPH_SOURCE_UPLOADED, 4096, a.repeat, lambda: S, a.host_members, last_host))
    scores = synthetic.topic_score_table(rng, 10000, 256)
    index.similarity_from_table(scores, hip_backend.TOP_BY_KEYPHRASE)
    cases.append(measure("similarity_10000x256_by_keyphrase", index, hip_backend.GRAPH_SOURCE_SIMILARITY, 10000, a.repeat,
                         lambda: index.similarity_matrix()[0], a.host_members, last_host))
    index.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/clusters_bench.py", "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
