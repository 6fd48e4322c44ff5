#!/usr/bin/env python3
"""Timing of complete and average linkage on the device (csrc/linkage.h, `east -j complete|average ... clusters`).  Cases:
random distinct weights at M = 256, 4 096 and 10 000; the zero plateau (tests/linkage_exact.py: 90 % exact +0.0) at 4 096
without a floor and with a floor of 0.1; the profile cosines of the keyphrases of a 10 000 x 256 score table with topic
structure (east.synthetic.topic_score_table, as tools/clusters_bench.py).  Per case and linkage, medians of --repeat after a
warm-up, with min and max:

  rounds, launches      of a build from the matrix where it lies (no symmetry check)
  build_ms              east_hip_last_clusters_ms of that build: the copy, the rounds, their read-backs, the ranking
  round_ms              build_ms / rounds
  single_build_ms       the single-linkage build of the same matrix: the yardstick
  kernels_ms            the handle's event profiler over one more build: per kernel (launches, total ms)
  best_full_read        lnk_best_kernel of a build whose floor (plus infinity) ends it after one round, in which every row is
                        alive: ms and the bytes/s of M^2 doubles
  host_route_s          fetching the matrix (uploaded cases: nothing to fetch) and scipy.cluster.hierarchy.linkage on 1 - s;
                        measured where M <= --host-members, else scaled from the largest measured case by M^2 and marked so;
                        left out of the cases with a floor

    python tools/linkage_bench.py [--repeat 5] [--sizes 256,4096,10000] [--out profiles/linkage_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINKAGES = ("complete", "average")


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def measure(name, index, source, M, repeat, host_matrix, host_members, last_host, floor=None):
    from east import hip_backend
    try:
        from scipy.cluster import hierarchy
    except ImportError:
        hierarchy = None
    single = []
    index.clusters_build(source)
    for _ in range(repeat):
        index.clusters_build(source)
        single.append(index.last_clusters_ms)
    cases = []
    for linkage in LINKAGES:
        index.clusters_build(source, linkage, floor)                  # warm-up
        build = []
        for _ in range(repeat):
            info = index.clusters_build(source, linkage, floor)
            build.append(index.last_clusters_ms)
        kernels = None                                                # (two events a launch: not over thousands of rounds)
        if info["rounds"] <= 500:
            index.profile_enable(True)
            index.clusters_build(source, linkage, floor)
            kernels = {k: (c, round(ms, 4)) for k, (c, ms) in index.profile_report().items() if k.startswith(("lnk_", "clu_"))}
            index.profile_enable(False)
        index.profile_enable(True)
        index.clusters_build(source, linkage, float("inf"))          # one round, every row alive, nothing merged
        full = index.profile_report().get("lnk_best_kernel", (0, 0.0))[1]
        index.profile_enable(False)
        index.clusters_build(source, linkage, floor)                  # (the result the host route is compared with)
        rounds = max(info["rounds"], 1)
        case = {"case": name, "linkage": linkage, "floor": floor, "members": M, "merges": info["merges"], "rounds": info["rounds"],
                "launches": info["launches"], "build_ms": spread(build), "round_ms": spread([b / rounds for b in build]),
                "single_build_ms": spread(single), "kernels_ms": kernels,
                "best_full_read": {"ms": round(full, 4), "bytes_per_s": round(M * M * 8.0 / (full * 1e-3), 0) if full > 0 else None},
                "repeat": repeat}
        key = (linkage,)
        if hierarchy is not None and M <= host_members and floor is None:
            t0 = time.perf_counter()
            S = host_matrix()
            Z = hierarchy.linkage(1.0 - S[np.triu_indices(M, 1)], linkage)
            case["host_route_s"] = round(time.perf_counter() - t0, 3)
            heights = 1.0 - index.clusters_merges()[2]
            case["largest_height_difference_to_scipy"] = float(np.max(np.abs(np.sort(heights) - Z[:, 2])))
            last_host[key] = (M, case["host_route_s"])
        elif key in last_host and floor is None:                      # (a floored host route was not timed: no figure)
            m0, s0 = last_host[key]
            case["host_route_s"] = round(s0 * (M * M) / float(m0 * m0), 2)
            case["host_route_scaled_from"] = m0
        print(json.dumps(case), flush=True)
        cases.append(case)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sizes", default="256,4096,10000")
    ap.add_argument("--host-members", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import linkage_exact
    from clusters_bench import random_distinct
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    rng = np.random.default_rng(16)
    index = hip_backend.HipIndex()
    cases, last_host = [], {}
    uploaded = hip_backend.GRAPH_SOURCE_UPLOADED
    for M in sorted(int(x) for x in a.sizes.split(",")):
        S = random_distinct(rng, M)
        index.clusters_build_host(S)
        cases += measure("distinct_%d" % M, index, uploaded, M, a.repeat, lambda: S, a.host_members, last_host)
        del S
    S = linkage_exact.family("zero_plateau", 4096)
    index.clusters_build_host(S)
    cases += measure("zero_plateau_4096", index, uploaded, 4096, a.repeat, lambda: S, a.host_members, last_host)
    cases += measure("zero_plateau_4096_floor_0.1", index, uploaded, 4096, a.repeat, lambda: S, a.host_members, last_host, floor=0.1)
    scores = synthetic.topic_score_table(rng, 10000, 256)
    index.similarity_from_table(scores, hip_backend.TOP_BY_KEYPHRASE)
    fetched = index.similarity_matrix()[0]
    np.fill_diagonal(fetched, 0.0)
    finite = bool(np.isfinite(fetched).all())
    del fetched
    if finite:
        cases += measure("similarity_10000x256_by_keyphrase", index, hip_backend.GRAPH_SOURCE_SIMILARITY, 10000, a.repeat,
                         lambda: index.similarity_matrix()[0], a.host_members, last_host)
    else:
        print(json.dumps({"case": "similarity_10000x256_by_keyphrase", "skipped": "the matrix has NaN off the diagonal"}), flush=True)
    index.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/linkage_bench.py", "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
