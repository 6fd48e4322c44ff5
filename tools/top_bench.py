#!/usr/bin/env python3
"""Timing of the ranked keyphrases (csrc/top.h, `east keyphrases top`) on synthetic score tables with topic structure
(east.synthetic.topic_score_table), K x D = 10 000 x 256 (BASELINE configs[2]), 30 000 x 256 and 10 000 x 4 096, by text
and by keyphrase, n = 10 and n = 100, medians:

  (a) what a user did before the selection ran on the device: the K x D table copied from the device to the host, then
      np.argsort(-scores, axis=..., kind="stable")[..., :n] over it;
  (b) the selection on the table where it lies in device memory: device ms (the library's events around the two kernels
      and the read-back of the counts) and wall ms of the call with the fetch of the three arrays.

The result of (b) is compared with (a)'s indices.  hbm_share = the table's bytes, read once, over the device time, as a
share of the 8 TB/s the HBM3E of an MI355X is specified for: the selection cannot be faster than one read of the table.
The per-kernel split comes from the library's profiler (one more build with it switched on).  One JSON line per case;
--out writes them to a file as well (profiles/top_bench.json).

    python tools/top_bench.py [--repeat 5] [--out profiles/top_bench.json]
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
NS = (10, 100)
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


def measure(index, scores, copy_ms, axis, n, repeat):
    K, D = scores.shape
    host_ms = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        if axis == 0:
            want = np.argsort(-scores, axis=0, kind="stable")[:n].T
        else:
            want = np.argsort(-scores, axis=1, kind="stable")[:, :n]
        host_ms.append((time.perf_counter() - t0) * 1e3)

    index.top_from_uploaded(axis, n)                                 # the warm-up of (b): its buffers are allocated here
    dev_ms, wall_ms = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        found = index.top_from_uploaded(axis, n)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(index.last_top_ms)
    assert np.array_equal(found.index, want), "the device ranking differs from the stable argsort"

    index.profile_enable(True)
    index.top_from_uploaded(axis, n)
    kernels = {name: round(ms, 4) for name, (count, ms) in index.profile_report().items()}
    index.profile_enable(False)

    a = copy_ms + statistics.median(host_ms)
    b, dev = statistics.median(wall_ms), statistics.median(dev_ms)
    return {"keyphrases": K, "docs": D, "by": ("text", "keyphrase")[axis], "n": n,
            "a_copy_to_host_ms": round(copy_ms, 3), "a_argsort_ms": round(statistics.median(host_ms), 1), "a_total_ms": round(a, 1),
            "b_device_ms": round(dev, 4), "b_wall_with_fetch_ms": round(b, 3), "a_over_b": round(a / b, 1),
            "table_bytes": int(scores.nbytes), "hbm_share": round(scores.nbytes / (dev * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
            "kernels_ms": kernels, "host_cpus": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(), "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="e.g. 10000x256,30000x256 (default: the three of the docstring)")
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
        index.top_from_table(scores, 0, 1)                           # the upload
        for axis in (0, 1):
            for n in NS:
                results.append(measure(index, scores, copy_ms, axis, n, a.repeat))
                print(json.dumps(results[-1]), flush=True)
    index.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/top_bench.py", "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "cases": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
