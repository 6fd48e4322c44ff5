#!/usr/bin/env python3
"""Kernel launches of the text front end (csrc/textfront.h, csrc/cosine.h) on four fixed inputs, as one JSON line
{input: {kernel: launches}} read through HipIndex.profile_report(): the streamed preparation and the preparation in one
piece of 16 MiB + three small texts, 40 separate texts of 300 KB through the pinned ring, and the cosine index of those.
A change that only moves host code leaves every count as it was (profiles/textfront_census.json).

    python tools/textfront_census.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from east import hip_backend, synthetic  # noqa: E402


def launches(build, texts, handle_of=lambda x: x):
    index = build()
    handle_of(index).profile_enable(True)
    index.build_texts(texts)
    return {k: int(v[0]) for k, v in sorted(handle_of(index).profile_report().items())}


def main():
    lib = hip_backend.load()
    text = synthetic.word_stream_document(np.random.default_rng(3), 16 << 20)[0]
    large = [text, text[: 1 << 20], b"", b"12 345 ab"]
    rng = np.random.default_rng(5)
    docs = [synthetic.word_stream_document(rng, 300000)[0] for _ in range(40)]
    out = {}
    for knob, name in ((-1, "16MiB_streamed"), (0, "16MiB_one_piece")):
        lib.east_hip_debug_set_text_stream(knob)
        out[name] = launches(hip_backend.HipIndex, large)
    lib.east_hip_debug_set_text_stream(-1)
    lib.east_hip_debug_set_text_ring(1, 0)
    out["40x300KB_ring"] = launches(hip_backend.HipIndex, docs)
    lib.east_hip_debug_set_text_ring(-1, 0)
    out["40x300KB_cosine"] = launches(hip_backend.HipCosineIndex, docs, lambda c: c.index)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
