#!/usr/bin/env python3
"""Timing of the BM25 score call (csrc/bm25.h, `east -s bm25`) against its yardstick, the tf-idf cosine score call
(east_hip_cosine_score_table) on the SAME index and the SAME queries, in the same process, alternating.  Collections: the
Zipf stand-in of tools/cosine_bench.py at 256 texts x 1 MiB and at 4 096 texts x 16 KiB, and the 30 sample texts (HSE
config 1); 10 000 keyphrases of one to three words of the texts (the sample texts: their own 10 and 10 000 drawn).  Device
ms: the library's events around its launches (east_hip_cosine_info: score_us), the median of --repeat calls; the first BM25
call of an index -- the one that also makes the weights -- is listed separately, as is the first cosine call.  The result
goes to profiles/bm25_bench.json (--out), one record a collection.

    python tools/bm25_bench.py [--repeat 5] [--keyphrases 10000] [--out profiles/bm25_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ast-text-analysis_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def measure(name, texts, keyphrases, repeat):
    from east import relevance, utils
    prepared = [utils.prepare_text(k) for k in keyphrases]
    m = relevance.BM25RelevanceMeasure("words", stopwords=[])
    m.set_text_collection(texts)
    ids, offsets = m._query_ids(prepared)
    index = m.index

    def bm25():
        index.bm25_table(ids, offsets, m.k1, m.b, fetch=False)
        return index.info()["score_us"] / 1e3

    def cosine():
        index.score_table(ids, offsets, True, fetch=False)
        return index.info()["score_us"] / 1e3

    first_bm25, first_cosine = bm25(), cosine()           # (each makes its weights; the BM25 one also reads N back)
    bm, cs = [], []
    for _ in range(repeat):
        bm.append(bm25())
        cs.append(cosine())
    assert index.bm25_info()["weights_computed"] == 1
    table = index.bm25_table(ids, offsets, m.k1, m.b)
    info = index.info()
    b, c = statistics.median(bm), statistics.median(cs)
    return {"shape": name, "docs": len(texts), "bytes": sum(len(t) for t in texts), "keyphrases": len(keyphrases),
            "query_tokens": int(ids.size), "terms": info["terms"], "postings": info["postings"],
            "table_bytes": int(table.size) * 8, "scores_above_zero": int((table > 0).sum()),
            "bm25_score_device_ms": round(b, 4), "bm25_first_call_device_ms": round(first_bm25, 4),
            "bm25_weights_pass_device_ms": round(first_bm25 - b, 4),
            "cosine_tfidf_score_device_ms": round(c, 4), "cosine_first_call_device_ms": round(first_cosine, 4),
            "bm25_over_cosine": round(b / c, 4) if c > 0 else None,
            "bm25_all_ms": [round(x, 4) for x in bm], "cosine_all_ms": [round(x, 4) for x in cs], "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--keyphrases", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_bench.json"))
    a = ap.parse_args()
    from cosine_bench import keyphrases_from, zipf_text
    from east import hip_backend, synthetic
    assert hip_backend.device_count() >= 1, "no HIP device (there is no CPU fallback)"
    rng = np.random.default_rng(2)
    vocab = synthetic.zipf_vocabulary(rng)
    records = []
    for name, n_texts, n_bytes in (("zipf_256x1MiB", 256, 1 << 20), ("zipf_4096x16KiB", 4096, 16 << 10)):
        texts = [zipf_text(rng, n_bytes, vocab) for _ in range(n_texts)]
        records.append(measure(name, texts, keyphrases_from(rng, texts, a.keyphrases), a.repeat))
        print(json.dumps(records[-1]), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "hse_config1.json"), encoding="utf-8") as f:
        hse = json.load(f)
    texts = [hse["texts"][n].encode("utf-8") for n in sorted(hse["texts"])]
    for name, keyphrases in (("hse_config1_own_keyphrases", hse["keyphrases"]), ("hse_config1", keyphrases_from(rng, texts, a.keyphrases))):
        records.append(measure(name, texts, keyphrases, a.repeat))
        print(json.dumps(records[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bm25_bench.py", "device": "MI355X (gfx950)", "records": records}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
