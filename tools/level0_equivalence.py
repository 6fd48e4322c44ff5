#!/usr/bin/env python3
"""The host decisions of the level-0 driver (csrc/level0.h), one library against another.

A fixed list of small builds runs once per library, each library in a fresh child process (EAST_HIP_LIBRARY selects it,
EAST_HIP_TRACE=1, the in-library profiler on, a time limit of its own).  Per build the child records every field of
east_hip_build_info and the launches per kernel name of east_hip_profile_report; the parent process adds the [east_hip]
trace lines the build wrote, without those that carry a time.  The list is chosen so that the PARENT's record alone shows
every branch of the driver at least once (COVERAGE below, asserted before anything is compared); then all three must be
equal between the two libraries, build by build.  With --bench-runs R, bench.py runs R times per library, alternating,
and every figure of the new library's lines is set against the range the parent's own runs span.

    python tools/level0_equivalence.py --parent libeast_hip_parent.so --new ast-text-analysis_amd/east/_lib/libeast_hip.so \\
        [--bench-runs 3] [--out profiles/level0_driver_refactor.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ast-text-analysis_amd"))
TERM = 0x0A00
CHILD_SECONDS = 240
BENCH_SECONDS = 300
MARK = "[level0_equivalence] build "


# ---- the builds -------------------------------------------------------------------------------------------------
def _one(sym, m=1):
    return [np.asarray(sym, dtype=np.uint32)], [m]


def _letters(rng, n, sigma=26):
    return rng.integers(65, 65 + sigma, size=n, dtype=np.uint32)


def _with_terminator(parts):
    return np.concatenate(list(parts) + [np.array([TERM], dtype=np.uint32)]).astype(np.uint32)


def builds():
    """[(name, handle, knobs, (symbols per document, strings per document))]; knobs: window_sort, seg, lds_rounds, persist."""
    from east import synthetic
    rng = np.random.default_rng(2026)
    vocab = synthetic.zipf_vocabulary(rng, size=200, exponent=1.0)
    words = lambda n: _one(*synthetic.word_stream_document(rng, n, want_text=False)[1:])
    zipf = _one(*synthetic.zipf_document(rng, 300000, vocab))
    zipf_big = _one(*synthetic.zipf_document(rng, 1500000, vocab))
    w300, w300b, w100, small = words(300000), words(300000), words(100000), words(3000)
    eight = [synthetic.word_stream_document(rng, 40000, want_text=False)[1:] for _ in range(8)]
    eight = ([d[0] for d in eight], [d[1] for d in eight])
    passage = _letters(rng, 5000)
    twice = _one(_with_terminator([_letters(rng, 100000), passage, _letters(rng, 100000), passage, _letters(rng, 1000)]))
    p600 = _letters(rng, 600)
    ten = _one(_with_terminator([np.concatenate([p600, _letters(rng, 15000)]) for _ in range(10)]))
    copies = _one(*synthetic.worst_case_collection(rng, 100, 1000))
    run = _one(_with_terminator([_letters(rng, 20000), np.full(100000, 65, dtype=np.uint32)]))
    abc = _one(_with_terminator([np.tile(np.array([65, 66, 67], dtype=np.uint32), 40000)]))
    mixed = _one(_with_terminator([zipf[0][0][zipf[0][0] < TERM], np.tile(np.array([65, 66, 67], dtype=np.uint32), 5000)]))
    out = []
    add = lambda name, handle, data, **knobs: out.append((name, handle, knobs, data))
    # one handle: a first build, a speculative build that confirms its guess, one that is repeated
    add("words, first build", "A", w300)
    add("words again: speculative, confirmed", "A", w300b)
    add("zipf behind words: speculative, repeated", "A", zipf)
    # the key plans
    add("words, 64-bit keys", None, w300, window_sort=3)
    add("words, no fused finish", None, w300, window_sort=4)
    add("words, 64-bit keys, no fused finish", None, w300, window_sort=5)
    add("words, variable-length keys", None, w300, window_sort=7)
    add("words, variable-length keys, no fused finish", None, w300, window_sort=9)
    add("zipf, first build", None, zipf)
    add("zipf, fused finish forced", None, zipf, window_sort=6)
    add("zipf 1.5 M", None, zipf_big)
    add("zipf 1.5 M, rounds by the global sort", None, zipf_big, lds_rounds=0)
    add("zipf 1.5 M, stand-alone classification", None, zipf_big, lds_rounds=2)
    add("small input", None, small)
    add("small input, variable-length keys", None, small, window_sort=7)
    # several documents: the document number in the keys, the segmented sort
    add("eight documents, document number in the keys", None, eight, seg=0)
    add("eight documents, segmented", None, eight, seg=1)
    add("eight documents, variable-length keys under the document number", None, eight, seg=0, window_sort=7)
    add("eight documents, segmented, variable-length keys", None, eight, seg=1, window_sort=7)
    # long repeats
    add("a passage twice: the fused finish gives up", None, twice)
    add("a passage twice, no fused finish", None, twice, window_sort=4)
    add("ten copies of 600 symbols", None, ten)
    add("ten copies, no persistent launch", None, ten, lds_rounds=3)
    add("ten copies, rounds by the global sort", None, ten, lds_rounds=0)
    add("100 identical strings", None, copies)
    add("100 identical strings, large form", None, copies, persist=(1, 3))
    add("100 identical strings, no persistent launch", None, copies, lds_rounds=3)
    add("100 identical strings, variable-length 64-bit keys", None, copies, window_sort=7)
    add("a run of one letter", None, run)
    add("zipf and a period of three", None, mixed)
    add("zipf and a period of three, no persistent launch", None, mixed, lds_rounds=3)
    add("zipf and a period of three, variable-length 64-bit keys", None, mixed, window_sort=7)
    # lean, and DC3's sample sort on the byte stream
    add("zipf, lean", None, zipf, window_sort=2)
    add("words through DC3", None, w100, window_sort=0)
    add("a period of three through DC3", None, abc, window_sort=0)
    return out


def child(out_path):
    from east import hip_backend
    lib = hip_backend.load()
    handles, last, records = {}, {}, []
    anon = 0
    for name, handle, knobs, (syms, ms) in builds():
        lib.east_hip_debug_set_window_sort(knobs.get("window_sort", 1))
        lib.east_hip_debug_set_segmented_sort(knobs.get("seg", -1))
        lib.east_hip_debug_set_lds_rounds(knobs.get("lds_rounds", 1))
        lib.east_hip_debug_set_persist(*knobs.get("persist", (0, 0)))
        if handle is None:
            anon += 1
            handle = "#%d" % anon
        if handle not in handles:                   # (never closed before the end: no handle comes back out of the pool)
            handles[handle] = hip_backend.HipIndex()
            handles[handle].profile_enable()
        index = handles[handle]
        sys.stderr.write(MARK + name + "\n")
        sys.stderr.flush()
        sym = np.concatenate(syms)
        off = np.concatenate([[0], np.cumsum([s.size for s in syms])]).astype(np.int64)
        index.build(sym, off, np.array(ms, dtype=np.int32))
        index.synchronize()
        report = {k: v[0] for k, v in index.profile_report().items()}
        before = last.get(handle, {})
        launches = {k: c - before.get(k, 0) for k, c in sorted(report.items()) if c != before.get(k, 0)}
        last[handle] = report
        records.append({"name": name, "knobs": {k: list(v) if isinstance(v, tuple) else v for k, v in knobs.items()},
                        "info": index.info(), "launches": launches})
    with open(out_path, "w") as f:
        json.dump(records, f)


def run_child(library, tmp):
    env = dict(os.environ, EAST_HIP_LIBRARY=os.path.abspath(library), EAST_HIP_TRACE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=env, stderr=subprocess.PIPE,
                       timeout=CHILD_SECONDS, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("the builds with %s failed (exit status %d): nothing further is run" % (library, p.returncode))
    with open(tmp) as f:
        records = json.load(f)
    traces, cur = [], None
    for line in p.stderr.splitlines():
        if line.startswith(MARK):
            cur = []
            traces.append(cur)
        elif cur is not None and line.lstrip().startswith("[east_hip]") and not re.search(r"\b(ms|us)\b", line):
            cur.append(line)
    assert len(traces) == len(records), (len(traces), len(records))
    for r, t in zip(records, traces):
        r["trace"] = t
    return records


# ---- what the parent's record has to show -------------------------------------------------------------------------
def _keys(r):
    """(key bits, variable-length, fused finish) of every attempt at the first level of an all-suffix build."""
    return [(int(m.group(1)), bool(m.group(2)), int(m.group(3)))
            for m in (re.search(r"level-0 keys: (\d+)-bit.*?spare( \(variable-length\))?.*fused finish (\d)", l) for l in r["trace"]) if m]


def _any(r, pattern):
    return any(re.search(pattern, l) for l in r["trace"])


def _lds_rounds(r):
    return [(int(m.group(1)), int(m.group(2))) for m in (re.search(r"round \d+: (\d+) of (\d+) sorted in LDS", l) for l in r["trace"]) if m]


def _marks(r, fused):
    # (the sort marks the k-gram bucket starts on its way where the input is not small and the keys are of fixed width:
    # the placement pass does it, or the fused finish in its place)
    return (r["info"]["window_sorted"] == 1 and r["info"]["n_total"] > 65536 and r["info"]["ht_keys"] == 0 and
            r["info"]["fused_finish"] == fused and not _any(r, "fused finish gave up"))


def _endgame(r):
    # (a round's domain of at most 262 144 with no long repeat known and no persistent launch: ordered by the endgame's limits)
    if _any(r, "too long|persistent launch|prefix doubling"):
        return False
    return any(int(m.group(1)) <= 262144 for m in (re.search(r"round \d+: domain (\d+),", l) for l in r["trace"]) if m)


COVERAGE = [
    ("32-bit keys", lambda r: (32, False) in [k[:2] for k in _keys(r)]),
    ("64-bit keys", lambda r: (64, False) in [k[:2] for k in _keys(r)]),
    ("variable-length keys, 32-bit", lambda r: (32, True) in [k[:2] for k in _keys(r)]),
    ("variable-length keys, 64-bit", lambda r: (64, True) in [k[:2] for k in _keys(r)]),
    ("document number in the keys", lambda r: r["info"]["n_docs"] > 1 and _any(r, "level-0 keys.*segmented by document 0")),
    ("segmented sort", lambda r: r["info"]["seg_sort"] == 1 and _any(r, "level-0 keys.*segmented by document 1")),
    ("fused finish taken", lambda r: r["info"]["fused_finish"] == 1 and "lvl0_finish_kernel" in r["launches"]),
    # (words of the same size, with the same key layout and the same estimate, take it: "words, first build")
    ("fused finish refused by the sample", lambda r: r["name"] == "zipf, first build" and [k[2] for k in _keys(r)] == [0] and
     _any(r, "level-0 keys: 32-bit, w = 6 x 5 bits")),
    ("fused finish gave up", lambda r: _any(r, "fused finish gave up")),
    ("small input", lambda r: r["info"]["n_total"] <= 65536 and r["info"]["window_sorted"] == 1),
    ("k-gram marks by the placement pass", lambda r: _marks(r, 0) and "lvl0_place_kernel" in r["launches"]),
    ("k-gram marks by the fused finish", lambda r: _marks(r, 1)),
    ("repeat too long, first domain", lambda r: _any(r, r"level-0 \(all suffixes.*a repeat too long to order directly")),
    ("repeat too long, in a round", lambda r: _any(r, r"round \d+: domain.*a repeat too long to order directly")),
    ("switching to prefix doubling", lambda r: _any(r, "switching to prefix doubling")),
    ("persistent launch done, resident form", lambda r: _any(r, "persistent launch.*: done") and "refine_persist_kernel<4>" in r["launches"]),
    ("persistent launch done, large form", lambda r: _any(r, "persistent launch.*: done") and "refine_persist2_kernel" in r["launches"]),
    ("persistent launch bails", lambda r: _any(r, "a group too long for a tile")),
    ("round wholly in LDS", lambda r: any(a == b for a, b in _lds_rounds(r))),
    ("round partly in LDS", lambda r: any(0 < a < b for a, b in _lds_rounds(r))),
    ("round wholly by the global sort", lambda r: r["info"]["refine_rounds"] > 0 and r["info"]["lds_sorted"] == 0 and
     "dc3_refine_writeback_kernel" in r["launches"]),
    ("lds_rounds 0", lambda r: r["knobs"].get("lds_rounds") == 0 and r["info"]["refine_rounds"] > 0),
    ("lds_rounds 2", lambda r: r["knobs"].get("lds_rounds") == 2 and r["info"]["refine_rounds"] > 0),
    ("lds_rounds 3", lambda r: r["knobs"].get("lds_rounds") == 3 and r["info"]["refine_rounds"] > 0),
    ("endgame", _endgame),
    ("lean build", lambda r: r["knobs"].get("window_sort") == 2 and r["info"]["window_sorted"] == 0 and _any(r, "in large groups")),
    ("DC3 on the byte stream, names scattered", lambda r: _any(r, r"level-0 \(sample") and "dc3_scatter_names_kernel" in r["launches"]),
    ("speculative build confirmed", lambda r: r["info"]["first_hist_fused"] == 1 and not _any(r, "guessed wrong")),
    ("speculative build repeated", lambda r: _any(r, "speculative build guessed wrong: building again")),
]


def coverage(records):
    shown = {what: [r["name"] for r in records if test(r)] for what, test in COVERAGE}
    missing = [what for what, names in shown.items() if not names]
    return shown, missing


# ---- bench.py, alternating ----------------------------------------------------------------------------------------
def _figures(line, prefix=""):
    out = {}
    for k, v in line.items():
        if isinstance(v, bool):
            continue
        if isinstance(v, (int, float)) and re.search(r"ms|per_s|value", prefix + k):
            out[prefix + k] = float(v)
        elif isinstance(v, dict):
            out.update(_figures(v, prefix + k + "."))
    return out


def bench(libraries, order, steps, warmup):
    runs = {"P": [], "N": []}
    for which in order:
        env = dict(os.environ, EAST_HIP_LIBRARY=os.path.abspath(libraries[which]))
        env.pop("EAST_HIP_TRACE", None)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=BENCH_SECONDS, text=True, cwd=ROOT)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit("bench.py with library %s failed (exit status %d): nothing further is run" % (which, p.returncode))
        runs[which].append(_figures(json.loads(p.stdout.strip().splitlines()[-1])))
        print("bench", which, {k: runs[which][-1][k] for k in ("ms_per_step", "build_ms") if k in runs[which][-1]}, flush=True)
    verdicts = {}
    for k in sorted(runs["P"][0]):
        ps, ns = [r[k] for r in runs["P"] if k in r], [r[k] for r in runs["N"] if k in r]
        if not ns:
            continue
        verdicts[k] = {"P": ps, "N": ns, "inside": all(min(ps) <= x <= max(ps) for x in ns),
                       "median_inside": min(ps) <= float(np.median(ns)) <= max(ps)}
    return {"order": order, "steps": steps, "warmup": warmup, "figures": verdicts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="RECORD")
    ap.add_argument("--parent")
    ap.add_argument("--new")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level0_driver_refactor.json"))
    ap.add_argument("--bench-runs", type=int, default=0)
    ap.add_argument("--bench-order", default=None, help="e.g. NPPNNPPNNPPN (default: PN repeated --bench-runs times)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    tmp = args.out + ".child"
    result = {}
    try:
        parent = run_child(args.parent, tmp)
        shown, missing = coverage(parent)
        result["coverage_on_parent"] = shown
        for what, names in shown.items():
            print("%-45s %s" % (what, "; ".join(names) if names else "NOT SHOWN"))
        if missing:
            for r in parent:
                print("\n== %s %r\n%s\n%s" % (r["name"], r["knobs"], "\n".join(r["trace"]), json.dumps(r["info"])))
            raise SystemExit("the parent's record does not show: " + ", ".join(missing))
        new = run_child(args.new, tmp)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    differences = []
    for p, n in zip(parent, new):
        for part in ("info", "launches", "trace"):
            if p[part] != n[part]:
                differences.append({"build": p["name"], "what": part, "parent": p[part], "new": n[part]})
    result.update({"builds": len(parent), "info_fields": len(parent[0]["info"]), "equal": not differences,
                   "differences": differences, "record": parent})
    print("%d builds: %s" % (len(parent), "info, launches and trace EQUAL" if not differences else "%d DIFFERENCES" % len(differences)))
    if args.bench_runs and not differences:
        order = list(args.bench_order or "PN" * args.bench_runs)
        result["bench"] = bench({"P": args.parent, "N": args.new}, order, args.steps, args.warmup)
        outside = [k for k, v in result["bench"]["figures"].items() if not v["inside"]]
        print("bench: %d figures, outside the parent's range: %s" % (len(result["bench"]["figures"]), ", ".join(outside) or "none"))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if differences:
        raise SystemExit(json.dumps(differences[:3], indent=1)[:4000])


if __name__ == "__main__":
    main()
