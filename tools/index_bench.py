#!/usr/bin/env python3
"""The inverted-index job on the device against the word job and the CPU engine's index.

For each input (the whole of Hamlet, its lines 0-700, synth1m = gen_text(lines=1_000_000)),
on one warm engine per input and with the variants alternating inside one process:

  (a) word job   Engine.run(): the word counts only (the lean job where it applies)
  (b) run_index  the word job with its records left on the device, then the index stage
                 (csrc/kernels/index.hip); gpu_ms and index_ms are the job's own device
                 events, wall its host timer
  (c) cpu index  CpuWordCount::run_index on the same bytes (host timer)

Host timers around whole calls (every call ends with the job's own device synchronisation).
Per block of --iters rounds the median of each variant; the table gives the median of the
block medians and their spread (min .. max over the blocks).  The GPU index is checked
against the CPU engine's before anything is timed.  One JSON line per input and a markdown
table on stdout.

  python tools/index_bench.py [--blocks 5] [--iters 7] [--only hamlet|hamlet700|synth1m]
                              [--skip-synth] [--skip-cpu]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import locust_amd as lc  # noqa: E402
from locust_amd.utils import oracle  # noqa: E402

_C = lc._C


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, data, blocks, iters, warm, cpu_iters):
    eng = _C.GpuEngine(lc.make_config("gpu"), len(data), _C.count_lines(data))
    text = _C.HostText.from_bytes(data)  # pinned: no staging copy in any variant
    cpu_cfg = lc.make_config("cpu")
    got = eng.run_index_text(text)
    if cpu_iters:
        want = _C.cpu_run_index(cpu_cfg, data)
        assert got.entries() == want.entries(), f"{name}: entries differ from the CPU engine's"
        assert got.postings_bytes() == want.postings_bytes(), f"{name}: postings differ"
        del want
    row = {"input": name, "bytes": len(data), "lines": got.num_lines, "tokens": got.num_tokens,
           "unique": got.num_unique, "wire_bytes": got.wire_bytes, "blocks": blocks,
           "iters": iters}
    del got
    for _ in range(warm):
        eng.run_text(text)
        eng.run_index_text(text)
    keys = ("word_wall", "index_wall", "index_gpu", "index_stage")
    med = {k: [] for k in keys}
    for _ in range(blocks):
        t = {k: [] for k in keys}
        for _ in range(iters):
            ms, r = timed(lambda: eng.run_text(text))
            t["word_wall"].append(ms)
            del r
            ms, x = timed(lambda: eng.run_index_text(text))
            t["index_wall"].append(ms)
            t["index_gpu"].append(x.times()["gpu_ms"])
            t["index_stage"].append(x.index_ms)
            del x
        for k in keys:
            med[k].append(statistics.median(t[k]))
    for k, v in med.items():
        row[k + "_ms"] = round(statistics.median(v), 4)
        row[k + "_ms_min"] = round(min(v), 4)
        row[k + "_ms_max"] = round(max(v), 4)
    cpu = [timed(lambda: _C.cpu_run_index(cpu_cfg, data))[0] for _ in range(cpu_iters)]
    if cpu:
        row["cpu_index_ms"] = round(statistics.median(cpu), 4)
        row["cpu_index_ms_min"] = round(min(cpu), 4)
        row["cpu_index_ms_max"] = round(max(cpu), 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    a = ap.parse_args()
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet, 5, 5),
              ("hamlet700", lambda: oracle.window(hamlet, 0, 700), 5, 5)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: _C.gen_text(lines=1_000_000), 2, 2))
    rows = []
    for name, make, warm, cpu_iters in inputs:
        if a.only and a.only != name:
            continue
        rows.append(measure(name, make(), a.blocks, a.iters, warm,
                            0 if a.skip_cpu else cpu_iters))

    print()
    print("| input | tokens | distinct keys | (a) word job wall ms | (b) run_index wall ms | "
          "(b) gpu_ms | (b) index_ms | (c) cpu index ms | wire bytes (b) |")
    print("|---|---|---|---|---|---|---|---|---|")

    def cell(r, key):
        if key + "_ms" not in r:
            return "--"
        return f"{r[key + '_ms']:.4g} ({r[key + '_ms_min']:.4g} .. {r[key + '_ms_max']:.4g})"

    for r in rows:
        print(f"| {r['input']} | {r['tokens']} | {r['unique']} | {cell(r, 'word_wall')} | "
              f"{cell(r, 'index_wall')} | {cell(r, 'index_gpu')} | {cell(r, 'index_stage')} | "
              f"{cell(r, 'cpu_index')} | {r['wire_bytes']} |")


if __name__ == "__main__":
    main()
