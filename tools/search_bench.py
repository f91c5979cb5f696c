#!/usr/bin/env python3
"""Index search on the device against the route without it: run_index plus the host
evaluation of the same queries.

For each input (the whole of Hamlet, synth1m = gen_text(lines=1_000_000)) and each batch

  two_frequent   the two most frequent words, `all`
  rare_frequent  a word of count 1 and the most frequent word, `all`
  eight_any      the eight most frequent words, `any`
  mixed_1024     1024 queries of 1-8 words drawn from the 2000 most frequent, both modes

on one warm engine per input and with the variants alternating inside one process:

  (a) run_search       the word job, the index stage and the search stage on the device
                       (csrc/kernels/search.hip); search_ms is the job's own device events
  (b) index + host     Engine.run_index() (postings and records cross PCIe), then
                       IndexResult.search() on the host
  (c) search_resident  the batch alone from the index (a) left on the device

Host timers around whole calls (every call ends with the job's own device synchronisation).
Per block of --iters rounds the median of each variant; the table gives the median of the
block medians and their spread (min .. max over the blocks).  (a) is checked against (b)
before anything is timed.  One JSON line per input and batch, and a markdown table.

  python tools/search_bench.py [--blocks 5] [--iters 7] [--only hamlet|synth1m] [--skip-synth]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import locust_amd as lc  # noqa: E402

_C = lc._C


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def batches(entries):
    by_count = sorted(entries, key=lambda e: (-e[2], e[0]))
    freq = [k for k, _v, _c in by_count]
    rare = [k for k, _v, c in by_count if c == 1][0]
    rng = random.Random(1)
    pool = freq[:2000]
    mixed = [[rng.choice(pool) for _ in range(rng.randrange(1, 9))] for _ in range(1024)]
    return [
        ("two_frequent", [freq[:2]], [0]),
        ("rare_frequent", [[rare, freq[0]]], [0]),
        ("eight_any", [freq[:8]], [1]),
        ("mixed_1024", mixed, [rng.randrange(2) for _ in mixed]),
    ]


def measure(name, data, blocks, iters, warm):
    eng = _C.GpuEngine(lc.make_config("gpu"), len(data), _C.count_lines(data))
    text = _C.HostText.from_bytes(data)  # pinned: no staging copy in any variant
    idx = eng.run_index_text(text)
    rows = []
    for bname, queries, flags in batches(idx.entries()):
        got = eng.run_search_text(text, queries, flags)
        ref = eng.run_index_text(text)._search(queries, flags)
        assert got.format() == ref.format(), f"{name}/{bname}: device and host answers differ"
        row = {"input": name, "batch": bname, "queries": len(queries), "tokens": got.num_tokens,
               "unique": got.num_unique, "hits": sum(got.hits()),
               "search_wire_bytes": got.wire_bytes, "index_wire_bytes": ref.wire_bytes,
               "blocks": blocks, "iters": iters}
        del got, ref
        for _ in range(warm):
            eng.run_search_text(text, queries, flags)
            eng.run_index_text(text)._search(queries, flags)
        keys = ("search_wall", "search_gpu", "search_stage", "host_wall", "host_eval",
                "resident_wall", "resident_stage")
        med = {k: [] for k in keys}
        for _ in range(blocks):
            t = {k: [] for k in keys}
            for _ in range(iters):
                ms, r = timed(lambda: eng.run_search_text(text, queries, flags))
                t["search_wall"].append(ms)
                t["search_gpu"].append(r.times()["gpu_ms"])
                t["search_stage"].append(r.search_ms)
                del r
                ms, r = timed(lambda: eng.search_resident(queries, flags))
                t["resident_wall"].append(ms)
                t["resident_stage"].append(r.search_ms)
                del r
                ms, r = timed(lambda: eng.run_index_text(text)._search(queries, flags))
                t["host_wall"].append(ms)
                t["host_eval"].append(r.search_ms)
                del r
            for k in keys:
                med[k].append(statistics.median(t[k]))
        for k, v in med.items():
            row[k + "_ms"] = round(statistics.median(v), 4)
            row[k + "_ms_min"] = round(min(v), 4)
            row[k + "_ms_max"] = round(max(v), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-synth", action="store_true")
    a = ap.parse_args()
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet, 5)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: _C.gen_text(lines=1_000_000), 2))
    rows = []
    for name, make, warm in inputs:
        if a.only and a.only != name:
            continue
        rows += measure(name, make(), a.blocks, a.iters, warm)

    print()
    print("| input | batch | hits | (a) run_search wall ms | (a) gpu_ms | (a) search_ms | "
          "(b) run_index + host search wall ms | (b) host evaluation ms | "
          "(c) search_resident wall ms | (c) search_ms | wire bytes (a) | wire bytes (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")

    def cell(r, key):
        return f"{r[key + '_ms']:.4g} ({r[key + '_ms_min']:.4g} .. {r[key + '_ms_max']:.4g})"

    for r in rows:
        print(f"| {r['input']} | {r['batch']} | {r['hits']} | {cell(r, 'search_wall')} | "
              f"{cell(r, 'search_gpu')} | {cell(r, 'search_stage')} | {cell(r, 'host_wall')} | "
              f"{cell(r, 'host_eval')} | {cell(r, 'resident_wall')} | "
              f"{cell(r, 'resident_stage')} | {r['search_wire_bytes']} | "
              f"{r['index_wire_bytes']} |")


if __name__ == "__main__":
    main()
