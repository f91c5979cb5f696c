#!/usr/bin/env python3
"""Ranked search against the unranked answer of the same batch, from the resident index.

For each input (the whole of Hamlet, synth1m = gen_text(lines=1_000_000)) the batches of
tools/search_bench.py

  two_frequent   the two most frequent words, `all`
  rare_frequent  a word of count 1 and the most frequent word, `all`
  eight_any      the eight most frequent words, `any`
  mixed_1024     1024 queries of 1-8 words drawn from the 2000 most frequent, both modes

on one warm engine per input, after one run_search, through search_resident

  (u) unranked     every matching line, ascending
  (r) rank=K       each query's best K lines with their scores (default K = 10)

alternating inside one process.  search_ms is the stage's own device events; the wall time
is a host timer around the call (every call ends with the stage's own synchronisation).  Per
block of --iters rounds the median of each variant; the table gives the median of the block
medians and their spread (min .. max over the blocks), the hits the stage sorted, the lines it
returned and the wire bytes of both.  (r) is checked against the host evaluation of the same
batch before anything is timed.  One JSON line per input and batch, and a markdown table.

--unranked-only measures (u) alone and needs no rank= in the tree it imports: with --root DIR
(a checkout of another commit, built) it gives that commit's figures for the same batches.
--profile VARIANT runs the batches --iters times in one variant (unranked | ranked) and
nothing else, or only the set-up all of them share (none: the index job and one run_search per
batch): the workloads of `rocprofv3 --kernel-trace --stats` runs, whose per-kernel totals
minus the set-up's, divided by --iters, are one call's kernels.  --batch NAME keeps one batch.

  python tools/rank_bench.py [--blocks 5] [--iters 9] [--rank 10] [--only hamlet|synth1m]
                             [--batch NAME] [--skip-synth] [--unranked-only] [--root DIR]
                             [--profile none|unranked|ranked]
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


def measure(lc, name, data, a):
    _C = lc._C
    eng = _C.GpuEngine(lc.make_config("gpu"), len(data), _C.count_lines(data))
    text = _C.HostText.from_bytes(data)  # pinned: no staging copy
    idx = eng.run_index_text(text)
    ranked = not a.unranked_only
    rows = []
    for bname, queries, flags in batches(idx.entries()):
        if a.batch and a.batch != bname:
            continue
        got = eng.run_search_text(text, queries, flags)
        if a.profile:
            del got
            for _ in range(a.iters if a.profile != "none" else 0):
                if a.profile == "ranked":
                    eng.search_resident(queries, flags, a.rank)
                else:
                    eng.search_resident(queries, flags)
            continue
        row = {"input": name, "batch": bname, "queries": len(queries), "tokens": got.num_tokens,
               "hits_sorted": sum(got.hits()), "unranked_lines": sum(got.hits()),
               "unranked_wire_bytes": eng.search_resident(queries, flags).wire_bytes,
               "blocks": a.blocks, "iters": a.iters}
        if ranked:
            top = eng.search_resident(queries, flags, a.rank)
            ref = idx._search(queries, flags, a.rank)
            assert top.format() == ref.format(), f"{name}/{bname}: device and host answers differ"
            assert sum(top.matches()) == sum(got.hits())
            row.update(rank_k=a.rank, ranked_lines=sum(top.hits()),
                       ranked_wire_bytes=top.wire_bytes)
            del top, ref
        del got
        variants = [("unranked", lambda: eng.search_resident(queries, flags))]
        if ranked:
            variants.append(("ranked", lambda: eng.search_resident(queries, flags, a.rank)))
        for _ in range(a.warm):
            for _v, fn in variants:
                fn()
        med = {v + k: [] for v, _f in variants for k in ("_search", "_wall")}
        for _ in range(a.blocks):
            t = {k: [] for k in med}
            for _ in range(a.iters):
                for v, fn in variants:
                    ms, r = timed(fn)
                    t[v + "_wall"].append(ms)
                    t[v + "_search"].append(r.search_ms)
                    del r
            for k in med:
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
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--unranked-only", action="store_true")
    ap.add_argument("--batch", default="")
    ap.add_argument("--profile", default="", choices=["", "none", "unranked", "ranked"])
    ap.add_argument("--root", default=ROOT, help="the built tree to import locust_amd from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import locust_amd as lc

    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: lc._C.gen_text(lines=1_000_000)))
    rows = []
    for name, make in inputs:
        if a.only and a.only != name:
            continue
        rows += measure(lc, name, make(), a)
    if a.profile:
        return

    def cell(r, key):
        return f"{r[key + '_ms']:.4g} ({r[key + '_ms_min']:.4g} .. {r[key + '_ms_max']:.4g})"

    print()
    if a.unranked_only:
        print("| input | batch | hits | unranked search_ms | unranked wall ms | wire bytes |")
        print("|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['input']} | {r['batch']} | {r['hits_sorted']} | "
                  f"{cell(r, 'unranked_search')} | {cell(r, 'unranked_wall')} | "
                  f"{r['unranked_wire_bytes']} |")
        return
    print("| input | batch | hits sorted | unranked search_ms | rank=K search_ms | "
          "unranked wall ms | rank=K wall ms | lines returned (u / r) | wire bytes (u / r) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['input']} | {r['batch']} | {r['hits_sorted']} | "
              f"{cell(r, 'unranked_search')} | {cell(r, 'ranked_search')} | "
              f"{cell(r, 'unranked_wall')} | {cell(r, 'ranked_wall')} | "
              f"{r['unranked_lines']} / {r['ranked_lines']} | "
              f"{r['unranked_wire_bytes']} / {r['ranked_wire_bytes']} |")


if __name__ == "__main__":
    main()
