#!/usr/bin/env python3
"""Proximity queries (`near`, within W tokens) on the device: what the verifier costs, and
that plain batches pay nothing for it.

Inputs are the whole of Hamlet and synth1m = gen_text(lines=1_000_000).  One warm engine
per input; every batch is answered by search_resident from the index one run_search left on
the device, the variants alternate inside one process, and the times are the jobs' own
device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

  (a) default  the same term lists as `all`, `phrase`, `near` W = 2 and `near` W = 5: the
               four have the same candidates (the `all` hits), so the differences are the
               verifiers and the sort and copy of the lines each of them keeps.  The batches:
               the two most frequent words, a rare and the most frequent word, and 256
               pairs drawn from the 200 most frequent words
  (b) --plain  plain batches, search_resident only: the four of tools/search_bench.py (`all`
               and `any`), the two most frequent words as a phrase and ranked (K = 10), and
               the widest one-letter prefix; run it from this tree and from a build of the
               parent commit (--root) in turn, and compare the difference with the
               parent-vs-parent spread of the same call
  (c) --once INPUT  the 256-pair `near` batch (W = 2) a few times, for a kernel trace:
               rocprofv3 --kernel-trace --stats

  python tools/near_bench.py [--blocks 5] [--iters 7] [--only hamlet|synth1m] [--skip-synth]
  python tools/near_bench.py --plain [--root TREE]
  python tools/near_bench.py --once synth1m

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, ANY, PHRASE, NEAR = 0, 1, 2, 3  # the native mode flags


def load(root):
    sys.path.insert(0, root)
    import locust_amd as lc
    return lc


def med_of_blocks(variants, blocks, iters):
    """variants: {name: callable -> SearchResult}; alternating; {name: (median, min, max)}."""
    med = {k: [] for k in variants}
    for _ in range(blocks):
        t = {k: [] for k in variants}
        for _ in range(iters):
            for k, fn in variants.items():
                t[k].append(fn().search_ms)
        for k in variants:
            med[k].append(statistics.median(t[k]))
    return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4))
            for k, v in med.items()}


def put(row, name, m):
    row[name + "_ms"], row[name + "_ms_min"], row[name + "_ms_max"] = m


def engine_for(lc, data):
    _C = lc._C
    eng = _C.GpuEngine(lc.make_config("gpu"), len(data), _C.count_lines(data))
    text = _C.HostText.from_bytes(data)
    return eng, text


def near_batches(entries):
    by_count = sorted(entries, key=lambda e: (-e[2], e[0]))
    freq = [k for k, _v, _c in by_count]
    rare = [k for k, _v, c in by_count if c == 1][0]
    rng = random.Random(1)
    return [("two_frequent", [freq[:2]]),
            ("rare_frequent", [[rare, freq[0]]]),
            ("pairs_256", [rng.sample(freq[:200], 2) for _ in range(256)])]


def measure(lc, name, data, blocks, iters):
    eng, text = engine_for(lc, data)
    entries = eng.run_index_text(text).entries()
    eng.run_search_text(text, [[entries[0][0]]], [ALL])  # leaves the index resident
    for bname, queries in near_batches(entries):
        n = len(queries)
        runs = {"all": lambda: eng.search_resident(queries, [ALL] * n),
                "phrase": lambda: eng.search_resident(queries, [PHRASE] * n),
                "near2": lambda: eng.search_resident(queries, [NEAR] * n, within=[2] * n),
                "near5": lambda: eng.search_resident(queries, [NEAR] * n, within=[5] * n)}
        hits = {k: sum(fn().hits()) for k, fn in runs.items()}
        assert hits["phrase"] <= hits["near2"] <= hits["near5"] <= hits["all"], (name, bname, hits)
        row = {"input": name, "case": "near", "batch": bname, "queries": n, "blocks": blocks,
               "iters": iters}
        row.update({k + "_hits": v for k, v in hits.items()})  # all_hits: the candidates
        for k, m in med_of_blocks(runs, blocks, iters).items():
            put(row, k + "_search", m)
        print(json.dumps(row), flush=True)


def plain(lc, root, name, data, blocks, iters):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from prefix_bench import wide_prefixes
    from search_bench import batches
    eng, text = engine_for(lc, data)
    entries = eng.run_index_text(text).entries()
    cases = [(b, q, f, None, False) for b, q, f in batches(entries)]
    two = cases[0][1]
    cases.append(("two_frequent_phrase", two, [PHRASE], None, False))
    cases.append(("two_frequent_rank10", two, [ALL], 10, False))
    cases.append(("one_letter_prefix", [[wide_prefixes(entries)[0] + b"*"]], [ALL], None, True))
    for bname, queries, flags, rank, wild in cases:
        eng.run_search_text(text, queries, flags, rank=rank, wildcard=wild)
        m = med_of_blocks({"r": lambda: eng.search_resident(queries, flags, rank, wild)},
                          blocks, iters)
        row = {"tree": os.path.relpath(root, ROOT), "input": name, "case": "plain",
               "batch": bname, "blocks": blocks, "iters": iters}
        put(row, "resident_search", m["r"])
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers (--plain)")
    ap.add_argument("--once", default="", help="INPUT: the 256-pair near batch five times")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    lc = load(root)
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: lc._C.gen_text(lines=1_000_000)))
    if a.once:
        eng, text = engine_for(lc, dict(inputs)[a.once]())
        queries = near_batches(eng.run_index_text(text).entries())[2][1]
        n = len(queries)
        r = eng.run_search_text(text, queries, [NEAR] * n, within=[2] * n)
        for _ in range(5):
            r = eng.search_resident(queries, [NEAR] * n, within=[2] * n)
        c = eng.search_resident(queries, [ALL] * n)
        print(json.dumps({"input": a.once, "batch": "pairs_256", "within": 2,
                          "candidates": sum(c.hits()), "hits": sum(r.hits())}))
        return
    for name, make in inputs:
        if a.only and a.only != name:
            continue
        if a.plain:
            plain(lc, root, name, make(), a.blocks, a.iters)
        else:
            measure(lc, name, make(), a.blocks, a.iters)


if __name__ == "__main__":
    main()
