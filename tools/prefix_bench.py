#!/usr/bin/env python3
"""Prefix terms (`ham*`) on the device: what the merge costs, and that plain batches pay
nothing for it.

Inputs are the whole of Hamlet and synth1m = gen_text(lines=1_000_000).  One warm engine
per input; every batch is answered by search_resident from the index one run_search left on
the device, the variants alternate inside one process, and the times are the jobs' own
device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

  (a) narrow   one prefix term that covers w <= 8 words against the `any` query that lists
               those w words: the same lines (asserted before anything is timed), once
               with the merge and once over lists that need none
  (b) wide     a one-letter and a two-letter prefix: X = merged and search_ms
  (c) --plain  the four plain batches of tools/search_bench.py, search_resident only; run it
               from this tree and from a build of the parent commit (--root) in turn, and
               compare the difference with the parent-vs-parent spread of the same call

  python tools/prefix_bench.py [--blocks 5] [--iters 7] [--only hamlet|synth1m] [--skip-synth]
  python tools/prefix_bench.py --plain [--root TREE]
  python tools/prefix_bench.py --once synth1m:auto1   (one wide batch a few times, for a kernel
                                                       trace: rocprofv3 --kernel-trace --stats)

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import bisect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def narrow_prefix(entries):
    """(prefix, its words): the most frequent words' prefixes, the first that covers 2..8
    words -- preferring more words."""
    keys = [k for k, _v, _c in entries]  # in key order: a prefix's words are one range
    best = None
    for k, _v, _c in sorted(entries, key=lambda e: (-e[2], e[0]))[:200]:
        for n in range(2, len(k) + 1):
            lo = bisect.bisect_left(keys, k[:n])
            hi = bisect.bisect_right(keys, k[:n] + b"\xff" * 32)
            if 2 <= hi - lo <= 8 and (best is None or hi - lo > len(best[1])):
                best = (k[:n], keys[lo:hi])
    return best


def wide_prefixes(entries):
    """The one-letter and the two-letter prefix with the most postings."""
    out = []
    for n in (1, 2):
        total = {}
        for k, _v, c in entries:
            if len(k) >= n:
                total[k[:n]] = total.get(k[:n], 0) + c
        out.append(max(sorted(total), key=lambda p: total[p]))
    return out


def engine_for(lc, data):
    _C = lc._C
    eng = _C.GpuEngine(lc.make_config("gpu"), len(data), _C.count_lines(data))
    text = _C.HostText.from_bytes(data)
    return eng, text


def measure(lc, name, data, blocks, iters):
    eng, text = engine_for(lc, data)
    entries = eng.run_index_text(text).entries()
    eng.run_search_text(text, [[entries[0][0]]], [0])  # leaves the index resident
    p, words = narrow_prefix(entries)
    a = eng.search_resident([[p + b"*"]], [1], wildcard=True)
    b = eng.search_resident([words], [1])
    assert a.lines(0) == b.lines(0), f"{name}: {p!r}* and its {len(words)} words differ"
    assert a.merged == sum(a.term_counts(0)) == sum(b.term_counts(0))
    row = {"input": name, "case": "narrow", "prefix": p.decode("latin-1"), "words": len(words),
           "merged": a.merged, "hits": a.hits()[0], "blocks": blocks, "iters": iters}
    m = med_of_blocks({"prefix": lambda: eng.search_resident([[p + b"*"]], [1], wildcard=True),
                       "any": lambda: eng.search_resident([words], [1])}, blocks, iters)
    put(row, "prefix_search", m["prefix"])
    put(row, "any_search", m["any"])
    print(json.dumps(row), flush=True)
    for w in wide_prefixes(entries):
        r = eng.search_resident([[w + b"*"]], [0], wildcard=True)
        k = eng.search_resident([[w + b"*"]], [0], 10, wildcard=True)
        row = {"input": name, "case": "wide", "prefix": w.decode("latin-1"), "X": r.merged,
               "merged": r.merged, "hits": r.hits()[0], "blocks": blocks, "iters": iters}
        assert k.merged == r.merged and k.matches() == r.hits()
        m = med_of_blocks(
            {"unranked": lambda: eng.search_resident([[w + b"*"]], [0], wildcard=True),
             "rank10": lambda: eng.search_resident([[w + b"*"]], [0], 10, wildcard=True)},
            blocks, iters)
        put(row, "search", m["unranked"])
        put(row, "rank10_search", m["rank10"])
        print(json.dumps(row), flush=True)


def plain(lc, root, name, data, blocks, iters):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from search_bench import batches
    eng, text = engine_for(lc, data)
    entries = eng.run_index_text(text).entries()
    for bname, queries, flags in batches(entries):
        eng.run_search_text(text, queries, flags)
        m = med_of_blocks({"r": lambda: eng.search_resident(queries, flags)}, blocks, iters)
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
    ap.add_argument("--once", default="", help="INPUT:PREFIX, one wide batch five times")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    lc = load(root)
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: lc._C.gen_text(lines=1_000_000)))
    if a.once:
        name, p = a.once.split(":")
        data = dict(inputs)[name]()
        eng, text = engine_for(lc, data)
        if p in ("auto1", "auto2"):  # the widest one- or two-letter prefix
            p = wide_prefixes(eng.run_index_text(text).entries())[int(p[-1]) - 1].decode("latin-1")
        q = [[p.encode("latin-1") + b"*"]]
        r = eng.run_search_text(text, q, [0], wildcard=True)
        for _ in range(5):
            r = eng.search_resident(q, [0], wildcard=True)
        print(json.dumps({"input": name, "prefix": p, "merged": r.merged, "hits": r.hits()[0]}))
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
