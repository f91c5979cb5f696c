#!/usr/bin/env python3
"""Fuzzy terms (`be~1`) on the device: what the dictionary scan with the banded edit-distance
matcher costs on Hamlet beside the pattern batch `b?`, which walks the same dictionary with the
pattern matcher -- and that the pattern batch costs what it cost before fuzzy terms existed.

One warm engine; every batch is one query answered by search_resident from the index one
run_search left on the device, the variants alternate inside one process, and the times are the
jobs' own device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

Run it from this tree and from a build of the parent commit (--root) in turn, twice each, and
compare the `b?` difference with the spread between two runs of the same tree.  A tree that has
no `fuzzy` keyword answers `b?` only.

  python tools/fuzzy_bench.py [--blocks 5] [--iters 21] [--root TREE] [--label NAME]

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers")
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import locust_amd as lc
    data = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    eng.run_search(data, [[b"to", b"be"]])  # leaves the index resident
    variants = {"b?": lambda: eng.search_resident([[b"b?"]], glob=True)}
    try:
        eng.search_resident([[b"be~1"]], fuzzy=True)
        variants["be~1"] = lambda: eng.search_resident([[b"be~1"]], fuzzy=True)
    except TypeError:  # a tree from before fuzzy terms
        pass
    shape = {}
    for name, fn in variants.items():
        for _ in range(3):  # warm: code objects, the pattern arrays, the merge workspace
            r = fn()
        shape[name] = dict(hits=sum(r.hits()), count=r.term_counts(0)[0], merged=r.merged)
    m = med_of_blocks(variants, a.blocks, a.iters)
    for name, (mid, lo, hi) in m.items():
        print(json.dumps(dict(input="hamlet", tree=a.label or os.path.relpath(root, ROOT),
                              blocks=a.blocks, iters=a.iters, batch=name, **shape[name],
                              search_ms=mid, search_ms_min=lo, search_ms_max=hi)), flush=True)


if __name__ == "__main__":
    main()
