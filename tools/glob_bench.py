#!/usr/bin/env python3
"""Pattern terms (`*ing`, `h?ml*t`) and ignore_case on the device: what the dictionary scan and
the merge cost on Hamlet, and that batches without pattern terms pay nothing for them.

One warm engine; every batch is answered by search_resident from the index one run_search left
on the device, the variants alternate inside one process, and the times are the jobs' own
device events (search_ms).  Per block of --iters rounds the median of each variant; the output
gives the median of the block medians and their spread (min .. max over the blocks).

  (default)  the pattern batches, each beside the prefix batch `Ham*` of the same run:
             `*ing`, `h?ml*t`, `to be` with ignore_case as phrase and as `all`, and 1024
             queries of one pattern term each
  --readme   the README's plain, prefix, phrase and ranked batches, search_resident only; run
             it from this tree and from a build of the parent commit (--root) in turn, and
             compare the difference with the parent-vs-parent spread of the same call

  python tools/glob_bench.py [--blocks 5] [--iters 7]
  python tools/glob_bench.py --readme [--root TREE]

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
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--readme", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers (--readme)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import locust_amd as lc
    data = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    eng.run_search(data, [[b"to", b"be"]])  # leaves the index resident
    base = {"input": "hamlet", "blocks": a.blocks, "iters": a.iters}
    if a.readme:
        batches = {
            "plain": lambda: eng.search_resident([[b"to", b"be"], [b"Ham", b"Hor"]], "any"),
            "prefix": lambda: eng.search_resident([[b"Ham*"]], wildcard=True),
            "phrase": lambda: eng.search_resident([[b"to", b"be"]], "phrase"),
            "ranked": lambda: eng.search_resident([[b"to", b"be"]], "any", rank=5),
        }
        for fn in batches.values():
            fn()
        m = med_of_blocks(batches, a.blocks, a.iters)
        for name, (mid, lo, hi) in m.items():
            print(json.dumps(dict(base, tree=os.path.relpath(root, ROOT), case="readme",
                                  batch=name, search_ms=mid, search_ms_min=lo,
                                  search_ms_max=hi)), flush=True)
        return
    ent = eng.run_index(data).entries()
    eng.run_search(data, [[b"to", b"be"]])
    words = [k for k, _v, _c in ent if k.isalpha() and 3 <= len(k) <= 8]
    many = [[w[:1] + b"?" + w[2:]] for w in words[:: max(1, len(words) // 1024)][:1024]]
    cases = {
        "*ing": lambda: eng.search_resident([[b"*ing"]], glob=True),
        "h?ml*t": lambda: eng.search_resident([[b"h?ml*t"]], glob=True),
        "to be, ignore_case, phrase": lambda: eng.search_resident([[b"to", b"be"]], "phrase",
                                                                  ignore_case=True),
        "to be, ignore_case, all": lambda: eng.search_resident([[b"to", b"be"]],
                                                               ignore_case=True),
        "%d queries of one pattern" % len(many): lambda: eng.search_resident(many, glob=True),
    }
    yard = lambda: eng.search_resident([[b"Ham*"]], wildcard=True)
    for name, fn in cases.items():
        r = fn()
        yard()
        m = med_of_blocks({"case": fn, "Ham*": yard}, a.blocks, a.iters)
        print(json.dumps(dict(base, case=name, queries=r.queries, hits=sum(r.hits()),
                              merged=r.merged, dictionary=len(ent),
                              search_ms=m["case"][0], search_ms_min=m["case"][1],
                              search_ms_max=m["case"][2], yardstick_Ham_ms=m["Ham*"][0],
                              yardstick_Ham_ms_min=m["Ham*"][1],
                              yardstick_Ham_ms_max=m["Ham*"][2])), flush=True)


if __name__ == "__main__":
    main()
