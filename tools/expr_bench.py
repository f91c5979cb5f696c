#!/usr/bin/env python3
"""Boolean expression queries (`--match expr`) on the device: what an expression costs on Hamlet
beside the same question asked the old way, and that the plain `to be` batch costs what it cost
before expressions existed.

  to AND be AND NOT not    as `expr`, beside `all` [to, be] with exclude [not]
  to AND NOT the           as `expr` (walks to's 634 postings), beside the one-term query [to]
  ( to AND be ) OR ( Ham* AND NOT Hamlet )    with wildcard: the 409-line example

One warm engine; every batch is one query answered by search_resident from the index one
run_search left on the device, the variants alternate inside one process, and the times are the
jobs' own device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

Run it from this tree and from a build of the parent commit (--root) in turn and compare the
`to be` difference with the spread between two processes of the same tree.  A tree that has no
`expr` mode answers the old-way variants only.

  python tools/expr_bench.py [--blocks 5] [--iters 21] [--root TREE] [--label NAME]

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzzy_bench import med_of_blocks  # noqa: E402  (the same blocks and medians)


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
    variants = {
        "to be": lambda: eng.search_resident([[b"to", b"be"]]),
        "to be -not": lambda: eng.search_resident([[b"to", b"be"]], exclude=[[b"not"]]),
        "to": lambda: eng.search_resident([[b"to"]]),
    }
    from locust_amd.models import wordcount
    if "expr" in wordcount._SEARCH_MODES:  # (a tree from before expressions has no such mode)
        variants["to AND be AND NOT not"] = \
            lambda: eng.search_resident([b"to AND be AND NOT not"], "expr")
        variants["to AND NOT the"] = lambda: eng.search_resident([b"to AND NOT the"], "expr")
        variants["( to AND be ) OR ( Ham* AND NOT Hamlet )"] = lambda: eng.search_resident(
            [b"( to AND be ) OR ( Ham* AND NOT Hamlet )"], "expr", wildcard=True)
    shape = {}
    for name, fn in variants.items():
        for _ in range(3):  # warm: code objects, the expression arrays, the merge workspace
            r = fn()
        shape[name] = dict(hits=sum(r.hits()), merged=r.merged, walked=getattr(r, "walked", None))
    m = med_of_blocks(variants, a.blocks, a.iters)
    for name, (mid, lo, hi) in m.items():
        print(json.dumps(dict(input="hamlet", tree=a.label or os.path.relpath(root, ROOT),
                              blocks=a.blocks, iters=a.iters, batch=name, **shape[name],
                              search_ms=mid, search_ms_min=lo, search_ms_max=hi)), flush=True)


if __name__ == "__main__":
    main()
