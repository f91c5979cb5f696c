#!/usr/bin/env python3
"""Regex terms (`/re/`) on the device: what the dictionary scan with the position-automaton
matcher costs on Hamlet beside the matchers it stands next to -- `/.*ing/` beside `*ing` under
`glob` (the same 212 words, the same merge: the difference is the matcher) and
`/\\[?Hamlet[!?\\]]?/` beside `Hamlet~1` (the same 5 words) -- and that the pattern batch `b?` and
the plain batch `to be` cost what they cost before regex terms existed.

One warm engine; every batch is one query answered by search_resident from the index one
run_search left on the device, the variants alternate inside one process, and the times are the
jobs' own device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

Run it from this tree and from a build of the parent commit (--root) in turn, four fresh
processes each, and compare the `b?` and `to be` spans of the two trees.  A tree that has no
`regex` keyword answers `b?` and `to be` only.

  python tools/regex_bench.py [--blocks 5] [--iters 21] [--root TREE] [--label NAME] [--out DIR]

One JSON line per measurement, printed and appended to DIR/search_ms.jsonl (default
profiles/regex); DIR/search_ms.txt is rewritten from all of the file's lines.
"""
from __future__ import annotations

import argparse
import inspect
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


def summary(rows):
    """search_ms.txt: per (tree, batch) the processes' medians and the span over them."""
    out = ["regex_bench.py, whole Hamlet, search_resident, device events; per process the median",
           "of block medians (ms); span: min .. max over the processes' medians", ""]
    keys = []
    for r in rows:
        if (r["tree"], r["batch"]) not in keys:
            keys.append((r["tree"], r["batch"]))
    for tree, batch in keys:
        mine = [r for r in rows if (r["tree"], r["batch"]) == (tree, batch)]
        meds = [r["search_ms"] for r in mine]
        out.append("%-8s %-22s hits %-5d count %-5d merged %-5d  %s  span %.4f .. %.4f" % (
            tree, batch, mine[0]["hits"], mine[0]["count"], mine[0]["merged"],
            " ".join("%.4f" % m for m in meds), min(meds), max(meds)))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers")
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regex"))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import locust_amd as lc
    data = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    eng.run_search(data, [[b"to", b"be"]])  # leaves the index resident
    variants = {"b?": lambda: eng.search_resident([[b"b?"]], glob=True),
                "to be": lambda: eng.search_resident([[b"to", b"be"]])}
    # (a tree from before regex terms has no `regex` keyword: it answers the two batches above)
    if "regex" in inspect.signature(eng.search_resident).parameters:
        variants["/.*ing/"] = lambda: eng.search_resident([[b"/.*ing/"]], regex=True)
        variants["*ing"] = lambda: eng.search_resident([[b"*ing"]], glob=True)
        variants["/\\[?Hamlet[!?\\]]?/"] = lambda: eng.search_resident(
            [[b"/\\[?Hamlet[!?\\]]?/"]], regex=True)
        variants["Hamlet~1"] = lambda: eng.search_resident([[b"Hamlet~1"]], fuzzy=True)
    else:
        print("no regex keyword in %s: measuring `b?` and `to be` only" % root, file=sys.stderr)
    shape = {}
    for name, fn in variants.items():
        for _ in range(3):  # warm: code objects, the pattern arrays, the merge workspace
            r = fn()
        shape[name] = dict(hits=sum(r.hits()), count=r.term_counts(0)[0], merged=r.merged)
    m = med_of_blocks(variants, a.blocks, a.iters)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "search_ms.jsonl")
    with open(path, "a") as f:
        for name, (mid, lo, hi) in m.items():
            line = json.dumps(dict(input="hamlet", tree=a.label or os.path.relpath(root, ROOT),
                                   blocks=a.blocks, iters=a.iters, batch=name, **shape[name],
                                   search_ms=mid, search_ms_min=lo, search_ms_max=hi))
            print(line, flush=True)
            f.write(line + "\n")
    rows = [json.loads(l) for l in open(path) if l.strip()]
    with open(os.path.join(a.out, "search_ms.txt"), "w") as f:
        f.write(summary(rows))


if __name__ == "__main__":
    main()
