#!/usr/bin/env python3
"""Search tally (`--tally K`) on the device: what a tally costs on Hamlet beside the same batch
without one, that the plain `to be` batch costs what it cost before the stage existed, and the
answer's bytes beside those `--show 65536` sends for the same lines.

  to be            `all`, 47 lines, 502 pair words
  the              `all`, 820 lines, 7,570 pair words
  king queen       `any`, 34 lines, 311 pair words
  --synth          one synthetic text whose tally sorts more than kSmallSortMax pair words

One warm engine; every batch is one query answered by search_resident from the index one
run_search left on the device, the variants alternate inside one process, and the times are the
jobs' own device events (search_ms, tally_ms).  Per block of --iters rounds the median of each
variant; the output gives the median of the block medians and their spread (min .. max over the
blocks).

Run it from this tree and from a build of the parent commit (--root) in turn and compare the
plain batches' difference with the spread between two processes of the same tree.  A tree that
has no tally answers the plain variants only.

  python tools/tally_bench.py [--blocks 5] [--iters 21] [--root TREE] [--label NAME] [--synth]

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzzy_bench import med_of_blocks  # noqa: E402  (the same blocks and medians)

K = 10


def synth_text(lines=20000, per_line=10, vocab=5000, seed=7):
    """Zipf-ish words, `the` on about every other line."""
    rng = random.Random(seed)
    words = [b"w%d" % i for i in range(vocab)]
    weights = [1.0 / (i + 1) for i in range(vocab)]
    out = []
    for _ in range(lines):
        row = rng.choices(words, weights, k=per_line)
        if rng.random() < 0.5:
            row[rng.randrange(per_line)] = b"the"
        out.append(b" ".join(row))
    return b"\n".join(out) + b"\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers")
    ap.add_argument("--label", default=None)
    ap.add_argument("--synth", action="store_true", help="the large-sort regime instead of Hamlet")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import locust_amd as lc
    if a.synth:
        name, data = "synth20k", synth_text()
        batches = {"the": ([[b"the"]], "all")}
    else:
        name, data = "hamlet", open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
        batches = {"to be": ([[b"to", b"be"]], "all"), "the": ([[b"the"]], "all"),
                   "king queen": ([[b"king", b"queen"]], "any")}
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    eng.run_search(data, [[b"to", b"be"]])  # leaves the index resident
    # (a tree from before the stage has no such argument)
    has_tally = "tally" in inspect.signature(lc.Engine.search_resident).parameters
    variants, shape = {}, {}

    def timed(q, mode, field, **kw):
        def fn():
            r = eng.search_resident(q, mode, **kw)
            ms = {"search": r.search_ms, "tally": r.tally_ms if kw else 0.0}
            return types.SimpleNamespace(search_ms=ms[field], r=r)
        return fn

    for b, (q, mode) in batches.items():
        variants[b] = timed(q, mode, "search")
        if has_tally:
            variants[b + " +tally search_ms"] = timed(q, mode, "search", tally=K)
            variants[b + " +tally tally_ms"] = timed(q, mode, "tally", tally=K)
    for v, fn in variants.items():
        for _ in range(3):  # warm: code objects, the stage's workspace
            r = fn().r
        shape[v] = dict(hits=sum(r.hits()), wire_bytes=r.wire_bytes,
                        tallied=getattr(r, "tallied", None))
    m = med_of_blocks(variants, a.blocks, a.iters)
    for v, (mid, lo, hi) in m.items():
        print(json.dumps(dict(input=name, tree=a.label or os.path.relpath(root, ROOT),
                              blocks=a.blocks, iters=a.iters, batch=v, k=K, **shape[v],
                              ms=mid, ms_min=lo, ms_max=hi)), flush=True)
    # the bytes a host-side count needs today: every returned line's text
    for b, (q, mode) in batches.items():
        r = eng.search_resident(q, mode, show=65536)
        print(json.dumps(dict(input=name, tree=a.label or os.path.relpath(root, ROOT),
                              batch=b + " +show 65536", hits=sum(r.hits()),
                              wire_bytes=r.wire_bytes)), flush=True)


if __name__ == "__main__":
    main()
