#!/usr/bin/env python3
"""The show stage (show=N: the returned lines' text and match spans, gathered on the device):
what it adds to a search batch, and that batches without it pay nothing.

One warm engine per input; every batch is answered by search_resident from the index one
run_search left on the device, the variants alternate inside one process, and the times are the
jobs' own device events (search_ms, show_ms).  Per block of --iters rounds the median of each
variant; the output gives the median of the block medians and their spread (min .. max over the
blocks).

  (default)  (a) whole Hamlet, `any` "to be" (the README's 737 lines) and the same batch with
             rank=5: search_ms with show=0 against search_ms + show_ms with show=80 and
             show=4096, and wire_bytes each;
             (c) synth1m = gen_text(lines=1_000_000), one frequent word, `any`, unranked,
             show=64: show_ms against the stage's payload -> GB/s (--skip-synth leaves it out)
  --noshow   (b) the two show=0 batches of (a) alone; run it from this tree and from a build of
             the parent commit (--root) in turn, twice each, and compare the difference with the
             parent's own spread

  python tools/show_bench.py [--blocks 5] [--iters 7] [--skip-synth]
  python tools/show_bench.py --noshow [--root TREE]

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med_of_blocks(variants, blocks, iters, show=True):
    """variants: {name: callable -> SearchResult}; alternating; per name the (median, min, max)
    of search_ms and of show_ms over the block medians."""
    med = {k: ([], []) for k in variants}
    for _ in range(blocks):
        t = {k: ([], []) for k in variants}
        for _ in range(iters):
            for k, fn in variants.items():
                r = fn()
                t[k][0].append(r.search_ms)
                t[k][1].append(r.show_ms if show else 0.0)
        for k in variants:
            med[k][0].append(statistics.median(t[k][0]))
            med[k][1].append(statistics.median(t[k][1]))
    three = lambda v: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4))
    return {k: (three(s), three(w)) for k, (s, w) in med.items()}


def payload_bytes(r):
    """What the stage copies besides its counters: both offset arrays, the spans, the text."""
    entries = sum(r.hits())
    if not entries or not r.show_bytes:
        return 0
    return 2 * (entries + 1) * 8 + 12 * r.span_count + r.text_off()[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--noshow", action="store_true")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose build answers (--noshow)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import locust_amd as lc
    data = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    eng.run_search(data, [[b"to", b"be"]])  # leaves the index resident
    base = {"blocks": a.blocks, "iters": a.iters}
    q = [[b"to", b"be"]]
    if a.noshow:
        batches = {"any": lambda: eng.search_resident(q, "any"),
                   "any rank=5": lambda: eng.search_resident(q, "any", rank=5)}
        for fn in batches.values():
            fn()
        m = med_of_blocks(batches, a.blocks, a.iters, show=False)
        for name, ((mid, lo, hi), _w) in m.items():
            print(json.dumps(dict(base, input="hamlet", tree=os.path.relpath(root, ROOT),
                                  case="noshow", batch=name, search_ms=mid, search_ms_min=lo,
                                  search_ms_max=hi)), flush=True)
        return
    for name, kw in (("any", {}), ("any rank=5", {"rank": 5})):
        variants = {"show=%d" % n: (lambda n=n: eng.search_resident(q, "any", show=n, **kw))
                    for n in (0, 80, 4096)}
        first = {k: fn() for k, fn in variants.items()}
        m = med_of_blocks(variants, a.blocks, a.iters)
        for k, ((s, slo, shi), (w, wlo, whi)) in m.items():
            r = first[k]
            print(json.dumps(dict(base, input="hamlet", case="a", batch=name, variant=k,
                                  entries=sum(r.hits()), spans=r.span_count,
                                  cut_lines=r.cut_lines, payload_bytes=payload_bytes(r),
                                  wire_bytes=r.wire_bytes, search_ms=s, search_ms_min=slo,
                                  search_ms_max=shi, show_ms=w, show_ms_min=wlo, show_ms_max=whi,
                                  total_ms=round(s + w, 4))), flush=True)
    if a.skip_synth:
        return
    del eng
    data = lc._C.gen_text(lines=1_000_000)
    eng = lc.Engine(lc.make_config("gpu"), len(data), data.count(b"\n") + 1)
    word = max(eng.run_index(data).entries(), key=lambda e: e[2])[0]
    eng.run_search(data, [[word]])
    variants = {"show=0": lambda: eng.search_resident([[word]], "any"),
                "show=64": lambda: eng.search_resident([[word]], "any", show=64)}
    first = {k: fn() for k, fn in variants.items()}
    m = med_of_blocks(variants, a.blocks, a.iters)
    for k, ((s, slo, shi), (w, wlo, whi)) in m.items():
        r = first[k]
        pay = payload_bytes(r)
        print(json.dumps(dict(base, input="synth1m", case="c", batch="any %s" % word.decode(),
                              variant=k, entries=sum(r.hits()), spans=r.span_count,
                              cut_lines=r.cut_lines, payload_bytes=pay, wire_bytes=r.wire_bytes,
                              search_ms=s, search_ms_min=slo, search_ms_max=shi, show_ms=w,
                              show_ms_min=wlo, show_ms_max=whi,
                              payload_gb_per_s=round(pay / w / 1e6, 2) if w else None)),
              flush=True)


if __name__ == "__main__":
    main()
