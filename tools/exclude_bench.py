#!/usr/bin/env python3
"""Exclusion terms (`exclude=`, `--not`) on the device: what one exclusion term costs a
batch, and what it saves the stages behind the hit kernel.

Inputs are the whole of Hamlet and synth1m = gen_text(lines=1_000_000).  One warm engine
per input; every batch is answered by search_resident from the index one run_search left on
the device, the variants alternate inside one process, and the times are the jobs' own
device events (search_ms).  Per block of --iters rounds the median of each variant; the
output gives the median of the block medians and their spread (min .. max over the blocks).

  (a) default  the positive batches of tools/near_bench.py (the two most frequent words, and
               256 pairs drawn from the 200 most frequent words) as `all`, `phrase`, `near`
               W = 2 and ranked `all` with K = 10, each without an exclusion term and with
               one: a frequent word (the third most frequent), a rare word (count 1) and
               the widest one-letter prefix, which the expand stage has to merge first.
               Every query of a batch gets the same exclusion term.  Per variant the time
               and the hits (ranked: the matches)
  (b) plain batches pay nothing: tools/near_bench.py --plain [--root TREE], from this tree
               and from a build of the parent commit in turn; nothing of it is in this file

  python tools/exclude_bench.py [--blocks 5] [--iters 7] [--only hamlet|synth1m] [--skip-synth]
                                [--skip-prefix]

--skip-prefix leaves the prefix variant out: on synth1m its merge moves hundreds of MB per
batch of 256 queries, and the variant that runs behind it starts from a cold cache.

One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from near_bench import ALL, NEAR, PHRASE, engine_for, load, med_of_blocks, near_batches, put  # noqa: E402
from prefix_bench import wide_prefixes  # noqa: E402

MODES = [("all", ALL, None, None), ("phrase", PHRASE, None, None), ("near2", NEAR, 2, None),
         ("rank10", ALL, None, 10)]


def exclusions(entries):
    by_count = sorted(entries, key=lambda e: (-e[2], e[0]))
    rare = [k for k, _v, c in by_count if c == 1][0]
    return [("none", None, 0), ("frequent", by_count[2][0], by_count[2][2]),
            ("rare", rare, 1), ("prefix", wide_prefixes(entries)[0] + b"*", None)]


def measure(lc, name, data, blocks, iters, skip_prefix=False):
    eng, text = engine_for(lc, data)
    entries = eng.run_index_text(text).entries()
    eng.run_search_text(text, [[entries[0][0]]], [ALL])  # leaves the index resident
    xs = [x for x in exclusions(entries) if not (skip_prefix and x[0] == "prefix")]
    for bname, queries in near_batches(entries):
        if bname == "rare_frequent":
            continue  # (no candidates: nothing to exclude)
        n = len(queries)
        for mname, flag, w, k in MODES:
            within = [w] * n if w else []

            def runner(x):
                ex = [[x]] * n if x else []
                return lambda: eng.search_resident(queries, [flag] * n, k, True, within, ex)

            runs = {xname: runner(x) for xname, x, _c in xs}
            first = {xname: fn() for xname, fn in runs.items()}
            row = {"input": name, "case": "exclude", "batch": bname, "mode": mname, "queries": n,
                   "blocks": blocks, "iters": iters, "variants": [x[0] for x in xs]}
            for xname, x, c in xs:
                r = first[xname]
                row[xname + "_hits"] = sum(r.matches()) if k else sum(r.hits())
                if x:
                    row[xname + "_term"] = x.decode("latin-1")
                    row[xname + "_count"] = r.term_counts(0)[-1]
                    row[xname + "_merged"] = r.merged
            assert all(row[x + "_hits"] <= row["none_hits"] for x, _t, _c in xs), row
            for xname, m in med_of_blocks(runs, blocks, iters).items():
                put(row, xname + "_search", m)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--skip-prefix", action="store_true")
    a = ap.parse_args()
    lc = load(ROOT)
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    inputs = [("hamlet", lambda: hamlet)]
    if not a.skip_synth:
        inputs.append(("synth1m", lambda: lc._C.gen_text(lines=1_000_000)))
    for name, make in inputs:
        if a.only and a.only != name:
            continue
        measure(lc, name, make(), a.blocks, a.iters, a.skip_prefix)


if __name__ == "__main__":
    main()
