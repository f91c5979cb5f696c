#!/usr/bin/env python3
"""What a phrase query costs on the device, and what keeping the text resident costs the
index stage.

  --search   For the whole of Hamlet and synth1m (gen_text(lines=1_000_000)): one engine per
             input, one run_search, then the same batch through search_resident in `all`
             and in `phrase` mode, alternating, --iters times each.  search_ms is the
             stage's own device events.  A phrase takes its candidates from the `all`
             evaluation, so the `all` hits are the phrase's candidate lines and the
             difference of the two medians is the verify stage (search_phrase_kernel) --
             less the sort and the copy of the lines the phrase rejected.  The batches: a
             rare pair, frequent pairs, and the three together.
  --index    index_ms (the index stage's device events) and the job's wall time of
             run_index on the whole of Hamlet, a zero-copy-sized input: 10 warm-up jobs, then
             3 * --iters jobs.  --root DIR measures another build of the project (the
             parent commit's, say); run the two alternately and compare.

  python tools/phrase_bench.py --search [--iters 40]
  python tools/phrase_bench.py --index [--root DIR --label parent] [--iters 40]
"""
from __future__ import annotations

import argparse
import os
import statistics as st
import sys
from collections import Counter

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=None, help="what to call the build in the output")
ap.add_argument("--search", action="store_true")
ap.add_argument("--index", action="store_true")
ap.add_argument("--iters", type=int, default=40)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
LABEL = args.label or ("this tree" if args.root == ap.get_default("root") else args.root)
sys.path.insert(0, ROOT)

import locust_amd as lc  # noqa: E402
from locust_amd.utils import oracle  # noqa: E402

assert os.path.abspath(lc.__file__).startswith(ROOT), lc.__file__
HAMLET = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()


def summary(xs):
    xs = sorted(xs)
    return "median %.4f  min %.4f  p10 %.4f  p90 %.4f  max %.4f  (n=%d)" % (
        st.median(xs), xs[0], xs[len(xs) // 10], xs[(len(xs) * 9) // 10], xs[-1], len(xs))


def index_ab():
    e = lc.Engine(lc.make_config("gpu"), len(HAMLET), HAMLET.count(b"\n") + 1)
    for _ in range(10):
        e.run_index(HAMLET)
    ms, wall = [], []
    for _ in range(args.iters * 3):
        x = e.run_index(HAMLET)
        ms.append(x.index_ms)
        wall.append(x.times()["wall_ms"])
    print("index_ms  [%s] hamlet %d B: %s" % (LABEL, len(HAMLET), summary(ms)))
    print("wall_ms   [%s]: %s" % (LABEL, summary(wall)), flush=True)


def synth_queries(text):
    """A rare pair (two words of six bytes or more that stand side by side once in the
    first 40,000 lines), the most frequent pair, and the two most frequent words."""
    words, pairs = Counter(), Counter()
    for line in oracle.split_lines(text)[:40000]:
        toks = oracle.tokenize(line)[0]
        words.update(toks)
        pairs.update(zip(toks, toks[1:]))
    (w1, _), (w2, _) = words.most_common(2)
    common = max(pairs.items(), key=lambda x: x[1])[0]
    rare = min(((p, c) for p, c in pairs.items() if len(p[0]) >= 6 and len(p[1]) >= 6),
               key=lambda x: (x[1], x[0]))[0]
    return [list(rare), list(common), [w1, w2]]


def search_cost():
    inputs = [("hamlet", HAMLET, [[b"Denmark", b"Ham"], [b"of", b"the"], [b"my", b"lord"]])]
    synth = lc._C.gen_text(lines=1_000_000)
    inputs.append(("synth1m", synth, synth_queries(synth)))
    for name, text, queries in inputs:
        nl = text.count(b"\n") + 1
        e = lc.Engine(lc.make_config("gpu"), len(text), nl)
        print("== %s: %d B, %d lines" % (name, len(text), nl), flush=True)
        for batch in [[q] for q in queries] + [queries]:
            first = e.run_search(text, batch, "phrase")
            for _ in range(5):
                for m in ("all", "phrase"):
                    e.search_resident(batch, m)
            ms = {"all": [], "phrase": []}
            hits = {}
            for _ in range(args.iters):
                for m in ("all", "phrase"):  # alternating
                    r = e.search_resident(batch, m)
                    ms[m].append(r.search_ms)
                    hits[m] = sum(r.hits())
            print("  batch %s" % [b" ".join(q).decode() for q in batch])
            print("    all    hits %8d (the phrase's candidates)  search_ms %s"
                  % (hits["all"], summary(ms["all"])))
            print("    phrase hits %8d                            search_ms %s"
                  % (hits["phrase"], summary(ms["phrase"])))
            print("    median phrase - median all: %+.4f ms; the run_search before them: "
                  "index_ms %.3f search_ms %.4f"
                  % (st.median(ms["phrase"]) - st.median(ms["all"]), first.index_ms,
                     first.search_ms), flush=True)


if args.index:
    index_ab()
if args.search:
    search_cost()
