#!/usr/bin/env python3
"""What dropping the oldest block of a sliding-window index costs on the device, against the
alternative it replaces: throwing the index away and rebuilding it over the window.

For every size of --kib (the block's size in KiB; Hamlet's 12 blocks are 16 KiB each), on
generated text (gen_text) cut at line ends into three blocks:

  (a) drop      an engine sized to one block: run_index of the first block, append_index of the
                other two, drop_index of the first block's lines -- drop_ms (hipEvents around
                the drop's kernels and the counters' copy)
  (b) rebuild   Engine.run_index of the last two blocks in a one-pass engine sized to them: the
                job's gpu_ms (upload, word job and index stage) and its index_ms alone

Both are run --warm times first, then --runs times alternating; every figure is the median over
the runs with min .. max.  The dropped index is checked against the rebuilt one before anything
is timed.

  python tools/drop_probe.py [--kib 16,1024,8192] [--runs 7] [--warm 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import locust_amd as lc  # noqa: E402

_C = lc._C


def med(v):
    return f"{statistics.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"


def probe(kib, runs, warm):
    data = _C.gen_text(bytes=3 * kib << 10)
    cuts = lc.split_blocks(data, -(-len(data) // 3) + 4096)
    pieces = [data[o:o + n] for o, n, _l, _f in cuts]
    assert len(pieces) == 3, len(pieces)
    window, first = pieces[1] + pieces[2], cuts[1][3]
    cfg = lc.make_config("gpu")
    sliding = lc.Engine(cfg, max(len(p) for p in pieces), max(c[2] for c in cuts))
    whole = lc.Engine(cfg, len(window), cuts[1][2] + cuts[2][2])

    def drop():
        sliding.run_index(pieces[0])
        sliding.append_index(pieces[1])
        sliding.append_index(pieces[2])
        return sliding.drop_index(cuts[0][2])

    def rebuild():
        return whole.run_index(window, first)

    dr, x = drop(), rebuild()
    y = sliding.index_resident()
    assert x.entries() == y.entries() and x.postings_bytes() == y.postings_bytes(), \
        "the index after the drop differs from the rebuilt one"
    assert (x.first_line, x.overflow_lines, x.truncated) == (y.first_line, y.overflow_lines,
                                                             y.truncated)
    shape = dict(block_kib=kib, window_bytes=len(window), window_lines=x.num_lines,
                 window_tokens=x.num_tokens, window_unique=x.num_unique,
                 dropped_lines=dr.dropped_lines, dropped_tokens=dr.dropped_tokens,
                 dropped_words=dr.dropped_words, store_bytes=dr.store_bytes)
    del x, y
    for _ in range(warm):
        drop()
        rebuild()
    D, G, I = [], [], []
    for _ in range(runs):
        D.append(drop().drop_ms)
        x = rebuild()
        G.append(x.times()["gpu_ms"])
        I.append(x.index_ms)
        del x
    return shape, D, G, I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kib", default="16,1024,8192")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop", "probe.txt"))
    a = ap.parse_args()
    out = ["drop_probe: gen_text, three blocks, the first dropped; median (min .. max) of %d runs "
           "after %d warm-ups, ms" % (a.runs, a.warm), "",
           "block KiB  window tokens  window words  drop_ms                     "
           "rebuild gpu_ms              rebuild index_ms"]
    for kib in [int(k) for k in a.kib.split(",")]:
        shape, D, G, I = probe(kib, a.runs, a.warm)
        out.append("%9d  %13d  %12d  %-26s  %-26s  %s" %
                   (kib, shape["window_tokens"], shape["window_unique"], med(D), med(G), med(I)))
        print(json.dumps(dict(shape, drop_ms=statistics.median(D),
                              rebuild_gpu_ms=statistics.median(G),
                              rebuild_index_ms=statistics.median(I))), flush=True)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
