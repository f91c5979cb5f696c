#!/usr/bin/env python3
"""What building an index block by block costs on the device, against one pass.

On generated text (gen_text, --mib MiB, 64 by default), two ways to the same resident index:

  (a) one pass   Engine.run_index of the whole text in an engine sized to it: what an engine
                 without append_index can do (wall, the job's gpu_ms and its index_ms)
  (b) blocks     --blocks blocks (8) of equal size cut at line ends, in an engine sized to one
                 block: run_index of the first, append_index of the rest; every block's
                 index_ms (its own index stage) and append_ms (the merge into the resident
                 index, hipEvents around its kernels and copies), and the whole build's wall

Both are run --warm times first (code objects loaded, the store and every workspace grown to
their final sizes), then --runs times (5) alternating; every figure is the median over the runs,
with min .. max.  The merge reads and writes about 40 nC + 4 T + text + 8 lines bytes twice
(read one half, write the other); the table gives that traffic over append_ms.  The blocked
index is checked against the one-pass index before anything is timed.

  python tools/append_probe.py [--mib 64] [--blocks 8] [--runs 5] [--warm 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import locust_amd as lc  # noqa: E402

_C = lc._C


def med(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append", "probe.txt"))
    a = ap.parse_args()

    data = _C.gen_text(bytes=a.mib << 20)
    nlines = _C.count_lines(data)
    cuts = lc.split_blocks(data, -(-len(data) // a.blocks) + 4096)
    pieces = [data[o:o + n] for o, n, _l, _f in cuts]
    cfg = lc.make_config("gpu")
    whole = lc.Engine(cfg, len(data), nlines)
    blocked = lc.Engine(cfg, max(len(p) for p in pieces), max(c[2] for c in cuts))

    def one_pass():
        t0 = time.perf_counter()
        x = whole.run_index(data)
        wall = (time.perf_counter() - t0) * 1e3
        return wall, x

    def by_blocks():
        t0 = time.perf_counter()
        first = blocked.run_index(pieces[0])
        aps = [blocked.append_index(p) for p in pieces[1:]]
        wall = (time.perf_counter() - t0) * 1e3
        return wall, first, aps

    # the same index either way
    _w, x = one_pass()
    by_blocks()
    y = blocked.index_resident()
    assert x.entries() == y.entries() and x.postings_bytes() == y.postings_bytes(), \
        "the blocked index differs from the one-pass index"
    shape = dict(bytes=len(data), lines=nlines, tokens=x.num_tokens, unique=x.num_unique,
                 blocks=len(pieces))
    del x, y
    for _ in range(a.warm):
        one_pass()
        by_blocks()

    A = {"wall": [], "gpu": [], "index": []}
    B = {"wall": [], "index_sum": [], "append_sum": []}
    per_index = [[] for _ in pieces]
    per_append = [[] for _ in pieces[1:]]
    traffic = []
    for _ in range(a.runs):
        wall, x = one_pass()
        A["wall"].append(wall)
        A["gpu"].append(x.times()["gpu_ms"])
        A["index"].append(x.index_ms)
        del x
        wall, first, aps = by_blocks()
        B["wall"].append(wall)
        per_index[0].append(first.index_ms)
        for i, ap in enumerate(aps):
            per_index[i + 1].append(ap.index_ms)
            per_append[i].append(ap.append_ms)
        B["index_sum"].append(first.index_ms + sum(ap.index_ms for ap in aps))
        B["append_sum"].append(sum(ap.append_ms for ap in aps))
        size, tr = len(pieces[0]), []
        for ap, p in zip(aps, pieces[1:]):
            size += len(p)
            tr.append(2 * (40 * ap.num_unique + 4 * ap.num_tokens + size + 8 * ap.num_lines))
        traffic = tr
        store = aps[-1].store_bytes if aps else 0
        del first

    out = []
    out.append("append_probe: gen_text %d MiB, %d lines, %d tokens, %d distinct words; %d blocks; "
               "median (min .. max) of %d runs after %d warm-ups, ms" %
               (a.mib, nlines, shape["tokens"], shape["unique"], len(pieces), a.runs, a.warm))
    out.append("")
    out.append("(a) one pass:  wall %s   gpu_ms %s   index_ms %s" %
               (med(A["wall"]), med(A["gpu"]), med(A["index"])))
    out.append("(b) blocks:    wall %s   sum index_ms %s   sum append_ms %s" %
               (med(B["wall"]), med(B["index_sum"]), med(B["append_sum"])))
    out.append("    index store %d bytes" % store)
    out.append("")
    out.append("block  resident MiB after  index_ms               append_ms              "
               "merge GB/s (read + write)")
    size = 0
    for i, p in enumerate(pieces):
        size += len(p)
        if i == 0:
            out.append("%5d  %18.1f  %-21s  %-21s  --" % (i, size / 2**20, med(per_index[0]), "--"))
        else:
            ms = statistics.median(per_append[i - 1])
            out.append("%5d  %18.1f  %-21s  %-21s  %.0f" %
                       (i, size / 2**20, med(per_index[i]), med(per_append[i - 1]),
                        traffic[i - 1] / ms / 1e6))
    text = "\n".join(out) + "\n"
    print(text)
    print(json.dumps(dict(shape, one_pass_wall_ms=statistics.median(A["wall"]),
                          blocks_wall_ms=statistics.median(B["wall"]),
                          append_sum_ms=statistics.median(B["append_sum"]),
                          append_ms=[statistics.median(v) for v in per_append])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
