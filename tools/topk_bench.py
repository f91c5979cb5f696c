#!/usr/bin/env python3
"""Top-K on the device against the full job plus a host selection.

For each input (the whole of Hamlet, synth1m = gen_text(lines=1_000_000), a generated
text of --stream-gib GiB streamed in 256 MiB chunks) and K in {10, 1000}, on one warm
engine per input and with the variants alternating inside one process:

  (a) full      Engine.run(): every record crosses PCIe
  (b) full+host (a) followed by Result.top(K), the host selection (top_entries)
  (c) run_top   the device selection: only the K winners cross PCIe

Host timers around whole calls (every call ends with the job's own device
synchronisation).  Per block of --iters rounds the median of each variant; the table
gives the median of the block medians and their spread (min .. max over the blocks),
run_top's own select_ms (device events) and the bytes the device wrote to host memory
for the result.  One JSON line per (input, K) and a markdown table on stdout.

  python tools/topk_bench.py [--blocks 5] [--iters 7] [--stream-gib 1] [--skip-stream]
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
from locust_amd.utils import oracle  # noqa: E402

_C = lc._C


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, full, full_host, top, ks, blocks, iters, warm):
    rows = []
    for k in ks:
        for _ in range(warm):  # warm: code objects, workspace, output buffers
            full()
            full_host(k)
            top(k)
        med = {"full": [], "full_host": [], "run_top": [], "select": []}
        wire_full = wire_top = uniq = 0
        for _ in range(blocks):
            t = {"full": [], "full_host": [], "run_top": [], "select": []}
            for _ in range(iters):
                ms, r = timed(full)
                t["full"].append(ms)
                wire_full, uniq = r.wire_bytes, r.num_unique
                del r
                ms, _r = timed(lambda: full_host(k))
                t["full_host"].append(ms)
                del _r
                ms, tr = timed(lambda: top(k))
                t["run_top"].append(ms)
                t["select"].append(tr.select_ms)
                wire_top = tr.wire_bytes
                del tr
            for key in med:
                med[key].append(statistics.median(t[key]))
        row = {"input": name, "k": k, "unique": uniq, "blocks": blocks, "iters": iters,
               "wire_bytes_full": wire_full, "wire_bytes_top": wire_top}
        for key, v in med.items():
            row[key + "_ms"] = round(statistics.median(v), 4)
            row[key + "_ms_min"] = round(min(v), 4)
            row[key + "_ms_max"] = round(max(v), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def check(name, text_entries, top_result, k):
    want = oracle.top(text_entries, k)
    assert top_result.entries() == want, f"{name}: run_top(k={k}) differs from the oracle"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--stream-gib", type=float, default=1.0)
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-synth", action="store_true")
    a = ap.parse_args()
    ks = (10, 1000)
    rows = []

    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    # every input sits in pinned host memory (HostText): no staging copy in any variant
    eng = _C.GpuEngine(lc.make_config("gpu"), len(hamlet), _C.count_lines(hamlet))
    text = _C.HostText.from_bytes(hamlet)
    ent = oracle.wordcount(hamlet)[0]
    for k in ks:
        check("hamlet", ent, eng.run_top_text(text, k), k)
    rows += measure("hamlet", lambda: eng.run_text(text), lambda k: eng.run_text(text).top(k),
                    lambda k: eng.run_top_text(text, k), ks, a.blocks, a.iters, 5)
    del eng, text

    if not a.skip_synth:
        synth = _C.gen_text(lines=1_000_000)
        eng = _C.GpuEngine(lc.make_config("gpu"), len(synth), _C.count_lines(synth))
        text = _C.HostText.from_bytes(synth)
        del synth
        full = eng.run_text(text)
        for k in ks:  # (the host selection is the reference here: the oracle takes minutes)
            assert eng.run_top_text(text, k).entries() == full.top(k).entries()
        del full
        rows += measure("synth1m", lambda: eng.run_text(text), lambda k: eng.run_text(text).top(k),
                        lambda k: eng.run_top_text(text, k), ks, a.blocks, a.iters, 3)
        del eng, text

    if not a.skip_stream:
        big = _C.HostText.from_bytes(_C.gen_text(bytes=int(a.stream_gib * (1 << 30))))
        cfg = lc.make_config("gpu", chunk_bytes=256 << 20)
        eng = _C.GpuEngine(cfg, big.size, big.size)
        full = eng.run_text(big)
        for k in ks:
            assert eng.run_top_text(big, k).entries() == full.top(k).entries()
        del full
        rows += measure(f"stream{a.stream_gib:g}g", lambda: eng.run_text(big),
                        lambda k: eng.run_text(big).top(k), lambda k: eng.run_top_text(big, k),
                        ks, max(2, a.blocks // 2), max(3, a.iters // 2), 1)

    print()
    print("| input | K | distinct keys | (a) full ms | (b) full + host top ms | (c) run_top ms | "
          "select_ms | wire bytes (a) | wire bytes (c) |")
    print("|---|---|---|---|---|---|---|---|---|")

    def cell(r, key):
        return f"{r[key + '_ms']:.4g} ({r[key + '_ms_min']:.4g} .. {r[key + '_ms_max']:.4g})"

    for r in rows:
        print(f"| {r['input']} | {r['k']} | {r['unique']} | {cell(r, 'full')} | "
              f"{cell(r, 'full_host')} | {cell(r, 'run_top')} | {cell(r, 'select')} | "
              f"{r['wire_bytes_full']} | {r['wire_bytes_top']} |")


if __name__ == "__main__":
    main()
