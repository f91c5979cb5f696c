#!/usr/bin/env python3
"""Word n-gram jobs against the word job on one GPU.

For each input (the whole of Hamlet, synth1m = gen_text(lines=1_000_000)) and N in
{1, 2, 3}, in a fresh process per (input, N) -- one step, under its own time limit; the
driver itself never opens the GPU and stops at the first step that fails:

  first_ms   the fresh engine's first job (host timer around the whole call)
  warm_ms    median of the block medians of the warm lean job (min .. max over blocks)
  fallbacks  stats()["fallbacks"] after all jobs: ordered builds that left the LDS tables
             for the HBM-table fallback
  wire_bytes bytes the device wrote to host memory for the result

Every step first checks its result: Hamlet against the oracle, synth1m against the CPU
engine.  One JSON line per step and a markdown table on stdout.

  python tools/ngram_bench.py [--blocks 5] [--iters 9] [--skip-synth] [--step-timeout 240]

The map kernel's own time per N comes from a separate run of one step under the profiler:

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/ngram_bench.py --step hamlet:2
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(name: str, n: int, blocks: int, iters: int) -> dict:
    import locust_amd as lc
    from locust_amd.utils import oracle

    _C = lc._C
    if name == "hamlet":
        raw = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
        ent, ntok, _over, _trunc = oracle.wordcount(raw, ngram=n, stats=True)
    else:
        raw = _C.gen_text(lines=1_000_000)
        ref = _C.cpu_run(lc.make_config("cpu", ngram=n), raw)
        ent, ntok = ref.entries(), ref.num_tokens
        del ref
    text = _C.HostText.from_bytes(raw)  # pinned host memory: no staging copy
    eng = _C.GpuEngine(lc.make_config("gpu", ngram=n), len(raw), _C.count_lines(raw))
    del raw
    t0 = time.perf_counter()
    r = eng.run_text(text)
    first_ms = (time.perf_counter() - t0) * 1e3
    assert r.entries() == ent and r.num_tokens == ntok, f"{name} N={n}: first job differs"
    first_fallbacks = eng.stats()["fallbacks"]
    del r
    for _ in range(3):
        eng.run_text(text)
    meds = []
    wire = uniq = 0
    for _ in range(blocks):
        t = []
        for _ in range(iters):
            t0 = time.perf_counter()
            r = eng.run_text(text)
            t.append((time.perf_counter() - t0) * 1e3)
            wire, uniq, tokens = r.wire_bytes, r.num_unique, r.num_tokens
            del r
        meds.append(statistics.median(t))
    r = eng.run_text(text)
    assert r.entries() == ent, f"{name} N={n}: warm job differs"
    st = eng.stats()
    jobs = 5 + blocks * iters
    return {"input": name, "ngram": n, "bytes": text.size, "records": tokens, "unique": uniq,
            "first_ms": round(first_ms, 4), "warm_ms": round(statistics.median(meds), 4),
            "warm_ms_min": round(min(meds), 4), "warm_ms_max": round(max(meds), 4),
            "jobs": jobs, "fallbacks": st["fallbacks"], "first_job_fallbacks": first_fallbacks,
            "retunes": st["retunes"], "planned_passes": st["planned_passes"],
            "wire_bytes": wire, "blocks": blocks, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--step", help="run one step in this process: INPUT:N")
    a = ap.parse_args()
    if a.step:
        name, n = a.step.split(":")
        print(json.dumps(step(name, int(n), a.blocks, a.iters)), flush=True)
        return 0
    rows = []
    for name in ["hamlet"] + ([] if a.skip_synth else ["synth1m"]):
        for n in (1, 2, 3):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step",
                                    f"{name}:{n}", "--blocks", str(a.blocks), "--iters",
                                    str(a.iters)],
                                   capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"step {name}:{n} ran into its time limit; stopping", file=sys.stderr)
                return 1
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"step {name}:{n} failed with status {p.returncode}; stopping", file=sys.stderr)
                return 1
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print()
    print("| input | N | records | distinct keys | first job ms | warm job ms | fallbacks / jobs | "
          "wire bytes |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['input']} | {r['ngram']} | {r['records']} | {r['unique']} | {r['first_ms']:.4g} | "
              f"{r['warm_ms']:.4g} ({r['warm_ms_min']:.4g} .. {r['warm_ms_max']:.4g}) | "
              f"{r['fallbacks']} / {r['jobs']} | {r['wire_bytes']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
