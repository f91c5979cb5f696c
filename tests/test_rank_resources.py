"""Register / scratch budgets of the ranked-search kernels of search.hip from the compiler's
own resource report, as tests/test_phrase_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the score and
top kernels are there by name, and neither uses scratch or spills VGPRs."""
import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

RANK_KERNELS = ("search_score_kernel", "search_top_kernel")


@functools.lru_cache(maxsize=None)
def resources(stem):
    src = os.path.join(ROOT, "csrc", "kernels", stem + ".hip")
    p = subprocess.run([HIPCC, "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "csrc/include"),
                        "-O3", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-c", src, "-o",
                        os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([\w ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


@pytest.mark.parametrize("kernel", RANK_KERNELS)
def test_rank_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("search")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    # neither kernel keeps anything in LDS, and both run at full occupancy (<= 64 VGPRs)
    assert r.get("LDS Size", 0) == 0 and r["VGPRs"] <= 64, (kernel, r)


def test_the_other_search_kernels_are_still_there():
    res = resources("search")
    for other in ("search_lookup_kernel", "search_scan_kernel", "search_hit_kernel",
                  "search_phrase_kernel", "search_seal_kernel", "search_emit_kernel"):
        assert any(other in n for n in res), other
