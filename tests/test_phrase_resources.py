"""Register / LDS / scratch budgets of search.hip and index.hip from the compiler's own
resource report, by tests/test_kernel_resources.py's method (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the phrase
kernel is there, and no kernel of either file -- index.hip now takes its tokeniser from the
header the phrase kernel shares -- uses scratch or spills VGPRs."""
import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


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


@pytest.mark.parametrize("stem", ["search", "index"])
def test_no_scratch_no_spills(stem):
    res = resources(stem)
    assert res, "no kernels reported"
    for name, r in res.items():
        assert r.get("ScratchSize", 0) == 0, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)


def test_phrase_kernel_is_reported():
    res = resources("search")
    names = [n for n in res if "search_phrase_kernel" in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    # a wave's row (96 B) and its query's term keys (8 x 32 B), four waves; full occupancy
    # needs at most 64 VGPRs
    assert r["LDS Size"] <= 4 * (96 + 256) and r["VGPRs"] <= 64, r
    for other in ("search_lookup_kernel", "search_hit_kernel", "search_seal_kernel",
                  "search_emit_kernel"):
        assert any(other in n for n in res), other
    assert any("index_map_kernel" in n for n in resources("index"))
