"""Register / scratch budgets of the prefix-term kernels of search.hip from the compiler's own
resource report, as tests/test_rank_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the gather and
strip kernels of the expand stage are there once by name, no kernel of the file uses scratch
or spills registers, and the figures are kept in profiles/prefix/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

PREFIX_KERNELS = ("search_gather_kernel", "search_strip_kernel")
OTHER_KERNELS = ("search_lookup_kernel", "search_scan_kernel", "search_hit_kernel",
                 "search_phrase_kernel", "search_seal_kernel", "search_emit_kernel",
                 "search_score_kernel", "search_top_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs","ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", PREFIX_KERNELS)
def test_prefix_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("search")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("LDS Size", 0) == 0, (kernel, r)  # neither keeps anything in LDS


def test_every_search_kernel_is_there_without_scratch_or_spills():
    res = resources("search")
    rows = []
    for kernel in OTHER_KERNELS + PREFIX_KERNELS:
        names = [n for n in res if kernel in n]
        assert len(names) == 1, (kernel, sorted(res))
        r = res[names[0]]
        print(kernel, r)
        assert r.get("ScratchSize", 0) == 0, (kernel, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (kernel, r)
        rows.append("%-22s %s" % (kernel, "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    out = os.path.join(ROOT, "profiles", "prefix")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("search.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
