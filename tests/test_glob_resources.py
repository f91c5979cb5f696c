"""Register / scratch budgets of the pattern-term kernels of search.hip from the compiler's own
resource report, as tests/test_prefix_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the match and
scatter kernels of the dictionary scan and the two verify siblings are there once by name, the
matcher (device/glob.hpp) brings no scratch and no spills into any of them, no kernel of the
file uses either, and the figures are kept in profiles/glob/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

GLOB_KERNELS = ("search_match_kernel", "search_scatter_kernel", "search_globphrase_kernel",
                "search_globnear_kernel")
OTHER_KERNELS = ("search_lookup_kernel", "search_scan_kernel", "search_gather_kernel",
                 "search_strip_kernel", "search_hit_kernel", "search_phrase_kernel",
                 "search_near_kernel", "search_seal_kernel", "search_emit_kernel",
                 "search_score_kernel", "search_top_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", GLOB_KERNELS)
def test_glob_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("search")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    if kernel in ("search_match_kernel", "search_scatter_kernel"):
        assert r.get("LDS Size", 0) == 0, (kernel, r)  # a pattern's bytes stay scalar


def test_every_search_kernel_is_there_without_scratch_or_spills():
    res = resources("search")
    rows = []
    for kernel in OTHER_KERNELS + GLOB_KERNELS:
        names = [n for n in res if kernel in n]
        assert len(names) == 1, (kernel, sorted(res))
        r = res[names[0]]
        print(kernel, r)
        assert r.get("ScratchSize", 0) == 0, (kernel, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (kernel, r)
        rows.append("%-26s %s" % (kernel, "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(OTHER_KERNELS + GLOB_KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "glob")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("search.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
