"""Register / scratch budgets of the regex-term kernels (csrc/kernels/regex.hip) from the
compiler's own resource report, as tests/test_fuzzy_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, the position-automaton matcher
(device/regex.hpp) beside the pattern and the fuzzy matcher brings no scratch and no spills into
any of them, the two dictionary-scan kernels use no LDS (the programs are read from global
memory), and the figures are kept in profiles/regex/resources.txt.  search.hip's, show.hip's,
fuzzy.hip's and expr.hip's kernels keep their own tests and their own profile files."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

SCAN_KERNELS = ("regex_match_kernel", "regex_scatter_kernel")
WALK_KERNELS = ("regex_phrase_kernel", "regex_near_kernel", "regex_showmeasure_kernel",
                "regex_showwrite_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", SCAN_KERNELS + WALK_KERNELS)
def test_regex_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("regex")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    if kernel in SCAN_KERNELS:
        assert r.get("LDS Size", 0) == 0, (kernel, r)  # the program is read from global memory


def test_every_regex_kernel_is_there_and_the_figures_are_kept():
    res = resources("regex")
    rows = []
    for kernel in SCAN_KERNELS + WALK_KERNELS:
        names = [n for n in res if kernel in n]
        assert len(names) == 1, (kernel, sorted(res))
        r = res[names[0]]
        assert r.get("ScratchSize", 0) == 0, (kernel, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (kernel, r)
        rows.append("%-26s %s" % (kernel,
                                  "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(SCAN_KERNELS + WALK_KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "regex")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("regex.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
