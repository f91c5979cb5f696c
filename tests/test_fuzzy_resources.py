"""Register / scratch budgets of the fuzzy-term kernels (csrc/kernels/fuzzy.hip) from the
compiler's own resource report, as tests/test_glob_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, the banded matcher (device/fuzzy.hpp)
beside the pattern matcher brings no scratch and no spills into any of them, the two
dictionary-scan kernels use no LDS, and the figures are kept in profiles/fuzzy/resources.txt.
search.hip's and show.hip's kernels, whose bodies these share, keep their own tests
(test_glob_resources.py, test_show_resources.py) and their own profile files."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

SCAN_KERNELS = ("fuzzy_match_kernel", "fuzzy_scatter_kernel")
WALK_KERNELS = ("fuzzy_phrase_kernel", "fuzzy_near_kernel", "fuzzy_showmeasure_kernel",
                "fuzzy_showwrite_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", SCAN_KERNELS + WALK_KERNELS)
def test_fuzzy_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("fuzzy")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    if kernel in SCAN_KERNELS:
        assert r.get("LDS Size", 0) == 0, (kernel, r)  # a word's bytes stay scalar


def test_every_fuzzy_kernel_is_there_and_the_figures_are_kept():
    res = resources("fuzzy")
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
    out = os.path.join(ROOT, "profiles", "fuzzy")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("fuzzy.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
