"""Register / LDS / scratch budget of the search kernels that exclusion terms touch, from the
compiler's own resource report, as tests/test_rank_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the lookup, hit,
phrase and near kernels of search.hip use no scratch and spill nothing, and the hit kernel,
which now searches the exclusion lists too, keeps the occupancy of 8 waves that
profiles/near/resources.txt records for it before exclusion terms existed.  The figures are
kept in profiles/exclude/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = ("search_lookup_kernel", "search_hit_kernel", "search_phrase_kernel",
           "search_near_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")
HIT_OCCUPANCY_BEFORE = 8  # search_hit_kernel in profiles/near/resources.txt


def one(res, kernel):
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (kernel, sorted(res))
    return res[names[0]]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(kernel):
    r = one(resources("search"), kernel)
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (kernel, r)


def test_hit_kernel_keeps_its_occupancy():
    r = one(resources("search"), "search_hit_kernel")
    assert r["Occupancy"] >= HIT_OCCUPANCY_BEFORE, r
    assert r.get("LDS Size", 0) == 0, r


def test_figures_are_kept():
    res = resources("search")
    rows = ["%-22s %s" % (k, "  ".join("%s %d" % (f, one(res, k)[f]) for f in FIGURES
                                        if f in one(res, k))) for k in KERNELS]
    out = os.path.join(ROOT, "profiles", "exclude")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("search.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
