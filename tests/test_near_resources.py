"""Register / LDS / scratch budget of the proximity kernel of search.hip from the compiler's
own resource report, as tests/test_rank_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU):
search_near_kernel is there once by name, uses no scratch and spills nothing, keeps no more
LDS than its sibling search_phrase_kernel and at most 64 VGPRs, so that it runs at the same
occupancy.  The figures are kept in profiles/near/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


def one(res, kernel):
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (kernel, sorted(res))
    return res[names[0]]


def test_near_kernel_budget():
    res = resources("search")
    near, phrase = one(res, "search_near_kernel"), one(res, "search_phrase_kernel")
    print("search_near_kernel", near)
    assert near.get("ScratchSize", 0) == 0, near
    assert near.get("VGPRs Spill", 0) == 0 and near.get("SGPRs Spill", 0) == 0, near
    assert near["LDS Size"] <= phrase["LDS Size"] <= 4 * (96 + 256), (near, phrase)
    assert near["VGPRs"] <= 64, near
    assert near["Occupancy"] >= phrase["Occupancy"], (near, phrase)


def test_figures_are_kept():
    res = resources("search")
    rows = []
    for kernel in ("search_hit_kernel", "search_phrase_kernel", "search_near_kernel"):
        r = one(res, kernel)
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (kernel, r)
        rows.append("%-22s %s" % (kernel, "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    out = os.path.join(ROOT, "profiles", "near")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("search.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
