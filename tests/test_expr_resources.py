"""Register / scratch budgets of the expression kernels (csrc/kernels/expr.hip) from the
compiler's own resource report, as tests/test_fuzzy_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, neither the plan (the 256-bit table in
registers, the greedy loop) nor the hit kernel (the mask loop over up to eight lists) brings
scratch or spills, the hit kernel uses no LDS and the plan only its scan's few words, and the
figures are kept in profiles/expr/resources.txt.
search.hip's and show.hip's kernels keep their own tests and their own profile files."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = ("expr_plan_kernel", "expr_hit_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", KERNELS)
def test_expr_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("expr")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    # the table stays in registers; LDS: none in the hit kernel, the block scan's words in the plan
    assert r.get("LDS Size", 0) <= (0 if kernel == "expr_hit_kernel" else 64), (kernel, r)


def test_every_expr_kernel_is_there_and_the_figures_are_kept():
    res = resources("expr")
    rows = []
    for kernel in KERNELS:
        names = [n for n in res if kernel in n]
        assert len(names) == 1, (kernel, sorted(res))
        r = res[names[0]]
        assert r.get("ScratchSize", 0) == 0, (kernel, r)
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (kernel, r)
        rows.append("%-26s %s" % (kernel,
                                  "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "expr")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("expr.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
