"""Register / scratch budgets of the show kernels (csrc/kernels/show.hip) from the compiler's own
resource report, as tests/test_rank_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): the measure and
write kernels, their siblings with the matcher and the scan are there once by name, none uses
scratch or spills, no kernel of the file is unaccounted for, and the figures are kept in
profiles/show/resources.txt.  search.hip's kernels keep their own tests
(tests/test_glob_resources.py records them in profiles/glob/resources.txt)."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

SHOW_KERNELS = ("show_measure_kernel", "show_write_kernel", "show_globmeasure_kernel",
                "show_globwrite_kernel", "show_scan_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")


@pytest.mark.parametrize("kernel", SHOW_KERNELS)
def test_show_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("show")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)


def test_every_show_kernel_is_accounted_for():
    res = resources("show")
    rows = []
    for kernel in SHOW_KERNELS:
        (name,) = [n for n in res if kernel in n]
        r = res[name]
        rows.append("%-26s %s" % (kernel, "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(SHOW_KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "show")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("show.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")


def test_the_search_kernels_keep_their_recorded_figures():
    """token_term_mask moved to a header both files share: the verify kernels of search.hip still
    compile to the figures profiles/glob/resources.txt records."""
    res = resources("search")
    recorded = open(os.path.join(ROOT, "profiles", "glob", "resources.txt")).read().splitlines()[1:]
    assert len(recorded) == len(res)
    for row in recorded:
        kernel, rest = row.split(None, 1)
        (name,) = [n for n in res if kernel in n]
        got = "  ".join("%s %d" % (f, res[name][f]) for f in FIGURES if f in res[name])
        assert rest.strip() == got, (kernel, rest, got)
