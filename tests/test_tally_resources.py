"""Register / scratch budgets of the tally kernels (csrc/kernels/tally.hip) from the compiler's
own resource report, as tests/test_expr_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, neither walk (the map packs and ranks a
key per lane) nor the run, offsets and top kernels bring scratch or spills, and the figures are
kept in profiles/tally/resources.txt.
search.hip's, show.hip's and index.hip's kernels keep their own tests and their own profile
files."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = ("tally_measure_kernel", "tally_scan_kernel", "tally_map_kernel", "tally_seal_kernel",
           "tally_runs_kernel", "tally_offsets_kernel", "tally_top_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")
# LDS: the map's four 96-byte rows; the scan's nine words; the offsets kernel's run_off[Q + 1]
# and its scan's five words, each array rounded up to 16 bytes
LDS_MAX = {"tally_map_kernel": 4 * 96, "tally_scan_kernel": 9 * 8,
           "tally_offsets_kernel": (1025 * 8 + 8) + (5 * 8 + 8)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_tally_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("tally")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("LDS Size", 0) <= LDS_MAX.get(kernel, 0), (kernel, r)


def test_every_tally_kernel_is_there_and_the_figures_are_kept():
    res = resources("tally")
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
    out = os.path.join(ROOT, "profiles", "tally")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("tally.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
