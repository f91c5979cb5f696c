"""Register / scratch budgets of the drop kernels (csrc/kernels/drop.hip) from the compiler's own
resource report, as tests/test_append_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, none brings scratch or spills, LDS stays
within what the tiles need, the scan kernels are the merge's own (device/tile_scan.hpp) with the
merge's figures, and the figures are kept in profiles/drop/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

SCANS = ("append_tile_sum_kernel", "append_tile_scan_kernel", "append_tile_apply_kernel")
KERNELS = ("drop_cut_kernel",) + SCANS + ("drop_records_kernel", "drop_postings_kernel",
                                          "drop_lines_kernel", "drop_text_kernel",
                                          "drop_stats_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")
TILE = 1024  # kAppendTile
# LDS: the postings tile stages one destination offset and one shift to the source per word, at
# most one word per element, and the offset behind the last word: (TILE + 1) + TILE u64 words --
# the merge's budget.  The statistics walk keeps one row of 64 + 32 bytes per wave (4).  The
# scans as in the merge.  Each array may be rounded up to 16 bytes.
LDS_MAX = {"drop_postings_kernel": ((TILE + 1) * 8 + 8) + TILE * 8,
           "drop_stats_kernel": 4 * 96,
           "append_tile_sum_kernel": 4 * 8,
           "append_tile_scan_kernel": 5 * 8 + 8,
           "append_tile_apply_kernel": 5 * 8 + 8}


def one(res, kernel):
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (kernel, sorted(res))
    return res[names[0]]


@pytest.mark.parametrize("kernel", KERNELS)
def test_drop_kernel_is_reported_without_scratch_or_spills(kernel):
    r = one(resources("drop"), kernel)
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("LDS Size", 0) <= LDS_MAX.get(kernel, 0), (kernel, r)
    assert r["VGPRs"] <= 64, (kernel, r)  # streaming passes: full occupancy


@pytest.mark.parametrize("kernel", SCANS)
def test_the_scan_kernels_are_the_merges_own(kernel):
    mine, theirs = one(resources("drop"), kernel), one(resources("append"), kernel)
    assert mine == theirs, (kernel, mine, theirs)


def test_every_drop_kernel_is_there_and_the_figures_are_kept():
    res = resources("drop")
    rows = []
    for kernel in KERNELS:
        r = one(res, kernel)
        rows.append("%-26s %s" % (kernel,
                                  "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "drop")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("drop.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
