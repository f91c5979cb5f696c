"""Register / scratch budgets of the append kernels (csrc/kernels/append.hip) from the compiler's
own resource report, as tests/test_tally_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, none brings scratch or spills, LDS stays
within what the tiles need, and the figures are kept in profiles/append/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = ("append_locate_kernel", "append_tile_sum_kernel", "append_tile_scan_kernel",
           "append_tile_apply_kernel", "append_records_kernel", "append_postings_kernel",
           "append_lines_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")
TILE = 1024  # kAppendTile
# LDS: the postings tile stages one source offset and one destination shift per word, at most one
# word per element, and the offset behind the last word: (TILE + 1) + TILE u64 words.  The scans
# keep one u64 per wave (4), the scanning two a fifth word for the total.  Each array may be
# rounded up to 16 bytes.
LDS_MAX = {"append_postings_kernel": ((TILE + 1) * 8 + 8) + TILE * 8,
           "append_tile_sum_kernel": 4 * 8,
           "append_tile_scan_kernel": 5 * 8 + 8,
           "append_tile_apply_kernel": 5 * 8 + 8}


@pytest.mark.parametrize("kernel", KERNELS)
def test_append_kernel_is_reported_without_scratch_or_spills(kernel):
    res = resources("append")
    names = [n for n in res if kernel in n]
    assert len(names) == 1, sorted(res)
    r = res[names[0]]
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("LDS Size", 0) <= LDS_MAX.get(kernel, 0), (kernel, r)


def test_every_append_kernel_is_there_and_the_figures_are_kept():
    res = resources("append")
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
    out = os.path.join(ROOT, "profiles", "append")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("append.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
