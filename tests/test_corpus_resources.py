"""Register / scratch budgets of the corpus kernels (csrc/kernels/corpus.hip) from the compiler's
own resource report, as tests/test_drop_resources.py reads it (hipcc
-Rpass-analysis=kernel-resource-usage; gfx950 cross-compiles without a GPU): every kernel of the
file is there once by name and none is unaccounted for, none brings scratch or spills, LDS stays
within what the staged table and the tiles' scans need, and the figures are kept in profiles/corpus/resources.txt."""
import os

import pytest

from tests.test_rank_resources import HIPCC, ROOT, resources

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = ("corpus_restrict_kernel", "corpus_seal_kernel", "corpus_resolve_kernel",
           "corpus_head_sum_kernel", "corpus_head_scan_kernel", "corpus_head_emit_kernel",
           "corpus_off_kernel")
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "LDS Size",
           "Occupancy")
BLOCK = 256  # kCorpusBlock
LDS_SEGS = 2048  # kCorpusLdsSegs
# LDS: the restrict kernel stages neither the table nor the tile -- the table is read through the
# caches and a thread keeps its kCorpusItems pairs in registers.  What it keeps is the workgroup
# scan's one u32 per wave and one more (block_exclusive_scan) and the tile's base, one u32; each
# array may be rounded up to 16 bytes.  The seal kernel is one thread and keeps nothing.
# The resolve kernel stages the table: kCorpusLdsSegs u32 first lines, and nothing else.  The head
# kernels keep a scan's or a sum's words only: one u32 per wave (sum), one more (emit), the same
# in u64 (the one-workgroup scan of the tile array).  The offsets kernel keeps nothing.
LDS_MAX = {"corpus_restrict_kernel": ((BLOCK // 64 + 1) * 4 + 12) + 16,
           "corpus_resolve_kernel": LDS_SEGS * 4,
           "corpus_head_sum_kernel": (BLOCK // 64) * 4,
           "corpus_head_emit_kernel": (BLOCK // 64 + 1) * 4 + 12,
           "corpus_head_scan_kernel": (BLOCK // 64 + 1) * 8 + 8}


def one(res, kernel):
    names = [n for n in res if kernel in n]
    assert len(names) == 1, (kernel, sorted(res))
    return res[names[0]]


@pytest.mark.parametrize("kernel", KERNELS)
def test_corpus_kernel_is_reported_without_scratch_or_spills(kernel):
    r = one(resources("corpus"), kernel)
    print(kernel, r)
    assert r.get("ScratchSize", 0) == 0, (kernel, r)
    assert r.get("VGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("SGPRs Spill", 0) == 0, (kernel, r)
    assert r.get("LDS Size", 0) <= LDS_MAX.get(kernel, 0), (kernel, r)
    assert r["VGPRs"] <= 64, (kernel, r)  # a streaming pass: full occupancy


def test_every_corpus_kernel_is_there_and_the_figures_are_kept():
    res = resources("corpus")
    rows = []
    for kernel in KERNELS:
        r = one(res, kernel)
        rows.append("%-26s %s" % (kernel,
                                  "  ".join("%s %d" % (f, r[f]) for f in FIGURES if f in r)))
    assert len(res) == len(KERNELS), sorted(res)  # no kernel unaccounted for
    out = os.path.join(ROOT, "profiles", "corpus")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "resources.txt"), "w") as f:
        f.write("corpus.hip, hipcc -O3 --offload-arch=gfx950, kernel-resource-usage remarks\n")
        f.write("\n".join(rows) + "\n")
