"""Top-K words by count on the device (csrc/kernels/topk.hip): the selection kernels alone
(``top_counts``), whole jobs (``run_top``: one pass, streamed, radix fallback), the
engine's state after a top job, and the CLI.  Every comparison is exact, against
``oracle.top`` over ``oracle.wordcount``: the order (count descending, key ascending) is
total, so there is exactly one right answer and no tolerance anywhere."""
import json
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = lc._C.kTopKMax
TILE = lc._C.kTopKTile


@pytest.fixture(scope="module")
def sel_engine():
    """One engine for every top_counts case: room for kTopKMax + TILE + 1 records."""
    return lc.Engine(lc.make_config("gpu", check=True), 1 << 20, 1 << 15)


def keys(n, seed=0):
    """n distinct keys of 1-29 bytes in unsigned-byte order, some with bytes >= 0x80."""
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        ln = rng.randrange(1, 30)
        hi = rng.random() < 0.2
        out.add(bytes(rng.randrange(0x80, 0x100) if hi and rng.random() < 0.5
                      else rng.randrange(0x21, 0x7f) for _ in range(ln)))
    return sorted(out)


def check_counts(eng, counts, k, seed=0):
    ks = keys(len(counts), seed)
    recs = list(zip(ks, counts))
    ent, pos = [], 0
    for key, c in recs:
        ent.append((key, pos, c))
        pos += c
    got = eng.top_counts(recs, k)
    assert got.entries() == oracle.top(ent, k)
    assert got.num_unique == len(counts) and got.k == k
    return got


@pytest.mark.parametrize("n", [0, 1, 9, 10, 11, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_top_counts_sizes(sel_engine, n):
    rng = random.Random(n)
    check_counts(sel_engine, [rng.randrange(1, 50) for _ in range(n)], 10, seed=n)


def test_top_counts_kmax(sel_engine):
    n = KMAX + TILE + 1
    rng = random.Random(7)
    got = check_counts(sel_engine, [rng.randrange(1, 3000) for _ in range(n)], KMAX)
    assert len(got.entries()) == KMAX


def test_top_counts_zipf_tie_quota_inside_a_tile(sel_engine):
    """Most counts are 1: the k-th count is 1, the quota of ties ends in the middle of a
    tile and the winners above it are spread over several tiles."""
    n = 3 * TILE + 500
    rng = random.Random(11)
    counts = [1] * n
    for i in rng.sample(range(n), 40):
        counts[i] = 2 + int(1000 / (1 + rng.randrange(200)))
    k = 40 + TILE + 300  # every larger count, then ties cut inside the second tile
    assert sorted(counts, reverse=True)[k - 1] == 1
    check_counts(sel_engine, counts, k)


def test_top_counts_all_equal(sel_engine):
    check_counts(sel_engine, [5] * (2 * TILE + 3), 10)  # the first 10 keys
    check_counts(sel_engine, [5] * (2 * TILE + 3), TILE + 1)


@pytest.mark.parametrize("order", ["increasing", "decreasing"])
def test_top_counts_monotone(sel_engine, order):
    counts = list(range(1, 2 * TILE + 100))
    if order == "decreasing":
        counts.reverse()
    check_counts(sel_engine, counts, 10)
    check_counts(sel_engine, counts, 1000)


@pytest.mark.parametrize("kind", ["low", "high", "mixed"])
def test_top_counts_wide_counts(sel_engine, kind):
    """Counts >= 2^32 that differ only in their low bytes, only in their high bytes, and a
    mix of both: every digit of the select matters."""
    rng = random.Random(3)
    n = TILE + 77
    low = [(1 << 33) + rng.randrange(5000) for _ in range(n)]
    high = [rng.randrange(1, 5000) << 32 for _ in range(n)]
    counts = {"low": low, "high": high,
              "mixed": [rng.choice((a, b)) for a, b in zip(low, high)]}[kind]
    check_counts(sel_engine, counts, 10)
    check_counts(sel_engine, counts, 700)


def test_top_counts_second_scan_round():
    """More than 256 tiles: topk_scan_kernel's one workgroup takes a second round and
    carries both running totals into it.  Keys already in byte order, every count 1 except
    60 winners in tile 0, tile 3 (one count >= 2^32: the carried prefix needs its high word),
    the last tile of the first round, the first of the second, and the last, partial tile.
    A winner's val is the sum of every count before it, so a winner behind tile 256 has the
    carried sum in its val; its slot has the carried number of winners in it."""
    n = 256 * TILE + TILE + 5
    tiles = -(-n // TILE)
    assert tiles > 256 and n % TILE  # a second round, a partial last tile
    rng = random.Random(13)
    counts = [1] * n
    where = {0: 18, 3: 1, 255: 19, 256: 19, tiles - 1: 3}
    assert sum(where.values()) == 60
    for tile, m in where.items():
        picked = rng.sample(range(tile * TILE, min((tile + 1) * TILE, n)), m)
        for i in picked:
            counts[i] = 2 + rng.randrange(5000)
        if tile != 255:  # one count >= 2^32 per tile, before and behind the carry
            counts[picked[0]] = (1 << 33) + 1000 * tile + 7
    assert sum(c > 1 for c in counts) == 60
    ent, pos = [], 0
    for i, c in enumerate(counts):
        ent.append((b"%07d" % i, pos, c))
        pos += c
    recs = [(key, c) for key, _v, c in ent]
    eng = lc.Engine(lc.make_config("gpu", check=True), 2 << 20, 1 << 16)
    assert eng.capacity >= n
    for k in (10, 60 + TILE + 300):  # the larger: every winner, then ties cut inside tile 1
        assert k <= KMAX
        want = oracle.top(ent, k)
        # among the expected: a record behind tile 256 whose val has the carried high word
        assert any(key >= b"%07d" % (256 * TILE) and val >= 1 << 33 for key, val, _c in want)
        got = eng.top_counts(recs, k)
        assert got.entries() == want
        assert got.num_unique == n and got.k == k
    assert want[-1][2] == 1 and TILE < int(want[-1][0]) < 2 * TILE


def test_top_counts_k_above_limit(sel_engine):
    with pytest.raises(lc.LocustError, match=str(KMAX)):
        sel_engine.top_counts([(b"a", 1), (b"b", 2)], KMAX + 1)


# ------------------------------------------------------------------------------------
# whole jobs
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hamlet_oracle(hamlet):
    win = oracle.window(hamlet, 0, 700)
    return {"window": (win, oracle.wordcount(win)), "whole": (hamlet, oracle.wordcount(hamlet))}


@pytest.mark.parametrize("map_path", ["fast", "compat"])
@pytest.mark.parametrize("which", ["window", "whole"])
def test_run_top_hamlet(hamlet_oracle, which, map_path):
    text, (ent, ntok, _) = hamlet_oracle[which]
    nl = lc._C.count_lines(text)
    eng = lc.Engine(lc.make_config("gpu", check=True, map_path=map_path), len(text), nl)
    for k in (1, 10, 1000):
        t = eng.run_top(text, k)
        assert t.entries() == oracle.top(ent, k)
        assert t.num_tokens == ntok and t.num_unique == len(ent) and t.num_lines == nl
        assert t.select_ms > 0 and "select_ms" in t.times()


def test_run_top_empty_and_few_keys():
    eng = lc.Engine(lc.make_config("gpu", check=True), 1 << 16, 1 << 10)
    t = eng.run_top(b"", 5)
    assert t.entries() == [] and t.num_unique == 0
    text = b"b a b\nc b a\n"
    t = eng.run_top(text, 10)
    assert t.entries() == oracle.top(oracle.wordcount(text)[0], 10) and len(t.entries()) == 3


def test_run_top_streamed_hamlet(hamlet_oracle):
    text, (ent, ntok, _) = hamlet_oracle["whole"]
    cfg = lc.make_config("gpu", check=True, chunk_bytes=16 << 10)
    eng = lc._C.GpuEngine(cfg, 1 << 30, 1 << 30)
    t = eng.run_top(text, 10)
    assert t.entries() == oracle.top(ent, 10) and t.num_tokens == ntok and t.chunks > 1
    assert eng.run_top_text(lc._C.HostText.from_bytes(text), 50).entries() == oracle.top(ent, 50)


def test_run_top_streamed_radix_fallback():
    """> 32,768 distinct keys: the streamed dictionary is ordered by the radix fallback,
    which also ends in the device record buffer the selection reads."""
    text = lc._C.gen_text(lines=60000, seed=3)
    ent, ntok, _ = oracle.wordcount(text)
    assert len(ent) > 32768
    cfg = lc.make_config("gpu", check=True, chunk_bytes=512 << 10)
    eng = lc._C.GpuEngine(cfg, 1 << 30, 1 << 30)
    t = eng.run_top_text(lc._C.HostText.from_bytes(text), 1000)
    assert t.entries() == oracle.top(ent, 1000)
    assert t.num_tokens == ntok and t.num_unique == len(ent)


def test_top_jobs_leave_the_engine_clean(hamlet_oracle):
    """Top jobs and full jobs interleaved on one engine, two texts: a top job must leave
    the scratch, the counters and the output pool as a full job expects them."""
    a, (ent_a, ntok_a, _) = hamlet_oracle["window"]
    b, (ent_b, ntok_b, _) = hamlet_oracle["whole"]
    eng = lc.Engine(lc.make_config("gpu", check=True), len(b), b.count(b"\n"))
    assert eng.run(a).entries() == ent_a  # (a lean job first: it leaves the scratch clean)
    assert eng.run_top(a, 5).entries() == oracle.top(ent_a, 5)
    r = eng.run(b)
    assert r.entries() == ent_b and r.num_tokens == ntok_b
    assert eng.run_top(b, 50).entries() == oracle.top(ent_b, 50)
    r = eng.run(a)
    assert r.entries() == ent_a and r.num_tokens == ntok_a
    assert eng.run(b).entries() == ent_b


def test_wire_bytes(hamlet_oracle):
    text, (ent, _, _) = hamlet_oracle["whole"]
    k = 10
    t = lc.top_words_text(text, k)
    assert t.entries() == oracle.top(ent, k)
    assert 0 < t.wire_bytes <= k * 48 + 64
    assert lc.wordcount_text(text).wire_bytes > 10 * t.wire_bytes


def test_run_top_rejects(hamlet):
    with pytest.raises(lc.LocustError, match=str(KMAX)):
        lc.top_words_text(hamlet, KMAX + 1)
    with pytest.raises(lc.LocustError, match="dict"):
        lc.top_words_text(hamlet, 3, sort="radix")
    with pytest.raises(lc.LocustError, match="ref_timers"):
        lc.top_words_text(hamlet, 3, ref_timers=True)


# ------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


def test_cli_top(cli, hamlet_oracle, tmp_path):
    ent = hamlet_oracle["whole"][1][0]
    j = tmp_path / "top.json"
    p = subprocess.run([cli, "data/hamlet.txt", "--top", "10", "--json", str(j)], cwd=ROOT,
                       capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_gpu(oracle.top(ent, 10))
    assert p.stdout.startswith(b"Running\nLength: ") and p.stdout.endswith(b"\nDone\n")
    rec = json.load(open(j))
    assert rec["top_k"] == 10 and rec["unique"] == len(ent)
    assert rec["select_ms"] > 0 and 0 < rec["wire_bytes"] <= 10 * 48 + 64
    # a line window (the loader path) and --result-file
    went = hamlet_oracle["window"][1][0]
    rf = tmp_path / "res.txt"
    p = subprocess.run([cli, "data/hamlet.txt", "0", "700", "--top", "10", "--result-file",
                        str(rf)], cwd=ROOT, capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert rf.read_bytes() == oracle.format_gpu(oracle.top(went, 10))
    assert b"print key:" not in p.stdout


def test_cli_top_errors(cli):
    p = subprocess.run([cli, "data/hamlet.txt", "--sort", "radix", "--top", "3"], cwd=ROOT,
                       capture_output=True, timeout=100)
    assert p.returncode != 0 and b"--sort dict" in p.stderr and b"print key" not in p.stdout
    p = subprocess.run([cli, "data/hamlet.txt", "--top", str(KMAX + 1)], cwd=ROOT,
                       capture_output=True, timeout=100)
    assert p.returncode != 0 and str(KMAX).encode() in p.stderr
