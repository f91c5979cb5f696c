"""Inverted index on the device (csrc/kernels/index.hip): ``Engine.run_index`` against
``oracle.index``.  Every comparison is exact -- the pairs are sorted by (key, line), so
there is exactly one right answer and no tolerance anywhere.  The shapes are the smallest
at which each part of the stage can go wrong: the 64-byte step of the line walk, the emit
cap, NULs, key truncation, the sort's two regimes and the binary search over thousands of
records.  The scale edges need their size: the second round of the one-workgroup tile scan
and the map grid's stride (more than 524,288 records and lines), the dictionary's radix
fallback (more than 32,768 distinct keys), the large-input path (more than 8 MiB), one line
of thousands of bytes, pinned host text, and the last line number a u32 holds."""
import functools
import json
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SORT = 8192  # kSmallSortMax: the single-workgroup sort's last size


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases: a small pass, zero-copy text."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, first_line=0, **okw):
    want_e, want_p = oracle.index(text, first_line=first_line, **okw)
    got = engine.run_index(text, first_line)
    assert got.entries() == want_e
    assert got.postings() == want_p
    assert got.num_tokens == len(want_p) and got.num_unique == len(want_e)
    assert got.first_line == first_line
    return got


# ------------------------------------------------------------------------------------
# the line walk
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word\n", b"word", b"\n", b"\n\n\n", b" ,.\n"])
def test_tiny_inputs(eng, text):
    got = check(eng, text)
    assert got.format() == oracle.format_index(*oracle.index(text))


def pad_line(n, tail):
    """A line of n bytes: two-letter words and spaces, then `tail` at its very end."""
    body = (b"ab " * n)[:n - len(tail)]
    return body[:-1] + b" " + tail if body else tail


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_step_boundaries(n):
    """Tokens that start in lane 63, span the 64-byte step boundary and end exactly at
    byte 64, in lines of 63, 64, 65 and 130 bytes with varied padding."""
    engine = lc.Engine(gpu_cfg(emits_per_line=100), 1 << 16, 1 << 10)
    lines = []
    for tail in (b"z", b"yz", b"wxyz", b"q" * 20):
        lines.append(pad_line(n, tail))
        assert len(lines[-1]) == n
    # a one-byte token in lane 63, a token spanning bytes 62..66, one ending at byte 64
    lines.append(b"a" * 62 + b" " + b"k")
    lines.append(b"b " * 31 + b"spans")
    lines.append(b"c" * 59 + b" " + b"ends" + b" after")
    lines.append(b" " * 63 + b"lane63start and more")
    lines.append(b"x" * n)  # one token as long as the line (truncated to max_key)
    text = b"\n".join(lines) + b"\n"
    check(engine, text, emits=100)
    check(engine, b"\n".join(reversed(lines)), emits=100)  # ... and no final newline


def test_emit_cap():
    forty = b" ".join(bytes([97 + i % 26]) for i in range(40))
    long3 = b" ".join(b"%03d" % i for i in range(51))  # 203 bytes of 3-byte words
    text = forty + b"\n" + long3 + b"\nnext line here\n" + forty + b"\n"
    e20 = lc.Engine(gpu_cfg(emits_per_line=20), 1 << 16, 1 << 10)
    got = check(e20, text, emits=20)  # the cap falls inside the first step
    assert got.overflow_lines == 3
    e30 = lc.Engine(gpu_cfg(emits_per_line=30), 1 << 16, 1 << 10)
    check(e30, text, emits=30)  # ... in a later step of the 3-byte words' line
    e1 = lc.Engine(gpu_cfg(emits_per_line=1), 1 << 16, 1 << 10)
    got = check(e1, text, emits=1)
    assert got.num_tokens == 4


def test_nul_ends_the_lines_tokens(eng):
    text = (b"one two\0three four\nfive six\n" +
            b"p" * 30 + b" " + b"q" * 30 + b" " + b"r" * 20 + b" late\0dropped words\n" +
            b"\0nothing here\nlast line\n" + b"tok\0")
    got = check(eng, text)
    keys = [k for k, _v, _c in got.entries()]
    assert b"three" not in keys and b"dropped" not in keys and b"nothing" not in keys
    assert b"five" in keys and b"late" in keys and b"last" in keys and b"tok" in keys


def test_truncation_merges_lists(eng):
    a = b"x" * 29 + b"AAAAAA"
    b = b"x" * 29 + b"BBBBBB"
    exact = b"y" * 29
    text = a + b" foo\nbar " + b + b"\n" + exact + b" " + a + b"\n"
    got = check(eng, text)
    assert got.lines(b"x" * 29) == [0, 1, 2] and got.lines(exact) == [2]
    assert got.truncated == 3
    short = lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)
    got = check(short, b"abcdefgh abcdeXYZ\nabcde abcd\n", max_key=5)
    assert got.lines(b"abcde") == [0, 0, 1] and got.lines(b"abcd") == [1]


def test_line_ends_and_high_bytes(eng):
    text = (b"caf\xc3\xa9 na\xefve \xff\xfe\r\nsecond line\r\n\r\n" +
            b"caf\xc3\xa9 again\r\nno newline at the end \x80")
    got = check(eng, text)
    assert got.lines(b"caf\xc3\xa9") == [0, 3]
    assert got.lines(b"line\r") == [1] and got.lines(b"\r") == [2]
    assert got.lines(b"\x80") == [4]


def test_same_word_three_times_on_a_line(eng):
    got = check(eng, b"a b a\nrose is a rose is a rose\nb\n")
    assert got.lines(b"rose") == [1, 1, 1] and got.lines(b"rose", unique=True) == [1]
    assert got.lines(b"a") == [0, 0, 1, 1] and got.lines(b"a", True) == [0, 1]
    assert got.lines(b"absent") == []


def test_first_line_offset(eng):
    text = b"alpha beta\nbeta gamma\n\nalpha\n"
    got = check(eng, text, first_line=1000)
    assert got.lines(b"alpha") == [1000, 1003]
    assert min(got.postings()) >= 1000 and max(got.postings()) < 1000 + 4


# ------------------------------------------------------------------------------------
# sort regimes and the search
# ------------------------------------------------------------------------------------
ALPHA = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"


def words(n, seed):
    """n distinct keys of 1-12 bytes (no delimiters), some with bytes >= 0x80."""
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        ln = rng.randrange(1, 13)
        hi = rng.random() < 0.2
        out.add(bytes(rng.randrange(0x80, 0x100) if hi and rng.random() < 0.5
                      else rng.choice(ALPHA) for _ in range(ln)))
    return sorted(out)


@pytest.mark.parametrize("tokens", [SMALL_SORT, SMALL_SORT + 1])
def test_small_sort_threshold(eng, tokens):
    rng = random.Random(tokens)
    vocab = words(300, 1)
    lines = [b" ".join(rng.choice(vocab) for _ in range(16)) for _ in range(SMALL_SORT // 16)]
    if tokens > SMALL_SORT:
        lines.append(vocab[0])
    text = b"\n".join(lines) + b"\n"
    got = check(eng, text)
    assert got.num_tokens == tokens


def test_one_long_list_on_the_device_wide_sort(eng):
    """One word on ~9,000 lines (a list longer than two 4096-key sort tiles) among a few
    hundred rare words."""
    rng = random.Random(5)
    rare = words(300, 2)
    lines = []
    for i in range(9000):
        line = [b"the"]
        if i % 30 == 0:
            line.insert(rng.randrange(2), rng.choice(rare))
        lines.append(b" ".join(line))
    got = check(eng, b"\n".join(lines) + b"\n")
    assert got.lines(b"the") == list(range(9000))


def test_search_over_thousands_of_records(eng):
    """~5,000 distinct words, exactly one of them twice; the first and the last key of the
    dictionary are in the text."""
    vocab = words(5000, 3)
    order = list(vocab)
    random.Random(4).shuffle(order)
    order.append(vocab[2500])
    lines = [b" ".join(order[i:i + 7]) for i in range(0, len(order), 7)]
    got = check(eng, b"\n".join(lines) + b"\n")
    ent = got.entries()
    assert ent[0][0] == vocab[0] and ent[-1][0] == vocab[-1] and len(ent) == 5000
    assert [c for _k, _v, c in ent].count(2) == 1 and len(got.lines(vocab[2500])) == 2


@functools.lru_cache(maxsize=None)
def past_zero_copy_text():
    rng = random.Random(9)
    vocab = words(3000, 6)
    lines = []
    size = 0
    while size < (3 << 19):
        lines.append(b" ".join(rng.choices(vocab, k=8)))
        size += len(lines[-1]) + 1
    return b"\n".join(lines) + b"\n"


def test_input_past_zero_copy():
    """1.5 MiB of generated lines: the text is copied to the device, not read in place."""
    text = past_zero_copy_text()
    assert len(text) > (1 << 20)
    engine = lc.Engine(gpu_cfg(), len(text), lc._C.count_lines(text))
    check(engine, text)


# ------------------------------------------------------------------------------------
# scale edges: each test asserts the property that makes it reach its edge
# ------------------------------------------------------------------------------------
INDEX_TILE = 2048      # kIndexTile: records per workgroup of the offsets kernels
SCAN_BLOCK = 256       # kIndexBlock: tile sums the one-workgroup scan takes per round
MAP_WAVES = 2048 * 4   # kIdxMapMaxBlocks workgroups of 4 waves
MAP_GROUP = 64         # the most lines a wave takes per slot reservation
RANK_SORT_MAX = 32768  # kRankSortMax: more distinct keys take the dictionary's radix fallback


def test_second_round_of_scan_and_grid():
    """~545,000 lines, a word of its own on almost every one: more records than one round
    of index_tile_scan_kernel covers (the carry between rounds), more lines than one sweep
    of index_map_kernel's full grid at group = 64 (the grid-stride step), and more distinct
    keys than the rank sort takes (the records reach the index stage by the radix fallback)."""
    n_lines = 545_000
    extra = b" " + b" ".join(b"t%d" % j for j in range(25))
    lines = []
    for i in range(n_lines):
        if i % 100 == 57:
            lines.append(b"")
            continue
        line = b"%05x" % i
        if i % 3 == 0:
            line += b" shared"
        if i % 1000 == 0:
            line += extra  # 26 or 27 tokens: past the emit cap
        lines.append(line)
    text = b"\n".join(lines) + b"\n"
    del lines
    want_e, want_p = oracle.index(text)
    num_lines = lc._C.count_lines(text)
    assert num_lines == n_lines and num_lines > MAP_GROUP * MAP_WAVES
    assert len(want_e) > SCAN_BLOCK * INDEX_TILE and len(want_e) > RANK_SORT_MAX
    engine = lc.Engine(gpu_cfg(), len(text), num_lines)
    got = engine.run_index(text)
    assert got.entries() == want_e
    assert got.postings() == want_p
    assert got.num_tokens == len(want_p) and got.num_unique == len(want_e)
    assert got.num_lines == n_lines and got.first_line == 0
    assert got.overflow_lines == len(range(0, n_lines, 1000)) and got.truncated == 0
    assert got.lines(b"shared") == [i for i in range(n_lines) if i % 3 == 0 and i % 100 != 57]
    assert got.lines(b"%05x" % (n_lines - 1)) == [n_lines - 1]


def test_dict_fallback_smallest():
    """Just past 32,768 distinct words: the dictionary job is finished on the radix path and
    the index stage reads the records from where that path leaves them.  Word jobs before
    and after it on the same engine."""
    vocab = words(33_000, 8)
    order = list(vocab)
    random.Random(12).shuffle(order)
    order += [order[5], order[20_000], order[5], vocab[0], vocab[-1]]  # repeats, lines apart
    lines = [b" ".join(order[i:i + 7]) for i in range(0, len(order), 7)]
    text = b"\n".join(lines) + b"\n"
    ent, ntok, _ = oracle.wordcount(text)
    engine = lc.Engine(gpu_cfg(), len(text), lc._C.count_lines(text))
    r = engine.run(text)
    assert r.entries() == ent and r.num_tokens == ntok
    got = check(engine, text)
    assert got.num_unique == 33_000 and got.num_unique > RANK_SORT_MAX
    assert got.entries() == ent
    assert got.lines(order[5]) == [0, 33_000 // 7, 33_000 // 7]
    assert got.lines(order[20_000]) == [20_000 // 7, 33_000 // 7]
    r = engine.run(text)
    assert r.entries() == ent and r.num_tokens == ntok


def test_above_large_input():
    """Just above 8 MiB (kMapLargeInput): large map tiles, piecewise upload, the two-kernel
    ordered build; index and top jobs against the CPU engine (tied to the oracle by
    test_index.py and test_topk.py).  Twice on one engine: the second round runs on the
    retuned partition map."""
    block = lc._C.gen_text(bytes=1 << 20, seed=5)
    text = block * (((8 << 20) // len(block)) + 1)
    assert (8 << 20) < len(text) < (10 << 20)
    cpu = lc.make_config("cpu")
    want = lc._C.cpu_run_index(cpu, text, 5)
    want_e, want_p = want.entries(), want.postings()
    want_top = lc._C.cpu_run_top(cpu, text, 1000).entries()
    assert len(want_top) == 1000 and want.num_unique <= RANK_SORT_MAX  # (no radix fallback)
    engine = lc.Engine(gpu_cfg(), len(text), lc._C.count_lines(text))
    for _ in range(2):
        got = engine.run_index(text, 5)
        assert got.entries() == want_e
        assert got.postings() == want_p
        assert (got.num_tokens, got.num_unique) == (want.num_tokens, want.num_unique)
        assert (got.overflow_lines, got.truncated) == (want.overflow_lines, want.truncated)
        assert engine.run_top(text, 1000).entries() == want_top


@pytest.mark.parametrize("which", ["hamlet_window", "past_zero_copy"])
def test_pinned_host_text(hamlet_index, which):
    """run_index_text on text in pinned host memory (the direct upload mode) gives what
    run_index gives on the same bytes."""
    text = hamlet_index["window"][0] if which == "hamlet_window" else past_zero_copy_text()
    want = oracle.index(text, first_line=3)
    engine = lc._C.GpuEngine(gpu_cfg(), len(text), lc._C.count_lines(text))
    pinned = lc._C.HostText.from_bytes(text)
    got = engine.run_index_text(pinned, first_line=3)
    assert (got.entries(), got.postings()) == want
    assert got.first_line == 3 and got.num_lines == lc._C.count_lines(text)
    plain = engine.run_index(text, 3)
    assert (plain.entries(), plain.postings()) == want
    assert (got.num_tokens, got.overflow_lines, got.truncated) == (
        plain.num_tokens, plain.overflow_lines, plain.truncated)
    got = engine.run_index_text(pinned, first_line=3)  # ... and again after a pageable job
    assert (got.entries(), got.postings()) == want


def test_one_long_line():
    """One line of 1,250 words of 1-6 bytes (5,000-odd bytes), no final newline: its one wave
    walks ~90 steps of 64 bytes.  With emits_per_line = 1000 the cap falls deep inside the
    line; a NUL at byte 3,000 ends the tokens before the cap; with emits_per_line = 5000 the
    cap is never reached."""
    rng = random.Random(21)
    toks = [bytes(rng.choice(ALPHA) for _ in range(rng.randrange(1, 7))) for _ in range(1250)]
    line = b" ".join(toks)
    assert len(toks) > 1200 and 5000 < len(line) < 6500
    cap_byte = len(b" ".join(toks[:1000]))
    assert 50 * 64 < cap_byte < len(line) - 64  # the 1000th token: far in, not at the end
    nul = line[:3000] + b"\0" + line[3001:]

    def run(engine, text, emits):
        got = check(engine, text, emits=emits)
        want = oracle.wordcount(text, emits=emits, stats=True)
        assert (got.num_tokens, got.overflow_lines, got.truncated) == want[1:]
        return got

    e1000 = lc.Engine(gpu_cfg(emits_per_line=1000), 1 << 16, 1 << 10)
    got = run(e1000, line, 1000)
    assert got.num_tokens == 1000 and got.overflow_lines == 1
    got = run(e1000, nul, 1000)
    assert got.num_tokens < 1000 and got.overflow_lines == 0
    e5000 = lc.Engine(gpu_cfg(emits_per_line=5000), 1 << 16, 1 << 10)
    got = run(e5000, line, 5000)
    assert got.num_tokens == len(toks) and got.overflow_lines == 0


def test_first_line_limit(eng):
    """first_line + num_lines == 2^32 is the last accepted value."""
    text = b"alpha beta\nbeta gamma\n\nalpha\n"
    got = check(eng, text, first_line=2**32 - 4)
    assert max(got.postings()) == 2**32 - 1
    assert got.lines(b"alpha") == [2**32 - 4, 2**32 - 1]
    with pytest.raises(lc.LocustError, match=r"2\^32"):
        eng.run_index(text, 2**32 - 3)
    check(eng, text, first_line=1)  # the refusal leaves the engine usable


# ------------------------------------------------------------------------------------
# Hamlet, engine state
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hamlet_index(hamlet):
    win = oracle.window(hamlet, 0, 700)
    return {"window": (win, oracle.index(win)), "whole": (hamlet, oracle.index(hamlet))}


@pytest.mark.parametrize("which", ["window", "whole"])
def test_hamlet(hamlet_index, which):
    text, (ent, post) = hamlet_index[which]
    engine = lc.Engine(gpu_cfg(), len(text), lc._C.count_lines(text))
    got = engine.run_index(text)
    assert got.entries() == ent and got.postings() == post
    assert engine.run(text).entries() == got.entries()
    assert got.index_ms > 0 and "index_ms" in got.times()
    assert got.wire_bytes >= 4 * len(post) + 40 * len(ent)
    assert got.format() == oracle.format_index(ent, post)


def test_index_text_and_file(hamlet_index):
    win, (ent, post) = hamlet_index["window"]
    got = lc.index_text(win, check=True)
    assert (got.entries(), got.postings()) == (ent, post)
    sub = lc.index_file(os.path.join(ROOT, "data", "hamlet.txt"), 100, 300, check=True)
    text = oracle.window(hamlet_index["whole"][0], 100, 300)
    assert (sub.entries(), sub.postings()) == oracle.index(text, first_line=100)
    assert sub.first_line == 100


def test_index_jobs_leave_the_engine_clean(hamlet_index):
    """run, run_index, run_top, run on one engine give what fresh engines give: the index
    job leaves the counters, the look-back scratch and the output pool usable."""
    a, (ent_a, post_a) = hamlet_index["window"]
    b, (ent_b, post_b) = hamlet_index["whole"]
    engine = lc.Engine(gpu_cfg(), len(b), lc._C.count_lines(b))
    assert engine.run(a).entries() == ent_a  # (a lean job first: it leaves the scratch clean)
    got = engine.run_index(a)
    assert (got.entries(), got.postings()) == (ent_a, post_a)
    assert engine.run_top(b, 20).entries() == oracle.top(ent_b, 20)
    r = engine.run(b)
    assert r.entries() == ent_b and r.num_tokens == len(post_b)
    got_b = engine.run_index(b)  # the workspace grows
    assert (got_b.entries(), got_b.postings()) == (ent_b, post_b)
    assert got.postings() == post_a  # the earlier result is its own copy
    assert engine.run(a).entries() == ent_a
    got = engine.run_index(a)  # ... and is reused for a smaller job
    assert (got.entries(), got.postings()) == (ent_a, post_a)


# ------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, msg", [
    ({"sort": "radix"}, "sort=dict"),
    ({"map_path": "compat"}, "map_path fast"),
    ({"ngram": 2}, "ngram"),
    ({"ref_timers": True}, "ref_timers"),
])
def test_refusals(kw, msg):
    engine = lc.Engine(gpu_cfg(**kw), 1 << 16, 1 << 10)
    with pytest.raises(lc.LocustError, match=msg):
        engine.run_index(b"some text\n")


def test_refuses_more_than_one_pass(hamlet):
    engine = lc._C.GpuEngine(gpu_cfg(chunk_bytes=16 << 10), 1 << 30, 1 << 30)
    with pytest.raises(lc.LocustError, match="--backend cpu"):
        engine.run_index(hamlet)


# ------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


def test_cli_index(cli, hamlet_index, tmp_path):
    ent, post = hamlet_index["window"][1]
    j = tmp_path / "index.json"
    p = subprocess.run([cli, "data/hamlet.txt", "0", "700", "--index", "--check", "--json",
                        str(j)], cwd=ROOT, capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_index(ent, post)
    assert p.stdout.startswith(b"Running\n") and p.stdout.endswith(b"\nDone\n")
    rec = json.load(open(j))
    assert rec["index"] is True and rec["postings"] == len(post)
    assert rec["index_ms"] > 0 and rec["wire_bytes"] >= 4 * len(post)
    assert rec["unique"] == len(ent)
