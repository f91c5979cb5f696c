"""Dropping the oldest lines without a GPU: the host trim of an index (``trim_index``) against the
oracle's index of the remaining text (exactly), the unmerge identity with ``merge_index``, and the
CLI's ``--keep-blocks`` with ``--backend cpu``, whose result lines are those of the run over the
window's lines."""
import json
import os
import random

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.test_append import SHAPES, cpu_index, fuzz_text, nlines, result_lines, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["all_new", "all_old", "interleaved", "all_before", "all_after"]


def lines_of(text):
    """The text's lines with their newlines (the last one may lack it)."""
    parts = text.split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def stats_of(text, **okw):
    """(overflow_lines, truncated) of the word job over `text`."""
    _e, _t, over, trunc = oracle.wordcount(text, stats=True, **okw)
    return over, trunc


def check_trim(text, d, first_line=0, cfg=None, **okw):
    """trim_index(index of `text`, d) against the oracle's index of the remaining lines."""
    cfg = cfg or {}
    ls = lines_of(text)
    gone, rest = b"".join(ls[:d]), b"".join(ls[d:])
    x = cpu_index(text, first_line, **cfg)
    over, trunc = stats_of(gone, **okw)
    got = lc.trim_index(x, d, over, trunc)
    ent, post = oracle.index(rest, first_line=first_line + d, **okw)
    assert got.entries() == ent
    assert got.postings() == post
    assert got.first_line == first_line + d and got.num_lines == len(ls) - d
    assert got.num_tokens == len(post) and got.num_unique == len(ent)
    assert (got.overflow_lines, got.truncated) == stats_of(rest, **okw)
    assert got.max_key_len == x.max_key_len
    return got


@pytest.mark.parametrize("shape", FIVE)
def test_trim_equals_the_index_of_the_remaining_text(shape):
    a, b = SHAPES[shape]
    for d in (1, nlines(a) - 1, nlines(a), nlines(a) + 1, nlines(a + b) - 1):
        check_trim(a + b, d)


def test_trim_under_truncation_and_the_emit_cap():
    text = (b"alphabet alpha alphas beta\nbetamax gamma gamma\nalphanumeric betas delta\n"
            b"gamma alpha\nalphabets\n")
    for d in range(0, 6):
        got = check_trim(text, d, cfg=dict(emits_per_line=2, max_key_len=5), emits=2, max_key=5)
    assert got.num_unique == 0
    full = cpu_index(text, emits_per_line=2, max_key_len=5)
    assert full.overflow_lines == 3 and full.truncated == 4


def test_trim_with_a_first_line():
    a, b = SHAPES["interleaved"]
    got = check_trim(a + b, 5, first_line=1000)
    assert min(got.postings()) == 1005


@pytest.mark.parametrize("seed", range(20))
def test_trim_fuzz(seed):
    rng = random.Random(7000 + seed)
    text = fuzz_text(rng) + fuzz_text(rng)
    if rng.random() < 0.3 and text:
        text = text[:-1]  # the last line may lack its newline
    n = nlines(text)
    d = rng.choice([0, n, rng.randrange(0, n + 1)])
    check_trim(text, d, first_line=seed * 3)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_trim_undoes_a_merge(shape):
    a, b = SHAPES[shape]
    ia, ib = cpu_index(a), cpu_index(b, nlines(a))
    got = lc.trim_index(lc.merge_index(ia, ib), ia.num_lines, ia.overflow_lines, ia.truncated)
    assert (got.entries(), got.postings(), got.first_line) == \
        (ib.entries(), ib.postings(), ib.first_line)
    assert (got.num_lines, got.num_tokens, got.num_unique, got.overflow_lines, got.truncated) == \
        (ib.num_lines, ib.num_tokens, ib.num_unique, ib.overflow_lines, ib.truncated)
    assert got.max_key_len >= ib.max_key_len


def test_trim_undoes_a_merge_under_the_statistics():
    a = b"alphabet alpha alphas beta\nbetamax gamma gamma\n"
    b = b"alphanumeric betas delta\ngamma alpha\n"
    kw = dict(emits_per_line=2, max_key_len=5)
    ia, ib = cpu_index(a, **kw), cpu_index(b, 2, **kw)
    assert ia.overflow_lines == 2 and ia.truncated == 2
    got = lc.trim_index(lc.merge_index(ia, ib), 2, ia.overflow_lines, ia.truncated)
    assert (got.entries(), got.postings()) == (ib.entries(), ib.postings())
    assert (got.overflow_lines, got.truncated) == (ib.overflow_lines, ib.truncated)


def test_trim_nothing_and_everything():
    a, b = SHAPES["interleaved"]
    x = cpu_index(a + b, 4)
    same = lc.trim_index(x, 0)
    assert (same.entries(), same.postings(), same.first_line, same.num_lines) == \
        (x.entries(), x.postings(), 4, x.num_lines)
    none = lc.trim_index(x, x.num_lines)
    assert (none.entries(), none.postings()) == ([], [])
    assert (none.first_line, none.num_lines, none.num_tokens, none.num_unique) == \
        (4 + x.num_lines, 0, 0, 0)
    # an unterminated last line goes with the rest, and an index goes on from an empty one
    y = cpu_index(b"a b\nb c", 0)
    assert lc.trim_index(y, 2).entries() == []
    again = lc.merge_index(none, cpu_index(b"x\n", 4 + x.num_lines))
    assert again.postings() == [4 + x.num_lines]


def test_trim_refuses_more_lines_than_the_index_holds():
    x = cpu_index(b"a b\nb c\n")
    with pytest.raises(lc.LocustError, match="3 lines.*holds 2"):
        lc.trim_index(x, 3)
    with pytest.raises(lc.LocustError, match="statistics"):
        lc.trim_index(x, 1, 1, 0)
    assert lc.trim_index(x, 2).num_lines == 0


def test_python_helpers_take_keep_blocks(hamlet):
    text = oracle.window(hamlet, 0, 600)
    blocks = lc.split_blocks(text, 4096)
    assert len(blocks) > 3
    off, _n, _l, first = blocks[-2]
    window = text[off:]
    x = lc.index_text(text, backend="cpu", block_bytes=4096, keep_blocks=2)
    assert (x.entries(), x.postings()) == oracle.index(window, first_line=first)
    assert x.first_line == first and x.num_lines == nlines(window)
    got = lc.search_text(text, [[b"my", b"lord"]], "phrase", backend="cpu", show=40,
                         block_bytes=4096, keep_blocks=2)
    want = lc.search_text(window, [[b"my", b"lord"]], "phrase", backend="cpu", show=40,
                          first_line=first)
    assert got.lines(0) == want.lines(0) and got.lines(0) and got.format() == want.format()
    assert got.first_line == first
    # fewer blocks than the window: nothing is dropped
    all_of_it = lc.index_text(text, backend="cpu", block_bytes=4096, keep_blocks=len(blocks))
    assert all_of_it.postings() == oracle.index(text)[1]
    with pytest.raises(ValueError, match="block_bytes"):
        lc.index_text(text, backend="cpu", keep_blocks=2)
    with pytest.raises(lc.LocustError, match="GPU engine"):
        lc.Engine(lc.make_config("cpu")).drop_index(1)


@pytest.mark.parametrize("args", [
    ["--index"],
    ["--search", "to be", "--match", "phrase", "--show", "80", "--mark"],
], ids=["index", "phrase"])
def test_cli_cpu_keep_blocks_gives_the_windows_result_lines(cli, hamlet, args, tmp_path):
    j = tmp_path / "k.json"
    blocks = lc.split_blocks(hamlet, 32 << 10)
    assert len(blocks) == 6
    start, total = blocks[-2][3], nlines(hamlet)
    want = run(cli, "data/hamlet.txt", start, total, *args, "--backend", "cpu")
    got = run(cli, "data/hamlet.txt", *args, "--backend", "cpu", "--block-kb", 32,
              "--keep-blocks", 2, "--json", j)
    assert want.returncode == 0 and got.returncode == 0, got.stderr.decode()[-2000:]
    assert result_lines(want.stdout) and result_lines(got.stdout) == result_lines(want.stdout)
    rec = json.load(open(j))
    assert rec["blocks"] == 6 and rec["dropped_blocks"] == 4 and rec["first_line"] == start
    assert rec["drop_ms"] == 0 and rec["index_store_bytes"] == 0


@pytest.mark.parametrize("args, msg", [
    (["--index", "--keep-blocks", "2"], "--block-kb"),
    (["--index", "--block-kb", "32", "--keep-blocks", "0"], "M >= 1"),
    (["--keep-blocks", "2", "--block-kb", "32"], "--index"),
])
def test_cli_keep_blocks_refusals(cli, args, msg):
    p = run(cli, "data/hamlet.txt", *args, "--backend", "cpu")
    assert p.returncode != 0
    assert msg.encode() in p.stderr and (b"--keep-blocks" in p.stderr or b"--block-kb" in p.stderr)
    assert b"print " not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--keep-blocks" in p.stdout
