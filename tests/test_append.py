"""Appending to the index without a GPU: the host merge of two indexes (``merge_index``) against
the oracle's index of the concatenated text (exactly), ``split_blocks``, and the CLI's
``--block-kb`` with ``--backend cpu``, whose result lines are those of the run without it."""
import json
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def nlines(text):
    return text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)


def cpu_index(text, first_line=0, **kw):
    return lc._C.cpu_run_index(lc.make_config("cpu", check=True, **kw), text, first_line)


def merged(pieces, first_line=0, **kw):
    """The fold of merge_index over the pieces' own indexes."""
    x = cpu_index(pieces[0], first_line, **kw)
    line = first_line + nlines(pieces[0])
    for p in pieces[1:]:
        x = lc.merge_index(x, cpu_index(p, line, **kw))
        line += nlines(p)
    return x


def words(prefix, n):
    return [b"%s%03d" % (prefix, i) for i in range(n)]


def text_of(ws, per_line=3):
    return b"".join(b" ".join(ws[i:i + per_line]) + b"\n" for i in range(0, len(ws), per_line))


A_WORDS = words(b"m", 30)
SHAPES = {
    "all_new": (text_of(A_WORDS), text_of(words(b"n", 30))),
    "all_old": (text_of(A_WORDS), text_of(A_WORDS[::-1] + A_WORDS[:7])),
    "interleaved": (text_of(words(b"m", 40)[0::2] + [b"zz"]),
                    text_of(words(b"m", 40)[1::2] + words(b"m", 40)[0:10] + [b"aa"])),
    "all_before": (text_of(A_WORDS), text_of(words(b"a", 25))),
    "all_after": (text_of(A_WORDS), text_of(words(b"z", 25))),
    "empty_a": (b"", text_of(A_WORDS)),
    "empty_b": (text_of(A_WORDS), b""),
    "blank_lines_a": (b"\n\n", b"x\n"),
    "no_final_newline": (b"a b\n", b"b c"),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_merge_equals_the_index_of_the_concatenation(shape):
    a, b = SHAPES[shape]
    got = merged([a, b])
    ent, post = oracle.index(a + b)
    assert (got.entries(), got.postings()) == (ent, post)
    assert got.num_lines == nlines(a) + nlines(b) and got.first_line == 0
    assert got.num_tokens == len(post) and got.num_unique == len(ent)


def test_merge_under_truncation_and_the_emit_cap():
    a = b"alphabet alpha alphas beta\nbetamax gamma gamma\n"
    b = b"alphanumeric betas delta\ngamma alpha\n"
    got = merged([a, b], max_key_len=5)
    assert (got.entries(), got.postings()) == oracle.index(a + b, max_key=5)
    assert dict((k, c) for k, _v, c in got.entries())[b"alpha"] == 5
    got = merged([a, b], emits_per_line=1)
    assert (got.entries(), got.postings()) == oracle.index(a + b, emits=1)
    one = cpu_index(a + b, emits_per_line=1)
    assert got.num_tokens == one.num_tokens == 4


def test_merge_with_a_first_line():
    a, b = SHAPES["interleaved"]
    got = merged([a, b], first_line=1000)
    assert (got.entries(), got.postings()) == oracle.index(a + b, first_line=1000)
    assert got.first_line == 1000 and min(got.postings()) == 1000


def test_merge_folds_over_eight_blocks(hamlet):
    text = oracle.window(hamlet, 0, 640)
    lines = text.split(b"\n")[:-1]
    pieces = [b"".join(l + b"\n" for l in lines[i:i + 80]) for i in range(0, 640, 80)]
    assert len(pieces) == 8 and b"".join(pieces) == text
    got = merged(pieces)
    assert (got.entries(), got.postings()) == oracle.index(text)
    assert got.format() == cpu_index(text).format()


def fuzz_text(rng):
    alphabet = rng.choice([b"ab", b"abc", b"xyZ01"])
    out = []
    for _ in range(rng.randrange(0, 30)):
        if rng.random() < 0.15:
            out.append(b"")
            continue
        line = bytearray()
        for _ in range(rng.randrange(1, 9)):
            line += bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 4)))
            line += bytes(rng.choice(b" \t,.;") for _ in range(rng.randrange(1, 4)))
            if rng.random() < 0.03:
                line += b"\0"
        out.append(bytes(line))
    return b"".join(l + b"\n" for l in out)


@pytest.mark.parametrize("seed", range(50))
def test_merge_fuzz(seed):
    rng = random.Random(seed)
    text = fuzz_text(rng)
    lines = text.split(b"\n")[:-1]
    cut = rng.randrange(0, len(lines) + 1)
    a = b"".join(l + b"\n" for l in lines[:cut])
    b = b"".join(l + b"\n" for l in lines[cut:])
    if rng.random() < 0.3 and b:
        b = b[:-1]  # the last block may lack its newline
        text = text[:-1]
    got = merged([a, b], first_line=seed)
    assert (got.entries(), got.postings()) == oracle.index(text, first_line=seed)


def test_merge_refuses_a_wrong_first_line():
    a, b = cpu_index(b"a b\nc\n"), cpu_index(b"b c\n", 3)
    with pytest.raises(lc.LocustError, match="line 3"):
        lc.merge_index(a, b)
    with pytest.raises(lc.LocustError, match="line 0"):
        lc.merge_index(a, cpu_index(b"b c\n"))
    lc.merge_index(a, cpu_index(b"b c\n", 2))


def test_split_blocks(hamlet):
    text = oracle.window(hamlet, 0, 900)
    for size in (97, 1000, 4096):
        blocks = lc.split_blocks(text, size, 5)
        pieces = [text[o:o + n] for o, n, _l, _f in blocks]
        assert b"".join(pieces) == text
        assert all(p.endswith(b"\n") and 0 < len(p) <= size for p in pieces)
        assert [l for _o, _n, l, _f in blocks] == [nlines(p) for p in pieces]
        assert sum(l for _o, _n, l, _f in blocks) == 900
        firsts = [f for _o, _n, _l, f in blocks]
        assert firsts[0] == 5
        assert firsts[1:] == [5 + sum(nlines(p) for p in pieces[:i]) for i in range(1, len(pieces))]
        # whole lines, as many as fit: the next line would not have fitted
        for p, q in zip(pieces, pieces[1:]):
            assert len(p) + len(q.split(b"\n")[0]) + 1 > size
    # the last block may lack its newline
    blocks = lc.split_blocks(b"aa\nbb\ncc", 6)
    assert blocks == [(0, 6, 2, 0), (6, 2, 1, 2)]
    # one block when the text fits, an empty text included
    assert lc.split_blocks(text, len(text)) == [(0, len(text), 900, 0)]
    assert lc.split_blocks(b"", 10) == [(0, 0, 0, 0)]
    # a line longer than the block
    with pytest.raises(lc.LocustError, match="--block-kb"):
        lc.split_blocks(b"short\n" + b"x" * 40 + b"\nshort\n", 16)


def test_python_helpers_take_block_bytes(hamlet):
    text = oracle.window(hamlet, 0, 600)
    x = lc.index_text(text, backend="cpu", block_bytes=4096)
    assert (x.entries(), x.postings()) == oracle.index(text)
    path = os.path.join(ROOT, "data", "hamlet.txt")
    f = lc.index_file(path, 300, 450, backend="cpu", block_bytes=1024)
    assert (f.entries(), f.postings()) == oracle.index(oracle.window(hamlet, 300, 450),
                                                       first_line=300)
    whole = lc.search_text(text, [[b"to", b"be"]], "phrase", backend="cpu", show=40)
    blocked = lc.search_text(text, [[b"to", b"be"]], "phrase", backend="cpu", show=40,
                             block_bytes=4096)
    assert blocked.format() == whole.format() and blocked.lines(0) == whole.lines(0)
    s = lc.search_file(path, [[b"Hamlet"]], line_start=300, line_end=450, backend="cpu",
                       block_bytes=1024)
    assert s.lines(0) == lc.search_file(path, [[b"Hamlet"]], line_start=300, line_end=450,
                                        backend="cpu").lines(0)
    cpu = lc.Engine(lc.make_config("cpu"))
    with pytest.raises(lc.LocustError, match="GPU engine"):
        cpu.append_index(b"a\n")
    with pytest.raises(lc.LocustError, match="GPU engine"):
        cpu.index_resident()


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n")
                    if l.startswith((b"print ", b"  ")))


@pytest.mark.parametrize("args", [
    ["--index", "--block-kb", "32"],
    ["--search", "to be", "--match", "phrase", "--block-kb", "32"],
    ["--search", "to be", "--match", "any", "--rank", "5", "--tally", "4", "--block-kb", "32"],
    ["1000", "1200", "--index", "--block-kb", "2"],
    ["1000", "1200", "--search", "my lord", "--match", "phrase", "--show", "60", "--block-kb", "2"],
], ids=["index", "phrase", "rank-tally", "window-index", "window-show"])
def test_cli_cpu_block_kb_gives_the_same_result_lines(cli, args, tmp_path):
    j = tmp_path / "b.json"
    plain = [a for i, a in enumerate(args) if a != "--block-kb" and args[i - 1] != "--block-kb"]
    want = run(cli, "data/hamlet.txt", *plain, "--backend", "cpu")
    got = run(cli, "data/hamlet.txt", *args, "--backend", "cpu", "--json", j)
    assert want.returncode == 0 and got.returncode == 0, got.stderr.decode()[-2000:]
    assert result_lines(want.stdout) and result_lines(got.stdout) == result_lines(want.stdout)
    rec = json.load(open(j))
    assert rec["blocks"] > 1 and rec["append_ms"] == 0 and rec["index_store_bytes"] == 0


@pytest.mark.parametrize("args, msg", [
    (["--block-kb", "32"], "--index"),
    (["--index", "--block-kb", "0"], "N >= 1"),
    (["--index", "--block-kb", "x"], "N >= 1"),
    (["--index", "--block-kb", "32", "--chunk-mb", "1"], "--chunk-mb"),
    (["--search", "to be", "--block-kb", "32", "--chunk-mb", "1"], "--chunk-mb"),
    (["--top", "5", "--block-kb", "32"], "--search"),
])
def test_cli_block_kb_refusals(cli, args, msg):
    p = run(cli, "data/hamlet.txt", *args, "--backend", "cpu")
    assert p.returncode != 0
    assert msg.encode() in p.stderr and b"--block-kb" in p.stderr
    assert b"print " not in p.stdout


def test_cli_refuses_a_line_longer_than_the_block(cli, tmp_path):
    f = tmp_path / "long.txt"
    f.write_bytes(b"short line\n" + b"w " * 1000 + b"\nshort\n")
    p = run(cli, f, "--index", "--block-kb", "1", "--backend", "cpu")
    assert p.returncode != 0 and b"--block-kb" in p.stderr


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--block-kb" in p.stdout
