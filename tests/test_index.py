"""Inverted index (word -> the lines it occurs on) without a GPU: the oracle's own
properties, the CPU engine against the oracle (exactly), the CLI's ``--backend cpu --index``
lines and every refused flag combination."""
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


def random_text(seed, lines=120, final_newline=True):
    """Lines of random tokens: bytes >= 0x80, '\\r', NULs, delimiter runs, empty lines and
    lines with more than 20 tokens."""
    rng = random.Random(seed)
    delims = oracle.DEFAULT_DELIMS
    vocab = []
    for _ in range(40):
        ln = rng.randrange(1, 36)
        hi = rng.random() < 0.3
        vocab.append(bytes(rng.randrange(0x80, 0x100) if hi and rng.random() < 0.5
                           else rng.choice(b"abcXYZ019_\r") for _ in range(ln)))
    out = []
    for _ in range(lines):
        kind = rng.random()
        if kind < 0.1:
            out.append(b"")
            continue
        ntok = rng.randrange(1, 8) if kind < 0.85 else rng.randrange(18, 30)
        line = bytearray()
        if rng.random() < 0.3:
            line += bytes(rng.choice(delims) for _ in range(rng.randrange(1, 4)))
        for _ in range(ntok):
            line += rng.choice(vocab)
            line += bytes(rng.choice(delims) for _ in range(rng.randrange(1, 4)))
            if rng.random() < 0.02:
                line += b"\0"
        out.append(bytes(line))
    text = b"\n".join(out)
    return text + b"\n" if final_newline else text + b" tail"


TEXTS = [(s, nl) for s in range(6) for nl in (True, False)]


@pytest.mark.parametrize("seed, final_newline", TEXTS)
@pytest.mark.parametrize("emits, max_key", [(20, 29), (3, 5)])
def test_oracle_properties(seed, final_newline, emits, max_key):
    text = random_text(seed, final_newline=final_newline)
    entries, postings = oracle.index(text, emits=emits, max_key=max_key, first_line=7)
    wc, ntok, _ = oracle.wordcount(text, emits=emits, max_key=max_key)
    assert entries == wc
    assert len(postings) == ntok
    lines = oracle.split_lines(text)
    for key, val, count in entries:
        mine = postings[val:val + count]
        assert mine == sorted(mine)
        for l in set(mine):
            toks, _ = oracle.tokenize(lines[l - 7], emits=emits, max_key=max_key)
            assert toks.count(key) == mine.count(l)
        assert oracle.index_lines(entries, postings, key) == mine
        assert oracle.index_lines(entries, postings, key, unique=True) == sorted(set(mine))
    # every emitted token of every line is in its word's list
    total = sum(len(oracle.tokenize(l, emits=emits, max_key=max_key)[0]) for l in lines)
    assert total == len(postings)


def cpu_index(text, first_line=0, **kw):
    eng = lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)
    return eng.run_index(text, first_line)


@pytest.mark.parametrize("seed, final_newline", TEXTS)
def test_cpu_engine_random_texts(seed, final_newline):
    text = random_text(seed, final_newline=final_newline)
    got = cpu_index(text)
    assert (got.entries(), got.postings()) == oracle.index(text)
    got = cpu_index(text, emits_per_line=3, max_key_len=5)
    assert (got.entries(), got.postings()) == oracle.index(text, emits=3, max_key=5)


def test_cpu_engine_hamlet_window_and_offset(hamlet):
    win = oracle.window(hamlet, 0, 700)
    got = cpu_index(win)
    ent, post = oracle.index(win)
    assert (got.entries(), got.postings()) == (ent, post)
    assert got.num_tokens == len(post) and got.num_unique == len(ent) and got.num_lines == 700
    assert got.format() == oracle.format_index(ent, post)
    assert got.lines(b"Hamlet") == oracle.index_lines(ent, post, b"Hamlet")
    assert got.lines(b"Hamlet", unique=True) == oracle.index_lines(ent, post, b"Hamlet", True)
    assert got.index_ms == 0 and "index_ms" in got.times()
    # a window with first_line > 0: global numbering
    sub = oracle.window(hamlet, 300, 450)
    got = cpu_index(sub, first_line=300)
    assert (got.entries(), got.postings()) == oracle.index(sub, first_line=300)
    assert min(got.postings()) >= 300 and max(got.postings()) < 450
    f = lc.index_file(os.path.join(ROOT, "data", "hamlet.txt"), 300, 450, backend="cpu")
    assert (f.entries(), f.postings()) == (got.entries(), got.postings()) and f.first_line == 300
    t = lc.index_text(sub, backend="cpu", first_line=300)
    assert t.postings() == got.postings()


def test_cpu_engine_first_line_limit():
    """first_line + num_lines == 2^32 is the last accepted value: the last line's posting
    is 2^32 - 1, the largest a u32 holds."""
    text = b"alpha beta\nbeta gamma\n\nalpha\n"
    cfg = lc.make_config("cpu", check=True)
    first = 2**32 - 4
    got = lc._C.cpu_run_index(cfg, text, first)
    assert (got.entries(), got.postings()) == oracle.index(text, first_line=first)
    assert max(got.postings()) == 2**32 - 1 and got.first_line == first
    with pytest.raises(lc.LocustError, match=r"2\^32"):
        lc._C.cpu_run_index(cfg, text, first + 1)


def test_cpu_engine_refuses_ngrams():
    with pytest.raises(lc.LocustError, match="ngram"):
        cpu_index(b"a b c\n", ngram=2)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


def test_cli_cpu_index(cli, hamlet, tmp_path):
    j = tmp_path / "i.json"
    p = run(cli, "data/hamlet.txt", 0, 700, "--backend", "cpu", "--index", "--check", "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    ent, post = oracle.index(oracle.window(hamlet, 0, 700))
    assert result_lines(p.stdout) == oracle.format_index(ent, post)
    rec = json.load(open(j))
    assert rec["index"] is True and rec["postings"] == len(post) and rec["index_ms"] == 0
    # a window that does not start at line 0, with its own caps
    p = run(cli, "data/hamlet.txt", 1000, 1200, "--backend", "cpu", "--index",
            "--emits-per-line", 4, "--max-key", 6)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = oracle.index(oracle.window(hamlet, 1000, 1200), emits=4, max_key=6, first_line=1000)
    assert result_lines(p.stdout) == oracle.format_index(*want)
    # --ref-compat: the CPU build takes the whole file less its last line
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--index", "--ref-compat")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = oracle.index(oracle.window(hamlet, ref_compat=True))
    assert result_lines(p.stdout) == oracle.format_index(*want)


@pytest.mark.parametrize("args, msg", [
    (["--index", "--top", "5"], "--top"),
    (["--index", "--ngram", "2"], "--ngram"),
    (["0", "100", "0", "1", "--index"], "stage"),
    (["0", "100", "0", "2", "--index"], "stage"),
    (["--index", "--gpus", "2"], "--gpus"),
    (["--index", "--chunk-mb", "1"], "--chunk-mb"),
    (["--index", "--sort", "radix"], "--sort dict"),
    (["--index", "--map-path", "compat"], "--map-path"),
])
def test_cli_index_refusals(cli, args, msg, tmp_path):
    p = run(cli, "data/hamlet.txt", *args, "--spill-dir", tmp_path)
    assert p.returncode != 0
    assert msg.encode() in p.stderr and b"--index" in p.stderr
    assert b"print key" not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--index" in p.stdout
