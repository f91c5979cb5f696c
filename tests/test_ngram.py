"""Word n-grams without a GPU: the oracle's rules, the CPU engine against the oracle
(N = 1, 2, 3; Hamlet and seeded random texts), the CLI's ``--ngram N`` on the host paths,
its refusals, and the n-gram map kernels' compile-time resources.  Every comparison is
exact against ``oracle.wordcount(text, ngram=N)``: entries, num_tokens, num_unique,
overflow_lines and truncated."""
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.ngram_texts import got, random_text, want
from tests.test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


def cpu(text, n, **kw):
    return lc.wordcount_text(text, backend="cpu", ngram=n, **kw)


# ---------------- the oracle's rules ----------------
def test_oracle_rules():
    assert oracle.ngrams(b"a, b--c", 2) == ([b"a b", b"b c"], False, 0)
    assert oracle.ngrams(b"a, b--c", 3) == ([b"a b c"], False, 0)
    assert oracle.ngrams(b"a b", 3) == ([], False, 0)
    assert oracle.ngrams(b"", 2) == ([], False, 0)
    assert oracle.ngrams(b"a b\0c d", 2) == ([b"a b"], False, 0)  # a NUL hides the rest
    assert oracle.ngrams(b"a b c d", 2, emits=2) == ([b"a b", b"b c"], True, 0)
    assert oracle.ngrams(b"a b c", 2, emits=2) == ([b"a b", b"b c"], False, 0)
    long = b"x" * 28
    assert oracle.ngrams(long + b" yz", 2) == ([long + b" "], False, 1)  # 31 bytes -> 29
    assert oracle.ngrams(long[:26] + b" yz", 2) == ([long[:26] + b" yz"], False, 0)  # 29 bytes
    # n-grams never cross a line
    ent, ntok, over, trunc = oracle.wordcount(b"a b\nc d\n", ngram=2, stats=True)
    assert [k for k, _v, _c in ent] == [b"a b", b"c d"] and (ntok, over, trunc) == (2, 0, 0)
    with pytest.raises(ValueError):
        oracle.ngrams(b"a", 4)


def test_oracle_defaults_unchanged(hamlet):
    assert oracle.wordcount(hamlet, ngram=1) == oracle.wordcount(hamlet)
    assert len(oracle.wordcount(hamlet)) == 3
    toks = [t for l in oracle.split_lines(hamlet) for t in oracle.tokenize(l)[0]]
    grams = [g for l in oracle.split_lines(hamlet) for g in oracle.ngrams(l, 1)[0]]
    assert toks == grams


def test_hamlet_figures(hamlet):
    """The key distribution the feature is for: ~4x the distinct keys of the word job."""
    for n, (ntok, uniq) in {1: (32940, 5608), 2: (28776, 20531), 3: (24669, 23601)}.items():
        ent, t, u, _over, _trunc = want(hamlet, n)
        assert (t, u) == (ntok, uniq)
    assert want(hamlet, 3)[4] == 7  # trigrams longer than 29 bytes


# ---------------- the CPU engine ----------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_cpu_engine_hamlet(hamlet, n):
    assert got(cpu(hamlet, n)) == want(hamlet, n)
    win = oracle.window(hamlet, 0, 700)
    assert got(cpu(win, n)) == want(win, n)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_cpu_engine_random_texts(n):
    for seed in range(300):
        text = random_text(seed)
        assert got(cpu(text, n)) == want(text, n), (seed, len(text))


def test_cpu_engine_parameters():
    text = random_text(7, 5120) + b"\n" + random_text(8, 3000)
    for n in (2, 3):
        assert got(cpu(text, n, emits_per_line=1)) == want(text, n, emits=1)
        assert got(cpu(text, n, max_key_len=8)) == want(text, n, max_key=8)
        assert got(cpu(text, n, delimiters="ae ")) == want(text, n, delims=b"ae ")


def test_ngram_one_is_the_word_job(hamlet):
    a = lc.wordcount_text(hamlet, backend="cpu")
    b = cpu(hamlet, 1)
    assert got(a) == got(b) and a.format() == b.format()


def test_top_and_multi_rank(hamlet):
    ent = want(hamlet, 2)[0]
    t = lc.top_words_text(hamlet, 10, backend="cpu", ngram=2)
    assert t.entries() == oracle.top(ent, 10)
    r = lc.run_multi(hamlet, 3, backend="cpu", ngram=2)
    assert r.entries() == ent


def test_python_surface():
    assert lc._C.kMaxNgram == 3
    assert lc.make_config("cpu").ngram == 1 and lc.make_config("cpu", ngram=3).ngram == 3
    for n in (0, 4, -1):
        with pytest.raises(lc.LocustError, match="ngram"):
            lc.wordcount_text(b"a b c\n", backend="cpu", ngram=n)


def test_stage_split_refused(tmp_path):
    path = os.path.join(ROOT, "data", "hamlet.txt")
    with pytest.raises(lc.LocustError, match="ngram"):
        lc.map_stage(path, str(tmp_path / "s.kv"), 0, 100, backend="cpu", ngram=2)
    lc.map_stage(path, str(tmp_path / "w.kv"), 0, 100, backend="cpu")
    with pytest.raises(lc.LocustError, match="ngram"):
        lc.reduce_stage([str(tmp_path / "w.kv")], backend="cpu", ngram=2)


# ---------------- the CLI ----------------
def test_cli_cpu_ngram(cli, hamlet, tmp_path):
    ent, ntok, uniq, _over, _trunc = want(hamlet, 2)
    j = tmp_path / "j.json"
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--ngram", 2, "--check", "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_cpu(ent)
    assert p.stdout.startswith(b"Running\n") and p.stdout.endswith(b"\nDone\n")
    rec = json.load(open(j))
    assert rec["ngram"] == 2 and rec["tokens"] == ntok and rec["unique"] == uniq
    # a line window, the GPU build's line format, a result file
    win = oracle.window(hamlet, 100, 700)
    rf = tmp_path / "r.txt"
    p = run(cli, "data/hamlet.txt", 100, 700, "--backend", "cpu", "--ngram", 3,
            "--output-format", "gpu", "--result-file", rf)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert rf.read_bytes() == oracle.format_gpu(want(win, 3)[0])


def test_cli_ngram_one_equals_no_flag(cli, tmp_path):
    j = tmp_path / "j.json"
    a = run(cli, "data/hamlet.txt", "--backend", "cpu")
    b = run(cli, "data/hamlet.txt", "--backend", "cpu", "--ngram", 1, "--json", j)
    assert a.returncode == 0 and b.returncode == 0
    assert result_lines(a.stdout) == result_lines(b.stdout) != b""
    assert json.load(open(j))["ngram"] == 1


def test_cli_cpu_ngram_top(cli, hamlet):
    p = run(cli, "data/hamlet.txt", "--ngram", 2, "--top", 10, "--backend", "cpu")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_cpu(oracle.top(want(hamlet, 2)[0], 10))


def test_cli_cpu_ranks_ngram(cli, hamlet, tmp_path):
    j = tmp_path / "m.json"
    p = run(cli, "data/hamlet.txt", "--gpus", 3, "--backend", "cpu", "--ngram", 2, "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    q = run(cli, "data/hamlet.txt", "--backend", "cpu", "--ngram", 2, "--output-format", "gpu")
    assert q.returncode == 0, q.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == result_lines(q.stdout) == oracle.format_gpu(want(hamlet, 2)[0])
    assert json.load(open(j))["ngram"] == 2


@pytest.mark.parametrize("args", [
    ("data/hamlet.txt", "--backend", "cpu", "--ngram", 0),
    ("data/hamlet.txt", "--backend", "cpu", "--ngram", 4),
    ("data/hamlet.txt", "--backend", "cpu", "--ngram", "two"),
    ("data/hamlet.txt", "--backend", "cpu", "--ngram"),
    ("data/hamlet.txt", 0, 700, 0, 1, "--backend", "cpu", "--ngram", 2),  # stage 1
    ("data/hamlet.txt", 0, 700, 0, 2, "--backend", "cpu", "--ngram", 2),  # stage 2
    ("data/hamlet.txt", "--backend", "cpu", "--stage", "map", "--ngram", 2),
    ("data/hamlet.txt", "--backend", "cpu", "--stage", "reduce", "--inputs", "a.kv", "--ngram", 2),
    ("data/hamlet.txt", "--backend", "cpu", "--reducer", "0/2", "--ngram", 3),
    ("data/hamlet.txt", "--map-path", "compat", "--ngram", 2),  # (refused before any GPU use)
])
def test_cli_ngram_refusals(cli, args, tmp_path):
    p = run(cli, *args, "--spill-dir", tmp_path)
    assert p.returncode != 0
    assert b"--ngram" in p.stderr or b"missing value" in p.stderr
    assert b"print key:" not in p.stdout
    assert os.listdir(tmp_path) == []  # no spill was written
    if "compat" in args:
        assert b"map_path fast" in p.stderr


def test_cli_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--ngram N" in p.stdout


# ---------------- the kernels' compile-time resources ----------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_ngram_kernel_resources():
    """No scratch and no VGPR spills (a dynamically indexed key array would be private
    memory, see tests/test_kernel_resources.py), and the word kernels' own LDS ceilings."""
    res = resources(os.path.join(ROOT, "csrc", "kernels", "ngram.hip"))
    small = [n for n in res if "map_ngram_kernelILi2ELi1ELi1024" in n or
             "map_ngram_kernelILi3ELi1ELi1024" in n]
    large = [n for n in res if "map_ngram_kernelILi2ELi16ELi256" in n or
             "map_ngram_kernelILi3ELi16ELi256" in n]
    assert len(small) == 2 and len(large) == 2 and len(res) == 4, sorted(res)
    for name, r in res.items():
        assert r.get("ScratchSize", 0) == 0, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
    for name in small:
        assert res[name]["LDS Size"] <= 8192, (name, res[name]["LDS Size"])
    for name in large:
        assert res[name]["LDS Size"] <= 20480, (name, res[name]["LDS Size"])


def test_partmap_cache_key_separates_ngrams(tmp_path, monkeypatch):
    """A partition map tuned on a file's words is never applied to its bigrams; a word
    job's cache name is what it was without the parameter."""
    monkeypatch.setenv("LOCUST_CACHE_DIR", str(tmp_path))
    path = os.path.join(ROOT, "data", "hamlet.txt")
    names = [lc._C.partmap_cache_path(path, lc.make_config("gpu", ngram=n)) for n in (1, 2, 3)]
    assert all(names) and len(set(names)) == 3
    assert names[0] == lc._C.partmap_cache_path(path, lc.make_config("gpu"))
