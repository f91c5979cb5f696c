"""Top-K words by count without a GPU: the host selection (``Result.top``, the CPU
backend's ``run_top``), the CLI's ``--top K`` on the paths that select on the host, its
usage errors, and the selection kernels' compile-time resources.  Exact comparisons
against ``oracle.top`` over ``oracle.wordcount``."""
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.test_kernel_resources import HIPCC, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


@pytest.fixture(scope="module")
def texts(hamlet):
    win = oracle.window(hamlet, 0, 700)
    return {"window": (win, oracle.wordcount(win)), "whole": (hamlet, oracle.wordcount(hamlet))}


@pytest.mark.parametrize("which", ["window", "whole"])
def test_host_selection(texts, which):
    text, (ent, ntok, _) = texts[which]
    full = lc.wordcount_text(text, backend="cpu")
    vals = {k: v for k, v, _c in full.entries()}
    for k in (1, 10, len(ent), len(ent) + 5):
        want = oracle.top(ent, k)
        assert len(want) == min(k, len(ent))
        for t in (full.top(k), lc.top_words_text(text, k, backend="cpu")):
            got = t.entries()
            assert got == want
            assert t.k == k and t.num_unique == len(ent) and t.num_tokens == ntok
            # val is the key's val in the full output: the lines are a subset of its lines
            assert all(vals[key] == val for key, val, _c in got)
        assert set(full.top(k).format().splitlines()) <= set(full.format().splitlines())
    assert full.top(3).format(cpu_format=True) == oracle.format_cpu(oracle.top(ent, 3))
    assert full.top(3).select_ms == 0 and full.top(3).wire_bytes == 0


def test_every_word_once():
    """All counts tie: the top K are the first K keys in key order."""
    words = [b"w%03d" % i for i in range(200)]
    text = b"\n".join(b" ".join(words[i::10][::-1]) for i in range(10)) + b"\n"
    ent = oracle.wordcount(text)[0]
    assert len(ent) == 200 and all(c == 1 for _k, _v, c in ent)
    got = lc.top_words_text(text, 7, backend="cpu").entries()
    assert got == oracle.top(ent, 7) == ent[:7]


def test_tie_at_the_kth_count():
    """Exactly K + 3 keys share the K-th count: the smallest keys among them win."""
    k = 6
    lines = [b"big big big big", b"mid mid mid"]
    lines += [b"t%02d t%02d" % (i, i) for i in range(k + 1)]  # k + 1 more keys of count 2 ...
    lines += [b"z z", b"a a"]                                  # ... and two: k + 3 ties
    lines += [b"one once single"]
    text = b"\n".join(lines) + b"\n"
    ent = oracle.wordcount(text)[0]
    want = oracle.top(ent, k)
    assert want[k - 1][2] == 2 and sum(1 for e in ent if e[2] == 2) == k + 3
    assert lc.top_words_text(text, k, backend="cpu").entries() == want
    assert lc.wordcount_text(text, backend="cpu").top(k).entries() == want


def test_python_surface():
    assert lc._C.kTopKMax >= 1024 and lc._C.kTopKTile > 0
    assert "top_words_text" in lc.__all__ and "top_words_file" in lc.__all__
    t = lc.top_words_file(os.path.join(ROOT, "data", "hamlet.txt"), 4, 0, 700, backend="cpu")
    win = oracle.window(open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read(), 0, 700)
    assert t.entries() == oracle.top(oracle.wordcount(win)[0], 4)
    assert "select_ms" in t.times()
    eng = lc.Engine(lc.make_config("cpu"))
    recs = [(b"a", 2), (b"b", 5), (b"c", 2)]
    assert eng.top_counts(recs, 2) == [(b"b", 2, 5), (b"a", 0, 2)]
    with pytest.raises(lc.LocustError):
        lc.top_words_text(b"a b\n", 0, backend="cpu")


def test_cli_cpu_top(cli, texts):
    ent = texts["whole"][1][0]
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--top", 10)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_cpu(oracle.top(ent, 10))
    assert p.stdout.startswith(b"Running\n") and p.stdout.endswith(b"\nDone\n")


def test_cli_multi_rank_top(cli, texts, tmp_path):
    ent = texts["whole"][1][0]
    j = tmp_path / "m.json"
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--gpus", 3, "--top", 5, "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    q = run(cli, "data/hamlet.txt", "--backend", "cpu", "--top", 5, "--output-format", "gpu")
    assert q.returncode == 0, q.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == result_lines(q.stdout) == oracle.format_gpu(oracle.top(ent, 5))
    assert json.load(open(j))["top_k"] == 5


def test_cli_stage_split_top(cli, texts, tmp_path):
    ent = texts["whole"][1][0]
    p = run(cli, "data/hamlet.txt", 0, 4463, 0, 1, "--backend", "cpu", "--spill-dir", tmp_path)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rf = tmp_path / "res.txt"
    p = run(cli, "data/hamlet.txt", 0, 4463, 0, 2, "--backend", "cpu", "--spill-dir", tmp_path,
            "--top", 7, "--result-file", rf)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    one = run(cli, "data/hamlet.txt", "--backend", "cpu", "--top", 7)
    assert rf.read_bytes() == result_lines(one.stdout) == oracle.format_cpu(oracle.top(ent, 7))
    # --reducer r/R: the top of that key range
    p = run(cli, "data/hamlet.txt", 0, 4463, 0, 2, "--backend", "cpu", "--spill-dir", tmp_path,
            "--top", 3, "--reducer", "1/2", "--output-format", "gpu")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = result_lines(p.stdout).splitlines()
    assert len(lines) == 3 and set(lines) <= set(oracle.format_gpu(ent).splitlines())


@pytest.mark.parametrize("args", [
    ("data/hamlet.txt", 0, 700, 0, 1, "--backend", "cpu", "--top", 3),  # stage 1
    ("data/hamlet.txt", "--backend", "cpu", "--stage", "map", "--top", 3),
    ("data/hamlet.txt", "--backend", "cpu", "--top", 3, "--export-kiv", "x.kiv"),
    ("data/hamlet.txt", "--backend", "cpu", "--top", 3, "--ref-timers"),
    ("data/hamlet.txt", "--sort", "radix", "--top", 3),  # (refused before any GPU use)
    ("data/hamlet.txt", "--backend", "cpu", "--top", 0),
    ("data/hamlet.txt", "--backend", "cpu", "--top", -2),
    ("data/hamlet.txt", "--backend", "cpu", "--top", "ten"),
    ("data/hamlet.txt", "--backend", "cpu", "--top"),
])
def test_cli_top_usage_errors(cli, args, tmp_path):
    p = run(cli, *args, "--spill-dir", tmp_path)
    assert p.returncode != 0
    assert b"--top" in p.stderr or b"missing value" in p.stderr
    assert b"print key:" not in p.stdout and not os.path.exists(os.path.join(ROOT, "x.kiv"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_topk_kernel_resources():
    res = resources(os.path.join(ROOT, "csrc", "kernels", "topk.hip"))
    assert len(res) >= 6, sorted(res)
    for name, r in res.items():
        assert r.get("ScratchSize", 0) == 0, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r["LDS Size"] <= 48 * 1024, (name, r["LDS Size"])
