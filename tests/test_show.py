"""Show (``show=N``: the returned lines' text and match spans, engine.hpp "show") without a GPU:
the oracle against hand-written expectations, the CPU engine (the host evaluation with the
text) against the oracle on edge texts and a seeded fuzz -- which also shows, with the oracle
alone, that the generator the GPU test shares produces no batch the rules refuse --,
``validate_search`` on hand-broken results, the CLI's ``--backend cpu --show N [--mark]`` against
the oracle's formatting, the README's counts and every refusal that needs no device.  Every
comparison is exact; ``check=True`` runs ``validate_search`` on every result."""
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.show_cases import (FUZZ_BATCHES, FUZZ_TEXTS, formatted_show, fuzz_batch, fuzz_expect,
                              fuzz_text, same_show, want_show)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def check(text, queries, modes, n, k=None, first_line=0, within=None, exclude=None, glob=False,
          ignore_case=False, **okw):
    ckw = {}
    if "max_key" in okw:
        ckw["max_key_len"] = okw["max_key"]
    if "emits" in okw:
        ckw["emits_per_line"] = okw["emits"]
    expect = want_show(text, queries, modes, n, k, first_line, within, exclude, glob, ignore_case,
                       **okw)
    eng = cpu_engine(text, **ckw)
    kw = dict(rank=k, within=within, exclude=exclude, glob=glob, ignore_case=ignore_case)
    got = eng.run_search(text, queries, modes, first_line, show=n, **kw)
    plain = eng.run_search(text, queries, modes, first_line, **kw)
    same_show(got, expect, n, k, plain)
    for mark in (False, True):
        assert got.format(mark=mark) == formatted_show(queries, expect, k, exclude, glob, mark)
    assert plain.format(mark=True) == plain.format()
    return got


TEXT = (b"to be, or not to be\n"          # 0
        b"  Hamlet's hamlets ham\n"       # 1
        b"\n"                             # 2
        b"be\0to be hidden\n"             # 3
        b"to-be to:be tobe\n"             # 4
        b"be")                            # 5: no newline


def test_oracle_by_hand():
    texts, spans, cut = oracle.show(TEXT, [0, 3, 4, 5], [b"to", b"be"], 10)
    assert texts == [b"to be, or ", b"be", b"to-be to:b", b"be"]
    assert spans == [[(0, 2, 1), (3, 2, 2), (14, 2, 1), (17, 2, 2)], [(0, 2, 2)],
                     [(0, 2, 1), (3, 2, 2), (6, 2, 1), (9, 2, 2)], [(0, 2, 2)]]
    assert cut == 2
    # a prefix term, a repeated term (two bits), the cut key and the token's full length
    texts, spans, cut = oracle.show(TEXT, [1], [b"ham*", b"Hamlet", b"ham*"], 80, glob=True)
    assert texts == [b"  Hamlet's hamlets ham"] and cut == 0
    assert spans == [[(2, 6, 2), (11, 7, 5), (19, 3, 5)]]
    assert oracle.show(TEXT, [1], [b"hamle"], 4, max_key=5) == ([b"  Ha"], [[(11, 7, 1)]], 1)
    assert oracle.show(TEXT, [1], [b"hamlet"], 1, ignore_case=True)[1] == [[(2, 6, 1)]]
    # the emit cap, an empty line, first_line
    assert oracle.show(TEXT, [0], [b"be"], 80, emits=5)[1] == [[(3, 2, 1)]]
    assert oracle.show(TEXT, [12], [b"be"], 80, first_line=10) == ([b""], [[]], 0)
    for bad in (0, 65537, True, None, 2.0):
        with pytest.raises(ValueError):
            oracle.show(TEXT, [0], [b"be"], bad)
    first = b"print query: to be \t hits: 1 \t lines: 4\n"
    assert oracle.format_show(first, [4], [b"to-be to:b"], [[(0, 2, 1), (9, 2, 2)]], True) == \
        first + b"  4: >>to<<-be to:>>b<<\n"
    assert oracle.format_show(first, [4], [b"to-be"]) == first + b"  4: to-be\n"


@pytest.mark.parametrize("n", [1, 2, 10, 19, 20, 21, 65536])
@pytest.mark.parametrize("mode", ["all", "any", "phrase", "near"])
def test_cpu_engine_small_text(mode, n):
    queries = [[b"to", b"be"], [b"be"], [b"nosuch", b"be"], [b"hamlets", b"ham"], [b"be", b"be"]]
    got = check(TEXT, queries, mode, n, within=3 if mode == "near" else None)
    assert sum(got.hits()) > 0
    check(TEXT, queries, mode, n, k=2, first_line=7, within=3 if mode == "near" else None)


def edge_text():
    """Lines of the lengths the device stage steps at, a matching token at bytes 63 and 64 and
    across the step edge, matching tokens of 70 and 130 bytes, a NUL, no final newline."""
    lines = []
    for n in (1, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200):
        lines.append((b"hit " + b"x" * n)[:n - 1].ljust(n - 1, b"x") + b"k" if n > 5 else b"k" * n)
    lines += [b"y" * 62 + b" hit z", b"y" * 63 + b" hit", b"y" * 60 + b" hit hit",
              b"hit " + b"L" * 70 + b" " + b"M" * 130 + b" hit", b"hit\0hit", b"", b"k hit"]
    return b"\n".join(lines)


def test_cpu_engine_edges():
    text = edge_text()
    queries = [[b"hit"], [b"k"], [b"L" * 70, b"M" * 130, b"hit"], [b"hit", b"k*"], [b"*"]]
    for n in (1, 63, 64, 65, 129, 65536):
        check(text, queries[:4], "any", n, glob=True)
        check(text, queries[:4], "any", n, k=3, glob=True, ignore_case=True)
    got = check(text, [[b"hit"]], "all", 64)
    assert got.cut_lines > 0 and any(s[0][1] == 3 for s in got.spans(0) if s)
    # max_key_len = 5: `hamlets` matches the cut term and its span is 7 bytes long
    got = check(b"the hamlets sing\n", [[b"hamlet"]], "all", 80, max_key=5)
    assert got.spans(0) == [[(4, 7, 1)]]
    # a matching token past the emit cap: no span
    got = check(b"a b c d hit\nhit a b c hit\n", [[b"hit"]], "any", 80, emits=4)
    assert got.lines(0) == [1] and got.spans(0) == [[(0, 3, 1)]]
    # eight positive terms: every mask bit; exclusion terms: never a span
    words = [b"w%d" % i for i in range(8)]
    got = check(b" ".join(words) + b" w0\nw1 gone\n", [words, [b"w1"]], "any", 80,
                exclude=[None, [b"gone"]])
    assert [m for _s, _l, m in got.spans(0)[0]] == [1, 2, 4, 8, 16, 32, 64, 128, 1]
    assert got.lines(1) == [0]


@pytest.mark.parametrize("text_seed", FUZZ_TEXTS)
def test_cpu_engine_fuzz(text_seed):
    text = fuzz_text(text_seed)
    assert len(oracle.split_lines(text)) <= 300
    eng = cpu_engine(text)
    spans = 0
    for seed in range(FUZZ_BATCHES):
        queries, modes, kw = fuzz_batch(seed, text_seed)
        n, k = kw.pop("show"), kw.pop("rank")
        # (the oracle alone first: the generator produces no batch the rules refuse)
        expect = fuzz_expect(text_seed, seed)
        got = eng.run_search(text, queries, modes, rank=k, show=n, **kw)
        same_show(got, expect, n, k, eng.run_search(text, queries, modes, rank=k, **kw))
        spans += got.span_count
    assert spans > 100


def test_validate_rejects_broken_results():
    # the result of [to, be] over the one line b"to be or to be": 14 bytes, two of its spans
    good = lc._C.validate_show([b"to", b"be"], [0], [14], [0, 2, 1, 3, 2, 2], [0, 2], 80)
    assert good is None
    for spans, msg in (([0, 4, 1, 3, 2, 2], "overlaps"),     # overlapping spans
                       ([3, 2, 2, 0, 2, 1], "overlaps"),     # not ascending
                       ([0, 2, 1, 2, 2, 2], "overlaps"),     # no delimiter between two tokens
                       ([0, 2, 1, 3, 0, 2], "overlaps"),     # an empty token
                       ([0, 2, 1, 3, 2, 4], "mask"),         # a bit at the term count
                       ([0, 2, 0, 3, 2, 2], "mask"),         # an empty mask
                       ([0, 2, 1, 13, 2, 2], "leaves the line")):
        with pytest.raises(lc.LocustError, match=msg):
            lc._C.validate_show([b"to", b"be"], [0], [14], spans, [0, 2], 80)
    with pytest.raises(lc.LocustError, match="offsets"):
        lc._C.validate_show([b"to", b"be"], [0], [14], [0, 2, 1], [0, 2], 80)
    with pytest.raises(lc.LocustError, match="N = 8"):
        lc._C.validate_show([b"to", b"be"], [0], [14], [], [0, 0], 8)


def test_cli_cpu_show(cli, hamlet, tmp_path):
    queries = [[b"to", b"be"], [b"my", b"lord"], [b"nosuchword"]]
    args = ["--search", "to be", "--search", "my lord", "--not", "good", "--search", "nosuchword"]
    exclude = [None, [b"good"], None]
    for mode, k, n, mark in (("phrase", None, 80, True), ("all", 3, 20, True),
                             ("any", None, 5, False), ("near", 2, 65536, True)):
        extra = (["--within", 4] if mode == "near" else []) + (["--rank", k] if k else []) + \
                (["--mark"] if mark else [])
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--show", n,
                "--check", *extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want_show(hamlet, queries, mode, n, k, within=4 if mode == "near" else None,
                           exclude=exclude)
        want_out = formatted_show(queries, expect, k, exclude, False, mark)
        assert p.stdout.count(want_out) == 1
    # --json reports the stage
    j = tmp_path / "show.json"
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--show", 8, "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _b, shown = want_show(hamlet, [[b"to", b"be"]], "all", 8)
    rec = json.loads(j.read_text())
    assert rec["show_bytes"] == 8 and rec["cut_lines"] == shown[0][2] and rec["show_ms"] >= 0
    assert rec["spans"] == sum(len(s) for s in shown[0][1]) and rec["hits"] == len(shown[0][0])
    # without --show the output is what it was: line numbers only
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "phrase")
    assert p.returncode == 0 and b"\n  " not in p.stdout[p.stdout.index(b"print query:"):]


@pytest.mark.parametrize("args, msg", [
    (["--show", 80], "--search"),
    (["--mark", "--search", "to"], "--show"),
    (["--search", "to", "--show", 0], "1 <= N <= 65536"),
    (["--search", "to", "--show", 65537], "1 <= N <= 65536"),
    (["--search", "to", "--show", "x"], "1 <= N <= 65536"),
    (["--show", 80, "--index"], "--search"),
])
def test_cli_show_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flags(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--show N" in p.stdout and b"--mark" in p.stdout


def test_refusals():
    eng = cpu_engine(TEXT)
    for bad in (65537, -1, 1 << 40, "80", 2.5):
        with pytest.raises((lc.LocustError, TypeError), match="show|N"):
            eng.run_search(TEXT, [[b"be"]], show=bad)
    assert eng.run_search(TEXT, [[b"be"]], show=0).show_bytes == 0
    assert eng.run_search(TEXT, [[b"be"]], show=None).text(0) == []
    # the host evaluation over an index alone has no text: refused like a phrase
    idx = eng.run_index(TEXT)
    with pytest.raises(lc.LocustError, match="four-argument"):
        idx.search([[b"be"]], show=80)
    assert idx.search([[b"be"]], show=None).lines(0) == [0, 3, 4, 5]
    # a window of 2^32 bytes or more (the check itself: no such text is built here)
    with pytest.raises(lc.LocustError, match="2\\^32"):
        lc._C.check_search_show(80, 1 << 32)
    lc._C.check_search_show(80, (1 << 32) - 1)
    lc._C.check_search_show(0, 1 << 40)
    with pytest.raises(lc.LocustError, match="65536"):
        lc._C.check_search_show(65537, 10)


def test_readme_counts(hamlet):
    readme = open(os.path.join(ROOT, "README.md"), "rb").read()
    base, shown = want_show(hamlet, [[b"to", b"be"]], "phrase", 80)
    n = base[0][1]
    line = b'--search "to be" --match phrase --show 80 --mark'
    at = readme.find(line)
    assert at >= 0
    assert (b"the %d lines" % n) in readme[at:at + 400]
    assert (b"%d spans" % sum(len(s) for s in shown[0][1])) in readme[at:at + 400]
