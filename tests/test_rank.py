"""Ranked search without a GPU: ``oracle.rank`` by hand, the figures of whole Hamlet through
the CPU engine and ``IndexResult.search(rank=...)``, a seeded fuzz of the CPU engine against
the oracle (exactly: scores are integers and the order is total), the refusals, the output
format, the CLI's ``--backend cpu --rank`` and the unranked answer left as it was."""
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


def want(text, queries, modes, k, first_line=0, **okw):
    """[(top, matches, counts)] of every query by the oracle."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    out = []
    for q, m in zip(queries, modes):
        if m == "phrase":
            lines, counts = oracle.phrase(text, q, first_line=first_line, **okw)
        else:
            lines, counts = oracle.search(ent, post, q, m, **skw)
        top, matches = oracle.rank(ent, post, lines, q, k, max_key=okw.get("max_key", 29))
        out.append((top, matches, counts))
    return out


def same(got, expect, k):
    assert got.queries == len(expect) and got.rank_k == k
    assert got.matches() == [m for _t, m, _c in expect]
    assert got.hits() == [min(k, m) for _t, m, _c in expect]
    for i, (top, _m, counts) in enumerate(expect):
        assert list(zip(got.lines(i), got.scores(i))) == top, i
        assert got.term_counts(i) == counts, i


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


# ------------------------------------------------------------------------------------
# the oracle, on a text whose answers are spelled out
# ------------------------------------------------------------------------------------
TEXT = (b"to be or not to be\n"        # 0
        b"that is the question\n"      # 1
        b"to sleep\n"                  # 2
        b"\n"                          # 3
        b"be all my sins\n"            # 4
        b"rose is a rose is a rose\n"  # 5
        b"not to be\n")                # 6
# N = 26 tokens; to: 4 (26 // 4 = 6: weight 3), be: 4 (3), rose: 3 (8: 4), is: 3 (4),
# a: 2 (13: 4), not: 2 (4), sleep: 1 (26: 5)


def test_oracle_by_hand():
    ent, post = oracle.index(TEXT)
    assert len(post) == 26

    def r(terms, k, mode="all"):
        return oracle.rank(ent, post, oracle.search(ent, post, terms, mode)[0], terms, k)

    assert r([b"to"], 10) == ([(0, 6), (2, 3), (6, 3)], 3)
    assert r([b"to"], 1) == ([(0, 6)], 3)
    assert r([b"to", b"be"], 10) == ([(0, 12), (6, 6)], 2)
    assert r([b"to", b"be"], 10, "any") == ([(0, 12), (6, 6), (2, 3), (4, 3)], 4)
    assert r([b"to", b"be"], 3, "any") == ([(0, 12), (6, 6), (2, 3)], 4)
    assert r([b"rose", b"is", b"a"], 5) == ([(5, 3 * 4 + 2 * 4 + 2 * 4)], 1)
    assert r([b"to", b"sleep"], 5, "any") == ([(2, 8), (0, 6), (6, 3)], 3)
    # a repeated term counts once, an absent one contributes nothing
    assert r([b"to", b"to", b"be", b"to"], 10) == r([b"to", b"be"], 10)
    assert r([b"to", b"absent"], 10, "any") == r([b"to"], 10)
    assert r([b"to", b"absent"], 10) == ([], 0)
    assert r([b"absent"], 4, "any") == ([], 0)
    with pytest.raises(ValueError):
        r([b"to"], 0)
    # a phrase matches by the phrase rule and scores its distinct terms
    lines = oracle.phrase(TEXT, [b"to", b"be"])[0]
    assert oracle.rank(ent, post, lines, [b"to", b"be"], 5) == ([(0, 12), (6, 6)], 2)
    lines = oracle.phrase(TEXT, [b"is", b"a", b"rose", b"is"])[0]
    assert oracle.rank(ent, post, lines, [b"is", b"a", b"rose", b"is"], 5) == ([(5, 28)], 1)
    # global numbering; truncated keys merge
    ent, post = oracle.index(TEXT, first_line=1000)
    assert oracle.rank(ent, post, [1000, 1006], [b"to", b"be"], 1) == ([(1000, 12)], 2)
    ent, post = oracle.index(b"abcdefgh abcdeXYZ\nabcde abcd\n", max_key=5)
    assert oracle.rank(ent, post, [0, 1], [b"abcdeQQQ", b"abcdeZ"], 2, max_key=5) == (
        [(0, 2), (1, 1)], 2)


def test_oracle_format():
    assert oracle.format_ranked([[b"to", b"be"], [b"gone"]], [[(0, 12), (6, 6)], []], [2, 0]) == (
        b"print query: to be \t hits: 2 \t top: 0:12 6:6\n"
        b"print query: gone \t hits: 0 \t top:\n")


# ------------------------------------------------------------------------------------
# the CPU engine and IndexResult.search
# ------------------------------------------------------------------------------------
def test_cpu_by_hand():
    queries = [[b"to", b"be"], [b"to", b"be"], [b"rose"], [b"to", b"absent"], [b"absent"],
               [b"to", b"to", b"be"], [b"to", b"be"]]
    modes = ["all", "any", "all", "all", "any", "all", "phrase"]
    eng = cpu_engine(TEXT)
    for k in (1, 2, 100):
        expect = want(TEXT, queries, modes, k)
        got = eng.run_search(TEXT, queries, modes, rank=k)
        same(got, expect, k)
        assert got.format() == oracle.format_ranked(queries, [t for t, _m, _c in expect],
                                                    [m for _t, m, _c in expect])
        # the host evaluation over the index alone ranks all / any
        got = eng.run_index(TEXT).search(queries[:6], modes[:6], rank=k)
        same(got, expect[:6], k)
    got = eng.run_search(TEXT, queries, modes, rank=2)
    assert list(zip(got.lines(1), got.scores(1))) == [(0, 12), (6, 6)] and got.matches()[1] == 4
    # module-level entry points, and a window that does not start at line 0
    got = lc.search_text(TEXT, [[b"to", b"be"], [b"is"]], "any", backend="cpu", first_line=10,
                         rank=3)
    same(got, want(TEXT, [[b"to", b"be"], [b"is"]], "any", 3, first_line=10), 3)
    assert got.lines(0) == [10, 16, 12]
    with pytest.raises(lc.LocustError, match="phrase"):
        eng.run_index(TEXT).search([[b"to", b"be"]], "phrase", rank=3)
    got = eng.run_search(TEXT, [], rank=3)
    assert got.hits() == [] and got.matches() == [] and got.rank_k == 3


HAMLET_FIGURES = [
    ([b"to", b"be"], "any", 737, [(209, 22), (1413, 22), (1915, 22), (2094, 22), (2817, 22)]),
    ([b"to", b"be"], "all", 47, [(209, 22), (1413, 22), (1915, 22), (2094, 22), (2817, 22)]),
    ([b"to", b"be"], "phrase", 27, [(209, 22), (1413, 22), (1915, 22), (2094, 22), (2817, 22)]),
    ([b"my", b"lord"], "all", 119, [(1145, 30), (2440, 29), (329, 22), (649, 22), (338, 15)]),
    ([b"the"], "any", 820, [(2073, 24), (2958, 18), (3838, 18), (15, 12), (111, 12)]),
]


def test_hamlet_figures(hamlet):
    queries = [q for q, _m, _n, _t in HAMLET_FIGURES]
    modes = [m for _q, m, _n, _t in HAMLET_FIGURES]
    ent, post = oracle.index(hamlet)
    counts = {k: c for k, _v, c in ent}
    assert len(post) == 32940 and counts[b"to"] == 634 and counts[b"be"] == 206
    assert (32940 // 634).bit_length() == 6 and (32940 // 206).bit_length() == 8
    expect = want(hamlet, queries, modes, 5)
    assert [(t, m) for t, m, _c in expect] == [(t, n) for _q, _m, n, t in HAMLET_FIGURES]
    eng = lc.Engine(lc.make_config("cpu", check=True), len(hamlet), 1)
    got = eng.run_search(hamlet, queries, modes, rank=5)
    same(got, expect, 5)
    assert got.num_tokens == 32940
    keep = [i for i, m in enumerate(modes) if m != "phrase"]
    got = eng.run_index(hamlet).search([queries[i] for i in keep], [modes[i] for i in keep],
                                       rank=5)
    same(got, [expect[i] for i in keep], 5)
    f = lc.search_file(os.path.join(ROOT, "data", "hamlet.txt"), [[b"to", b"be"]], "any", 300,
                       450, backend="cpu", rank=4)
    same(f, want(oracle.window(hamlet, 300, 450), [[b"to", b"be"]], "any", 4, first_line=300), 4)
    assert f.first_line == 300 and all(300 <= l < 450 for l in f.lines(0))


def fuzz_case(seed, nlines=200, nvocab=40, nqueries=120):
    rng = random.Random(seed)
    stem = b"q" * 29
    vocab = [bytes(rng.choice(b"abcdeXYZ") for _ in range(rng.randrange(1, 7)))
             for _ in range(nvocab - 4)]
    # words of 29, 30 and 40 bytes: the last two merge with every word of their prefix
    vocab += [stem, stem + b"A", stem + b"B" * 11, b"r" * 28 + b"s"]
    lines = [b" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 12)))
             for _ in range(nlines)]
    text = b"\n".join(lines) + b"\n"
    extra = [b"absent", b"zzz", stem + b"C", b"q" * 40, b"q" * 30, b"q" * 28]
    queries, modes = [], []
    for _ in range(nqueries):
        q = [rng.choice(vocab + extra) for _ in range(rng.randrange(1, 9))]
        if rng.random() < 0.3:
            q[rng.randrange(len(q))] = q[0]  # a repeated term
        mode = rng.choice(["all", "any", "phrase"])
        if mode == "phrase":  # mostly short, so that some match
            q = q[:rng.randrange(1, 3)]
        queries.append(q)
        modes.append(mode)
    return text, queries, modes


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 10**6])
def test_cpu_fuzz(seed, k):
    text, queries, modes = fuzz_case(seed)
    assert any(len(t) in (29, 30, 40) for q in queries for t in q)
    assert {"all", "any", "phrase"} == set(modes)
    expect = want(text, queries, modes, k, first_line=5)
    assert any(m > k for _t, m, _c in expect) or k == 10**6
    assert any(m == 0 for _t, m, _c in expect)
    assert any(m for (_t, m, _c), mode in zip(expect, modes) if mode == "phrase")
    same(cpu_engine(text).run_search(text, queries, modes, 5, rank=k), expect, k)
    # a short key cap: terms are cut as the map cuts keys, and more of them merge
    expect = want(text, queries, modes, k, max_key=3)
    same(cpu_engine(text, max_key_len=3).run_search(text, queries, modes, rank=k), expect, k)


# ------------------------------------------------------------------------------------
# refusals, and the unranked answer
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -3, 2**32, 2**80, "5", 2.5])
def test_refuses_a_rank_that_is_no_k(bad):
    eng = cpu_engine(TEXT)
    with pytest.raises((lc.LocustError, TypeError), match="rank"):
        eng.run_search(TEXT, [[b"to"]], rank=bad)
    with pytest.raises((lc.LocustError, TypeError), match="rank"):
        eng.run_index(TEXT).search([[b"to"]], rank=bad)


def test_largest_k():
    got = cpu_engine(TEXT).run_search(TEXT, [[b"to"]], rank=2**32 - 1)
    assert got.rank_k == 2**32 - 1 and got.lines(0) == [0, 2, 6]


def test_emit_limit():
    over = cpu_engine(TEXT, emits_per_line=oracle.RANK_MAX_EMITS + 1)
    with pytest.raises(lc.LocustError, match="emits_per_line"):
        over.run_search(TEXT, [[b"to"]], rank=1)
    with pytest.raises(lc.LocustError, match="emits_per_line"):
        over.run_index(TEXT).search([[b"to"]], rank=1)
    assert over.run_search(TEXT, [[b"to"]]).lines(0) == [0, 2, 6]  # unranked: no such limit
    at = cpu_engine(TEXT, emits_per_line=oracle.RANK_MAX_EMITS)
    got = at.run_search(TEXT, [[b"to"]], rank=1)
    assert got.lines(0) == [0] and got.scores(0) == [6]
    assert lc._C.kRankMaxEmits == oracle.RANK_MAX_EMITS


BAD_QUERIES = [[b""], [b"a\0b"], [b"a\nb"], [b"a b"], [b"semi;colon"], [],
               [b"t%d" % i for i in range(9)]]


@pytest.mark.parametrize("terms", BAD_QUERIES)
def test_refuses_invalid_queries_as_before(terms):
    eng = cpu_engine(TEXT)
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(TEXT, [[b"to"], terms], rank=2)
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_index(TEXT).search([terms], rank=2)


def test_no_rank_is_the_unranked_answer():
    queries, modes = [[b"to", b"be"], [b"is", b"rose"], [b"absent"], [b"to", b"be"]], \
        ["all", "any", "any", "phrase"]
    eng = cpu_engine(TEXT)
    got = eng.run_search(TEXT, queries, modes, rank=None)
    pos = eng.run_search(TEXT, queries, modes, 0)  # existing positional calls keep working
    ent, post = oracle.index(TEXT)
    lines = [oracle.search(ent, post, q, m)[0] for q, m in zip(queries[:3], modes)]
    lines.append(oracle.phrase(TEXT, queries[3])[0])
    for r in (got, pos):
        assert r.rank_k == 0 and r.matches() == r.hits() == [len(l) for l in lines]
        assert [r.lines(i) for i in range(4)] == lines
        assert [r.scores(i) for i in range(4)] == [[]] * 4
        assert r.format() == oracle.format_search(queries, lines)
    idx = eng.run_index(TEXT).search(queries[:3], modes[:3])
    assert idx.rank_k == 0 and idx.matches() == idx.hits() and idx.scores(1) == []
    assert idx.format() == oracle.format_search(queries[:3], lines[:3])


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_rank(cli, hamlet, tmp_path):
    j = tmp_path / "r.json"
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--search",
            "my lord", "--search", "nosuchword", "--match", "any", "--rank", 5, "--check",
            "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"to", b"be"], [b"my", b"lord"], [b"nosuchword"]]
    expect = want(hamlet, queries, "any", 5)
    assert expect[0][:2] == (HAMLET_FIGURES[0][3], 737)
    assert result_lines(p.stdout) == oracle.format_ranked(
        queries, [t for t, _m, _c in expect], [m for _t, m, _c in expect])
    assert b"print key" not in p.stdout
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 3 and rec["rank_k"] == 5
    assert rec["hits"] == 10 and rec["matches"] == sum(m for _t, m, _c in expect)
    # every mode, over a window that does not start at line 0
    for mode in ("all", "phrase"):
        p = run(cli, "data/hamlet.txt", 1000, 1400, "--backend", "cpu", "--search", "my lord",
                "--match", mode, "--rank", 3)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want(oracle.window(hamlet, 1000, 1400), [[b"my", b"lord"]], mode, 3,
                      first_line=1000)
        assert expect[0][1] > 3 and min(l for l, _s in expect[0][0]) >= 1000
        assert result_lines(p.stdout) == oracle.format_ranked([[b"my", b"lord"]], [expect[0][0]],
                                                              [expect[0][1]])
    # without --rank the record says so
    p = run(cli, "data/hamlet.txt", 0, 300, "--backend", "cpu", "--search", "to be", "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rec = json.load(open(j))
    assert rec["rank_k"] == 0 and rec["matches"] == rec["hits"] > 0
    assert b" \t lines: " in p.stdout and b"top:" not in p.stdout


@pytest.mark.parametrize("args, msg", [
    (["--rank", "5"], "--search"),
    (["--search", "to", "--rank", "0"], "--rank"),
    (["--search", "to", "--rank", "-2"], "--rank"),
    (["--search", "to", "--rank", "five"], "--rank"),
    (["--search", "to", "--rank", "4294967296"], "--rank"),
    (["--search", "to", "--rank", "3", "--top", "5"], "--top"),
    (["--search", "to", "--rank", "3", "--emits-per-line", "65537"], "emits_per_line"),
])
def test_cli_rank_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"--rank" in p.stderr or b"--search" in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--rank K" in p.stdout
