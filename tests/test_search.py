"""All/any word queries over the inverted index without a GPU: the oracle on hand-written
texts, the CPU engine and ``IndexResult.search`` against the oracle (exactly: the answer is a
pure function of the index), term validation, the CLI's ``--backend cpu --search`` lines and
every refused flag combination."""
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


def want(text, queries, modes, first_line=0, **okw):
    """[(lines, counts)] of every query by the oracle."""
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {k: v for k, v in okw.items() if k in ("delims", "max_key")}
    return [oracle.search(ent, post, q, m, **skw) for q, m in zip(queries, modes)]


def same(got, expect):
    assert got.queries == len(expect)
    assert got.hits() == [len(l) for l, _c in expect]
    for i, (lines, counts) in enumerate(expect):
        assert got.lines(i) == lines, i
        assert got.term_counts(i) == counts, i


# ------------------------------------------------------------------------------------
# the oracle, on texts whose answers are spelled out
# ------------------------------------------------------------------------------------
TEXT = (b"to be or not to be\n"        # 0
        b"that is the question\n"      # 1
        b"to sleep\n"                  # 2
        b"\n"                          # 3
        b"be all my sins\n"            # 4
        b"rose is a rose is a rose\n"  # 5
        b"not to be\n")                # 6


def test_oracle_by_hand():
    ent, post = oracle.index(TEXT)
    s = lambda terms, mode="all": oracle.search(ent, post, terms, mode)
    assert s([b"to"]) == ([0, 2, 6], [4])
    assert s([b"to", b"be"]) == ([0, 6], [4, 4])
    assert s([b"to", b"be"], "any") == ([0, 2, 4, 6], [4, 4])
    assert s([b"rose"]) == ([5], [3])                      # three times on a line: one hit
    assert s([b"rose", b"is", b"a"]) == ([5], [3, 3, 2])
    assert s([b"is", b"rose"], "any") == ([1, 5], [3, 3])
    assert s([b"to", b"absent"]) == ([], [4, 0])           # all: empty with one absent term
    assert s([b"to", b"absent"], "any") == ([0, 2, 6], [4, 0])
    assert s([b"absent", b"gone"], "any") == ([], [0, 0])
    assert s([b"to", b"to", b"be", b"to"]) == s([b"to", b"be"])[0:1] + ([4, 4, 4, 4],)
    assert s([b"be", b"be"], "any") == ([0, 4, 6], [4, 4])
    assert s([b"not", b"to", b"be", b"or"]) == ([0], [2, 4, 4, 1])
    # global numbering
    ent, post = oracle.index(TEXT, first_line=1000)
    assert oracle.search(ent, post, [b"to", b"be"]) == ([1000, 1006], [4, 4])


def test_oracle_truncation():
    a, b = b"x" * 29 + b"AAAA", b"x" * 29 + b"BBBB"
    text = a + b" foo\nbar " + b + b"\nfoo\n"
    ent, post = oracle.index(text)
    # a 35-byte term is cut to 29 bytes: the merged list of both long words
    assert oracle.search(ent, post, [b"x" * 35]) == ([0, 1], [2])
    assert oracle.search(ent, post, [a, b"foo"]) == ([0], [2, 2])
    ent, post = oracle.index(b"abcdefgh abcdeXYZ\nabcde abcd\n", max_key=5)
    assert oracle.search(ent, post, [b"abcdeQQQ"], max_key=5) == ([0, 1], [3])
    assert oracle.search(ent, post, [b"abcd"], max_key=5) == ([1], [1])


BAD_QUERIES = [[b""], [b"a\0b"], [b"a\nb"], [b"a b"], [b"semi;colon"], [],
               [b"t%d" % i for i in range(9)]]


@pytest.mark.parametrize("terms", BAD_QUERIES)
def test_oracle_refuses_invalid_queries(terms):
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.search(ent, post, terms, "all")


def test_oracle_format():
    assert oracle.format_search([[b"to", b"be"], [b"gone"]], [[0, 6], []]) == (
        b"print query: to be \t hits: 2 \t lines: 0 6\n"
        b"print query: gone \t hits: 0 \t lines:\n")


# ------------------------------------------------------------------------------------
# the CPU engine and IndexResult.search
# ------------------------------------------------------------------------------------
def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def both_routes(text, queries, modes, first_line=0, **kw):
    """CpuWordCount.run_search and IndexResult.search: the same evaluation, two doors."""
    eng = cpu_engine(text, **kw)
    a = eng.run_search(text, queries, modes, first_line)
    b = eng.run_index(text, first_line).search(queries, modes)
    assert a.format() == b.format()
    return a, b


def test_cpu_by_hand():
    queries = [[b"to", b"be"], [b"to", b"be"], [b"rose"], [b"to", b"absent"], [b"absent"],
               [b"to", b"to", b"be"]]
    modes = ["all", "any", "all", "all", "any", "all"]
    expect = want(TEXT, queries, modes)
    for got in both_routes(TEXT, queries, modes):
        same(got, expect)
        assert got.lines(0) == [0, 6] and got.lines(1) == [0, 2, 4, 6] and got.lines(2) == [5]
        assert got.format() == oracle.format_search(queries, [l for l, _c in expect])
        assert got.search_ms >= 0 and "search_ms" in got.times() and got.first_line == 0
    # one mode for the whole batch, and module-level entry points
    got = lc.search_text(TEXT, [[b"to", b"be"], [b"is"]], "any", backend="cpu", first_line=10)
    same(got, want(TEXT, [[b"to", b"be"], [b"is"]], ["any", "any"], first_line=10))
    assert got.lines(1) == [11, 15]
    # an empty batch is an empty result on the host
    assert cpu_engine(TEXT).run_search(TEXT, []).hits() == []


def test_cpu_hamlet(hamlet):
    win = oracle.window(hamlet, 0, 700)
    queries = [[b"to", b"be"], [b"Ham", b"Hor"], [b"the"], [b"Ham", b"Hor"], [b"to", b"be"],
               [b"the", b"and", b"of", b"to", b"a", b"in", b"my", b"you"]]
    modes = ["all", "all", "all", "any", "any", "any"]
    expect = want(win, queries, modes)
    assert expect[0][0] and expect[3][0]
    for got in both_routes(win, queries, modes):
        same(got, expect)
        assert got.num_lines == 700
    f = lc.search_file(os.path.join(ROOT, "data", "hamlet.txt"), [[b"to", b"be"]], "all", 300,
                       450, backend="cpu")
    sub = oracle.window(hamlet, 300, 450)
    same(f, want(sub, [[b"to", b"be"]], ["all"], first_line=300))
    assert f.first_line == 300 and all(300 <= l < 450 for l in f.lines(0))


def fuzz_case(seed, nlines=300, nvocab=50, nqueries=200):
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
        queries.append(q)
        modes.append(rng.choice(["all", "any"]))
    return text, queries, modes


@pytest.mark.parametrize("seed", [1, 2])
def test_cpu_fuzz(seed):
    text, queries, modes = fuzz_case(seed)
    assert any(len(t) in (29, 30, 40) for q in queries for t in q)
    expect = want(text, queries, modes, first_line=5)
    assert any(l for l, _c in expect) and any(not l for l, _c in expect)
    for got in both_routes(text, queries, modes, first_line=5):
        same(got, expect)
    # a short key cap: terms are cut as the map cuts keys
    expect = want(text, queries, modes, max_key=3)
    for got in both_routes(text, queries, modes, max_key_len=3):
        same(got, expect)


@pytest.mark.parametrize("terms", BAD_QUERIES)
def test_cpu_refuses_invalid_queries(terms):
    eng = cpu_engine(TEXT)
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(TEXT, [[b"to"], terms])
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_index(TEXT).search([terms])


def test_cpu_validation_follows_the_delimiter_set():
    eng = cpu_engine(TEXT, delimiters=" ")
    got = eng.run_search(b"semi;colon x\nx\n", [[b"semi;colon"], [b"x"]])
    assert got.lines(0) == [0] and got.lines(1) == [0, 1]
    with pytest.raises(ValueError):
        eng.run_search(TEXT, [[b"to"]], "most")
    with pytest.raises(ValueError):
        eng.run_search(TEXT, [[b"to"]], ["all", "any"])
    with pytest.raises(lc.LocustError, match="GPU"):
        eng.search_resident([[b"to"]])
    with pytest.raises(lc.LocustError, match="ngram"):
        cpu_engine(TEXT, ngram=2).run_search(TEXT, [[b"to"]])


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_search(cli, hamlet, tmp_path):
    j = tmp_path / "s.json"
    p = run(cli, "data/hamlet.txt", 0, 700, "--backend", "cpu", "--search", "to be", "--search",
            "Ham, Hor", "--search", "nosuchword", "--check", "--json", j)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"to", b"be"], [b"Ham", b"Hor"], [b"nosuchword"]]
    expect = want(oracle.window(hamlet, 0, 700), queries, ["all"] * 3)
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
    assert b"print key" not in p.stdout
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 3
    assert rec["hits"] == sum(len(l) for l, _c in expect) and rec["search_ms"] >= 0
    # --match any over a window that does not start at line 0, with its own key cap
    p = run(cli, "data/hamlet.txt", 1000, 1200, "--backend", "cpu", "--search", "the and",
            "--match", "any", "--max-key", 6)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    expect = want(oracle.window(hamlet, 1000, 1200), [[b"the", b"and"]], ["any"], first_line=1000,
                  max_key=6)
    assert result_lines(p.stdout) == oracle.format_search([[b"the", b"and"]], [expect[0][0]])
    assert expect[0][0] and min(expect[0][0]) >= 1000


@pytest.mark.parametrize("args, msg", [
    (["--search", "to", "--top", "5"], "--top"),
    (["--search", "to", "--ngram", "2"], "--ngram"),
    (["0", "100", "0", "1", "--search", "to"], "stage"),
    (["0", "100", "0", "2", "--search", "to"], "stage"),
    (["--search", "to", "--gpus", "2"], "--gpus"),
    (["--search", "to", "--chunk-mb", "1"], "--chunk-mb"),
    (["--search", "to", "--sort", "radix"], "--sort dict"),
    (["--search", "to", "--map-path", "compat"], "--map-path"),
    (["--search", "to", "--index"], "--index"),
    (["--search", " ,. "], "no word"),
    (["--search", "a b c d e f g h i"], "terms"),
    (["--search", "to", "--match", "most"], "--match"),
    (["--match", "any"], "--search"),
])
def test_cli_search_refusals(cli, args, msg, tmp_path):
    p = run(cli, "data/hamlet.txt", *args, "--spill-dir", tmp_path)
    assert p.returncode != 0
    assert msg.encode() in p.stderr and b"earch" in p.stderr
    assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flags(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--search" in p.stdout and b"--match" in p.stdout
