"""Proximity (`near`) queries without a GPU: ``oracle.near`` on a hand-written text (one
assertion per rule of the semantics), the CPU engine's ``run_search`` against it (exactly:
the answer is a pure function of the text), ``IndexResult.search`` and its refusal, the
window rules of every interface, mixed batches, fuzz, the CLI's ``--backend cpu --match near
--within W`` lines and whole Hamlet."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from near_cases import BY_HAND, TEXT, W_MAX, fuzz_case, same, same_ranked, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


# ------------------------------------------------------------------------------------
# the oracle, rule by rule
# ------------------------------------------------------------------------------------
def test_oracle_by_hand():
    assert len(oracle.split_lines(TEXT)) == 10
    for terms, w, wild, lines in BY_HAND:
        assert oracle.near(TEXT, terms, w, wildcard=wild)[0] == lines, (terms, w, wild)
    # the counts are `all`'s: every emitted token that matches
    assert oracle.near(TEXT, [b"to", b"be"], 2) == ([0], [7, 6])
    assert oracle.near(TEXT, [b"Ham*", b"Hamlet"], 1, wildcard=True) == ([6, 7], [3, 2])
    assert oracle.near(TEXT, [b"bye", b"bye"], 1) == ([5], [1, 1])
    # one term, and W >= the emit cap, answer as `all` does
    ent, post = oracle.index(TEXT)
    assert oracle.near(TEXT, [b"to"], 1) == oracle.search(ent, post, [b"to"], "all")
    assert oracle.near(TEXT, [b"to", b"be"], 20) == oracle.search(ent, post, [b"to", b"be"], "all")
    # global numbering
    assert oracle.near(TEXT, [b"to", b"be"], 3, first_line=1000)[0] == [1000, 1001]


def test_oracle_emit_cap_and_truncation():
    line = b" ".join(b"w%d" % i for i in range(25))
    text = line + b"\n"
    assert oracle.near(text, [b"w19", b"w17"], 3) == ([0], [1, 1])
    assert oracle.near(text, [b"w20", b"w19"], 2) == ([], [0, 1])  # the 21st token does not exist
    assert oracle.near(text, [b"w20", b"w19"], W_MAX) == ([], [0, 1])
    assert oracle.near(text, [b"w2", b"w0"], 3, emits=3) == ([0], [1, 1])
    assert oracle.near(text, [b"w3", b"w2"], 3, emits=3) == ([], [0, 1])
    a = b"x" * 29 + b"AAAAAA"
    text = a + b" foo\nfoo bar " + a + b"\n" + b"x" * 28 + b" foo\n"
    assert oracle.near(text, [b"foo", b"x" * 35], 2) == ([0], [3, 2])
    assert oracle.near(text, [b"foo", b"x" * 29], 3) == ([0, 1], [3, 2])
    text = b"abcdefgh abcdeXYZ\nabcd abcde\n"
    assert oracle.near(text, [b"abcdeQ", b"abcd"], 2, max_key=5) == ([1], [3, 1])
    # another delimiter set
    assert oracle.near(b"a-b c\n", [b"b", b"a"], 2, delims=b" ") == ([], [0, 0])
    assert oracle.near(b"a-b c\n", [b"c", b"a-b"], 2, delims=b" ") == ([0], [1, 1])


@pytest.mark.parametrize("terms", [[b""], [b"a\0b"], [b"a\nb"], [b"a b"], [],
                                   [b"t%d" % i for i in range(9)]])
def test_oracle_refuses_invalid_terms(terms):
    with pytest.raises(ValueError):
        oracle.near(TEXT, terms, 2)


@pytest.mark.parametrize("w", [0, -1, 1 << 32, None, 2.0, True])
def test_oracle_refuses_invalid_windows(w):
    with pytest.raises(ValueError):
        oracle.near(TEXT, [b"to", b"be"], w)


def test_oracle_search_keeps_its_modes():
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.search(ent, post, [b"to", b"be"], "near")


# ------------------------------------------------------------------------------------
# the CPU engine
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wild", [False, True])
def test_cpu_by_hand(wild):
    cases = [c for c in BY_HAND if c[2] == wild]
    queries, within = [c[0] for c in cases], [c[1] for c in cases]
    expect = want(TEXT, queries, "near", within, wildcard=wild)
    assert [l for l, _c in expect] == [c[3] for c in cases]
    got = cpu_engine(TEXT).run_search(TEXT, queries, "near", wildcard=wild, within=within)
    same(got, expect)
    assert got.format() == oracle.format_search(queries, [c[3] for c in cases])
    # one window for the whole batch, the last line without its newline, another first line
    text = TEXT + b"be to"
    q = [[b"to", b"be"], [b"be", b"to"]]
    got = lc.search_text(text, q, "near", backend="cpu", first_line=10, within=3)
    same(got, want(text, q, "near", 3, first_line=10))
    assert got.lines(0) == got.lines(1) == [10, 11, 20]


def test_cpu_emit_cap_and_truncation():
    line = b" ".join(b"w%d" % i for i in range(25)) + b"\n"
    queries = [[b"w19", b"w17"], [b"w20", b"w19"], [b"w20", b"w19"]]
    within = [3, 2, W_MAX]
    got = cpu_engine(line).run_search(line, queries, "near", within=within)
    same(got, want(line, queries, "near", within))
    assert got.hits() == [1, 0, 0]
    got = cpu_engine(line, emits_per_line=3).run_search(line, [[b"w2", b"w0"], [b"w3", b"w2"]],
                                                        "near", within=3)
    assert got.hits() == [1, 0]
    a = b"x" * 29 + b"AAAAAA"
    text = a + b" foo\nfoo bar " + a + b"\n" + b"x" * 28 + b" foo\n"
    queries, within = [[b"foo", b"x" * 35], [b"foo", b"x" * 29]], [2, 3]
    got = cpu_engine(text).run_search(text, queries, "near", within=within)
    same(got, want(text, queries, "near", within))
    assert got.lines(0) == [0] and got.lines(1) == [0, 1]
    text = b"abcdefgh abcdeXYZ\nabcd abcde\n"
    got = cpu_engine(text, max_key_len=5).run_search(text, [[b"abcdeQ", b"abcd"]], "near", within=2)
    same(got, want(text, [[b"abcdeQ", b"abcd"]], "near", 2, max_key=5))
    assert got.lines(0) == [1]


def test_cpu_mixed_batch():
    queries = [[b"to", b"be"]] * 4 + [[b"be", b"to"]] * 4 + [[b"be"], [b"be"]]
    modes = ["all", "any", "phrase", "near"] * 2 + ["near", "all"]
    within = [None, None, None, 3] * 2 + [1, None]
    expect = want(TEXT, queries, modes, within)
    got = cpu_engine(TEXT).run_search(TEXT, queries, modes, within=within)
    same(got, expect)
    assert got.hits()[:4] == [4, 7, 1, 2] and got.hits()[4:8] == [4, 7, 0, 2]
    assert got.lines(8) == got.lines(9)
    # an int window goes to the batch's near queries
    same(cpu_engine(TEXT).run_search(TEXT, queries[:8], modes[:8], within=3), expect[:8])


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("wild", [False, True])
def test_cpu_fuzz(seed, wild):
    text, queries, modes, within = fuzz_case(seed, wildcard=wild)
    assert W_MAX in within and {1, 2, 8} <= set(within) and set(modes) == {"all", "any", "phrase",
                                                                         "near"}
    expect = want(text, queries, modes, within, first_line=5, wildcard=wild)
    nr = [(e, w, q) for e, m, w, q in zip(expect, modes, within, queries)
          if m == "near" and len(q) >= 2]
    assert sum(bool(l) for (l, _c), _w, _q in nr) > 10 and sum(not l for (l, _c), _w, _q in nr) > 10
    # the window decides: some near answer is a proper, non-empty subset of the `all` answer
    ent, post = oracle.index(text, first_line=5)
    assert any(l and len(l) < len(oracle.search(ent, post, q, "all", wildcard=wild)[0])
               for (l, _c), _w, q in nr)
    eng = cpu_engine(text)
    same(eng.run_search(text, queries, modes, 5, wildcard=wild, within=within), expect)
    same_ranked(eng.run_search(text, queries, modes, 5, rank=3, wildcard=wild, within=within),
                text, queries, expect, 3, first_line=5, wildcard=wild)
    # a short key cap and a small emit cap (W >= 4 is `all` there)
    expect = want(text, queries, modes, within, wildcard=wild, max_key=3, emits=4)
    got = cpu_engine(text, max_key_len=3, emits_per_line=4).run_search(
        text, queries, modes, wildcard=wild, within=within)
    same(got, expect)


# ------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------
def test_index_result_search_and_its_refusal():
    eng = cpu_engine(TEXT)
    x = eng.run_index(TEXT)
    # one term: answered from the index, as `all`
    got = x.search([[b"to"], [b"to"]], ["near", "all"], within=[4, None])
    assert got.lines(0) == got.lines(1) == [0, 1, 2, 3, 8, 9]
    for batch, modes, within in (([[b"to", b"be"]], "near", 3),
                                 ([[b"to"], [b"to", b"be"]], ["all", "near"], [None, W_MAX])):
        with pytest.raises(lc.LocustError, match=r"near.*needs the text.*search_index\(index, "
                                                 r"text, queries, cfg\)"):
            x.search(batch, modes, within=within)
    with pytest.raises(ValueError, match="within"):
        x.search([[b"to", b"be"]], "near")
    with pytest.raises(ValueError, match="within"):
        x.search([[b"to", b"be"]], "all", within=2)


@pytest.mark.parametrize("mode, within", [
    ("near", None), ("near", 0), ("near", -3), ("near", 1 << 32), ("near", 2.5), ("near", True),
    ("near", [None, None]), ("near", [2]), ("near", [2, 0]),
    ("all", 2), ("any", 2), ("phrase", 2), ("all", [2, None]), (["near", "all"], [2, 2]),
    (["all", "phrase"], 2)])
def test_invalid_windows_are_refused(mode, within):
    eng = cpu_engine(TEXT)
    with pytest.raises(ValueError, match="within"):
        eng.run_search(TEXT, [[b"to", b"be"], [b"be", b"to"]], mode, within=within)
    with pytest.raises(ValueError, match="within"):
        lc.search_text(TEXT, [[b"to", b"be"], [b"be", b"to"]], mode, backend="cpu", within=within)


def test_other_refusals_and_accepted_windows():
    eng = cpu_engine(TEXT)
    with pytest.raises(ValueError, match="near"):
        eng.run_search(TEXT, [[b"to"]], "most")
    with pytest.raises(ValueError):
        eng.run_search(TEXT, [[b"to"]], ["near", "all"], within=[2, None])
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(TEXT, [[b"to", b"a b"]], "near", within=2)
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(TEXT, [[b"t%d" % i for i in range(9)]], "near", within=2)
    with pytest.raises(lc.LocustError, match="search_resident"):
        eng.search_resident([[b"to", b"be"]], "near", within=2)
    # every W up to 2^32 - 1 is accepted; existing calls keep working without the argument
    got = eng.run_search(TEXT, [[b"to", b"be"]] * 2, "near", within=[1, W_MAX])
    assert got.hits() == [0, 4]
    assert eng.run_search(TEXT, [[b"to", b"be"]], "all").hits() == [4]
    assert eng.run_search(TEXT, [[b"to", b"be"]], "all", 0, None, False).hits() == [4]


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_near(cli, hamlet):
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "the king", "--match", "near",
            "--within", 3)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines, _counts = oracle.near(hamlet, [b"the", b"king"], 3)
    assert len(lines) == 5
    assert result_lines(p.stdout) == oracle.format_search([[b"the", b"king"]], [lines])
    # a window of the file, a batch, --wildcard and the delimiters of the argument itself
    p = run(cli, "data/hamlet.txt", 1000, 2000, "--backend", "cpu", "--search", "lord, my",
            "--search", "Ham* lord", "--match", "near", "--within", 2, "--wildcard", "--check")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"lord", b"my"], [b"Ham*", b"lord"]]
    expect = want(oracle.window(hamlet, 1000, 2000), queries, "near", 2, first_line=1000,
                  wildcard=True)
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
    assert expect[0][0] and min(expect[0][0]) >= 1000
    # ranked
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "near",
            "--within", 4, "--rank", 2)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"hits: 34 \t top:" in p.stdout


def test_cli_misuse_is_refused(cli):
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "near")
    assert p.returncode != 0 and b"--within" in p.stderr and b"print query" not in p.stdout
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--within", 2)
    assert p.returncode != 0 and b"--within" in p.stderr and b"--match near" in p.stderr
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "phrase",
            "--within", 2)
    assert p.returncode != 0 and b"--within" in p.stderr and b"print query" not in p.stdout
    for w in ("0", "-1", "4294967296", "two", ""):
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "near",
                "--within", w)
        assert p.returncode != 0 and b"--within" in p.stderr, w
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--match", "near",
            "--within", 4294967295)
    assert p.returncode == 0 and b"hits: 47 " in p.stdout
    p = run(cli, "--help")
    assert p.returncode == 0 and b"all|any|phrase|near" in p.stdout and b"--within W" in p.stdout


# ------------------------------------------------------------------------------------
# whole Hamlet: oracle.near is authoritative, the counts a cross-check of it
# ------------------------------------------------------------------------------------
HAMLET = [([b"to", b"be"], {2: 27, 3: 31, 4: 34, 5: 39, 8: 46, 20: 47}),
          ([b"my", b"lord"], {2: 110, 3: 115}),
          ([b"the", b"king"], {2: 3, 3: 5, 8: 7}),
          ([b"to", b"be", b"not"], {3: 2, 5: 4, 8: 6})]


def test_cpu_hamlet(hamlet):
    queries = [q for q, ws in HAMLET for _w in ws]
    within = [w for _q, ws in HAMLET for w in ws]
    expect = want(hamlet, queries, "near", within)
    assert [len(l) for l, _c in expect] == [n for _q, ws in HAMLET for n in ws.values()]
    eng = cpu_engine(hamlet)
    got = eng.run_search(hamlet, queries, "near", within=within)
    same(got, expect)
    # between phrase and all: near with W = 2 holds the phrase's lines in either order
    ph = set(oracle.phrase(hamlet, [b"to", b"be"])[0]) | set(oracle.phrase(hamlet, [b"be", b"to"])[0])
    assert set(got.lines(0)) == ph
    assert all(set(got.lines(i)) <= set(got.lines(i + 1)) for i in range(5))
    f = lc.search_file(os.path.join(ROOT, "data", "hamlet.txt"), [[b"lord", b"my"]], "near",
                       300, 450, backend="cpu", within=2)
    same(f, want(oracle.window(hamlet, 300, 450), [[b"lord", b"my"]], "near", 2, first_line=300))
    assert f.first_line == 300 and f.lines(0) and all(300 <= l < 450 for l in f.lines(0))
