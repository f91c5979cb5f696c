"""Exclusion terms (``exclude=``, ``--not``) without a GPU: the oracle on a hand-written text
(one assertion per rule of ``oracle.EXCLUDE_RULES``), the CPU engine's ``run_search`` and the
host evaluation ``IndexResult.search`` against it (exactly: the answer is a pure function of
the text), the refusals of every interface, ranked answers, ``format()``, fuzz, the CLI's
``--not`` and whole Hamlet."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from exclude_cases import BY_HAND, TEXT, W_MAX, fuzz_case, same, same_ranked, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def cases(wild):
    cs = [c for c in BY_HAND if c[4] == wild]
    return ([c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs],
            [c[5] for c in cs])


# ------------------------------------------------------------------------------------
# the oracle, rule by rule
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wild", [False, True])
def test_oracle_by_hand(wild):
    assert len(oracle.split_lines(TEXT)) == 16
    queries, exclude, modes, within, lines = cases(wild)
    expect = want(TEXT, queries, modes, within, exclude, wildcard=wild)
    assert [l for l, _c in expect] == lines


def test_oracle_counts_and_shapes():
    ent, post = oracle.index(TEXT)
    # positive terms first, then the exclusion terms in the order given; an absent one: 0
    assert oracle.search(ent, post, [b"alpha", b"beta"], exclude=[b"gone", b"gamma"]) == \
        ([0, 3, 10], [10, 5, 0, 7])
    assert oracle.phrase(TEXT, [b"alpha", b"beta"], exclude=[b"gamma"]) == ([0, 10], [10, 5, 7])
    assert oracle.near(TEXT, [b"beta", b"alpha"], 2, exclude=[b"gamma", b"gamma"]) == \
        ([0, 10], [5, 10, 7, 7])
    # a merged count
    assert oracle.search(ent, post, [b"alpha"], wildcard=True, exclude=[b"ab*"])[1] == [10, 5]
    # no exclusion terms, either way of saying so: what the call answered before
    for x in (None, []):
        assert oracle.search(ent, post, [b"alpha", b"beta"], exclude=x) == \
            oracle.search(ent, post, [b"alpha", b"beta"])
        assert oracle.phrase(TEXT, [b"alpha", b"beta"], exclude=x) == \
            oracle.phrase(TEXT, [b"alpha", b"beta"])
    # global numbering
    assert oracle.phrase(TEXT, [b"alpha", b"beta"], first_line=100, exclude=[b"gamma"])[0] == \
        [100, 110]
    # a token past the emit cap is not in the index: it excludes nothing
    text = b" ".join(b"w%d" % i for i in range(25)) + b"\n"
    e2, p2 = oracle.index(text)
    assert oracle.search(e2, p2, [b"w0"], exclude=[b"w20"]) == ([0], [1, 0])
    assert oracle.search(e2, p2, [b"w0"], exclude=[b"w19"]) == ([], [1, 1])
    assert oracle.phrase(text, [b"w0", b"w1"], exclude=[b"w20"])[0] == [0]
    assert oracle.near(text, [b"w1", b"w0"], 2, exclude=[b"w19"])[0] == []
    # an exclusion term is cut like any term
    a = b"x" * 29
    text = a + b"AAAA foo\n" + a + b" foo\nfoo\n"
    e3, p3 = oracle.index(text)
    assert oracle.search(e3, p3, [b"foo"], exclude=[a + b"ZZ"]) == ([2], [3, 2])


def test_oracle_merged_and_rank():
    ent, post = oracle.index(TEXT)
    # ab* covers three words (ab, abc, abd: 2 + 2 + 1 postings), gam* one, zz* none
    assert oracle.merged_elements(ent, [[b"alpha"]], exclude=[[b"ab*"]]) == 5
    assert oracle.merged_elements(ent, [[b"alpha"]], exclude=[[b"gam*", b"zz*"]]) == 0
    # a term whose words repeat an earlier term's is left out, whichever kind it is
    assert oracle.merged_elements(ent, [[b"ab*"], [b"ab*", b"alpha"]],
                                  exclude=[[b"ab*", b"ab*"], None]) == 10
    assert oracle.merged_elements(ent, [[b"ab*"]]) == oracle.merged_elements(
        ent, [[b"ab*"]], exclude=[None]) == 5
    # ranked: the exclusion terms take lines away and add nothing to a score
    lines = oracle.search(ent, post, [b"alpha", b"beta"], "any")[0]
    top, matches = oracle.rank(ent, post, lines, [b"alpha", b"beta"], 3)
    xtop, xmatches = oracle.rank(ent, post, lines, [b"alpha", b"beta"], 99, exclude=[b"gamma"])
    assert matches == 10 and xmatches == 8 and [l for l, _s in xtop][:2] == [0, 3]
    full = dict(oracle.rank(ent, post, lines, [b"alpha", b"beta"], 99)[0])
    assert all(full[l] == s for l, s in xtop) and not {1, 2} & {l for l, _s in xtop}
    # ... from the answer before or after the exclusion
    after = oracle.search(ent, post, [b"alpha", b"beta"], "any", exclude=[b"gamma"])[0]
    assert oracle.rank(ent, post, after, [b"alpha", b"beta"], 99, exclude=[b"gamma"]) == \
        (xtop, xmatches)
    # Ham* keeps its full merged count beside `not Hamlet`
    assert oracle.rank(ent, post, [13], [b"Ham*"], 1, wildcard=True, exclude=[b"Hamlet"]) == \
        oracle.rank(ent, post, [13], [b"Ham*"], 1, wildcard=True)


@pytest.mark.parametrize("terms, exclude", [
    ([], [b"gamma"]),                                     # no positive term
    ([b"alpha"], [b"t%d" % i for i in range(8)]),         # 9 in all
    ([b"t%d" % i for i in range(8)], [b"gamma"]),
    ([b"alpha"], [b""]), ([b"alpha"], [b"a b"]), ([b"alpha"], [b"a\0b"]), ([b"alpha"], [b"a\nb"]),
    ([b"alpha"], ["gamma"])])
def test_oracle_refuses(terms, exclude):
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.search(ent, post, terms, exclude=exclude)
    with pytest.raises(ValueError):
        oracle.phrase(TEXT, terms, exclude=exclude)
    with pytest.raises(ValueError):
        oracle.near(TEXT, terms, 2, exclude=exclude)
    with pytest.raises(ValueError):
        oracle.rank(ent, post, [0], terms, 1, exclude=exclude)


def test_oracle_refuses_a_lone_star():
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.search(ent, post, [b"alpha"], wildcard=True, exclude=[b"*"])
    assert oracle.search(ent, post, [b"alpha"], exclude=[b"*"])[1] == [10, 0]  # a literal token
    with pytest.raises(ValueError):
        oracle.merged_elements(ent, [[b"alpha"]], exclude=[])


# ------------------------------------------------------------------------------------
# the CPU engine and the host evaluation
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wild", [False, True])
def test_cpu_by_hand(wild):
    queries, exclude, modes, within, lines = cases(wild)
    expect = want(TEXT, queries, modes, within, exclude, wildcard=wild)
    got = cpu_engine(TEXT).run_search(TEXT, queries, modes, wildcard=wild, within=within,
                                      exclude=exclude)
    same(got, expect)
    assert [got.lines(i) for i in range(len(queries))] == lines
    assert got.format() == oracle.format_search(queries, lines, exclude=exclude)
    # None and [] both say "no exclusion terms"; another first line
    ex = [x or None for x in exclude]
    got = lc.search_text(TEXT, queries, modes, backend="cpu", first_line=10, wildcard=wild,
                         within=within, exclude=ex)
    same(got, want(TEXT, queries, modes, within, exclude, first_line=10, wildcard=wild))


def test_host_evaluation_from_the_index():
    """``IndexResult.search``: all/any and one-term phrase/near queries, any number of them;
    what it refuses is decided by the positive terms."""
    x = cpu_engine(TEXT).run_index(TEXT)
    queries = [[b"alpha", b"beta"], [b"alpha", b"beta"], [b"alpha"], [b"bye"], [b"ab*"]] * 300
    exclude = [[b"gamma"], [b"beta", b"gone"], [b"gamma", b"beta"], [b"x"], [b"abc"]] * 300
    modes = ["all", "any", "near", "near", "all"] * 300
    within = [None, None, 3, 1, None] * 300
    expect = want(TEXT, queries, modes, within, exclude, wildcard=True)
    same(x.search(queries, modes, wildcard=True, within=within, exclude=exclude), expect)
    assert len(queries) > 1024 and expect[3][0] == [6] and expect[4][0] == [10]
    with pytest.raises(lc.LocustError, match="phrase query needs the text"):
        x.search([[b"bye"]], "phrase", exclude=[[b"x"]])
    with pytest.raises(lc.LocustError, match="near.*needs the text"):
        x.search([[b"alpha", b"beta"]], "near", within=2, exclude=[[b"gamma"]])
    # ranked on the host
    r = x.search(queries[:5], modes[:5], rank=2, wildcard=True, within=within[:5],
                 exclude=exclude[:5])
    same_ranked(r, TEXT, queries[:5], exclude[:5], expect[:5], 2, wildcard=True)


def test_cpu_ranked():
    queries = [[b"alpha", b"beta"], [b"alpha", b"beta"], [b"Ham*"], [b"Ham*", b"Hamlet"],
               [b"gamma", b"alpha"]]
    exclude = [[b"gamma"], [b"delta", b"x"], [b"Hamlet"], [b"alpha"], [b"beta"]]
    modes = ["any", "phrase", "all", "any", "any"]
    expect = want(TEXT, queries, modes, None, exclude, wildcard=True)
    eng = cpu_engine(TEXT)
    for k in (1, 3, 99):
        got = eng.run_search(TEXT, queries, modes, rank=k, wildcard=True, exclude=exclude)
        same_ranked(got, TEXT, queries, exclude, expect, k, wildcard=True)
    # the best line of `gamma alpha` is line 15 (gamma three times), then 2: both hold no
    # beta; with `not gamma` ... the best-scoring line does not come back
    got = eng.run_search(TEXT, [[b"gamma", b"alpha"]] * 2, "any", rank=1,
                         exclude=[None, [b"gamma"]])
    assert got.lines(0) == [15] and got.lines(1) != [15] and got.matches() == [12, 8]
    assert 15 not in eng.run_search(TEXT, [[b"gamma", b"alpha"]], "any", rank=99,
                                    exclude=[[b"gamma"]]).lines(0)
    # Ham* keeps its full weight beside `not Hamlet`: line 13's score is the unexcluded one
    a = eng.run_search(TEXT, [[b"Ham*"]] * 2, rank=9, wildcard=True, exclude=[None, [b"Hamlet"]])
    assert a.lines(1) == [13] and a.scores(1) == [a.scores(0)[a.lines(0).index(13)]]
    assert a.format() == oracle.format_ranked(
        [[b"Ham*"]] * 2, [list(zip(a.lines(i), a.scores(i))) for i in range(2)], a.matches(),
        exclude=[None, [b"Hamlet"]])


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("wild", [False, True])
def test_cpu_fuzz(seed, wild):
    text, queries, modes, within, exclude = fuzz_case(seed, wildcard=wild)
    assert set(modes) == {"all", "any", "phrase", "near"} and W_MAX in within
    expect = want(text, queries, modes, within, exclude, first_line=5, wildcard=wild)
    eng = cpu_engine(text)
    same(eng.run_search(text, queries, modes, 5, wildcard=wild, within=within, exclude=exclude),
         expect)
    same_ranked(eng.run_search(text, queries, modes, 5, rank=3, wildcard=wild, within=within,
                               exclude=exclude),
                text, queries, exclude, expect, 3, first_line=5, wildcard=wild)
    # a short key cap and a small emit cap (W >= 4 is `all` there)
    expect = want(text, queries, modes, within, exclude, wildcard=wild, max_key=3, emits=4)
    got = cpu_engine(text, max_key_len=3, emits_per_line=4).run_search(
        text, queries, modes, wildcard=wild, within=within, exclude=exclude)
    same(got, expect)


# ------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------
def test_term_budget_and_refusals():
    eng = cpu_engine(TEXT)
    t = [b"t%d" % i for i in range(8)]
    for q, x in (([b"alpha"], t[:7]), (t[:7] + [b"alpha"], None), (t[:6] + [b"alpha"], [b"gamma"])):
        got = eng.run_search(TEXT, [q], exclude=[x])
        same(got, want(TEXT, [q], "all", None, [x]))
        assert len(got.term_counts(0)) == 8
    with pytest.raises(lc.LocustError, match="9 terms.*exclusion"):
        eng.run_search(TEXT, [[b"alpha"]], exclude=[t])
    with pytest.raises(lc.LocustError, match="9 terms"):
        eng.run_search(TEXT, [t], exclude=[[b"gamma"]])
    with pytest.raises(lc.LocustError, match="no positive term"):
        eng.run_search(TEXT, [[]], exclude=[[b"gamma"]])
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(TEXT, [[b"alpha"]], exclude=[[b"a b"]])
    with pytest.raises(lc.LocustError, match="empty term"):
        eng.run_search(TEXT, [[b"alpha"]], exclude=[[b""]])
    with pytest.raises(lc.LocustError, match=r"lone \*"):
        eng.run_search(TEXT, [[b"alpha"]], wildcard=True, exclude=[[b"*"]])
    assert eng.run_search(TEXT, [[b"alpha"]], exclude=[[b"*"]]).hits() == [10]  # a literal token
    x = eng.run_index(TEXT)
    with pytest.raises(lc.LocustError, match="no positive term"):
        x.search([[]], exclude=[[b"gamma"]])


@pytest.mark.parametrize("exclude", [[[b"gamma"]], [[b"gamma"]] * 3, [b"gamma", b"beta"],
                                     b"gamma", [b"gamma", None], [[b"gamma"], b"beta"]])
def test_exclude_takes_one_entry_per_query(exclude):
    eng = cpu_engine(TEXT)
    with pytest.raises(ValueError, match="exclude"):
        eng.run_search(TEXT, [[b"alpha"], [b"beta"]], exclude=exclude)
    with pytest.raises(ValueError, match="exclude"):
        lc.search_text(TEXT, [[b"alpha"], [b"beta"]], backend="cpu", exclude=exclude)
    with pytest.raises(ValueError, match="exclude"):
        eng.run_index(TEXT).search([[b"alpha"], [b"beta"]], exclude=exclude)


def test_existing_calls_keep_working():
    eng = cpu_engine(TEXT)
    assert eng.run_search(TEXT, [[b"alpha", b"beta"]], "all", 0, None, False, None).hits() == [5]
    assert lc._C.cpu_run_search(eng.cfg, TEXT, [[b"alpha", b"beta"]], [0]).hits() == [5]
    assert eng.run_index(TEXT)._search([[b"alpha", b"beta"]], [0]).hits() == [5]
    with pytest.raises(lc.LocustError, match="search_resident"):
        eng.search_resident([[b"alpha"]], exclude=[[b"gamma"]])


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_not(cli, hamlet):
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--not", "not")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    ent, post = oracle.index(hamlet)
    lines, _counts = oracle.search(ent, post, [b"to", b"be"], exclude=[b"not"])
    assert len(lines) == 41
    assert result_lines(p.stdout) == oracle.format_search([[b"to", b"be"]], [lines],
                                                          exclude=[[b"not"]])
    # a batch: --not goes to the nearest --search before it, repeats add up, a query without
    # one prints what it printed before; the argument is split like the text
    p = run(cli, "data/hamlet.txt", 1000, 2000, "--backend", "cpu", "--search", "lord, my",
            "--not", "good", "--not", "Ham*, the", "--search", "my lor*", "--search", "Ham*",
            "--not", "Hamlet", "--match", "phrase", "--wildcard", "--check")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"lord", b"my"], [b"my", b"lor*"], [b"Ham*"]]
    exclude = [[b"good", b"Ham*", b"the"], [], [b"Hamlet"]]
    expect = want(oracle.window(hamlet, 1000, 2000), queries, "phrase", None, exclude,
                  first_line=1000, wildcard=True)
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect],
                                                          exclude=exclude)
    assert b"print query: my lor* \t hits: " in p.stdout and expect[2][0]
    # ranked, near
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "be to", "--not", "not",
            "--match", "near", "--within", 3, "--rank", 2)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"print query: be to \t not: not \t hits: 27 \t top:" in p.stdout


def test_cli_without_not_prints_what_it_printed(cli, hamlet):
    """The README's commands: the result lines are the oracle's, which take no ``exclude``
    here, byte for byte."""
    ent, post = oracle.index(hamlet)
    for args, queries, mode, wild in (
            (["--search", "my lord", "--search", "to be"], [[b"my", b"lord"], [b"to", b"be"]],
             "all", False),
            (["--search", "to be", "--match", "phrase"], [[b"to", b"be"]], "phrase", False),
            (["--search", "Ham*", "--wildcard"], [[b"Ham*"]], "all", True)):
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want(hamlet, queries, mode, None, None, wildcard=wild)
        assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
        assert b"not:" not in p.stdout


def test_cli_misuse_is_refused(cli):
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--not", "not", "--search", "to be")
    assert p.returncode != 0 and b"--not" in p.stderr and b"--search" in p.stderr
    assert b"print query" not in p.stdout
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--not", "not")
    assert p.returncode != 0 and b"--not" in p.stderr
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--not")
    assert p.returncode != 0 and b"--not" in p.stderr
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "a b c d e", "--not", "f g",
            "--not", "h i")
    assert p.returncode != 0 and b"9 terms" in p.stderr and b"print query" not in p.stdout
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--not", "*",
            "--wildcard")
    assert p.returncode != 0 and b"lone *" in p.stderr
    # a --not of delimiters only names no word: nothing is excluded
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "to be", "--not", " , ")
    assert p.returncode == 0 and b"print query: to be \t hits: 47 " in p.stdout
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--not \"w1 w2 ...\"" in p.stdout


# ------------------------------------------------------------------------------------
# whole Hamlet: the oracle is authoritative, the counts a cross-check of it
# ------------------------------------------------------------------------------------
# (terms, exclusion terms, mode, W, without, with)
HAMLET = [([b"to", b"be"], [b"not"], "all", None, 47, 41),
          ([b"to", b"be"], [b"not"], "phrase", None, 27, 24),
          ([b"be", b"to"], [b"not"], "near", 3, 31, 27),
          ([b"to", b"be"], [b"not"], "any", None, 737, 680),
          ([b"Ham*"], [b"Hamlet"], "all", None, 464, 371),
          ([b"my", b"lor*"], [b"lord"], "phrase", None, 144, 34)]


def test_cpu_hamlet(hamlet):
    queries = [c[0] for c in HAMLET] * 2
    exclude = [None] * len(HAMLET) + [c[1] for c in HAMLET]
    modes, within = [c[2] for c in HAMLET] * 2, [c[3] for c in HAMLET] * 2
    expect = want(hamlet, queries, modes, within, exclude, wildcard=True)
    assert [len(l) for l, _c in expect] == [c[4] for c in HAMLET] + [c[5] for c in HAMLET]
    eng = cpu_engine(hamlet)
    got = eng.run_search(hamlet, queries, modes, wildcard=True, within=within, exclude=exclude)
    same(got, expect)
    assert got.format() == oracle.format_search(queries, [l for l, _c in expect], exclude=exclude)
    f = lc.search_file(os.path.join(ROOT, "data", "hamlet.txt"), [[b"lord", b"my"]], "all",
                       300, 450, backend="cpu", exclude=[[b"good"]])
    same(f, want(oracle.window(hamlet, 300, 450), [[b"lord", b"my"]], "all", None, [[b"good"]],
                 first_line=300))
    assert f.first_line == 300 and f.lines(0) and all(300 <= l < 450 for l in f.lines(0))
