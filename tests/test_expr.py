"""Boolean expression queries (``mode="expr"``: ``( to AND be ) OR ( Ham* AND NOT Hamlet )``)
without a GPU: how an expression is read and refused (``make_search_expr``, Python, the CLI),
precedence, the implicit AND and glued parentheses, the term identification and the truth table,
the host evaluation and the CPU engine against the oracle's tree evaluation on the 256-line text
that holds every mask of eight words once -- unranked, in a line window, ranked and with
``show`` -- the agreement with ``all``, ``any`` and ``exclude``, the issue's counts over the whole
of Hamlet, and the CLI's output bytes.  Every comparison is exact; ``check=True`` runs
``validate_search`` on every result."""
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd._native import load
from locust_amd.utils import oracle
from tests import expr_cases as ec
from tests.show_cases import same_show

_C = load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def parsed(expr, **kw):
    return _C.make_search_expr(lc.make_config("cpu"), expr, **kw)


def truth_bit(q, mask):
    return q["truth"][mask >> 5] >> (mask & 31) & 1


# ------------------------------------------------------------------------------------
# reading an expression
# ------------------------------------------------------------------------------------
REFUSALS = [
    (b"", "empty expression"),
    (b" \t ", "empty expression"),
    (b"( to AND be", "unbalanced"),
    (b"to AND be )", "unbalanced"),
    (b"( to AND ( be OR not )", "unbalanced"),
    (b"()", "holds no operand"),
    (b"to AND ( )", "holds no operand"),
    (b"to AND", "dangling"),
    (b"OR be", "dangling"),
    (b"to AND OR be", "dangling"),
    (b"NOT", "dangling"),
    (b"to OR NOT", "dangling"),
    (b"( to AND ) be", "dangling"),
    (b"a b c d e f g h i", "more than 8 distinct terms"),
    (b"(" * (_C.kExprMaxDepth + 1) + b"a" + b")" * (_C.kExprMaxDepth + 1), "deeper than"),
    (b"(" * 100000 + b"a", "deeper than"),  # (deep input: refused, the stack is not run down)
    (b"NOT a", "none of its words"),
    (b"a OR NOT b", "none of its words"),
    (b"NOT ( a AND b )", "none of its words"),
    (b"to,be", "delimiter"),
    (b"to AND be\nnot", "newline"),
    (b"to AND b\0e", "NUL"),
]


@pytest.mark.parametrize("expr, msg", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refused_by_make_search_expr_python_and_the_oracle(expr, msg):
    with pytest.raises(lc.LocustError, match=msg):
        parsed(expr)
    text = b"to be a b\nnot\n"
    eng = cpu_engine(text)
    with pytest.raises(lc.LocustError, match=msg):
        eng.run_search(text, [expr], "expr")
    with pytest.raises(lc.LocustError, match=msg):
        eng.run_index(text).search([[expr]], "expr")
    with pytest.raises(lc.LocustError, match=msg):
        lc.search_text(text, [[b"to"], expr], ["all", "expr"], backend="cpu")
    assert ec.refused(expr)


def test_refused_term_readings_and_query_shapes():
    with pytest.raises(lc.LocustError, match="1 or 2"):
        parsed(b"to AND ham~3", fuzzy=True)
    with pytest.raises(lc.LocustError, match="lone \\*"):
        parsed(b"to AND *", wildcard=True)
    with pytest.raises(lc.LocustError, match="stars alone"):
        parsed(b"to AND **", glob=True)
    text = b"to be\n"
    eng = cpu_engine(text)
    for call in (lambda **kw: eng.run_search(text, [b"to AND be"], "expr", **kw),
                 lambda **kw: eng.run_index(text).search([b"to AND be"], "expr", **kw)):
        with pytest.raises(ValueError, match="NOT"):
            call(exclude=[[b"be"]])
        with pytest.raises(ValueError, match="near"):
            call(within=3)
        with pytest.raises(ValueError, match="near"):
            call(within=[3])
    # behind the wrapper the engines refuse the same: check_search_queries, before anything runs
    cfg = lc.make_config("cpu", check=True)
    for kw in (dict(within=[3]), dict(exclude=[[b"be"]]), dict(exclude=[[b"b%d" % i for i in range(8)]])):
        with pytest.raises(lc.LocustError, match="write NOT in the expression"):
            _C.cpu_run_search(cfg, text, [[b"to AND be"]], [4], **kw)
        with pytest.raises(lc.LocustError, match="write NOT in the expression"):
            eng.run_index(text)._search([[b"to AND be"]], [4], None, False, kw.get("within", []),
                                        kw.get("exclude", []), False, False, None, False)
    with pytest.raises(ValueError, match="one expression"):
        eng.run_search(text, [[b"to", b"be"]], "expr")
    with pytest.raises(ValueError, match="'expr'"):
        eng.run_search(text, [[b"to"]], "tree")
    # the depth the rule promises is accepted, glued or spaced
    n = _C.kExprMaxDepth
    assert n >= 32
    q = parsed(b"(" * n + b"to" + b")" * n + b" AND " + b"( " * n + b"be" + b" )" * n)
    assert q["terms"] == [b"to", b"be"]


def test_precedence_association_and_the_implicit_and():
    # NOT > AND > OR: a OR b AND NOT c  ==  a OR ( b AND ( NOT c ) )
    q = parsed(b"a OR b AND NOT c")
    assert q["terms"] == [b"a", b"b", b"c"]
    for m in range(8):
        a, b, c = m & 1, m >> 1 & 1, m >> 2 & 1
        assert truth_bit(q, m) == (a or (b and not c)), m
    # side by side is AND, and binds as AND does
    assert parsed(b"a b OR c")["truth"] == parsed(b"( a AND b ) OR c")["truth"]
    assert parsed(b"a OR b c")["truth"] == parsed(b"a OR ( b AND c )")["truth"]
    assert parsed(b"a NOT b")["truth"] == parsed(b"a AND NOT b")["truth"]
    assert parsed(b"a ( b OR c )")["truth"] == parsed(b"a AND ( b OR c )")["truth"]
    # NOT NOT folds; NOT applies to the nearest operand only
    assert parsed(b"a AND NOT NOT b")["truth"] == parsed(b"a AND b")["truth"]
    assert parsed(b"a AND NOT b OR c")["truth"] == parsed(b"( a AND ( NOT b ) ) OR c")["truth"]
    # left association changes nothing for AND and OR, but the terms keep their first-seen order
    assert parsed(b"c OR a OR b")["terms"] == [b"c", b"a", b"b"]
    # the bits above the query's terms repeat the table: no term beyond them is ever set
    q = parsed(b"a")
    assert q["truth"] == [0xAAAAAAAA] * 8


def test_words_parentheses_and_repeated_operands():
    # lower-case and, or, not are words
    q = parsed(b"to and be or not")
    assert q["terms"] == [b"to", b"and", b"be", b"or", b"not"]
    q = parsed(b"to AND and")
    assert q["terms"] == [b"to", b"and"]
    # parentheses are tokens wherever they stand; the text keeps them as asked
    q = parsed(b"(to AND be)OR(not)")
    assert q["terms"] == [b"to", b"be", b"not"] and q["expr"] == b"(to AND be)OR(not)"
    assert q["truth"] == parsed(b"( to AND be ) OR ( not )")["truth"]
    assert parsed(b"  ( to \t AND   be )  ")["expr"] == b"( to AND be )"
    # repeated operands are one term; kind and bytes make the term
    q = parsed(b"( to AND be ) OR ( to AND not ) OR be")
    assert q["terms"] == [b"to", b"be", b"not"] and q["excluded"] == 0
    q = parsed(b"ham* OR ham OR ham* OR h?m OR ham~1 OR ham~2", glob=True, fuzzy=True)
    assert q["terms"] == [b"ham", b"ham", b"h?m", b"ham", b"ham"]
    assert q["kinds"] == ["prefix", "plain", "pattern", "fuzzy", "fuzzy"]
    assert parsed(b"ham* OR ham*")["kinds"] == ["plain"]  # (no wildcard: the star is literal)
    # eight distinct terms fit, each as often as asked; nine do not
    q = parsed(b"a b c d e f g h a b c d e f g h")
    assert len(q["terms"]) == 8
    with pytest.raises(lc.LocustError, match="more than 8"):
        parsed(b"a b c d e f g h OR i")


# ------------------------------------------------------------------------------------
# the 256-line text: every mask once
# ------------------------------------------------------------------------------------
EXPRS = ec.random_exprs(20260, 200)


def split_refused(exprs, **gkw):
    ok = [e for e in exprs if not ec.refused(e, **gkw)]
    bad = [e for e in exprs if ec.refused(e, **gkw)]
    return ok, bad


def test_random_expressions_the_refused_ones():
    ok, bad = split_refused(EXPRS)
    assert len(ok) >= 60 and len(bad) >= 30, (len(ok), len(bad))
    for e in bad:  # syntactically sound: only truth[0] refuses them
        with pytest.raises(lc.LocustError, match="none of its words"):
            parsed(e)
    for e in ok:
        q = parsed(e)
        tree, terms = oracle.expr_parse(e)
        assert q["terms"] == terms and q["expr"] == oracle.expr_text(e)
        for m in range(1 << len(terms)):  # the table against the tree
            have = {t for t in range(len(terms)) if m >> t & 1}
            assert truth_bit(q, m) == oracle.expr_holds(tree, have), (e, m)


@pytest.mark.parametrize("first_line, repeat", [(0, 1), (1000, 2)])
def test_random_expressions_host_engine_against_the_oracle(first_line, repeat):
    text = ec.mask_text(repeat)
    ok, _bad = split_refused(EXPRS)
    expect = ec.want(text, ok, first_line=first_line)
    assert sum(m for _a, m, _c in expect) > 1000
    eng = cpu_engine(text)
    got = eng.run_search(text, ok, "expr", first_line)
    ec.same(got, expect)
    assert got.merged == 0 and got.walked == 0  # a host evaluation walks nothing on a device
    assert got.format() == ec.formatted(ok, expect)
    ec.same(eng.run_index(text, first_line).search(ok, "expr"), expect)


def test_random_expressions_ranked():
    text = ec.mask_text(2)
    ok, _bad = split_refused(EXPRS)
    eng = cpu_engine(text)
    for k in (3, 1000):
        expect = ec.want(text, ok, k)
        got = eng.run_search(text, ok, "expr", rank=k)
        ec.same(got, expect, k)
        assert got.format() == ec.formatted(ok, expect, k)
        ec.same(eng.run_index(text).search(ok, "expr", rank=k), expect, k)


def test_random_expressions_with_show():
    text = ec.mask_text(2)
    ok, _bad = split_refused(EXPRS)
    eng = cpu_engine(text)
    for k in (None, 3):
        shown = ec.want_show(text, ok, 24, k)
        got = eng.run_search(text, ok, "expr", rank=k, show=24)
        same_show(got, shown, 24, k, eng.run_search(text, ok, "expr", rank=k))
        assert got.format(mark=True) == ec.formatted_show(ok, shown, k, mark=True)
    assert any(s for _t, spans, _c in shown[1] for s in spans)


# ------------------------------------------------------------------------------------
# agreement with the other modes, and Hamlet
# ------------------------------------------------------------------------------------
def test_agreement_with_all_any_and_exclude(hamlet):
    eng = cpu_engine(hamlet)
    got = eng.run_search(hamlet, [b"to be", [b"to", b"be"], b"to OR be", [b"to", b"be"],
                                  b"to AND be AND NOT not", [b"to", b"be"]],
                         ["expr", "all", "expr", "any", "expr", "all"],
                         exclude=[None, None, None, None, None, [b"not"]])
    for i in (0, 2, 4):
        assert got.lines(i) == got.lines(i + 1) and got.lines(i), i
    assert got.term_counts(4) == got.term_counts(5)
    ranked = eng.run_search(hamlet, [b"to OR be", [b"to", b"be"]], ["expr", "any"], rank=7)
    assert ranked.lines(0) == ranked.lines(1) and ranked.scores(0) == ranked.scores(1)


HAMLET_COUNTS = [
    (b"to AND be AND NOT not", {}, 41),
    (b"( to AND be ) OR ( Ham* AND NOT Hamlet )", {"wildcard": True}, 409),
    (b"( king OR queen ) AND NOT ( the OR a )", {}, 17),
    (b"( to OR be ) AND NOT ( to AND be )", {}, 690),
    (b"to AND NOT the", {}, 439),
    (b"Haml* AND NOT Hamle*", {"wildcard": True}, 0),
    (b"Haml* OR Hamle*", {"wildcard": True}, 107),  # (both terms cover the same words)
]


@pytest.mark.parametrize("expr, gkw, count", HAMLET_COUNTS, ids=[str(c) for _e, _g, c in HAMLET_COUNTS])
def test_whole_hamlet(hamlet, expr, gkw, count):
    expect = ec.want(hamlet, [expr], **gkw)
    assert expect[0][1] == count
    got = cpu_engine(hamlet).run_search(hamlet, [expr], "expr", **gkw)
    ec.same(got, expect)
    assert got.format() == ec.formatted([expr], expect)


def test_hamlet_walked_sets_by_the_oracle(hamlet):
    ent, post = oracle.index(hamlet)
    assert oracle.expr_walked(ent, post, b"to AND NOT the") == 634
    assert oracle.expr_walked(ent, post, b"( to AND be ) OR ( Ham* AND NOT Hamlet )",
                              wildcard=True) == 470 + 206
    assert oracle.expr_walked(ent, post, b"to AND NOT to") == 0
    assert oracle.expr_walked(ent, post, b"nosuchword AND to") == 0


def test_glob_fuzzy_and_ignore_case_terms(hamlet):
    text = oracle.window(hamlet, 0, 600)
    eng = cpu_engine(text)
    for expr, gkw in [(b"( *ing OR h?mlet ) AND NOT the", dict(glob=True)),
                      (b"Hamlet~1 AND NOT ( lord~1 OR my )", dict(fuzzy=True)),
                      (b"( to AND BE ) OR ( QUEEN AND NOT hamlet )", dict(ignore_case=True)),
                      (b"HAM* AND NOT hamlet", dict(ignore_case=True, wildcard=True))]:
        expect = ec.want(text, [expr], **gkw)
        assert expect[0][1] > 0, expr
        got = eng.run_search(text, [expr], "expr", **gkw)
        ec.same(got, expect)
        ec.same(eng.run_index(text).search([expr], "expr", rank=5, **gkw),
                ec.want(text, [expr], 5, **gkw), 5)


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_expr(cli, hamlet, tmp_path):
    exprs = [b"( to AND be ) OR ( Ham* AND NOT Hamlet )", b"(king OR queen)  AND NOT (the OR a)",
             b"to be", b"nosuchword OR ( to AND NOT to )"]
    args = [x for e in exprs for x in ("--search", e.decode())]
    base = ["data/hamlet.txt", "--backend", "cpu", *args, "--match", "expr", "--wildcard", "--check"]
    p = run(cli, *base)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    expect = ec.want(hamlet, exprs, wildcard=True)
    assert [expect[i][1] for i in (0, 1, 3)] == [409, 17, 0] and expect[2][1] > 0
    assert result_lines(p.stdout) == ec.formatted(exprs, expect)
    p = run(cli, *base, "--rank", 4)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == ec.formatted(exprs, ec.want(hamlet, exprs, 4, wildcard=True), 4)
    p = run(cli, *base, "--rank", 3, "--show", 80, "--mark")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    shown = ec.want_show(hamlet, exprs, 80, 3, wildcard=True)
    want_out = ec.formatted_show(exprs, shown, 3, mark=True)
    assert want_out in p.stdout and b">>Ham" in want_out
    p = run(cli, *base, "--json", tmp_path / "job.json")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    record = json.loads((tmp_path / "job.json").read_text().splitlines()[-1])
    assert record["walked"] == 0 and record["merged"] == 0  # (a host evaluation)


@pytest.mark.parametrize("args, msg", [
    (["--search", "NOT to", "--match", "expr"], "none of its words"),
    (["--search", "to OR NOT be", "--match", "expr"], "none of its words"),
    (["--search", "(" * (_C.kExprMaxDepth + 1) + "to" + ")" * (_C.kExprMaxDepth + 1),
      "--match", "expr"], "deeper than"),
    (["--search", "(" * 100000 + "to", "--match", "expr"], "deeper than"),
    (["--search", "( to AND be", "--match", "expr"], "unbalanced"),
    (["--search", "()", "--match", "expr"], "holds no operand"),
    (["--search", "to AND", "--match", "expr"], "dangling"),
    (["--search", "", "--match", "expr"], "empty expression"),
    (["--search", "a b c d e f g h i", "--match", "expr"], "more than 8"),
    (["--search", "to,be AND not", "--match", "expr"], "delimiter"),
    (["--search", "to AND be", "--not", "not", "--match", "expr"], "--not"),
    (["--search", "to AND be", "--within", 3, "--match", "expr"], "--within"),
    (["--search", "to AND be", "--match", "tree"], "--match"),
])
def test_cli_expr_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_mode(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"expr" in p.stdout and b"AND NOT Hamlet" in p.stdout
