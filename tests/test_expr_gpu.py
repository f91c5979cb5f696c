"""Boolean expression queries on the device (csrc/kernels/expr.hip: the plan and the hit kernel
behind the lookup of search.hip): ``Engine.run_search(..., mode="expr")`` and ``search_resident``
against the oracle's tree evaluation, exactly, ``merged`` included, and ``walked`` (the greedy
walked set, ``oracle.expr_walked``) on batches made only of ``expr`` queries.  The shapes are the
smallest at which each part can go wrong: the 256-line text that holds every mask of eight words
once, eight queries to a batch and a full batch of 1024; walked lists at the tile (1024) and wave
(64) edges with a second list of the walked set behind them; a word twice on a line; a line in
two walked lists; absent terms under AND, OR and NOT; a query that walks nothing; two prefix
terms over the same words, the second never merged; prefix, pattern and fuzzy terms and the
fold; a line window; ranked with ties; show; batches mixed with the four other modes and their
exclusion terms; a plain batch behind an ``expr`` batch and the other way round; and the issue's
queries over the whole of Hamlet."""
import os

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests import expr_cases as ec
from tests import fuzzy_cases
from tests.show_cases import same_show

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, exprs, k=None, first_line=0, show=None, walked=None, **gkw):
    """run_search, then search_resident, both against the oracle; ``merged`` and ``walked`` too
    (``walked``: what the case expects the oracle's greedy rule to give)."""
    expect = ec.want(text, exprs, k, first_line, **gkw)
    x = ec.merged(text, exprs, first_line, **gkw)
    w = ec.walked(text, exprs, first_line, **gkw)
    assert walked is None or w == walked
    got = engine.run_search(text, exprs, "expr", first_line, rank=k, **gkw)
    ec.same(got, expect, k)
    assert (got.merged, got.walked, got.first_line) == (x, w, first_line)
    again = engine.search_resident(exprs, "expr", rank=k, **gkw)
    ec.same(again, expect, k)
    assert (again.merged, again.walked) == (x, w)
    if show:
        shown = ec.want_show(text, exprs, show, k, first_line, **gkw)
        same_show(engine.search_resident(exprs, "expr", rank=k, show=show, **gkw), shown, show, k,
                  again)
    return again, expect


# ------------------------------------------------------------------------------------
# every mask once
# ------------------------------------------------------------------------------------
EXPRS = [e for e in ec.random_exprs(20260, 200) if not ec.refused(e)]


def test_random_expressions_eight_to_a_batch(eng):
    text = ec.mask_text()
    eng.run_index(text)
    for at in range(0, 48, 8):
        batch = EXPRS[at:at + 8]
        expect = ec.want(text, batch)
        got = eng.search_resident(batch, "expr")
        ec.same(got, expect)
        assert got.walked == ec.walked(text, batch) and got.merged == 0


def test_random_expressions_a_full_batch_ranked_and_shown(eng):
    text = ec.mask_text(2)
    batch = (EXPRS * 10)[:1024]
    expect = ec.want(text, EXPRS)
    expect = (expect * 10)[:1024]
    got = eng.run_search(text, batch, "expr")
    ec.same(got, expect)
    assert got.walked == sum(ec.walked(text, [e]) for e in EXPRS[:1024 % len(EXPRS)]) + \
        (1024 // len(EXPRS)) * ec.walked(text, EXPRS)
    check(eng, text, EXPRS[:24], k=3, show=24)  # ties: the lines of one mask class score alike
    check(eng, text, EXPRS[24:40], show=24)


# ------------------------------------------------------------------------------------
# the walk: tile and wave edges, duplicates, two lists of S
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_walked_list_at_the_tile_and_wave_edges(eng, n):
    """``aa OR bb``: both lists are walked, aa's n elements first and bb's behind them; every
    third aa line holds bb too (emitted once), and bb has lines of its own."""
    lines = [b"aa" + (b" bb" if i % 3 == 0 else b"") for i in range(n)]
    lines += [b"bb cc"] * 70 + [b"cc"]
    text = b"\n".join(lines) + b"\n"
    got, expect = check(eng, text, [b"aa OR bb", b"( aa OR bb ) AND NOT cc", b"aa AND NOT bb"],
                        walked=(n + (n + 2) // 3 + 70) * 2 + n)
    assert expect[0][1] == n + 70 and expect[1][1] == n


def test_adjacent_duplicates_and_a_line_in_two_walked_lists(eng):
    text = b"aa aa aa bb\nbb bb\naa\ncc aa cc aa\nbb aa bb\ndd\n"
    got, expect = check(eng, text, [b"aa OR bb", b"( aa OR bb ) AND NOT cc", b"aa bb OR cc dd",
                                    b"( aa AND NOT bb ) OR ( bb AND NOT aa )"], k=None, show=16)
    assert expect[0][0] == [0, 1, 2, 3, 4] and expect[3][0] == [1, 2, 3]
    check(eng, text, [b"aa OR bb", b"bb OR aa OR cc"], k=2)


def test_absent_terms_and_a_query_that_walks_nothing(eng):
    text = b"to be\nto\nbe not\n"
    got, expect = check(eng, text, [b"to AND nosuch", b"to OR nosuch", b"to AND NOT nosuch",
                                    b"nosuch", b"nosuch OR ( nosuch2 AND to )"])
    assert [a for a, _m, _c in expect] == [[], [0, 1], [0, 1], [], []]
    got, _ = check(eng, text, [b"to AND NOT to", b"nosuch AND NOT be"], walked=0)
    assert got.hits() == [0, 0]
    check(eng, text, [b"to AND NOT to"], k=2, show=8, walked=0)


def test_equal_range_prefix_pair_the_second_never_merged(eng, hamlet):
    """``Haml*`` and ``Hamle*`` cover the same words: two terms, one merged list.  The second
    term's own CSR range is an unsorted concatenation and must never be searched."""
    ent, _post = oracle.index(hamlet)
    words = [k for k, _v, _c in ent if k.startswith(b"Haml")]
    assert len(words) >= 2 and all(k.startswith(b"Hamle") for k in words)
    got, expect = check(eng, hamlet, [b"Haml* AND NOT Hamle*", b"Haml* OR Hamle*",
                                      b"Hamle* AND NOT Haml*", b"( Haml* AND to ) OR ( Hamle* AND be )"],
                        wildcard=True)
    assert [m for _a, m, _c in expect[:2]] == [0, 107]
    assert got.merged == 4 * expect[0][2][0]  # once per query, not once per term


def test_prefix_glob_fuzzy_and_the_fold(eng, hamlet):
    text = oracle.window(hamlet, 0, 900)
    for expr, gkw in [(b"Ham* AND NOT ( Hamlet OR the )", dict(wildcard=True)),
                      (b"( *ing OR h?mlet ) AND NOT the", dict(glob=True)),
                      (b"Hamlet~1 AND NOT ( lord~1 OR my )", dict(fuzzy=True)),
                      (b"( to AND BE ) OR ( QUEEN AND NOT hamlet )", dict(ignore_case=True)),
                      (b"( Ham OR ham ) AND NOT HAM", dict(ignore_case=True)),
                      (b"HAM* AND NOT hamlet~1", dict(ignore_case=True, wildcard=True, fuzzy=True))]:
        _got, expect = check(eng, text, [expr, b"to AND NOT the"], **gkw)
        check(eng, text, [expr], k=4, show=40, **gkw)
        assert expect[0][2][0] > 0, expr


def test_a_line_window(eng, hamlet):
    text = oracle.window(hamlet, 1000, 1400)
    check(eng, text, [b"( to AND be ) OR ( Ham* AND NOT Hamlet )", b"the AND NOT ( to OR a )"],
          first_line=1000, show=30, wildcard=True)
    check(eng, text, [b"my lord OR ( king AND NOT queen )"], k=3, first_line=1000)


# ------------------------------------------------------------------------------------
# routing: mixed batches, and batches of either kind behind one another
# ------------------------------------------------------------------------------------
def test_mixed_batch_every_query_answers_as_alone(eng, hamlet):
    text = oracle.window(hamlet, 0, 1200)
    queries = [[b"to", b"be"], b"to AND be AND NOT not", [b"my", b"lord"], b"Ham* OR ( king AND NOT the )",
               [b"king", b"queen"], [b"my", b"lord"], b"( to OR be ) AND NOT ( to AND be )",
               [b"Ham*", b"lord"]]
    modes = ["all", "expr", "phrase", "expr", "any", "near", "expr", "any"]
    exclude = [[b"not"], None, [b"good"], None, [b"the"], [b"good"], None, [b"Hamlet"]]
    within = [None, None, None, None, None, 3, None, None]
    kw = dict(wildcard=True)
    eng.run_index(text)
    for k in (None, 3):
        got = eng.search_resident(queries, modes, rank=k, within=within, exclude=exclude, **kw)
        for i, (q, m) in enumerate(zip(queries, modes)):
            if m == "expr":
                one = ec.want(text, [q], k, **kw)
            else:
                one = fuzzy_cases.want(text, [q], [m], k, within=[within[i]],
                                       exclude=[exclude[i]], wildcard=True, fuzzy=False)
            alone = eng.search_resident([q], [m], rank=k, within=[within[i]],
                                        exclude=[exclude[i]], **kw)
            ec.same(alone, one, k)
            assert (got.lines(i), got.scores(i), got.term_counts(i), got.matches()[i]) == \
                (alone.lines(0), alone.scores(0), alone.term_counts(0), alone.matches()[0]), i
            assert one[0][1] > 0, i
    shown = eng.search_resident(queries, modes, within=within, exclude=exclude, show=30, **kw)
    for i, (q, m) in enumerate(zip(queries, modes)):
        alone = eng.search_resident([q], [m], within=[within[i]], exclude=[exclude[i]], show=30, **kw)
        assert (shown.text(i), shown.spans(i)) == (alone.text(0), alone.spans(0)), i


def test_plain_batch_behind_an_expr_batch_and_back(eng, hamlet):
    text = oracle.window(hamlet, 0, 800)
    plain = [[b"to", b"be"], [b"my", b"lord"]]
    expect_plain = fuzzy_cases.want(text, plain, ["all", "any"], fuzzy=False)
    exprs = [b"to AND NOT be", b"my OR lord"]
    eng.run_search(text, plain, ["all", "any"])
    for _ in range(2):
        check(eng, text, exprs)
        got = eng.search_resident(plain, ["all", "any"])
        ec.same(got, expect_plain)
        assert got.walked == min(got.term_counts(0)) + sum(got.term_counts(1))


# ------------------------------------------------------------------------------------
# Hamlet, and refusals
# ------------------------------------------------------------------------------------
def test_whole_hamlet(hamlet):
    engine = lc.Engine(gpu_cfg(), len(hamlet), hamlet.count(b"\n") + 1)
    exprs = [b"to AND be AND NOT not", b"( to AND be ) OR ( Ham* AND NOT Hamlet )",
             b"( king OR queen ) AND NOT ( the OR a )", b"( to OR be ) AND NOT ( to AND be )",
             b"to AND NOT the", b"Haml* AND NOT Hamle*", b"Haml* OR Hamle*"]
    got, expect = check(engine, hamlet, exprs, wildcard=True, show=60)
    assert [m for _a, m, _c in expect] == [41, 409, 17, 690, 439, 0, 107]
    assert engine.search_resident([b"to AND NOT the"], "expr").walked == 634
    assert engine.search_resident([exprs[1]], "expr", wildcard=True).walked == 470 + 206
    check(engine, hamlet, exprs, k=5, wildcard=True)
    assert got.format() == ec.formatted(exprs, expect)


def test_every_refusal_starts_nothing_on_the_device(eng):
    text = b"to be\nnot to\n"
    eng.run_search(text, [b"to AND NOT be"], "expr")
    for bad in (b"", b"( to", b"to )", b"()", b"to AND", b"NOT to", b"to OR NOT be",
                b"a b c d e f g h i", b"(" * 65 + b"to" + b")" * 65, b"to,be"):
        with pytest.raises(lc.LocustError):
            eng.run_search(text, [[b"to"], bad], ["all", "expr"])
        with pytest.raises(lc.LocustError):
            eng.search_resident([bad], "expr")
    with pytest.raises(ValueError):
        eng.search_resident([b"to AND be"], "expr", exclude=[[b"not"]])
    with pytest.raises(ValueError):
        eng.search_resident([b"to AND be"], "expr", within=2)
    for kw in (dict(within=[2]), dict(exclude=[[b"not"]])):  # (behind the wrapper: the engine's check)
        with pytest.raises(lc.LocustError, match="write NOT in the expression"):
            eng._eng.search_resident([[b"to AND be"]], [4], None, False, kw.get("within", []),
                                     kw.get("exclude", []), False, False, None, False)
    # the index is still resident: no refused batch had started to write
    got = eng.search_resident([b"to AND NOT be"], "expr")
    assert got.lines(0) == [1] and got.walked == 2
