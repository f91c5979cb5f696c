"""Exclusion terms on the device (csrc/kernels/search.hip: the lookup kernel's exclusion mask,
the hit kernel's drop before the hit / candidate split): ``Engine.run_search`` and then the
same batch through ``Engine.search_resident``, both compared exactly with the oracle
(``oracle.search`` / ``phrase`` / ``near`` / ``rank`` / ``merged_elements`` with
``exclude=``).  The shapes are the smallest at which each part can go wrong: absent and
repeated terms, duplicates at the ends of an exclusion list, exclusion lists shorter and
longer than the driver's, the term budget, merged prefix lists on either side, the verify
kernels' rounds and the candidate list they share, the ranked path, the sort's two regimes
and a full batch."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from exclude_cases import BY_HAND, TEXT, W_MAX, fuzz_case, same, same_ranked, want

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SORT = 8192          # kSmallSortMax: the single-workgroup sort's last size
MAX_QUERIES = 1024         # kSearchMaxQueries
ROUND = 64                 # candidates a wave takes per round, at most


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, queries, modes="all", within=None, exclude=None, first_line=0,
          wildcard=False, expect=None, **okw):
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if expect is None:
        expect = want(text, queries, modes, within, exclude, first_line, wildcard, **okw)
    got = engine.run_search(text, queries, modes, first_line, wildcard=wildcard, within=within,
                            exclude=exclude)
    same(got, expect)
    assert got.first_line == first_line
    # ... and once more from the index and the text the job left on the device
    same(engine.search_resident(queries, modes, wildcard=wildcard, within=within,
                                exclude=exclude), expect)
    return got


def lines_of(got):
    return [got.lines(i) for i in range(got.queries)]


# ------------------------------------------------------------------------------------
# tiny inputs, the rules by hand
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word", b"\n\n", b"word word\n", b"\nword\n\n"])
def test_tiny_inputs(eng, text):
    queries = [[b"word"], [b"word"], [b"word"], [b"gone"], [b"word", b"gone"], [b"word"],
               [b"gone"]]
    exclude = [[b"word"], [b"word"], [b"gone"], [b"word"], [b"word"], None, [b"away"]]
    modes = ["all", "any", "all", "all", "any", "all", "any"]
    got = check(eng, text, queries, modes, None, exclude)
    n = [b"", b"word", b"\n\n", b"word word\n", b"\nword\n\n"].index(text)
    word = [[], [0], [], [0], [1]][n]
    # the exclusion is the only positive term: nothing; an absent exclusion term: nothing
    # is removed and nothing goes dead; an absent positive term: nothing, whatever is excluded
    assert lines_of(got) == [[], [], word, [], [], word, []]
    assert got.format() == oracle.format_search(queries, lines_of(got), exclude=exclude)


@pytest.mark.parametrize("wild", [False, True])
def test_by_hand(eng, wild):
    cs = [c for c in BY_HAND if c[4] == wild]
    queries, exclude = [c[0] for c in cs], [c[1] for c in cs]
    modes, within = [c[2] for c in cs], [c[3] for c in cs]
    got = check(eng, TEXT, queries, modes, within, exclude, wildcard=wild)
    assert lines_of(got) == [c[5] for c in cs]
    got = check(eng, TEXT + b"\n", queries, modes, within, exclude, first_line=10, wildcard=wild)
    assert lines_of(got) == [[10 + l for l in c[5]] for c in cs]


def test_duplicates_at_the_ends_of_an_exclusion_list(eng):
    """A line that holds the exclusion word two or three times: adjacent duplicates in its
    list, in the middle, as its first and as its last elements."""
    text = (b"x a x\n"        # 0: x's list begins 0, 0
            b"a\n"
            b"a x b x x\n"    # 2: 2, 2, 2 in the middle
            b"a b\n"
            b"b x\n"
            b"a\n"
            b"x x b a x")     # 6: ... and ends 6, 6, 6; no newline
    queries = [[b"a"], [b"a", b"b"], [b"a", b"b"], [b"b", b"a"], [b"a"], [b"x"]]
    exclude = [[b"x"], [b"x"], [b"x"], [b"x"], [b"x", b"b"], [b"x"]]
    got = check(eng, text, queries, ["all", "all", "any", "near", "phrase", "any"],
                [None, None, None, 2, None, None], exclude)
    assert lines_of(got) == [[1, 3, 5], [3], [1, 3, 5], [3], [1, 5], []]
    assert got.term_counts(0) == [6, 9]


# ------------------------------------------------------------------------------------
# the driver, the bound, the term budget
# ------------------------------------------------------------------------------------
def driver_text():
    """p and q on 60 lines each, 40 of them shared; r on 3 lines, s on 1, z on 300."""
    lines = []
    for i in range(320):
        w = []
        if i < 60:
            w.append(b"p")
        if 20 <= i < 80:
            w.append(b"q")
        if i in (25, 45, 70):
            w.append(b"r")
        if i == 30:
            w.append(b"s")
        if i % 16 != 3:
            w.append(b"z")
        lines.append(b" ".join(w))
    return b"\n".join(lines) + b"\n"


def test_driver_choice(eng):
    """The exclusion list is shorter than every positive list, longer than all of them, or
    one element: it is never the driver and adds nothing to the bound."""
    text = driver_text()
    pq = [b"p", b"q"]
    queries = [pq, pq, pq, pq, pq, [b"r"], [b"s"], [b"z"], pq]
    exclude = [[b"r"], [b"z"], [b"s"], [b"s", b"r", b"z"], None, [b"z"], [b"z"], [b"s"], [b"r"]]
    modes = ["all"] * 8 + ["any"]
    got = check(eng, text, queries, modes, None, exclude)
    assert got.term_counts(0) == [60, 60, 3] and got.term_counts(1) == [60, 60, 300]
    assert got.hits() == [38, 2, 39, 2, 40, 0, 0, 299, 77]
    assert got.lines(1) == [35, 51] and 30 not in got.lines(2) and 30 in got.lines(0)
    check(eng, text, queries[:4], ["phrase", "near", "near", "phrase"], [None, 2, 20, None],
          exclude[:4])


def test_term_budget(eng):
    t = [b"t%d" % i for i in range(8)]
    text = b"\n".join([b" ".join(t), b" ".join(t[:7]), b"t0 x1", b"t0 x2 x7", b"t0"] * 3) + b"\n"
    x = [b"x%d" % i for i in range(1, 8)]
    queries = [[b"t0"], t[:7], t, [b"t0"], t[:7]]
    exclude = [x, [b"t7"], None, t[1:], [b"x1"]]
    got = check(eng, text, queries, "all", None, exclude)
    assert got.hits() == [9, 3, 3, 9, 6] and all(len(got.term_counts(i)) == 8 for i in range(5))
    check(eng, text, queries, ["any", "phrase", "phrase", "near", "near"],
          [None, None, None, 1, 7], exclude)
    # refused before anything runs: the index stays resident
    for q, xs, msg in (([b"t0"], t, "9 terms"), (t, [b"x1"], "9 terms"),
                       ([], [b"x1"], "no positive term")):
        with pytest.raises(lc.LocustError, match=msg):
            eng.run_search(text, [q], exclude=[xs])
        with pytest.raises(lc.LocustError, match=msg):
            eng.search_resident([q], exclude=[xs])
    same(eng.search_resident(queries, exclude=exclude), want(text, queries, "all", None, exclude))


def test_repeated_terms(eng):
    """Repeated exclusion terms, and an exclusion term that repeats a positive term: its
    list is the positive term's own slot."""
    text = (TEXT + b"\n") * 20
    ab, x = [b"alpha", b"beta"], [b"gamma", b"gamma", b"x", b"gamma", b"x"]
    queries = [ab, ab, ab, ab, ab, ab, [b"alpha"], [b"beta", b"alpha", b"beta"]]
    exclude = [x, [b"alpha"], [b"beta", b"beta"], [b"beta"], [b"beta", b"gamma"], [b"alpha"],
               [b"alpha"], [b"beta"]]
    modes = ["all", "all", "any", "phrase", "near", "any", "any", "any"]
    got = check(eng, text, queries, modes, [None] * 4 + [2] + [None] * 3, exclude)
    assert got.hits() == [40, 0, 100, 0, 0, 0, 0, 100]
    assert got.term_counts(0) == [200, 100, 140, 140, 40, 140, 40]


# ------------------------------------------------------------------------------------
# prefix terms on either side
# ------------------------------------------------------------------------------------
def test_prefix_exclusions(eng):
    text = (TEXT + b"\n") * 30
    ent, _post = oracle.index(text)
    queries = [[b"alpha"], [b"alpha"], [b"alpha"], [b"abc"], [b"ab*"], [b"ab*"], [b"alpha"],
               [b"ab*", b"alpha"], [b"alpha", b"b*"], [b"Ham*"], [b"alpha"], [b"a*"]]
    exclude = [[b"zz*"], [b"gam*"], [b"ab*"], [b"ab*"], [b"abc"], [b"ab*"], [b"ab*", b"ab*"],
               [b"ab*"], [b"g*", b"ab"], [b"Hamlet"], [b"Ham*", b"ab*", b"g*"], [b"al*"]]
    modes = ["all"] * 5 + ["any", "all", "any", "all", "all", "all", "any"]
    got = check(eng, text, queries, modes, None, exclude, wildcard=True)
    # 0, 1 and 3 words; the range that holds the positive word; `ab* not abc`
    assert got.hits()[:5] == [300, 240, 240, 0, 30] and got.hits()[5] == 0
    assert got.merged == oracle.merged_elements(ent, queries, exclude=exclude) > 0
    assert got.term_counts(2) == [300, 150] and got.term_counts(9) == [120, 60]
    # the same prefix list as a positive term of one query and an exclusion term of another
    got = check(eng, text, [[b"ab*"], [b"alpha"], [b"ab*", b"alpha"]], ["all", "all", "phrase"],
                None, [None, [b"ab*"], [b"ab*"]], wildcard=True)
    assert got.hits() == [90, 240, 0]
    assert got.merged == oracle.merged_elements(
        ent, [[b"ab*"], [b"alpha"], [b"ab*", b"alpha"]], exclude=[None, [b"ab*"], [b"ab*"]]) == 450
    # an exclusion range of one word merges nothing
    got = check(eng, text, [[b"alpha"]], "all", None, [[b"gam*", b"zz*"]], wildcard=True)
    assert got.merged == 0 and got.hits() == [240]


# ------------------------------------------------------------------------------------
# phrase and near: the verify kernels see the positive terms only
# ------------------------------------------------------------------------------------
def test_phrase_and_near(eng):
    text = (TEXT + b"\n") * 3
    ab = [b"alpha", b"beta"]
    queries = [ab, ab, [b"bye", b"bye"], [b"bye", b"bye"], ab, ab, [b"bye", b"bye"],
               [b"beta", b"alpha"], [b"Ham*", b"alpha"]]
    exclude = [[b"gamma"], None, [b"x"], None, [b"gamma"], [b"gamma"], [b"x"], [b"delta", b"ab"],
               [b"Hamlet"]]
    modes = ["phrase", "phrase", "phrase", "phrase", "near", "near", "near", "near", "phrase"]
    within = [None] * 4 + [20, W_MAX, 1, 2, None]  # W at the emit cap: `all`, nothing verified
    got = check(eng, text, queries, modes, within, exclude, wildcard=True)
    assert got.lines(0)[:2] == [0, 10] and got.lines(1)[:3] == [0, 1, 10]
    assert got.lines(2)[:2] == [6, 22] and got.lines(4) == got.lines(5)
    assert got.lines(6) == got.lines(2) and got.lines(7)[:2] == [1, 2]
    assert got.lines(8) == [13, 29, 45]
    short = lc.Engine(gpu_cfg(emits_per_line=3), 1 << 16, 1 << 10)
    # the third token is the last one in the index: a gamma behind it excludes nothing
    text = b"alpha beta x gamma\nalpha beta gamma\nx alpha beta\n"
    got = check(short, text, [ab] * 3, ["phrase", "near", "all"], [None, 2, None],
                [[b"gamma"]] * 3, emits=3)
    assert lines_of(got) == [[0, 2], [0, 2], [0, 2]]


def rounds_text():
    """130 candidate lines of [v w], every other one with an x, between lines that hold one
    of the words only; 70 lines on which w v stand the other way round, y on some."""
    lines = []
    for i in range(130):
        lines.append(b"v w x" if i % 2 else b"pad v, w")
        lines.append(b"v pad" if i % 3 else b"w")
    for i in range(70):
        lines.append(b"w v y" if i % 5 == 0 else b"w v")
    return b"\n".join(lines) + b"\n"


def test_candidates_per_round(eng):
    """Rounds of 64 candidates: 130 lines pass the `all` test, every other one is excluded
    before it becomes a candidate, 65 are verified; a near query fills the candidate list
    from its other end."""
    text = rounds_text()
    assert 65 == ROUND + 1
    queries = [[b"v", b"w"], [b"w", b"v"], [b"v", b"w"], [b"w", b"v"]]
    exclude = [[b"x"], [b"y"], None, [b"x", b"y"]]
    got = check(eng, text, queries, ["phrase", "near", "phrase", "near"], [None, 2, None, 2],
                exclude)
    assert got.hits() == [65, 130 + 56, 130, 65 + 56]
    got = check(eng, text, queries[:2], ["phrase", "near"], [None, 2], exclude[:2])
    assert got.hits() == [65, 186]


# ------------------------------------------------------------------------------------
# ranked
# ------------------------------------------------------------------------------------
def test_ranked(eng):
    text = (TEXT + b"\n") * 5
    queries = [[b"alpha", b"beta"], [b"alpha", b"beta"], [b"Ham*"], [b"Ham*", b"Hamlet"],
               [b"gamma", b"alpha"], [b"gamma", b"alpha"], [b"alpha", b"gone"]]
    exclude = [[b"gamma"], [b"delta", b"x"], [b"Hamlet"], [b"alpha"], [b"gamma"], None,
               [b"gone", b"beta"]]
    modes = ["any", "phrase", "all", "any", "any", "any", "any"]
    expect = want(text, queries, modes, None, exclude, wildcard=True)
    assert [len(l) for l, _c in expect] == [40, 10, 5, 5, 40, 60, 25]
    for k in (1, 3, 99):  # 99: more than the matches
        got = eng.run_search(text, queries, modes, rank=k, wildcard=True, exclude=exclude)
        same_ranked(got, text, queries, exclude, expect, k, wildcard=True)
        same_ranked(eng.search_resident(queries, modes, rank=k, wildcard=True, exclude=exclude),
                    text, queries, exclude, expect, k, wildcard=True)
    # the best line of `gamma alpha` holds gamma three times: excluded, it does not come back
    assert got.lines(5)[0] == 15 and got.lines(5)[0] not in got.lines(4)
    assert not {15, 31, 47, 63, 79} & set(got.lines(4)) and got.matches()[4] == 40
    # Ham* keeps its full weight beside `not Hamlet`: the surviving line's score is the one
    # it has without the exclusion
    a = eng.search_resident([[b"Ham*"]] * 2, rank=99, wildcard=True, exclude=[None, [b"Hamlet"]])
    assert a.lines(1) == [13, 29, 45, 61, 77] and a.matches() == [15, 5]
    assert a.scores(1) == [a.scores(0)[a.lines(0).index(l)] for l in a.lines(1)]
    assert a.format() == oracle.format_ranked(
        [[b"Ham*"]] * 2, [list(zip(a.lines(i), a.scores(i))) for i in range(2)], a.matches(),
        exclude=[None, [b"Hamlet"]])


# ------------------------------------------------------------------------------------
# the sort's two regimes, a full batch, fuzz
# ------------------------------------------------------------------------------------
def test_sort_regimes():
    """About 20,000 short lines; the surviving hits of a batch are just under, exactly and
    just over what the single-workgroup sort takes."""
    n = 20000
    lines = [b"v" if i < SMALL_SORT else b"v y" if i == SMALL_SORT else b"v x" for i in range(n)]
    lines[100] = b"v u"
    text = b"\n".join(lines) + b"\n"
    engine = lc.Engine(gpu_cfg(), len(text), n + 1)
    got = check(engine, text, [[b"v"]], "all", None, [[b"x", b"y", b"u"]])
    assert got.hits() == [SMALL_SORT - 1]
    got = check(engine, text, [[b"v"]], "all", None, [[b"y", b"x"]])
    assert got.hits() == [SMALL_SORT]
    got = check(engine, text, [[b"v"], [b"y"], [b"v"]], ["all", "any", "any"], None,
                [[b"x"], None, [b"v"]])
    assert got.hits() == [SMALL_SORT + 1, 1, 0]
    r = engine.search_resident([[b"v"], [b"v"]], rank=2, exclude=[[b"x"], [b"x", b"y", b"u"]])
    assert r.matches() == [SMALL_SORT + 1, SMALL_SORT - 1] and r.lines(1) == [0, 1]


def test_full_batch(eng):
    text, queries, modes, within, exclude = fuzz_case(11, nlines=200, nqueries=MAX_QUERIES)
    assert {"all", "any", "phrase", "near"} == set(modes)
    assert 300 < sum(1 for x in exclude if not x) and 500 < sum(1 for x in exclude if x)
    got = check(eng, text, queries, modes, within, exclude, first_line=7)
    assert got.queries == MAX_QUERIES and sum(1 for h in got.hits() if h) > 300


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(eng, seed):
    for wild in (False, True):
        text, queries, modes, within, exclude = fuzz_case(seed, wildcard=wild)
        expect = want(text, queries, modes, within, exclude, first_line=5, wildcard=wild)
        got = check(eng, text, queries, modes, within, exclude, first_line=5, wildcard=wild,
                    expect=expect)
        assert (got.merged > 0) == wild
        if wild:
            ent, _post = oracle.index(text, first_line=5)
            assert got.merged == oracle.merged_elements(ent, queries, exclude=exclude)
        r = eng.search_resident(queries, modes, rank=3, wildcard=wild, within=within,
                                exclude=exclude)
        same_ranked(r, text, queries, exclude, expect, 3, first_line=5, wildcard=wild)


# ------------------------------------------------------------------------------------
# whole Hamlet, the CLI
# ------------------------------------------------------------------------------------
# (terms, exclusion terms, mode, W, without, with)
HAMLET = [([b"to", b"be"], [b"not"], "all", None, 47, 41),
          ([b"to", b"be"], [b"not"], "phrase", None, 27, 24),
          ([b"be", b"to"], [b"not"], "near", 3, 31, 27),
          ([b"to", b"be"], [b"not"], "any", None, 737, 680),
          ([b"Ham*"], [b"Hamlet"], "all", None, 464, 371),
          ([b"my", b"lor*"], [b"lord"], "phrase", None, 144, 34)]


def test_whole_hamlet(hamlet):
    engine = lc.Engine(gpu_cfg(), len(hamlet), len(oracle.split_lines(hamlet)) + 1)
    queries = [c[0] for c in HAMLET] * 2
    exclude = [None] * len(HAMLET) + [c[1] for c in HAMLET]
    modes, within = [c[2] for c in HAMLET] * 2, [c[3] for c in HAMLET] * 2
    got = check(engine, hamlet, queries, modes, within, exclude, wildcard=True)
    assert got.hits() == [c[4] for c in HAMLET] + [c[5] for c in HAMLET]
    assert got.format() == oracle.format_search(queries, lines_of(got), exclude=exclude)
    r = engine.search_resident(queries[6:], modes[6:], rank=10, wildcard=True, within=within[6:],
                               exclude=exclude[6:])
    assert r.matches() == [c[5] for c in HAMLET]


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_not(cli, hamlet):
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "to be", "--not", "not", "--search",
                        "Ham*", "--not", "Hamlet", "--search", "my lord", "--wildcard", "--check"],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries, exclude = [[b"to", b"be"], [b"Ham*"], [b"my", b"lord"]], [[b"not"], [b"Hamlet"], []]
    expect = want(hamlet, queries, "all", None, exclude, wildcard=True)
    assert [len(l) for l, _c in expect][:2] == [41, 371]
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect],
                                                          exclude=exclude)
