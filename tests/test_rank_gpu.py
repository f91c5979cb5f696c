"""Ranked search on the device (the score and top kernels of csrc/kernels/search.hip):
``Engine.run_search(..., rank=K)`` and ``Engine.search_resident(..., rank=K)`` against
``oracle.rank`` over ``oracle.search`` / ``oracle.phrase``.  Scores are exact integers and the
order (score descending, line ascending) is total, so every comparison is exact.  The shapes
are the smallest at which each part can go wrong: the wave (64), the score kernel's step
(256) and tile (1024) for a tf whose postings straddle them, words adjacent in key order for
a tf count that leaves its CSR range, N // c on either side of a power of two for the weight,
more equal scores than K for the cut, empty segments between full ones, a score past the
8- and 12-bit boundaries of the score field, the sort's two regimes and the last line window."""
import functools
import json
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SORT = 8192    # kSmallSortMax: the single-workgroup sort's last size
SCORE_BLOCK = 256    # kSearchBlock: pairs per step of a score workgroup
SCORE_TILE = 1024    # kSearchTile: pairs per score workgroup and grid stride
MAX_QUERIES = 1024   # kSearchMaxQueries
RANK_MAX_EMITS = 65536


def test_mirrored_constants():
    assert lc._C.kSearchMaxQueries == MAX_QUERIES and lc._C.kSearchMaxTerms == 8
    assert lc._C.kRankMaxEmits == RANK_MAX_EMITS == oracle.RANK_MAX_EMITS


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


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


def check(engine, text, queries, modes, k, first_line=0, **okw):
    expect = want(text, queries, modes, k, first_line, **okw)
    got = engine.run_search(text, queries, modes, first_line, rank=k)
    same(got, expect, k)
    assert got.first_line == first_line
    # ... and once more from the index the job left on the device
    same(engine.search_resident(queries, modes, rank=k), expect, k)
    return got


def unranked(text, queries, modes, first_line=0):
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ent, post = oracle.index(text, first_line=first_line)
    return [oracle.phrase(text, q, first_line=first_line)[0] if m == "phrase"
            else oracle.search(ent, post, q, m)[0] for q, m in zip(queries, modes)]


# ------------------------------------------------------------------------------------
# tiny inputs
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word", b"\n\n"])
@pytest.mark.parametrize("k", [1, 7])
def test_tiny_inputs(eng, text, k):
    queries = [[b"word"], [b"word"], [b"word", b"gone"], [b"gone", b"word"], [b"gone", b"away"],
               [b"word", b"word"]]
    got = check(eng, text, queries, ["all", "any", "all", "any", "any", "phrase"], k)
    tops = [list(zip(got.lines(i), got.scores(i))) for i in range(6)]
    assert got.format() == oracle.format_ranked(queries, tops, got.matches())
    assert got.scores(1) == ([1] if text == b"word" else [])


def test_k_above_and_below_the_matches(eng):
    text = b"a a a\na\nb\na a\n\na b\n"
    queries = [[b"a"], [b"b"], [b"a", b"b"]]
    got = check(eng, text, queries, ["all", "all", "any"], 1)
    assert got.lines(0) == [0] and got.matches() == [4, 2, 5]
    got = check(eng, text, queries, ["all", "all", "any"], 100)
    assert got.lines(0) == [0, 3, 1, 5] and got.hits() == [4, 2, 5]


def test_empty_batch(eng):
    got = eng.run_search(b"to be\n", [], rank=3)
    assert got.hits() == [] and got.matches() == [] and got.rank_k == 3
    got = eng.search_resident([], rank=3)
    assert got.hits() == [] and got.matches() == [] and got.queries == 0


# ------------------------------------------------------------------------------------
# tf: postings of one line across the wave, step and tile edges; the CSR range's ends
# ------------------------------------------------------------------------------------
def tf_text(length, at, copies):
    """`w` with a list of `length` postings, once per line, but `copies` times on the line
    whose postings start at position `at`; `all` on every line."""
    lines, pos = [], 0
    while pos < length:
        n = copies if pos == at else 1
        lines.append(b" ".join([b"w"] * n + [b"all"]))
        pos += n
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("edge", [64, SCORE_BLOCK, SCORE_TILE])
@pytest.mark.parametrize("copies", [2, 3])
def test_tf_across_an_edge(eng, edge, copies):
    """One line's postings at positions edge - 1, edge (and edge + 1) of a list: its tf
    is 2 (3), and it ranks first."""
    text = tf_text(edge + 40, edge - 1, copies)
    ent, post = oracle.index(text)
    v = [e for e in ent if e[0] == b"w"][0][1]
    span = post[v + edge - 1:v + edge - 1 + copies]
    assert len(set(span)) == 1 and post[v + edge - 2] != span[0] != post[v + edge - 1 + copies]
    queries = [[b"w"], [b"w", b"all"], [b"w", b"all"], [b"w", b"all"]]
    got = check(eng, text, queries, ["all", "all", "any", "phrase"], 5)
    assert got.lines(0)[0] == span[0] and got.scores(0)[0] == copies * got.scores(0)[1]
    assert got.lines(1)[0] == span[0]


def test_neighbour_trap(eng):
    """`ab`, `abc` and `abd` are adjacent in key order, so their postings are adjacent in
    memory, and the last line of `ab`'s list is the first of `abc`'s (and `abc`'s last is
    `abd`'s first): a tf count that runs one element past either end of a CSR range counts
    the neighbour's posting too."""
    lines = [b"pad pad"] * 12
    lines[3] = b"ab"              # ab : [3, 5]
    lines[5] = b"ab abc"          # abc: [5, 7]
    lines[7] = b"abc abd"         # abd: [7, 9]
    lines[9] = b"abd"
    text = b"\n".join(lines) + b"\n"
    ent, post = oracle.index(text)
    keys = [k for k, _v, _c in ent]
    i = keys.index(b"ab")
    assert keys[i:i + 3] == [b"ab", b"abc", b"abd"]
    assert post[ent[i][1]:ent[i + 2][1] + 2] == [3, 5, 5, 7, 7, 9]
    queries = [[b"ab"], [b"abc"], [b"abd"], [b"ab", b"abd"], [b"abc", b"ab"], [b"abc", b"abd"]]
    got = check(eng, text, queries, ["all"] * 3 + ["any"] * 3, 10)
    w = got.scores(0)[0]
    assert got.scores(0) == [w, w] and got.scores(1) == [w, w] and got.scores(2) == [w, w]
    assert got.lines(3) == [3, 5, 7, 9] and got.scores(3) == [w] * 4


# ------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------
def test_weights_on_either_side_of_a_power_of_two(eng):
    """N = 64 tokens; `a` occurs 9 times (64 // 9 = 7 = 2^3 - 1: weight 3) and `b` 8 times
    (64 // 8 = 8 = 2^3: weight 4).  Line 0 holds `a` five times (15), line 1 `b` four times
    (16): line 1 first.  With b's weight 3, or a's 4, line 0 would come first."""
    lines = [b"a a a a a", b"b b b b", b"a a a a", b"b b b b"]
    fill = 64 - 9 - 8
    lines += [b" ".join(b"f%d" % (i * 20 + j) for j in range(min(20, fill - i * 20)))
              for i in range((fill + 19) // 20)]
    text = b"\n".join(lines) + b"\n"
    ent, post = oracle.index(text)
    assert len(post) == 64
    counts = {k: c for k, _v, c in ent}
    assert counts[b"a"] == 9 and counts[b"b"] == 8
    assert (64 // 9).bit_length() == 3 and (64 // 8).bit_length() == 4
    got = check(eng, text, [[b"a", b"b"], [b"a"], [b"b"]], "any", 4)
    assert list(zip(got.lines(0), got.scores(0))) == [(1, 16), (3, 16), (0, 15), (2, 12)]
    assert got.scores(1) == [15, 12] and got.scores(2) == [16, 16]


# ------------------------------------------------------------------------------------
# ties and the cut
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties_text():
    return b"".join(b"tie x%d\n" % i for i in range(1025)) + b"other\n"


@pytest.mark.parametrize("k", [63, 64, 65, 1024, 1025, 1026])
def test_ties_and_the_cut(eng, k):
    """1025 matching lines of one score: the first min(K, 1025) lines, ascending."""
    got = check(eng, ties_text(), [[b"tie"]], "all", k)
    assert got.matches() == [1025] and got.lines(0) == list(range(min(k, 1025)))
    assert len(set(got.scores(0))) == 1


# ------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------
def test_segments(eng):
    """A query without a match between two with matches; K below the matches of some
    queries and above those of others; one line hit by neighbouring queries."""
    text = (b"red green\n" * 3 + b"green green blue\n" + b"blue\n" * 6 + b"red red red\n" +
            b"pad\n" * 4)
    queries = [[b"red"], [b"gone"], [b"green"], [b"green", b"blue"], [b"blue"], [b"gone", b"pad"],
               [b"red", b"green"], [b"gone"], [b"gone"], [b"pad"]]
    modes = ["all", "all", "all", "any", "any", "all", "phrase", "any", "any", "all"]
    got = check(eng, text, queries, modes, 4)
    assert got.matches() == [4, 0, 4, 10, 7, 0, 3, 0, 0, 4]
    assert got.hits() == [4, 0, 4, 4, 4, 0, 3, 0, 0, 4]
    assert got.lines(0)[0] == 10 and got.lines(2)[0] == 3 == got.lines(3)[0] == got.lines(4)[0]
    check(eng, text, queries, modes, 3)
    check(eng, text, queries[1:2] + queries[7:9], "any", 2)  # a batch without any match


def fuzz_case(seed, nlines, nqueries, nvocab=50):
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


def test_full_mixed_batch(eng):
    text, queries, modes = fuzz_case(17, 300, MAX_QUERIES)
    assert {"all", "any", "phrase"} == set(modes)
    got = check(eng, text, queries, modes, 3, first_line=7)
    assert got.queries == MAX_QUERIES and 0 in got.matches() and max(got.matches()) > 100
    assert any(m > 0 for m, mode in zip(got.matches(), modes) if mode == "phrase")
    # queries 0 and 1023 hold the first and the last segment: on their own they answer alike
    for i in (0, MAX_QUERIES - 1):
        alone = eng.search_resident(queries[i:i + 1], modes[i:i + 1], rank=3)
        assert (alone.lines(0), alone.scores(0)) == (got.lines(i), got.scores(i))
        assert alone.matches() == got.matches()[i:i + 1]


# ------------------------------------------------------------------------------------
# the score field
# ------------------------------------------------------------------------------------
def test_score_past_the_8_and_12_bit_boundaries():
    """One line holds `w` 4096 times under emits_per_line = 4096; 4200 other tokens make
    N // 4097 = 2, so w's weight is 2 and the line scores 8192 -- and ranks first."""
    lines = [b"w"] + [b"x " * 20] * 210 + [b"w " * 4096]
    text = b"\n".join(l.strip() for l in lines) + b"\n"
    engine = lc.Engine(gpu_cfg(emits_per_line=4096), len(text), len(lines))
    got = check(engine, text, [[b"w"], [b"w", b"x"]], ["all", "any"], 3, emits=4096)
    n = 4097 + 4200
    assert (n // 4097).bit_length() == 2
    assert list(zip(got.lines(0), got.scores(0))) == [(211, 8192), (0, 2)]
    assert got.lines(1)[0] == 211 and got.scores(1)[0] == 8192 and got.matches()[1] == 212


# ------------------------------------------------------------------------------------
# the sort's regimes
# ------------------------------------------------------------------------------------
def test_sort_regimes():
    n = SMALL_SORT + 1
    text = b"".join((b"v w w\n" if i % 3 == 0 else b"v w\n") if i < SMALL_SORT else b"w\n"
                    for i in range(n))
    engine = lc.Engine(gpu_cfg(), len(text), n)
    got = check(engine, text, [[b"v"]], "all", 5)     # exactly kSmallSortMax hits: the LDS sort
    assert got.matches() == [SMALL_SORT] and got.lines(0) == [0, 1, 2, 3, 4]
    got = check(engine, text, [[b"w"]], "any", 5)     # one more: the device-wide passes
    assert got.matches() == [SMALL_SORT + 1] and got.lines(0) == [0, 3, 6, 9, 12]
    got = check(engine, text, [[b"w"]], "any", SMALL_SORT + 1)
    assert got.hits() == [SMALL_SORT + 1] and got.lines(0)[-1] == SMALL_SORT


# ------------------------------------------------------------------------------------
# line numbers
# ------------------------------------------------------------------------------------
def test_last_window_and_largest_k(eng):
    text = b"alpha beta\nbeta gamma\n\nalpha alpha\n"
    queries = [[b"alpha"], [b"alpha", b"beta"], [b"gamma", b"alpha"]]
    first = 2**32 - 4  # the last accepted window
    got = check(eng, text, queries, ["all", "all", "any"], 2**32 - 1, first_line=first)
    assert got.lines(0) == [2**32 - 1, first] and got.lines(1) == [first]
    assert got.rank_k == 2**32 - 1
    got = check(eng, text, queries, ["all", "all", "any"], 1, first_line=first)
    assert got.lines(0) == [2**32 - 1] and got.lines(2) == [2**32 - 1]


# ------------------------------------------------------------------------------------
# modes and repeated terms
# ------------------------------------------------------------------------------------
def test_modes_and_repeated_terms(eng):
    text = (b"bye bye\n"            # 0
            b"bye now bye\n"        # 1: no phrase [bye, bye]
            b"bye bye bye bye\n"    # 2
            b"now\n"                # 3
            b"good bye\n"           # 4
            b"now now good\n")      # 5
    queries = [[b"bye", b"bye"], [b"bye", b"bye"], [b"bye", b"bye"], [b"gone", b"now", b"lost"],
               [b"now", b"gone", b"now", b"good"], [b"good", b"bye"], [b"bye", b"gone"]]
    modes = ["phrase", "all", "any", "any", "any", "phrase", "phrase"]
    got = check(eng, text, queries, modes, 10)
    w = got.scores(0)[-1] // 2  # bye's weight: line 0 holds it twice
    # the phrase matches by the phrase rule, and `bye` scores once
    assert list(zip(got.lines(0), got.scores(0))) == [(2, 4 * w), (0, 2 * w)]
    assert got.lines(1) == [2, 0, 1, 4] and got.scores(1) == [4 * w, 2 * w, 2 * w, w]
    assert got.lines(1) == got.lines(2) and got.scores(1) == got.scores(2)
    assert got.lines(3) == [5, 1, 3] and got.term_counts(3) == [0, 4, 0]
    assert got.lines(4)[0] == 5 and got.matches()[4] == 4
    assert got.lines(5) == [4] and got.matches()[6] == 0


def test_truncated_and_merged_keys(eng):
    a, b = b"x" * 29 + b"AAAAAA", b"x" * 29 + b"BBBBBB"
    text = a + b" foo " + b + b"\nbar " + b + b"\nfoo\n"
    queries = [[b"x" * 35], [a, b"foo"], [b, a], [a, b], [b"x" * 28]]
    got = check(eng, text, queries, ["all", "all", "any", "phrase", "all"], 5)
    # the merged list holds line 0 twice; [b, a] and [a, b] are one distinct term
    assert got.lines(0) == [0, 1] and got.scores(0)[0] == 2 * got.scores(0)[1]
    assert got.scores(2) == got.scores(0) and got.matches()[3] == 0 and got.matches()[4] == 0
    short = lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)
    got = check(short, b"abcdefgh abcdeXYZ\nabcde abcd\n", [[b"abcdeQQQ"], [b"abcd"]], "all", 2,
                max_key=5)
    assert got.lines(0) == [0, 1] and got.matches() == [2, 1]


# ------------------------------------------------------------------------------------
# engine state
# ------------------------------------------------------------------------------------
def test_ranked_and_unranked_alternate(hamlet):
    win = oracle.window(hamlet, 0, 700)
    queries, modes = [[b"to", b"be"], [b"Ham", b"Hor"], [b"the"], [b"my", b"lord"]], \
        ["any", "any", "all", "phrase"]
    plain = unranked(win, queries, modes)
    f = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    fresh = [f.run_search(win, queries, modes), f.search_resident(queries, modes)]
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    for k in (3, None, 50, None, 1):
        if k is None:
            again = [e.run_search(win, queries, modes), e.search_resident(queries, modes)]
            for got, was in zip(again, fresh):
                assert [got.lines(i) for i in range(4)] == plain
                assert got.rank_k == 0 and got.scores(0) == [] and got.matches() == got.hits()
                assert got.format() == was.format() and got.wire_bytes == was.wire_bytes
        else:
            check(e, win, queries, modes, k)


def test_stale_index_and_refused_batches(hamlet):
    win = oracle.window(hamlet, 0, 300)
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    q = [[b"to", b"be"]]
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q, rank=3)  # a fresh engine holds no index
    check(e, win, q, "any", 3)
    e.run(win)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q, rank=3)
    check(e, win, q, "any", 3)
    # a refused ranked batch starts nothing: the index stays resident, the engine usable
    for bad in (0, -1, 2**32, 2**70, "3"):
        with pytest.raises((lc.LocustError, TypeError), match="rank"):
            e.search_resident(q, "any", rank=bad)
        with pytest.raises((lc.LocustError, TypeError), match="rank"):
            e.run_search(win, q, "any", rank=bad)
        same(e.search_resident(q, "any", rank=2), want(win, q, "any", 2), 2)
    with pytest.raises(lc.LocustError, match="search"):
        e.search_resident([[b"a b"]], rank=2)
    same(e.search_resident(q, "all", rank=2), want(win, q, "all", 2), 2)


def test_emit_limit():
    text = b"to be or not to be\nbe\n"
    e = lc.Engine(gpu_cfg(emits_per_line=RANK_MAX_EMITS + 1), 1 << 16, 1 << 10)
    with pytest.raises(lc.LocustError, match="emits_per_line"):
        e.run_search(text, [[b"be"]], rank=1)
    got = e.run_search(text, [[b"be"]])  # an unranked search knows no such limit
    assert got.lines(0) == [0, 1]
    with pytest.raises(lc.LocustError, match="emits_per_line"):
        e.search_resident([[b"be"]], rank=1)
    assert e.search_resident([[b"be"]]).lines(0) == [0, 1]
    e = lc.Engine(gpu_cfg(emits_per_line=RANK_MAX_EMITS), 1 << 16, 1 << 10)
    got = check(e, text, [[b"be"]], "all", 1, emits=RANK_MAX_EMITS)
    assert got.lines(0) == [0]


# ------------------------------------------------------------------------------------
# whole Hamlet: the figures, the wire, the CLI
# ------------------------------------------------------------------------------------
TO_BE_TOP5 = [(209, 22), (1413, 22), (1915, 22), (2094, 22), (2817, 22)]


def test_whole_hamlet_figures_and_wire(hamlet):
    nlines = hamlet.count(b"\n") + 1
    engine = lc.Engine(gpu_cfg(), len(hamlet), nlines)
    queries = [[b"to", b"be"]] * 3 + [[b"my", b"lord"], [b"the"]]
    modes = ["any", "all", "phrase", "all", "any"]
    got = check(engine, hamlet, queries, modes, 5)
    assert got.num_tokens == 32940 and got.term_counts(0) == [634, 206]
    assert got.matches() == [737, 47, 27, 119, 820]
    for i in range(3):
        assert list(zip(got.lines(i), got.scores(i))) == TO_BE_TOP5
    assert list(zip(got.lines(3), got.scores(3))) == [(1145, 30), (2440, 29), (329, 22),
                                                      (649, 22), (338, 15)]
    assert list(zip(got.lines(4), got.scores(4))) == [(2073, 24), (2958, 18), (3838, 18),
                                                      (15, 12), (111, 12)]
    # only the winners cross PCIe
    plain = engine.search_resident([[b"the"]], "any")
    top = engine.search_resident([[b"the"]], "any", rank=10)
    assert len(top.lines(0)) == 10 and top.matches() == [820] and plain.hits() == [820]
    assert top.wire_bytes < plain.wire_bytes
    assert plain.wire_bytes - top.wire_bytes == 4 * 820 - (2 * 4 * 10 + 4)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_rank(cli, tmp_path):
    j = tmp_path / "rank.json"
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "to be", "--match", "any", "--rank",
                        "5", "--check", "--json", str(j)], capture_output=True, timeout=300,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_ranked([[b"to", b"be"]], [TO_BE_TOP5], [737])
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 1 and rec["rank_k"] == 5
    assert rec["hits"] == 5 and rec["matches"] == 737
    assert rec["search_ms"] > 0 and rec["index_ms"] > 0 and rec["wire_bytes"] > 0
