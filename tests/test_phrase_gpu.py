"""Phrase queries on the device (csrc/kernels/search.hip, search_phrase_kernel):
``Engine.run_search`` and then the same batch through ``Engine.search_resident``, both
compared exactly with ``oracle.phrase`` (``oracle.search`` for the other modes).  The shapes
are the smallest at which each part can go wrong: the automaton's restarts, the 64-byte step
of the line walk and the 32 bytes staged behind it, the emit cap, key truncation, the 64
candidates of a wave's round, the capped grid, the sort's two regimes, and the text that has
to stay resident beside the index."""
import functools
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from test_phrase import fuzz_case

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SORT = 8192          # kSmallSortMax: the single-workgroup sort's last size
SORT_TILE = 4096           # kSortTile: the hit workspace grows in whole sort tiles
MAX_QUERIES = 1024         # kSearchMaxQueries
PHRASE_MAX_BLOCKS = 2048   # kPhraseMaxBlocks: the verify kernel's grid cap
PHRASE_WAVES = 4           # waves per verify workgroup
ROUND = 64                 # candidates a wave takes per round, at most


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


@functools.lru_cache(maxsize=8)
def _index(text, first_line, okw):
    return oracle.index(text, first_line=first_line, **dict(okw))


def want(text, queries, modes, first_line=0, **okw):
    """[(lines, counts)] of every query by the oracle, each distinct query computed once."""
    skw = {k: v for k, v in okw.items() if k in ("delims", "max_key")}
    memo = {}
    out = []
    for q, m in zip(queries, modes):
        key = (tuple(q), m)
        if key not in memo:
            if m == "phrase":
                memo[key] = oracle.phrase(text, q, first_line=first_line, **okw)
            else:
                ent, post = _index(text, first_line, tuple(sorted(okw.items())))
                memo[key] = oracle.search(ent, post, q, m, **skw)
        out.append(memo[key])
    return out


def same(got, expect):
    assert got.queries == len(expect)
    assert got.hits() == [len(l) for l, _c in expect]
    for i, (lines, counts) in enumerate(expect):
        assert got.lines(i) == lines, i
        assert got.term_counts(i) == counts, i


def check(engine, text, queries, modes="phrase", first_line=0, **okw):
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    expect = want(text, queries, modes, first_line, **okw)
    got = engine.run_search(text, queries, modes, first_line)
    same(got, expect)
    assert got.first_line == first_line
    # ... and once more from the index and the text the job left on the device
    same(engine.search_resident(queries, modes), expect)
    return got


# ------------------------------------------------------------------------------------
# tiny inputs
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word", b"\n\n", b"word word\n"])
def test_tiny_inputs(eng, text):
    queries = [[b"word"], [b"word", b"word"], [b"word", b"gone"], [b"gone", b"away"], [b"word"]]
    got = check(eng, text, queries, ["phrase"] * 4 + ["all"])
    assert got.lines(0) == got.lines(4)  # a one-term phrase answers as `all`
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(5)])


def test_one_term_absent_reversed_apart(eng):
    text = b"to be or not\nbe to\nto sleep be\nto\nbe\n\nnot to be\n"
    queries = [[b"to"], [b"to"], [b"gone"], [b"to", b"gone"], [b"gone", b"to", b"be"],
               [b"to", b"be"], [b"be", b"to"], [b"to", b"be"], [b"sleep", b"to"]]
    got = check(eng, text, queries, ["phrase", "all"] + ["phrase"] * 5 + ["all", "phrase"])
    assert got.lines(0) == got.lines(1) == [0, 1, 2, 3, 6]
    assert got.hits()[2:5] == [0, 0, 0] and got.term_counts(4) == [0, 5, 5]
    # lines 1 and 2 hold both words -- `all` candidates -- reversed or apart: rejected
    assert got.lines(5) == [0, 6] and got.lines(6) == [1] and got.lines(7) == [0, 1, 2, 6]
    assert got.lines(8) == []


# ------------------------------------------------------------------------------------
# the automaton
# ------------------------------------------------------------------------------------
def test_automaton(eng):
    t8 = [b"t%d" % i for i in range(8)]
    text = (b"a b a b c\n"                                # 0: an overlapping prefix
            b"bye now bye\n"                              # 1
            b"bye bye\n"                                  # 2
            b"rose is a rose is a rose\n"                 # 3
            b"rose is a tulip is a rose\n"                # 4
            b"t0 t1 t2 t0 t1 t2 t3 t4 t5 t6 t7 x\n"       # 5
            b"t0 t1 t2 t3 t4 t5 t6 x t7\n"                # 6
            b"a a b\n"                                    # 7
            b"a b a b a b d c\n")                         # 8
    queries = [[b"a", b"b", b"c"], [b"bye", b"bye"], [b"rose", b"is", b"a", b"rose"], t8,
               [b"a", b"a", b"b"], [b"a", b"b", b"a", b"b", b"c"], [b"bye", b"now", b"bye"],
               [b"rose", b"rose"]]
    got = check(eng, text, queries)
    assert got.lines(0) == [0] and got.lines(1) == [2] and got.lines(2) == [3]
    assert got.lines(3) == [5] and got.lines(4) == [7] and got.lines(5) == [0]
    assert got.lines(6) == [1] and got.lines(7) == []
    assert got.term_counts(1) == [4, 4] and got.term_counts(2)[0] == got.term_counts(2)[3]


# ------------------------------------------------------------------------------------
# the 64-byte step
# ------------------------------------------------------------------------------------
def fill(n):
    """n bytes of short filler words (at most 9 tokens per 64 bytes), the last one a space."""
    assert n == 0 or n >= 2
    out = b""
    while len(out) + 8 <= n:
        out += b"fffffff "
    rest = n - len(out)
    return out + (b"g" * (rest - 1) + b" " if rest else b"")


def step_text():
    ab = b"alpha beta"
    lines = [
        fill(58) + b"alpha" + b" " + b"beta",                 # 0: alpha = bytes 58-62, beta at 64
        fill(59) + b"alpha" + b" " + b"beta",                 # 1: alpha ends at byte 63, beta at 65
        fill(60) + b"alphaalpha1" + b" beta",                 # 2: a token on bytes 60-70
        fill(60) + b"alphaalpha1" + b" beta alpha beta",      # 3: ... and the phrase behind it
        fill(64) + ab,                                        # 4: the phrase starts at byte 64
        fill(63 - 10) + ab, fill(64 - 10) + ab, fill(65 - 10) + ab,   # 5-7: 63, 64, 65 bytes
        fill(128 - 10) + ab, fill(129 - 10) + ab,                     # 8-9: 128, 129 bytes
        b"alpha" + b" " * 70 + b"beta",                       # 10: > 64 delimiter bytes between
        b"alpha" + b" ,;" * 50 + b"beta",                     # 11: ... more than two steps of them
        (b"f" * 27 + b" ") * 14 + ab,                         # 12: 402 bytes, phrase in the last step
        b"beta alpha\0 beta",                                 # 13: a NUL between the words
        fill(56) + b"beta alpha\0beta",                       # 14: ... in the second step
        b"beta alpha",                                        # 15: reversed
        fill(62) + b"alpha beta",                             # 16: alpha straddles bytes 62-66
        b"alpha " + b"x" * 70 + b" beta",                     # 17: a 70-byte token between
        b"x" * 40 + b"alpha beta",                            # 18: `alpha` inside a longer token
    ]
    for i, want_len in ((5, 63), (6, 64), (7, 65), (8, 128), (9, 129)):
        assert len(lines[i]) == want_len
    assert lines[0].index(b"beta") == 64 and lines[1].index(b"alpha") + 4 == 63
    assert lines[2].index(b"alphaalpha1") == 60 and lines[4].index(b"alpha") == 64
    assert len(lines[12]) > 400 and all(b"\n" not in l for l in lines)
    # the last line without its newline
    return b"\n".join(lines) + b"\nbeta alpha beta"


def test_step_edges(eng):
    text = step_text()
    queries = [[b"alpha", b"beta"], [b"alpha", b"beta"], [b"alphaalpha1", b"beta"],
               [b"beta", b"alpha"], [b"alphaalpha1", b"beta", b"alpha", b"beta"]]
    got = check(eng, text, queries, ["phrase", "all", "phrase", "phrase", "phrase"])
    assert got.lines(0) == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 19]
    # every line but 2 and 18 (no `alpha` token) holds both words
    assert got.lines(1) == [l for l in range(20) if l not in (2, 18)]
    assert got.lines(2) == [2, 3] and got.lines(3) == [3, 13, 14, 15, 19] and got.lines(4) == [3]
    # the same text behind another upload path (the default engine maps small texts from
    # the pinned staging buffer)
    check(lc.Engine(gpu_cfg(zero_copy_text=0), 1 << 20, 1 << 15), text, queries[:1])


# ------------------------------------------------------------------------------------
# the emit cap
# ------------------------------------------------------------------------------------
def test_emit_cap(eng):
    f = [b"f%d" % i for i in range(30)]
    text = (b" ".join(f[:18] + [b"alpha", b"beta"] + f[18:22]) + b"\n"          # ordinals 18-19
            + b" ".join([b"beta"] + f[:18] + [b"alpha", b"beta"]) + b"\n"       # ordinals 19-20
            + b" ".join(f[:19] + [b"alpha", b"beta"]) + b"\n")                  # beta capped: no candidate
    got = check(eng, text, [[b"alpha", b"beta"], [b"alpha", b"beta"], [b"f17", b"alpha"]],
                ["phrase", "all", "phrase"])
    assert got.lines(0) == [0] and got.lines(1) == [0, 1] and got.lines(2) == [0, 1]
    assert got.term_counts(0) == [3, 2] and got.overflow_lines == 3
    short = lc.Engine(gpu_cfg(emits_per_line=3), 1 << 16, 1 << 10)
    text = b"f alpha beta x\nbeta f alpha beta\nalpha beta\n" + fill(64) + b"alpha beta\n"
    got = check(short, text, [[b"alpha", b"beta"], [b"alpha", b"beta"]], ["phrase", "all"],
                emits=3)
    assert got.lines(0) == [0, 2] and got.lines(1) == [0, 1, 2]


# ------------------------------------------------------------------------------------
# truncation
# ------------------------------------------------------------------------------------
def test_truncation(eng):
    a, b = b"x" * 29 + b"AAAAAA", b"x" * 29 + b"BBBBBB"
    text = (a + b" foo\nfoo " + b + b"\n" + b"x" * 28 + b" foo\n"
            + fill(40) + a + b" foo\n" + fill(60) + b + b" foo " + a + b"\n")
    queries = [[b"x" * 35, b"foo"], [b"foo", a], [a, b"foo", b], [b"x" * 28, b"foo"],
               [b"x" * 29, b"x" * 29]]
    got = check(eng, text, queries)
    assert got.lines(0) == [0, 3, 4] and got.lines(1) == [1, 4] and got.lines(2) == [4]
    assert got.lines(3) == [2] and got.lines(4) == [] and got.term_counts(0) == [5, 5]
    short = lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)
    text = b"abcdefgh abcdeXYZ\nabcd abcde\nabcde abcd\n"
    queries = [[b"abcdeQ", b"abcde"], [b"abcd", b"abcdeZZZ"], [b"abcde", b"abcd"]]
    got = check(short, text, queries, max_key=5)
    assert got.hits() == [1, 1, 1] and got.lines(1) == [1]


# ------------------------------------------------------------------------------------
# group and grid edges
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounds_text():
    """For n in (63, 64, 65, 1025): n candidate lines of [v<n>, w<n>], every third one
    reversed (no hit), between lines that hold one of the words only.  `z` stands on
    130,000 further lines: as an `any` query beside a phrase it lifts the batch's bound past
    63 * 2048, where a wave of the verify kernel takes 64 candidates per round."""
    lines = []
    for n in (63, 64, 65, 1025):
        v, w = b"v%d" % n, b"w%d" % n
        for i in range(n):
            lines.append(w + b" " + v if i % 3 == 2 else b"pad " + v + b", " + w)
            lines.append(v if i % 2 else w + b" pad")
    lines += [b"z"] * 130000
    return b"\n".join(lines) + b"\n"


@pytest.fixture(scope="module")
def rounds_engine():
    text = rounds_text()
    return lc.Engine(gpu_cfg(), len(text), text.count(b"\n") + 1)


@pytest.mark.parametrize("n", [63, 64, 65, 1025])
@pytest.mark.parametrize("pad", [False, True])
def test_candidates_per_round(rounds_engine, n, pad):
    text = rounds_text()
    assert 130000 > (ROUND - 1) * PHRASE_MAX_BLOCKS
    queries = [[b"v%d" % n, b"w%d" % n]] + ([[b"z"]] if pad else [])
    got = check(rounds_engine, text, queries, ["phrase", "any"][:len(queries)])
    assert got.hits()[0] == n - n // 3 and got.term_counts(0) == [n + n // 2, n + (n + 1) // 2]


def test_full_batch(eng):
    text, queries, modes = fuzz_case(11, nlines=300, nqueries=MAX_QUERIES)
    assert {"all", "any", "phrase"} == set(modes)
    got = check(eng, text, queries, modes, first_line=7)
    ph = [h for h, m, q in zip(got.hits(), modes, queries) if m == "phrase" and len(q) > 1]
    assert got.queries == MAX_QUERIES and 0 in ph and sum(1 for h in ph if h) > 100


def test_more_than_one_sweep():
    """More candidates than one sweep of the capped verify grid: the waves stride on."""
    words = [b"w%d" % i for i in range(8)]
    nlines, nq = 3000, 180
    text = (b" ".join(words) + b"\n") * nlines
    assert nq * nlines > PHRASE_MAX_BLOCKS * PHRASE_WAVES * ROUND
    engine = lc.Engine(gpu_cfg(), len(text), nlines)
    queries = [[words[i % 7], words[i % 7 + 1]][::1 if i % 2 == 0 else -1] for i in range(nq)]
    got = check(engine, text, queries)
    assert got.hits() == [nlines if i % 2 == 0 else 0 for i in range(nq)]


def test_sort_regimes():
    n = SMALL_SORT + 1
    text = b"v w\n" * n
    engine = lc.Engine(gpu_cfg(), len(text), n)
    got = check(engine, text, [[b"v", b"w"]])      # one more than the LDS sort takes
    assert got.hits() == [n]
    got = check(engine, text, [[b"w", b"v"], [b"v", b"w"], [b"v"]], ["phrase", "phrase", "any"])
    assert got.hits() == [0, n, n]
    text = b"v w\n" * SMALL_SORT + b"w v\n"
    got = check(engine, text, [[b"v", b"w"]])      # exactly kSmallSortMax hits of n candidates
    assert got.hits() == [SMALL_SORT]


# ------------------------------------------------------------------------------------
# engine state
# ------------------------------------------------------------------------------------
def test_resident_and_stale(hamlet):
    win = oracle.window(hamlet, 0, 700)
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    q1, q2 = [[b"my", b"lord"]], [[b"to", b"be"], [b"lord", b"my"], [b"my", b"lord"]]
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "phrase")
    e.run_search(win, q1, "all")
    same(e.search_resident(q2, "phrase"), want(win, q2, ["phrase"] * 3))  # after run_search
    e.run_index(win, 50)
    got = e.search_resident(q2, ["phrase", "phrase", "all"])              # after run_index
    same(got, want(win, q2, ["phrase", "phrase", "all"], first_line=50))
    assert got.first_line == 50 and got.index_ms == 0 and got.search_ms > 0
    e.run(win)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "phrase")
    e.run_index(win)
    e.run_top(win, 5)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "phrase")
    same(e.run_search(win, q1, "phrase"), want(win, q1, ["phrase"]))


@pytest.mark.parametrize("zero_copy", [1, None])
def test_staging_buffer_is_not_the_resident_text(hamlet, zero_copy):
    """The map of a zero-copy job reads the pinned staging buffer, which load() refills
    without starting a job: the resident text must be the engine's own copy."""
    win = oracle.window(hamlet, 0, 2000)
    assert len(win) <= 1 << 20
    e = lc.Engine(gpu_cfg(zero_copy_text=zero_copy), 1 << 20, 1 << 15)
    queries = [[b"my", b"lord"], [b"to", b"be"], [b"lord", b"my"]]
    expect = want(win, queries, ["phrase"] * 3)
    same(e.run_search(win, queries, "phrase"), expect)
    e._eng.load(b"x" * len(win))
    same(e.search_resident(queries, "phrase"), expect)
    e.run_index(win)
    e._eng.load(b"\n" * len(win))
    same(e.search_resident(queries, "phrase"), expect)
    assert expect[0][0] and expect[1][0]


def test_search_bytes():
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    stats = lambda: e._eng.stats()["search_bytes"]
    small = b"v w\n" * 100
    large = b"v w\n" * (SORT_TILE + 1)
    e.run(small)
    e.run_index(small)
    assert stats() == 0
    check(e, small, [[b"v", b"w"]])
    first = stats()
    assert first > 0
    e.run(large)
    e.run_top(large, 3)
    e.run_index(large)
    assert stats() == first  # a word, top or index job allocates nothing for search
    check(e, large, [[b"v", b"w"]])
    grown = stats()
    # one more sort tile of list elements: per element seven 8-byte words (pairs, cands,
    # zeros, sorted, spare, the sort's two key buffers) and three 4-byte ones
    assert grown - first >= SORT_TILE * (7 * 8 + 3 * 4)
    check(e, small, [[b"w", b"v"]])
    assert stats() == grown


# ------------------------------------------------------------------------------------
# whole Hamlet, the CLI
# ------------------------------------------------------------------------------------
HAMLET = [([b"to", b"be"], 27), ([b"my", b"lord"], 109), ([b"lord", b"my"], 2),
          ([b"of", b"the"], 57), ([b"be", b"to"], 0)]


def test_whole_hamlet(hamlet):
    lines = oracle.split_lines(hamlet)
    assert sum(len(l) > 64 for l in lines) == 430
    assert max(len(oracle.tokenize(l, emits=10**6)[0]) for l in lines) <= 20
    engine = lc.Engine(gpu_cfg(), len(hamlet), len(lines) + 1)
    queries = [q for q, _n in HAMLET] * 2
    modes = ["phrase"] * 5 + ["all"] * 5
    got = check(engine, hamlet, queries, modes)
    assert got.hits()[:5] == [n for _q, n in HAMLET]
    for i in range(5):
        ph, al = set(got.lines(i)), set(got.lines(i + 5))
        assert ph <= al and (ph == al or ph < al) and len(al) > len(ph)
    assert got.hits()[5] == got.hits()[9] == 47
    assert got.wire_bytes < 4 * got.num_tokens  # less than the postings alone would be
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(10)])


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_phrase(cli, hamlet, tmp_path):
    j = tmp_path / "phrase.json"
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "to be", "--search", "my lord",
                        "--match", "phrase", "--check", "--json", str(j)], capture_output=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"to", b"be"], [b"my", b"lord"]]
    expect = want(hamlet, queries, ["phrase"] * 2)
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 2
    assert rec["hits"] == sum(len(l) for l, _c in expect) == 27 + 109
    assert rec["search_ms"] > 0 and rec["index_ms"] > 0
