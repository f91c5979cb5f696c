"""Index search on the device (csrc/kernels/search.hip): ``Engine.run_search`` and
``Engine.search_resident`` against ``oracle.search(*oracle.index(text, ...))``.  The answer
is a pure function of the index, so every comparison is exact.  The shapes are the smallest
at which each part of the stage can go wrong: the wave (64) and the hit kernel's step (256)
and tile (1024) for the adjacent-duplicate rule, list lengths around them for the driver
choice and the list searches, words adjacent in key order for a search that leaves its CSR
range, the sort's two regimes, a full batch, and an element space past one sweep of the
capped grid."""
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
SMALL_SORT = 8192         # kSmallSortMax: the single-workgroup sort's last size
SEARCH_BLOCK = 256        # kSearchBlock: elements per step of a hit workgroup
SEARCH_TILE = 1024        # kSearchTile: elements per workgroup and grid stride
SEARCH_MAX_BLOCKS = 2048  # kSearchMaxBlocks: the hit kernel's grid cap
MAX_QUERIES = 1024        # kSearchMaxQueries


def test_mirrored_constants():
    assert lc._C.kSearchMaxQueries == MAX_QUERIES and lc._C.kSearchMaxTerms == 8
    assert oracle.MAX_SEARCH_TERMS == 8


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def want(text, queries, modes, first_line=0, **okw):
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {k: v for k, v in okw.items() if k in ("delims", "max_key")}
    return [oracle.search(ent, post, q, m, **skw) for q, m in zip(queries, modes)]


def same(got, expect):
    assert got.queries == len(expect)
    assert got.hits() == [len(l) for l, _c in expect]
    for i, (lines, counts) in enumerate(expect):
        assert got.lines(i) == lines, i
        assert got.term_counts(i) == counts, i


def check(engine, text, queries, modes, first_line=0, **okw):
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    expect = want(text, queries, modes, first_line, **okw)
    got = engine.run_search(text, queries, modes, first_line)
    same(got, expect)
    assert got.first_line == first_line
    # ... and once more from the index the job left on the device
    same(engine.search_resident(queries, modes), expect)
    return got


# ------------------------------------------------------------------------------------
# tiny inputs
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word\n", b"word", b"\n\n"])
def test_tiny_inputs(eng, text):
    queries = [[b"word"], [b"word"], [b"word", b"gone"], [b"gone", b"word"], [b"gone", b"away"],
               [b"gone", b"away"]]
    got = check(eng, text, queries, ["all", "any", "all", "any", "all", "any"])
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(6)])


def test_absent_terms(eng):
    text = b"to be or not\nto sleep\nbe all\n"
    queries = [[b"gone", b"away", b"lost"], [b"to", b"gone", b"be"], [b"gone"], [b"to", b"be"],
               [b"gone", b"away"], [b"gone", b"be", b"away"]]
    got = check(eng, text, queries, ["all", "all", "all", "all", "any", "any"])
    assert got.hits() == [0, 0, 0, 1, 0, 2]
    assert got.term_counts(1) == [2, 0, 2]


# ------------------------------------------------------------------------------------
# one hit per line: adjacent duplicates
# ------------------------------------------------------------------------------------
def test_rose_is_a_rose(eng):
    text = b"a b a\nrose is a rose is a rose\nb\n"
    queries = [[b"rose"], [b"rose", b"is", b"a"], [b"a"], [b"a", b"b"], [b"rose", b"b"]]
    got = check(eng, text, queries, ["all", "all", "any", "all", "any"])
    assert got.lines(0) == [1] and got.lines(2) == [0, 1] and got.lines(4) == [0, 1, 2]
    assert got.term_counts(0) == [3]


def dup_text(length, dup_at):
    """`w` with a list of `length` postings: once per line, but twice on the line whose
    postings fall on positions dup_at and dup_at + 1.  `all` is on every line, `odd` on
    every other line."""
    lines, pos, i = [], 0, 0
    while pos < length:
        twice = pos == dup_at and pos + 1 < length
        words = [b"w", b"w"] if twice else [b"w"]
        lines.append(b" ".join(words + [b"all"] + ([b"odd"] if i % 2 else [])))
        pos += 2 if twice else 1
        i += 1
    lines += [b"all all", b"odd all"]  # `all`'s list is the longer one: `w` drives
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("edge", [64, SEARCH_BLOCK, SEARCH_TILE])
def test_duplicates_across_an_edge(eng, edge):
    """The two postings of one line at positions edge - 1 and edge of a list: the last
    element of one wave / step / tile and the first of the next."""
    text = dup_text(edge + 40, edge - 1)
    ent, post = oracle.index(text)
    v = [e for e in ent if e[0] == b"w"][0][1]
    assert post[v + edge - 1] == post[v + edge] and post[v + edge - 2] != post[v + edge - 1]
    queries = [[b"w"], [b"w"], [b"w", b"all"], [b"w", b"odd"], [b"odd", b"w"], [b"w", b"all"]]
    check(eng, text, queries, ["all", "any", "all", "all", "any", "any"])


# ------------------------------------------------------------------------------------
# driver choice and list searches
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lengths_text():
    """Words L<n> with lists of n postings for the lengths below, each on lines 0 .. n-1;
    `first` only on line 0 and `last` only on the last line; `every` on every line."""
    top = SEARCH_TILE + 1
    lens = [1, 63, 64, 65, top]
    lines = []
    for i in range(top):
        words = [b"every"] + [b"L%d" % n for n in lens if i < n]
        if i == 0:
            words.append(b"first")
        if i == top - 1:
            words.append(b"last")
        lines.append(b" ".join(words))
    return b"\n".join(lines) + b"\n", lens


def test_list_lengths_and_drivers(eng):
    text, lens = lengths_text()
    names = [b"L%d" % n for n in lens]
    queries, modes = [], []
    for a in names:
        for b in names:
            queries += [[a, b], [a, b]]
            modes += ["all", "any"]
    # the hit is the first element of the other list, then its last
    queries += [[b"first", b"every"], [b"every", b"first"], [b"last", b"every"],
                [b"every", b"last"], [b"last", names[-1]], [b"first", b"last"],
                [b"L63", b"L64", b"L65", b"every"], [b"every", b"L65", b"L1"]]
    modes += ["all"] * 8
    got = check(eng, text, queries, modes)
    assert got.lines(len(queries) - 8) == [0] and got.lines(len(queries) - 6) == [SEARCH_TILE]
    assert got.lines(len(queries) - 3) == []


def test_neighbour_trap(eng):
    """`ab`, `abc` and `abd` are adjacent in key order, so their postings are adjacent in
    memory.  The line sought is in `ab`'s and `abd`'s lists but not in `abc`'s: a search
    that runs one element past either end of `abc`'s range finds it all the same."""
    lines = [b"pad"] * 12
    lines[3] = b"ab"          # ab : [3, 5]
    lines[5] = b"ab abd"      # abc: [4, 6]   (5 is not in it)
    lines[4] = b"abc"         # abd: [5, 7]
    lines[6] = b"abc"
    lines[7] = b"abd"
    text = b"\n".join(lines) + b"\n"
    ent, post = oracle.index(text)
    keys = [k for k, _v, _c in ent]
    i = keys.index(b"ab")
    assert keys[i:i + 3] == [b"ab", b"abc", b"abd"]
    assert post[ent[i][1]:ent[i + 2][1] + 2] == [3, 5, 4, 6, 5, 7]
    queries = [[b"ab", b"abc"], [b"abd", b"abc"], [b"ab", b"abd"], [b"ab", b"abc", b"abd"],
               [b"abc", b"ab"], [b"abc", b"abd"], [b"abc", b"ab", b"abd"]]
    got = check(eng, text, queries, ["all"] * 4 + ["any"] * 3)
    assert got.hits()[:4] == [0, 0, 1, 0]
    assert got.lines(4) == [3, 4, 5, 6] and got.lines(6) == [3, 4, 5, 6, 7]


# ------------------------------------------------------------------------------------
# any
# ------------------------------------------------------------------------------------
def test_any_overlapping_lists(eng):
    rng = random.Random(5)
    words = [b"t%d" % i for i in range(8)]
    lines = []
    for i in range(700):
        here = [w for k, w in enumerate(words) if rng.random() < 0.9 - 0.1 * k]
        rng.shuffle(here)
        lines.append(b" ".join(here * rng.randrange(1, 3)))
    lines[13] = b""
    text = b"\n".join(lines) + b"\n"
    queries = [words, words[::-1], [words[0], words[0]], [words[7], words[0], words[7]],
               words[:4] + words[:4], words, [b"gone"] + words[1:]]
    got = check(eng, text, queries, ["any"] * 5 + ["all", "any"])
    assert got.term_counts(2)[0] == got.term_counts(2)[1] > 0
    # terms whose union is every line
    text = b"".join(b"even\n" if i % 2 == 0 else b"odd\n" for i in range(301))
    got = check(eng, text, [[b"even", b"odd"], [b"odd", b"even"], [b"even", b"odd"]],
                ["any", "any", "all"])
    assert got.lines(0) == list(range(301)) and got.lines(2) == []


# ------------------------------------------------------------------------------------
# the sort's regimes, a full batch, the capped grid
# ------------------------------------------------------------------------------------
def test_sort_regimes():
    n = SMALL_SORT + 1
    text = b"".join(b"v w\n" if i < SMALL_SORT else b"w\n" for i in range(n))
    engine = lc.Engine(gpu_cfg(), len(text), n)
    got = check(engine, text, [[b"v"]], "all")      # exactly kSmallSortMax hits: the LDS sort
    assert sum(got.hits()) == SMALL_SORT
    got = check(engine, text, [[b"w"]], "any")      # one more: the device-wide passes
    assert sum(got.hits()) == SMALL_SORT + 1
    got = check(engine, text, [[b"v"], [b"v", b"w"], [b"w"]], ["all", "all", "any"])
    assert got.hits() == [SMALL_SORT, SMALL_SORT, n]


def fuzz_case(seed, nlines, nqueries, nvocab=50):
    rng = random.Random(seed)
    stem = b"q" * 29
    vocab = [bytes(rng.choice(b"abcdeXYZ") for _ in range(rng.randrange(1, 7)))
             for _ in range(nvocab - 4)]
    vocab += [stem, stem + b"A", stem + b"B" * 11, b"r" * 28 + b"s"]
    lines = [b" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 12)))
             for _ in range(nlines)]
    text = b"\n".join(lines) + b"\n"
    extra = [b"absent", b"zzz", stem + b"C", b"q" * 40, b"q" * 30, b"q" * 28]
    queries, modes = [], []
    for _ in range(nqueries):
        q = [rng.choice(vocab + extra) for _ in range(rng.randrange(1, 9))]
        if rng.random() < 0.3:
            q[rng.randrange(len(q))] = q[0]
        queries.append(q)
        modes.append(rng.choice(["all", "any"]))
    return text, queries, modes


def test_full_batch_and_one_more(eng):
    text, queries, modes = fuzz_case(11, 300, MAX_QUERIES + 1)
    assert "all" in modes and "any" in modes
    got = check(eng, text, queries[:MAX_QUERIES], modes[:MAX_QUERIES], first_line=7)
    assert got.queries == MAX_QUERIES and 0 in got.hits() and max(got.hits()) > 100
    with pytest.raises(lc.LocustError, match="kSearchMaxQueries = 1024"):
        eng.run_search(text, queries, modes)
    with pytest.raises(lc.LocustError, match="kSearchMaxQueries = 1024"):
        eng.search_resident(queries, modes)
    # a refused batch starts nothing: the index is still resident, the engine usable
    same(eng.search_resident(queries[1:], modes[1:]), want(text, queries[1:], modes[1:], 7))
    check(eng, text, queries[-3:], modes[-3:])
    assert eng.run_search(text, []).hits() == [] and eng.search_resident([]).hits() == []


def test_capped_grid():
    """More list elements than one sweep of the capped grid: the workgroups stride on."""
    words = [b"w%d" % i for i in range(8)]
    nlines, nq = 3000, 100
    text = (b" ".join(words) + b"\n") * nlines
    assert nq * 8 * nlines > SEARCH_MAX_BLOCKS * SEARCH_TILE
    engine = lc.Engine(gpu_cfg(), len(text), nlines)
    queries = [words[i % 8:] + words[:i % 8] for i in range(nq)]
    got = engine.run_search(text, queries, "any")
    assert got.hits() == [nlines] * nq
    every = list(range(nlines))
    assert all(got.lines(i) == every for i in range(nq))
    assert got.term_counts(99) == [nlines] * 8


# ------------------------------------------------------------------------------------
# line numbers, truncation
# ------------------------------------------------------------------------------------
def test_first_line(eng):
    text = b"alpha beta\nbeta gamma\n\nalpha\n"
    queries = [[b"alpha"], [b"alpha", b"beta"], [b"gamma", b"alpha"]]
    got = check(eng, text, queries, ["all", "all", "any"], first_line=1000)
    assert got.lines(0) == [1000, 1003] and got.lines(2) == [1000, 1001, 1003]
    first = 2**32 - 4  # the last accepted window
    got = check(eng, text, queries, ["all", "all", "any"], first_line=first)
    assert got.lines(0) == [first, 2**32 - 1] and got.lines(1) == [first]
    with pytest.raises(lc.LocustError, match=r"2\^32"):
        eng.run_search(text, queries, "all", first + 1)
    check(eng, text, queries, "any", first_line=1)  # the refusal leaves the engine usable


def test_truncation_merges_lists(eng):
    a, b = b"x" * 29 + b"AAAAAA", b"x" * 29 + b"BBBBBB"
    text = a + b" foo\nbar " + b + b"\nfoo\n"
    queries = [[b"x" * 35], [a, b"foo"], [b, a], [b"x" * 28]]
    got = check(eng, text, queries, ["all", "all", "any", "all"])
    assert got.lines(0) == [0, 1] and got.term_counts(0) == [2] and got.lines(3) == []
    short = lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)
    got = check(short, b"abcdefgh abcdeXYZ\nabcde abcd\n", [[b"abcdeQQQ"], [b"abcd"]], "all",
                max_key=5)
    assert got.lines(0) == [0, 1] and got.term_counts(0) == [3] and got.lines(1) == [1]


BAD_QUERIES = [[b""], [b"a\0b"], [b"a\nb"], [b"a b"], [b"semi;colon"], [],
               [b"t%d" % i for i in range(9)]]


@pytest.mark.parametrize("terms", BAD_QUERIES)
def test_refuses_invalid_queries(eng, terms):
    text = b"to be\nor not\n"
    check(eng, text, [[b"to"]], "all")
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(text, [[b"to"], terms])
    with pytest.raises(lc.LocustError, match="search"):
        eng.search_resident([terms])
    assert eng.search_resident([[b"not"]]).lines(0) == [1]  # ... and nothing was started


# ------------------------------------------------------------------------------------
# engine state
# ------------------------------------------------------------------------------------
def test_jobs_on_one_engine(hamlet):
    win = oracle.window(hamlet, 0, 700)
    other = oracle.window(hamlet, 700, 1100)
    queries, modes = [[b"to", b"be"], [b"Ham", b"Hor"], [b"the"]], ["all", "any", "all"]

    def fresh():
        return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)

    e = fresh()
    stats = lambda: e._eng.stats()["search_bytes"]
    r_run = e.run(win)
    assert stats() == 0
    s1 = e.run_search(win, queries, modes)
    first_bytes = stats()
    assert first_bytes > 0
    r_top = e.run_top(other, 10)
    r_idx = e.run_index(other)
    assert stats() == first_bytes  # a word, top or index job allocates nothing for search
    s2 = e.run_search(other, queries, modes, 700)
    assert r_run.entries() == fresh().run(win).entries()
    assert r_top.entries() == fresh().run_top(other, 10).entries()
    f_idx = fresh().run_index(other)
    assert (r_idx.entries(), r_idx.postings()) == (f_idx.entries(), f_idx.postings())
    same(s1, want(win, queries, modes))
    same(s2, want(other, queries, modes, 700))
    f2 = fresh().run_search(other, queries, modes, 700)
    assert [f2.lines(i) for i in range(3)] == [s2.lines(i) for i in range(3)]
    assert s1.num_tokens == r_run.num_tokens and s1.num_unique == r_run.num_unique
    assert s1.search_ms > 0 and s1.index_ms > 0 and s1.times()["gpu_ms"] > 0


def test_search_resident_and_stale_index(hamlet):
    win = oracle.window(hamlet, 0, 700)
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    q1, q2 = [[b"to", b"be"]], [[b"Ham", b"Hor"], [b"my", b"lord"]]
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1)  # a fresh engine holds no index
    r1 = e.run_search(win, q1)
    kept = r1.lines(0)
    same(e.search_resident(q2, "any"), want(win, q2, ["any"] * 2))  # after run_search
    assert r1.lines(0) == kept == want(win, q1, ["all"])[0][0]  # r1 keeps its own copy
    e.run_index(win, 50)
    got = e.search_resident(q2, "all")  # after run_index
    same(got, want(win, q2, ["all"] * 2, first_line=50))
    assert got.first_line == 50 and got.num_lines == 700 and got.index_ms == 0
    e.run(win)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1)
    e.run_index(win)
    e.run_top(win, 5)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1)
    e.run_search(win, q1)
    with pytest.raises(lc.LocustError, match=r"2\^32"):
        e.run_index(win, 2**32 - 3)  # a refused job
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1)
    same(e.run_search(win, q1), want(win, q1, ["all"]))


def test_workspace_grows_and_is_reused():
    text, lens = lengths_text()
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    stats = lambda: e._eng.stats()["search_bytes"]
    small, large = [[b"L1"]], [[b"every", b"L%d" % lens[-1]]] * 40
    check(e, text, small, "all")
    first = stats()
    assert first > 0
    check(e, text, large, "any")  # 40 x 2050 list elements: more than the first batch's tile
    grown = stats()
    assert 40 * 2 * SEARCH_TILE > 4096 and grown > first
    check(e, text, small, "any")
    check(e, text, large[:3], "all")
    assert stats() == grown


# ------------------------------------------------------------------------------------
# whole Hamlet, refusals, the CLI
# ------------------------------------------------------------------------------------
HAMLET_QUERIES = [[b"to", b"be"], [b"Ham", b"Hor"], [b"the"]]


def test_whole_hamlet(hamlet):
    nlines = hamlet.count(b"\n") + 1
    engine = lc.Engine(gpu_cfg(), len(hamlet), nlines)
    queries = HAMLET_QUERIES * 2
    modes = ["all"] * 3 + ["any"] * 3
    got = check(engine, hamlet, queries, modes)
    assert got.hits()[0] > 0 and got.hits()[2] > 0 and got.hits()[4] > got.hits()[1]
    assert got.wire_bytes < 4 * got.num_tokens  # less than the postings alone would be
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(6)])


@pytest.mark.parametrize("kw, msg", [
    ({"sort": "radix"}, "sort=dict"),
    ({"map_path": "compat"}, "map_path fast"),
    ({"ngram": 2}, "ngram"),
    ({"ref_timers": True}, "ref_timers"),
])
def test_refusals(kw, msg):
    engine = lc.Engine(gpu_cfg(**kw), 1 << 16, 1 << 10)
    with pytest.raises(lc.LocustError, match=msg):
        engine.run_search(b"some text\n", [[b"some"]])
    with pytest.raises(lc.LocustError, match="stale"):
        engine.search_resident([[b"some"]])


def test_refuses_more_than_one_pass(hamlet):
    engine = lc._C.GpuEngine(gpu_cfg(chunk_bytes=16 << 10), 1 << 30, 1 << 30)
    with pytest.raises(lc.LocustError, match="--backend cpu"):
        engine.run_search(hamlet, [[b"to"]], [0])


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_search(cli, hamlet, tmp_path):
    j = tmp_path / "search.json"
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "to be", "--search", "Ham Hor",
                        "--match", "any", "--check", "--json", str(j)], capture_output=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"to", b"be"], [b"Ham", b"Hor"]]
    expect = want(hamlet, queries, ["any", "any"])
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 2
    assert rec["hits"] == sum(len(l) for l, _c in expect)
    assert rec["search_ms"] > 0 and rec["index_ms"] > 0
    assert 0 < rec["wire_bytes"] < 4 * rec["tokens"]
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "to be"], capture_output=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    expect = want(hamlet, queries[:1], ["all"])
    assert result_lines(p.stdout) == oracle.format_search(queries[:1], [expect[0][0]])
