"""Proximity (`near`) queries on the device (csrc/kernels/search.hip, search_near_kernel):
``Engine.run_search`` and then the same batch through ``Engine.search_resident``, both
compared exactly with ``oracle.near`` (``oracle.phrase`` / ``oracle.search`` for the other
modes).  The shapes are the smallest at which each part can go wrong: the window's edge, the
per-term ordinals carried across the 64-byte steps of the line walk, the emit cap, ordinals
past 8 bits, the shortcut for wide windows, the 64 candidates of a wave's round, the
candidate list the two verify kernels share, the sort's two regimes, merged prefix lists,
the ranked path and the text that has to stay resident beside the index."""
import functools
import json
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from near_cases import BY_HAND, TEXT, W_MAX, fuzz_case, same, same_ranked, want

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_SORT = 8192          # kSmallSortMax: the single-workgroup sort's last size
MAX_QUERIES = 1024         # kSearchMaxQueries
VERIFY_MAX_BLOCKS = 2048   # kPhraseMaxBlocks: the verify kernels' grid cap
ROUND = 64                 # candidates a wave takes per round, at most


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, queries, modes="near", within=None, first_line=0, wildcard=False,
          expect=None, **okw):
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if expect is None:
        expect = want(text, queries, modes, within, first_line, wildcard, **okw)
    got = engine.run_search(text, queries, modes, first_line, wildcard=wildcard, within=within)
    same(got, expect)
    assert got.first_line == first_line
    # ... and once more from the index and the text the job left on the device
    same(engine.search_resident(queries, modes, wildcard=wildcard, within=within), expect)
    return got


# ------------------------------------------------------------------------------------
# tiny inputs, the rules by hand
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [b"", b"word", b"\n\n", b"word word\n"])
def test_tiny_inputs(eng, text):
    queries = [[b"word"], [b"word", b"word"], [b"word", b"gone"], [b"gone", b"away"], [b"word"]]
    got = check(eng, text, queries, ["near"] * 4 + ["all"], [1, 1, 2, 3, None])
    assert got.lines(0) == got.lines(1) == got.lines(4)  # one (distinct) term answers as `all`
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(5)])


@pytest.mark.parametrize("wild", [False, True])
def test_by_hand(eng, wild):
    cases = [c for c in BY_HAND if c[2] == wild]
    queries, within = [c[0] for c in cases], [c[1] for c in cases]
    got = check(eng, TEXT, queries, "near", within, wildcard=wild)
    assert [got.lines(i) for i in range(len(cases))] == [c[3] for c in cases]
    # the last line without its newline, another first line, one window for the batch
    text = TEXT + b"be to"
    got = check(eng, text, [[b"to", b"be"], [b"be", b"to"]], "near", 3, first_line=10)
    assert got.lines(0) == got.lines(1) == [10, 11, 20]


# ------------------------------------------------------------------------------------
# the 64-byte step: the ordinals and the seen terms carry across it
# ------------------------------------------------------------------------------------
F = b"f" * 27 + b" "  # 28 bytes, one token: a three-step line stays under the emit cap


def at(n):
    """n bytes of filler tokens of at most 28 bytes, the last byte a space."""
    rest = n % 28
    assert rest != 1
    return F * (n // 28) + (b"g" * (rest - 1) + b" " if rest else b"")


def step_text():
    lines = [
        b"alpha " + F * 5 + b"beta",             # 0: ordinals 0 and 6, bytes 0 and 146 (step 2)
        at(62) + b"alpha beta",                  # 1: alpha straddles bytes 62-66
        at(58) + b"alpha beta",                  # 2: alpha = bytes 58-62, beta starts step 1
        at(59) + b"beta alpha",                  # 3: the other order, alpha at byte 64
        b"beta " + F * 3 + b"alpha\0 beta",      # 4: a NUL: the beta behind it does not exist
        at(60) + b"beta f alpha\0beta",          # 5: ... in the second step
        b"alpha" + b" " * 70 + b"beta",          # 6: more than a step of delimiters between
        b"alpha" + b" ,;" * 50 + b"beta",        # 7: ... more than two steps
        b"x" * 40 + b"alpha beta",               # 8: `alpha` inside a longer token
        b"beta " + F * 6 + b"gamma " + F * 6 + b"alpha",  # 9: three terms, one per 190 bytes
        at(120) + b"alpha f beta",               # 10: both in the second step
        at(128) + b"beta alpha",                 # 11: the match begins with step 2
    ]
    assert lines[0].index(b"beta") == 146 and lines[1].index(b"alpha") == 62
    assert lines[2].index(b"beta") == 64 and lines[3].index(b"alpha") == 64
    assert lines[9].index(b"alpha") > 320 and all(b"\n" not in l for l in lines)
    # the last line without its newline
    return b"\n".join(lines) + b"\nbeta x alpha"


def test_step_edges(eng):
    text = step_text()
    ab, ba = [b"alpha", b"beta"], [b"beta", b"alpha"]
    queries = [ab, ba, ab, ab, ab, ab, ab, [b"gamma", b"alpha", b"beta"],
               [b"gamma", b"alpha", b"beta"], ab]
    modes = ["near"] * 9 + ["all"]
    within = [2, 2, 3, 4, 5, 6, 7, 14, 15, None]
    got = check(eng, text, queries, modes, within)
    assert got.lines(0) == got.lines(1) == [1, 2, 3, 6, 7, 11]
    assert got.lines(2) == [1, 2, 3, 5, 6, 7, 10, 11, 12]
    assert got.lines(3) == got.lines(2) and got.lines(4) == sorted(got.lines(2) + [4])
    assert got.lines(5) == got.lines(4) and got.lines(6) == sorted(got.lines(5) + [0])
    assert got.lines(9) == sorted(got.lines(6) + [9])  # line 9 holds both, 15 tokens apart
    assert got.lines(7) == [] and got.lines(8) == [9]
    # the same text behind another upload path (the default engine maps small texts from
    # the pinned staging buffer)
    check(lc.Engine(gpu_cfg(zero_copy_text=0), 1 << 20, 1 << 15), text, queries[:3], "near",
          within[:3])


# ------------------------------------------------------------------------------------
# the emit cap, wide ordinals, wide windows
# ------------------------------------------------------------------------------------
def test_emit_cap(eng):
    f = [b"f%d" % i for i in range(30)]
    text = (b" ".join(f[:18] + [b"alpha", b"beta"] + f[18:22]) + b"\n"        # ordinals 18, 19
            + b" ".join([b"beta"] + f[:18] + [b"alpha", b"beta"]) + b"\n"     # 0, 19 (20: capped)
            + b" ".join(f[:19] + [b"alpha", b"beta"]) + b"\n")                # beta is the 21st
    ab = [b"alpha", b"beta"]
    got = check(eng, text, [ab, ab, ab, ab, ab], ["near"] * 4 + ["all"], [2, 19, 20, W_MAX, None])
    assert got.lines(0) == got.lines(1) == [0] and got.lines(2) == got.lines(3) == [0, 1]
    assert got.lines(4) == [0, 1] and got.term_counts(0) == [3, 2] and got.overflow_lines == 3
    short = lc.Engine(gpu_cfg(emits_per_line=3), 1 << 16, 1 << 10)
    text = b"f alpha beta x\nbeta f alpha beta\nbeta alpha\n" + at(64) + b"alpha beta\n"
    got = check(short, text, [ab, ab, ab], ["near", "near", "all"], [2, 3, None], emits=3)
    assert got.lines(0) == [0, 2] and got.lines(1) == got.lines(2) == [0, 1, 2]


def test_wide_ordinals():
    """Ordinals past 8 bits on a line of 15 steps: a window or an ordinal narrowed to a
    byte, or reset per step, answers these wrongly."""
    def line(marks, n=300):
        toks = [b"ff"] * n
        for o, t in marks.items():
            toks[o] = t
        return b" ".join(toks)
    text = b"\n".join([line({0: b"s0", 256: b"s1"}),            # 0: 257 tokens
                       line({1: b"s1", 257: b"s0"}),            # 1: the other order
                       line({43: b"s0", 299: b"s1"}),           # 2: ... up to the last ordinal
                       line({44: b"s0", 300: b"s1"}, 301),      # 3: s1 is the 301st token
                       line({0: b"s0", 255: b"s1"}),            # 4: 256 tokens
                       line({0: b"s0", 1: b"s1"})]) + b"\n"     # 5
    e = lc.Engine(gpu_cfg(emits_per_line=300), len(text), 8)
    q = [b"s0", b"s1"]
    got = check(e, text, [q] * 6, ["near"] * 5 + ["all"], [257, 256, 2, 300, W_MAX, None],
                emits=300)
    assert got.lines(0) == [0, 1, 2, 4, 5] and got.lines(1) == [4, 5] and got.lines(2) == [5]
    assert got.lines(3) == got.lines(4) == got.lines(5) == [0, 1, 2, 4, 5]
    assert got.overflow_lines == 1


def test_wide_windows_answer_as_all(eng, hamlet):
    win = oracle.window(hamlet, 0, 700)
    queries = [[b"to", b"be"], [b"my", b"lord"], [b"the", b"King", b"of"]]
    got = check(eng, win, queries * 4, ["near"] * 9 + ["all"] * 3,
                [19] * 3 + [20] * 3 + [W_MAX] * 3 + [None] * 3)
    for i in range(3):
        assert got.lines(3 + i) == got.lines(6 + i) == got.lines(9 + i) and got.lines(9 + i)
        assert set(got.lines(i)) <= set(got.lines(9 + i))


# ------------------------------------------------------------------------------------
# group and grid edges, the shared candidate list
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rounds_text():
    """For n in (63, 64, 65, 1025): n candidate lines of [v<n>, w<n>], every third one with
    two tokens between the words (no hit for W = 2), between lines that hold one of the
    words only.  `z` stands on 130,000 further lines: as an `any` query beside a near query
    it lifts the batch's bound past 63 * 2048, where a wave of the verify kernel takes 64
    candidates per round."""
    lines = []
    for n in (63, 64, 65, 1025):
        v, w = b"v%d" % n, b"w%d" % n
        for i in range(n):
            lines.append(w + b" a b " + v if i % 3 == 2 else b"pad " + v + b", " + w)
            lines.append(v if i % 2 else w + b" pad")
    lines += [b"z"] * 130000
    return b"\n".join(lines) + b"\n"


@functools.lru_cache(maxsize=None)
def rounds_expect(n, pad):
    text = rounds_text()
    queries = [[b"w%d" % n, b"v%d" % n]] + ([[b"z"]] if pad else [])
    return queries, want(text, queries, ["near", "any"][:len(queries)], 2)


@pytest.fixture(scope="module")
def rounds_engine():
    text = rounds_text()
    return lc.Engine(gpu_cfg(), len(text), text.count(b"\n") + 1)


@pytest.mark.parametrize("n", [63, 64, 65, 1025])
@pytest.mark.parametrize("pad", [False, True])
def test_candidates_per_round(rounds_engine, n, pad):
    assert 130000 > (ROUND - 1) * VERIFY_MAX_BLOCKS
    queries, expect = rounds_expect(n, pad)
    got = check(rounds_engine, rounds_text(), queries, ["near", "any"][:len(queries)], 2,
                expect=expect)
    assert got.hits()[0] == n - n // 3 and got.term_counts(0) == [n + (n + 1) // 2, n + n // 2]


def test_both_verify_kernels_in_one_batch(eng):
    """phrase, near, all and any queries interleaved over the same lines: the candidates of
    the two verify kernels meet in one list, from its two ends."""
    lines = []
    for i in range(400):
        lines.append([b"v w", b"w v", b"v x w", b"w x x v", b"v", b"w x"][i % 6] + b" t%d" % (i % 5))
    text = b"\n".join(lines) + b"\n"
    queries, modes, within = [], [], []
    for i in range(64):
        q = [[b"v", b"w"], [b"w", b"v"], [b"v", b"w", b"t%d" % (i % 5)]][i % 3]
        m = ["phrase", "near", "all", "near", "any"][i % 5]
        queries.append(q)
        modes.append(m)
        within.append(1 + i % 4 if m == "near" else None)
    got = check(eng, text, queries, modes, within)
    hits = {m: [h for h, mm in zip(got.hits(), modes) if mm == m] for m in set(modes)}
    assert all(hits["phrase"]) and any(hits["near"]) and 0 in hits["near"]
    # two near windows for the same terms beside a phrase: 1 -> none, 3 -> more than the phrase
    got = check(eng, text, [[b"v", b"w"]] * 4, ["near", "phrase", "near", "all"],
                [1, None, 3, None])
    assert got.hits()[0] == 0 < got.hits()[1] < got.hits()[2] < got.hits()[3]


def test_full_batch(eng):
    text, queries, modes, within = fuzz_case(11, nlines=300, nqueries=MAX_QUERIES)
    assert {"all", "any", "phrase", "near"} == set(modes)
    got = check(eng, text, queries, modes, within, first_line=7)
    nr = [h for h, m, q in zip(got.hits(), modes, queries) if m == "near" and len(q) > 1]
    assert got.queries == MAX_QUERIES and 0 in nr and sum(1 for h in nr if h) > 100


def test_sort_regimes():
    n = SMALL_SORT + 1
    text = b"v x w\n" * n
    engine = lc.Engine(gpu_cfg(), len(text), n)
    got = check(engine, text, [[b"w", b"v"]], "near", 3)  # one more than the LDS sort takes
    assert got.hits() == [n]
    got = check(engine, text, [[b"w", b"v"], [b"v", b"w"], [b"v"]], ["near", "near", "any"],
                [2, 3, None])
    assert got.hits() == [0, n, n]


# ------------------------------------------------------------------------------------
# prefix terms, ranking
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_with_prefix_terms_and_ranked(eng, seed):
    """Merged lists as candidates, the mask compare in verification, and the ranked path
    over the near answers."""
    for wild in (False, True):
        text, queries, modes, within = fuzz_case(seed, wildcard=wild)
        expect = want(text, queries, modes, within, first_line=5, wildcard=wild)
        got = check(eng, text, queries, modes, within, first_line=5, wildcard=wild, expect=expect)
        assert (got.merged > 0) == wild
        for k in (1, 3):
            r = eng.run_search(text, queries, modes, 5, rank=k, wildcard=wild, within=within)
            same_ranked(r, text, queries, expect, k, first_line=5, wildcard=wild)
        r = eng.search_resident(queries, modes, rank=W_MAX, wildcard=wild, within=within)
        same_ranked(r, text, queries, expect, W_MAX, first_line=5, wildcard=wild)


def test_one_token_for_two_terms(eng):
    text = b"Hamlet speaks\nHam and Hamlet\nHam\nhamlet Ham\n" * 40
    queries = [[b"Ham*", b"Hamlet"], [b"Ham*", b"Hamlet"], [b"Hamle*", b"Hamlet"],
               [b"H*", b"Ha*", b"Ham*"], [b"Ham*", b"and"]]
    got = check(eng, text, queries, "near", [1, 2, 1, 1, 2], wildcard=True)
    assert got.hits() == [80, 80, 80, 160, 40] and got.merged > 0


# ------------------------------------------------------------------------------------
# engine state
# ------------------------------------------------------------------------------------
def test_resident_and_stale(hamlet):
    win = oracle.window(hamlet, 0, 700)
    e = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    q1, q2 = [[b"my", b"lord"]], [[b"to", b"be"], [b"lord", b"my"], [b"my", b"lord"]]
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "near", within=2)
    e.run_search(win, q1, "all")
    same(e.search_resident(q2, "near", within=[2, 2, 3]), want(win, q2, "near", [2, 2, 3]))
    e.run_index(win, 50)
    got = e.search_resident(q2, ["near", "phrase", "all"], within=[4, None, None])
    same(got, want(win, q2, ["near", "phrase", "all"], [4, None, None], first_line=50))
    assert got.first_line == 50 and got.index_ms == 0 and got.search_ms > 0
    e.run(win)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "near", within=2)
    e.run_index(win)
    e.run_top(win, 5)
    with pytest.raises(lc.LocustError, match="stale"):
        e.search_resident(q1, "near", within=2)
    same(e.run_search(win, q1, "near", within=2), want(win, q1, "near", 2))
    # the window rules hold on the device engine too, and refuse before anything runs
    with pytest.raises(ValueError, match="within"):
        e.search_resident(q1, "near")
    with pytest.raises(ValueError, match="within"):
        e.search_resident(q1, "all", within=2)
    same(e.search_resident(q1, "near", within=2), want(win, q1, "near", 2))


# ------------------------------------------------------------------------------------
# whole Hamlet, the CLI
# ------------------------------------------------------------------------------------
HAMLET = [([b"to", b"be"], {2: 27, 3: 31, 4: 34, 5: 39, 8: 46, 20: 47}),
          ([b"my", b"lord"], {2: 110, 3: 115}),
          ([b"the", b"king"], {2: 3, 3: 5, 8: 7}),
          ([b"to", b"be", b"not"], {3: 2, 5: 4, 8: 6})]


def test_whole_hamlet(hamlet):
    lines = oracle.split_lines(hamlet)
    engine = lc.Engine(gpu_cfg(), len(hamlet), len(lines) + 1)
    queries = [q for q, ws in HAMLET for _w in ws] + [[b"to", b"be"]] * 2
    within = [w for _q, ws in HAMLET for w in ws] + [None, None]
    modes = ["near"] * (len(queries) - 2) + ["phrase", "all"]
    got = check(engine, hamlet, queries, modes, within)
    assert got.hits()[:-2] == [n for _q, ws in HAMLET for n in ws.values()]
    ph, al = set(got.lines(len(queries) - 2)), set(got.lines(len(queries) - 1))
    assert ph <= set(got.lines(0)) < set(got.lines(1)) < al == set(got.lines(5))
    assert got.wire_bytes < 4 * got.num_tokens  # less than the postings alone would be
    assert got.format() == oracle.format_search(queries, [got.lines(i) for i in range(len(queries))])


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_near(cli, hamlet, tmp_path):
    j = tmp_path / "near.json"
    p = subprocess.run([cli, "data/hamlet.txt", "--search", "be to", "--search", "lord my",
                        "--match", "near", "--within", "3", "--check", "--json", str(j)],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    queries = [[b"be", b"to"], [b"lord", b"my"]]
    expect = want(hamlet, queries, "near", 3)
    assert result_lines(p.stdout) == oracle.format_search(queries, [l for l, _c in expect])
    rec = json.load(open(j))
    assert rec["search"] is True and rec["queries"] == 2
    assert rec["hits"] == sum(len(l) for l, _c in expect) == 31 + 115
    assert rec["search_ms"] > 0 and rec["index_ms"] > 0
