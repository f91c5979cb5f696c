"""The tally stage on the device (csrc/kernels/tally.hip): ``Engine.run_search(..., tally=K)``
and then ``Engine.search_resident`` against the oracle, exactly -- every query's words,
tally_words, tally_tokens and the batch's ``tallied`` -- and against a run of the same batch
without tally for everything else.  The shapes are the smallest at which each part can go wrong:
returned lines around the wave's round (64), line lengths and tokens around the 64-byte step and
the look-ahead row, the emit cap, pair words and runs around ``kSmallSortMax`` (8192) for either
sort, a run longer than a sort tile, one-word and two-word dictionaries, every selection edge.

A returned line holds at least the token that matched, so "empty lines among the returned ones"
are empty lines between them in the text (the line numbers skip) and lines whose tokens end at a
NUL right behind the match."""
import pytest

import locust_amd as lc
from tests.tally_cases import OPTS, lines_of_words, same, want, wire_bytes_of_tally, word
from tests.test_tally import HAMLET

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for every case."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, queries, modes, tally, k=None, first_line=0, within=None, exclude=None,
          expect=None, **okw):
    """run_search, then search_resident, both with tally against the oracle, and against the run
    of the same batch without tally; wire_bytes grows by exactly what the stage copies."""
    if expect is None:
        expect = want(text, queries, modes, tally, k, first_line, within, exclude, **okw)
    opts = {key: v for key, v in okw.items() if key in OPTS}  # (the rest: the engine's own job)
    kw = dict(rank=k, within=within, exclude=exclude, **opts)
    got = engine.run_search(text, queries, modes, first_line, tally=tally, **kw)
    same(got, expect, tally, k, device=True)
    plain = engine.search_resident(queries, modes, **kw)
    again = engine.search_resident(queries, modes, tally=tally, **kw)
    same(again, expect, tally, k, device=True)
    assert plain.tally_k == 0 and plain.tally_words() == [] and plain.tallied == 0
    assert plain.tally_ms == 0
    for i in range(again.queries):
        assert plain.lines(i) == again.lines(i) and plain.scores(i) == again.scores(i), i
        assert plain.tally(i) == []
    assert again.wire_bytes == plain.wire_bytes + wire_bytes_of_tally(again)
    assert again.tally_ms > 0 or sum(again.hits()) == 0
    return again


# ---- the walk ----

@pytest.mark.parametrize("lines", [1, 63, 64, 65, 130])
def test_returned_lines_around_the_wave_round(eng, lines):
    text = b"".join(b"hit %s %s\n\n" % (word(i % 9), word(i)) for i in range(lines))
    got = check(eng, text, [[b"hit"], [word(3)]], "all", 5)
    assert got.hits()[0] == lines and got.tally_tokens()[0] == 3 * lines


@pytest.mark.parametrize("newline", [True, False])
def test_line_lengths_and_step_edges(eng, newline):
    rows = [
        (b"hit " + b"x" * 64)[:62] + b" k",          # exactly 64 bytes
        (b"hit " + b"x" * 64)[:63] + b" k",          # 65
        (b"hit " + b"x" * 128)[:126] + b" k",        # 128
        b"y" * 60 + b" hit hit",                     # a token that straddles the step
        b"y" * 60 + b" hit",                         # one that ends at it
        b"y" * 63 + b" hit",                         # one that starts the next step
        b"y" * 59 + b" " + b"K" * 29 + b" hit",      # a 29-byte key from byte 60: the look-ahead
        b"y" * 59 + b" " + b"K" * 40 + b" hit",      # ... cut to 29 bytes, merged with that one
        b"hit " + b"M" * 130 + b" z",                # a token longer than the row
        b"",
        b"hit k\0 hit hidden",                       # a NUL mid-line
        b"hit\0",                                    # nothing behind the match
        b"",
        b" ,.- ",                                    # delimiters only
        b"hit " + b"a" * 29 + b" " + b"a" * 30 + b" " + b"a" * 35 + b"X",  # three tokens, one key
        b"x" * 70 + b" hit k",                       # the last line
    ]
    text = b"\n".join(rows) + (b"\n" if newline else b"")
    queries = [[b"hit"], [b"k"], [b"K" * 29], [b"a" * 29]]
    got = check(eng, text, queries, "all", 8)
    assert dict(got.tally(0))[b"K" * 29] == 2 and dict(got.tally(3))[b"a" * 29] == 3
    check(eng, text, queries, "all", 3, first_line=1000)
    check(eng, text, queries, "any", 4096, k=3, first_line=1 << 31)


def test_the_emit_cap(eng):
    rows = [b" ".join([b"hit"] + [word(i) for i in range(n - 1)]) for n in (19, 20, 21, 40)]
    rows.append(b" ".join([word(i) for i in range(25)] + [b"hit"]))  # the match past the cap
    text = b"\n".join(rows) + b"\n"
    got = check(eng, text, [[b"hit"]], "all", 30)
    assert got.hits() == [4] and got.tally_tokens() == [19 + 20 + 20 + 20]
    # another job: its own delimiters, cap and key cut
    cfg = dict(emits_per_line=3, max_key_len=2, delimiters=" x\t")
    small = lc.Engine(gpu_cfg(**cfg), 1 << 16, 1 << 10)
    check(small, text, [[b"hi"], [b"wa"]], "any", 6, emits=3, max_key=2, delims=b" x\t")


# ---- the sorts and the runs ----

@pytest.mark.parametrize("tokens", [8191, 8192, 8193])
def test_pair_words_around_the_small_sort(eng, tokens):
    last = b" ".join([b"hit", b"a", b"b", b"c", b"d"][:tokens - 8188])
    text = b"hit a b c\n" * 2047 + last + b"\n"
    got = check(eng, text, [[b"hit"]], "all", 4)
    assert got.tallied == tokens


@pytest.mark.parametrize("runs", [8191, 8192, 8193])
def test_runs_around_the_small_sort(eng, runs):
    text = lines_of_words(runs - 1, 12)
    got = check(eng, text, [[b"hit"]], "all", 7)
    assert got.tally_words() == [runs]


def test_a_run_longer_than_a_sort_tile(eng):
    text = b"".join(b"the %s\n" % word(i % 7) for i in range(5000))
    got = check(eng, text, [[b"the"], [word(2)]], "all", 3)
    assert got.tally(0)[0] == (b"the", 5000) and got.tallied == 10000 + 2 * len(range(2, 5000, 7))


def test_one_count_of_ten_thousand(eng):
    text = (b" ".join([b"a"] * 20) + b"\n") * 500
    got = check(eng, text, [[b"a"]], "all", 2)
    assert got.tally(0) == [(b"a", 10000)] and got.tally_words() == [1]


@pytest.mark.parametrize("words", [1, 2, 4097])
def test_dictionary_sizes(eng, words):
    text = {1: b"hit\nhit hit\n", 2: b"hit b\nb\nhit\n"}.get(words) or lines_of_words(4096, 16)
    got = check(eng, text, [[b"hit"]], "all", 5)
    assert got.num_unique == words


# ---- the selection ----

def test_ties_and_k(eng):
    text = b"hit b a c\nhit c b\nhit zz\n"
    for k, top in ((1, [(b"hit", 3)]), (2, [(b"hit", 3), (b"b", 2)]),
                   (5, [(b"hit", 3), (b"b", 2), (b"c", 2), (b"a", 1), (b"zz", 1)]),
                   (9, [(b"hit", 3), (b"b", 2), (b"c", 2), (b"a", 1), (b"zz", 1)])):
        got = check(eng, text, [[b"hit"]], "all", k)
        assert got.tally(0) == top and got.tally_words() == [5]


def test_k_4096_over_4100_words(eng):
    text = lines_of_words(4099, 16)
    got = check(eng, text, [[b"hit"]], "all", 4096)
    assert got.tally_words() == [4100] and len(got.tally(0)) == 4096


def test_queries_without_a_hit_and_shared_lines(eng):
    text = b"to be or\nnot to be\nthat is\n\nthe question\n"
    queries = [[b"nosuch"], [b"to"], [b"zz"], [b"be"], [b"to", b"be"], [b"qq"], [b"is"], [b"none"]]
    got = check(eng, text, queries, "all", 3)
    assert got.tally(1) == got.tally(3) == got.tally(4) and got.tally_words()[0] == 0
    # nothing returned at all: nothing launched, an empty answer
    none = check(eng, text, [[b"nosuch"], [b"zz"]], "all", 3)
    assert none.tallied == 0 and none.tally_ms == 0 and none.tally_words() == [0, 0]


def test_a_full_batch(eng):
    text = b"".join(b"%s %s both\n" % (word(i), word(i % 16)) for i in range(256))
    queries = [[word(i % 256)] if i % 5 else [b"both"] for i in range(1024)]
    got = check(eng, text, queries, "all", 2)
    assert got.tally_words()[0] == 256 + 1 and got.queries == 1024


# ---- with the other features ----

def test_ranked_tallies_the_winners_only(eng, hamlet):
    q = [[b"to", b"be"]]
    ranked = check(eng, hamlet[:1 << 17], q, "any", 6, k=5)
    unranked = check(eng, hamlet[:1 << 17], q, "any", 6)
    assert ranked.tally_tokens()[0] < unranked.tally_tokens()[0]
    assert ranked.tally(0) != unranked.tally(0)


def test_with_show_the_payload_is_untouched(eng, hamlet):
    text = hamlet[:1 << 16]
    queries = [[b"to", b"be"], [b"the"]]
    for k in (None, 3):
        first = eng.run_search(text, queries, "any", rank=k, show=40, tally=4)
        same(first, want(text, queries, "any", 4, k), 4, k, device=True)
        shown = eng.search_resident(queries, "any", rank=k, show=40)
        both = eng.search_resident(queries, "any", rank=k, show=40, tally=4)
        same(both, want(text, queries, "any", 4, k), 4, k, device=True)
        for i in range(2):
            assert both.text(i) == shown.text(i) and both.spans(i) == shown.spans(i)
        assert both.text_off() == shown.text_off() and both.span_off() == shown.span_off()
        assert both.cut_lines == shown.cut_lines
        assert both.wire_bytes == shown.wire_bytes + wire_bytes_of_tally(both)
        assert both.format(mark=True).count(b"  words: ") == 2


@pytest.mark.parametrize("mode", ["all", "any", "phrase", "near"])
def test_each_mode_with_exclusion(eng, hamlet, mode):
    text = hamlet[:1 << 17]
    queries = [[b"to", b"be"], [b"my", b"lord"], [b"the", b"king"]]
    exclude = [None, [b"good"], [b"of"]]
    check(eng, text, queries, mode, 5, within=3 if mode == "near" else None, exclude=exclude)


def test_a_pattern_batch(eng, hamlet):
    text = hamlet[:1 << 16]
    got = check(eng, text, [[b"?o"], [b"ham*"], [b"/(king|queen)/"]], "any", 4096, glob=True,
                ignore_case=True, regex=True)
    assert {b"To", b"to"} <= {key for key, _c in got.tally(0)}  # tallied apart under the fold


# ---- residency and regression ----

def test_plain_and_tally_batches_alternate(eng, hamlet):
    text = hamlet[:1 << 16]
    queries = [[b"to", b"be"], [b"Hamlet"]]
    expect = want(text, queries, "all", 4)
    eng.run_search(text, queries, "all")
    first = eng.search_resident(queries, "all")               # before any tally of this text
    t = eng.search_resident(queries, "all", tally=4)
    same(t, expect, 4, device=True)
    plain = eng.search_resident(queries, "all")               # a plain batch behind a tally batch
    assert plain.wire_bytes == first.wire_bytes
    assert plain.format() == first.format() and plain.tally_k == 0
    for i in range(2):
        assert plain.lines(i) == expect[0][i][0] and plain.term_counts(i) == expect[0][i][2]
    same(eng.search_resident(queries, "all", tally=4), expect, 4, device=True)


def test_the_workspace_grows(eng, hamlet):
    fresh = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    check(fresh, hamlet[:1 << 12], [[b"to"]], "all", 3)
    check(fresh, hamlet, [[b"the"], [b"to"], [b"and"]], "any", 50)
    check(fresh, hamlet[:1 << 12], [[b"to"]], "all", 3)


def test_a_refused_batch_leaves_the_index_resident(eng, hamlet):
    text = hamlet[:1 << 16]
    queries = [[b"to", b"be"]]
    eng.run_search(text, queries, "all", tally=3)
    for bad in (4097, -1):
        with pytest.raises(lc.LocustError, match="tally"):
            eng.search_resident(queries, "all", tally=bad)
    same(eng.search_resident(queries, "all", tally=3), want(text, queries, "all", 3), 3,
         device=True)
    with pytest.raises(lc.LocustError, match="tally"):
        eng.run_search(text, queries, "all", tally=4097)      # refused before it starts anything
    same(eng.search_resident(queries, "all", tally=3), want(text, queries, "all", 3), 3,
         device=True)


# ---- real data ----

def test_hamlet_figures(eng, hamlet):
    for q, mode, k, returned, words, tokens, top in HAMLET:
        tally = len(top) or 6
        got = check(eng, hamlet, [q], mode, tally, k)
        assert got.hits() == [returned] and got.tally(0) == top, q
        assert (got.tally_words(), got.tally_tokens(), got.tallied) == ([words], [tokens], tokens)
