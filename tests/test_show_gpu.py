"""The show stage on the device (csrc/kernels/show.hip): ``Engine.run_search(..., show=N)`` and
then ``Engine.search_resident`` against the oracle, exactly -- text, text_off, spans, span_off,
cut_lines -- and against a ``show=0`` run of the same batch for everything else.  The shapes are
the smallest at which the stage can go wrong: line lengths around the 64-byte step and the
96-byte row, tokens at and across the step edge and longer than the row, N around the step and
around the line's length, entry counts around the wave round (64) and past one round of the
grid, empty segments, every mask bit, every kind of term and every mode."""
import pytest

import locust_amd as lc
from tests.show_cases import (FUZZ_BATCHES, FUZZ_TEXTS, fuzz_batch, fuzz_expect, fuzz_text,
                              same_show, want_show, wire_bytes_of_show)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, queries, modes, n, k=None, first_line=0, within=None, exclude=None,
          glob=False, ignore_case=False, expect=None, **okw):
    """run_search, then search_resident, both with show=n against the oracle, and against the
    show=0 run of the same batch; wire_bytes grows by exactly what the stage copies."""
    if expect is None:
        expect = want_show(text, queries, modes, n, k, first_line, within, exclude, glob,
                           ignore_case, **okw)
    kw = dict(rank=k, within=within, exclude=exclude, glob=glob, ignore_case=ignore_case)
    got = engine.run_search(text, queries, modes, first_line, show=n, **kw)
    plain = engine.search_resident(queries, modes, **kw)
    same_show(got, expect, n, k, plain)
    again = engine.search_resident(queries, modes, show=n, **kw)
    same_show(again, expect, n, k, plain)
    assert again.wire_bytes == plain.wire_bytes + wire_bytes_of_show(again)
    assert again.show_ms > 0 or sum(again.hits()) == 0
    return again


LENGTHS = (1, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200)


def length_text(newline=True):
    """One line of every length in LENGTHS, each ending in the token `k` and (from 8 bytes on)
    starting with `hit`; a line holding a NUL; the last line with or without its newline."""
    lines = [(b"hit " + b"x" * n)[:n - 2] + b" k" if n >= 8 else b"k" * n for n in LENGTHS]
    assert [len(l) for l in lines] == list(LENGTHS)
    lines += [b"hit k\0 hit k", b"", b"x" * 70 + b" k"]
    return b"\n".join(lines) + (b"\n" if newline else b"")


@pytest.mark.parametrize("newline", [True, False])
def test_line_lengths(eng, newline):
    text = length_text(newline)
    queries = [[b"k"], [b"hit", b"k"], [b"x" * 29]]
    for n in (1, 63, 64, 65, 96, 128, 129, 65536):
        got = check(eng, text, queries, "any", n)
        assert got.hits()[0] == len(LENGTHS) + 2
    check(eng, text, queries, "any", 64, first_line=1000)
    check(eng, text, queries, "any", 64, k=3, first_line=1 << 31)


@pytest.mark.parametrize("length", [64, 97, 200])
def test_n_around_the_line_length(eng, length):
    text = (b"hit " + b"y" * length)[:length - 2] + b" k\nshort k\n"
    for n in (length - 1, length, length + 1):
        got = check(eng, text, [[b"k"], [b"hit"]], "all", n)
        assert got.cut_lines == (2 if n < length else 0)  # the long line, under both queries


def test_tokens_at_the_step_edge(eng):
    text = b"\n".join([
        b"y" * 62 + b" hit z",               # starts at byte 63
        b"y" * 63 + b" hit",                 # starts at byte 64
        b"y" * 60 + b" hit hit",             # one straddles the edge
        b"y" * 61 + b" hitter",              # a prefix match across the edge
        b"hit " + b"L" * 70 + b" z",         # 70 bytes: ends in the next step
        b"z " + b"M" * 130 + b" hit",        # 130 bytes: past the row, open over a whole step
        b"N" * 128,                          # a token that ends with the line at a step edge
        b"N" * 128 + b" hit",
        b"z " + b"N" * 126,
        b"hit " + b"M" * 200,                # a matching token open at the line's end
    ]) + b"\n"
    queries = [[b"hit*", b"L" * 70, b"M" * 130, b"N" * 128], [b"M*"], [b"hit"]]
    for n in (1, 64, 80, 65536):
        got = check(eng, text, queries, "any", n, glob=True)
    lens = sorted({l for s in got.spans(0) for _s, l, _m in s})
    assert lens == [3, 6, 70, 126, 128, 130, 200]
    check(eng, text, queries, "any", 80, glob=True, ignore_case=True)


def test_emit_cap_and_key_cut():
    text = b"a b c d hit\nhit a b c hit\nhit hit hit hit hit hit\n"
    capped = lc.Engine(gpu_cfg(emits_per_line=4), 1 << 16, 1 << 10)
    got = check(capped, text, [[b"hit"]], "any", 80, emits=4)
    assert got.lines(0) == [1, 2] and got.spans(0) == [[(0, 3, 1)], [(i * 4, 3, 1) for i in range(4)]]
    short = lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)
    got = check(short, b"the hamlets sing\nhamle hamlet\n", [[b"hamlet"], [b"ham*", b"hamlets"]],
                "all", 80, glob=True, max_key=5)
    assert got.spans(0)[0] == [(4, 7, 1)] and got.spans(1)[0] == [(4, 7, 3)]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 8193])  # (4096: the scan's tile)
def test_entry_counts_around_the_round(eng, count):
    text = b"".join(b"w%d hit w%d\n" % (i % 7, i) for i in range(count)) + b"none\n"
    got = check(eng, text, [[b"hit"]], "all", 80)
    assert got.hits() == [count]
    check(eng, text, [[b"hit"], [b"w3", b"hit"]], "all", 8, k=count)


def test_full_batch_and_empty_segments(eng):
    text = b"".join(b"w%d common w%d\n" % (i, i) for i in range(1024))
    queries = [[b"w%d" % i] for i in range(1024)]
    got = check(eng, text, queries, "all", 80)
    assert got.hits() == [1] * 1024 and got.spans(511) == [[(0, 4, 1), (12, 4, 1)]]
    # a query with zero hits between two with hits; the same line under two queries
    got = check(eng, text, [[b"w5", b"common"], [b"nosuch"], [b"common", b"w5"], [b"w7"]], "all", 80)
    assert got.hits() == [1, 0, 1, 1]
    assert got.spans(0) == [[(0, 2, 1), (3, 6, 2), (10, 2, 1)]]
    assert got.spans(2) == [[(0, 2, 2), (3, 6, 1), (10, 2, 2)]]
    check(eng, text, [[b"nosuch"], [b"nosuch2"]], "any", 80)  # nothing returned: nothing shown


def test_terms(eng, hamlet):
    words = [b"w%d" % i for i in range(8)]
    text = b" ".join(words) + b" w0\nw1 gone\nHamlet hamlet HAM ham hams\n"
    # eight positive terms: every mask bit; a repeated term: two bits; an absent term
    got = check(eng, text, [words, [b"w1", b"zz", b"w1"]], "any", 80)
    assert [m for _s, _l, m in got.spans(0)[0]] == [1, 2, 4, 8, 16, 32, 64, 128, 1]
    assert got.spans(1) == [[(3, 2, 5)], [(0, 2, 5)]]
    # nested prefix terms; a pattern term and a plain term on one token
    got = check(eng, text, [[b"h*", b"ha*", b"ham*", b"hams"], [b"h?m", b"ham", b"*s"]], "any", 80,
                glob=True)
    assert got.spans(0) == [[(7, 6, 7), (18, 3, 7), (22, 4, 15)]]
    assert got.spans(1) == [[(18, 3, 3), (22, 4, 4)]]
    # ignore_case with and without glob: the matcher siblings
    for glob in (False, True):
        got = check(eng, text, [[b"ham*" if glob else b"ham", b"HAMLET"]], "any", 80, glob=glob,
                    ignore_case=True)
        assert len(got.spans(0)[0]) == (5 if glob else 4)
    # exclusion terms never produce a span, and the lines they drop stay dropped
    got = check(eng, text, [[b"w1"], [b"w1"]], "all", 80, exclude=[[b"gone"], [b"w0", b"nosuch"]])
    assert got.lines(0) == [0] and got.lines(1) == [1] and got.spans(1) == [[(0, 2, 1)]]
    check(eng, hamlet, [[b"to", b"be"], [b"Ham*", b"*ing"]], "any", 80, glob=True,
          exclude=[[b"not"], None])


@pytest.mark.parametrize("mode", ["all", "any", "phrase", "near"])
def test_modes(eng, hamlet, mode):
    w = 3 if mode == "near" else None
    queries = [[b"to", b"be"], [b"my", b"lord"], [b"be", b"be"]]
    got = check(eng, hamlet, queries, mode, 80, within=w)
    assert got.hits()[0] > 3
    # rank=3 on a query with more than 3 matches: only the winners, in rank order
    got = check(eng, hamlet, queries, mode, 80, k=3, within=w)
    assert got.hits()[0] == 3 and len(got.text(0)) == 3 and got.matches()[0] > 3
    check(eng, hamlet, queries, mode, 4096, k=3, within=w, ignore_case=True)


def test_engine_state(eng, hamlet):
    queries = [[b"to", b"be"]]
    base, _shown = want_show(hamlet, queries, "phrase", 80)
    shown = eng.run_search(hamlet, queries, "phrase", show=80)
    plain = eng.search_resident(queries, "phrase")       # show=0 after a show batch
    assert plain.show_bytes == 0 and plain.text(0) == [] and plain.lines(0) == base[0][0]
    assert shown.wire_bytes >= plain.wire_bytes + wire_bytes_of_show(shown)
    eng.run_index(hamlet)                                # a show batch after run_index
    same_show(eng.search_resident(queries, "phrase", show=80),
              want_show(hamlet, queries, "phrase", 80), 80)
    # a refused show leaves the index resident: the next search_resident answers
    for bad in (65537, -1):
        with pytest.raises((lc.LocustError, TypeError)):
            eng.search_resident(queries, "phrase", show=bad)
    assert eng.search_resident(queries, "phrase").lines(0) == base[0][0]
    same_show(eng.search_resident(queries, "phrase", show=1),
              want_show(hamlet, queries, "phrase", 1), 1)
    with pytest.raises(lc.LocustError):
        eng.run_search(hamlet, queries, "phrase", show=1 << 20)
    assert eng.search_resident(queries, "phrase", show=None).lines(0) == base[0][0]


@pytest.mark.parametrize("text_seed", FUZZ_TEXTS)
def test_fuzz(eng, text_seed):
    text = fuzz_text(text_seed)
    first = (0, 17, 1 << 20)[text_seed % 3]
    eng.run_search(text, [[b"a"]], first_line=first)
    spans = cut = 0
    for seed in range(FUZZ_BATCHES):
        queries, modes, kw = fuzz_batch(seed, text_seed)
        n, k = kw.pop("show"), kw.pop("rank")
        expect = fuzz_expect(text_seed, seed, first)
        got = eng.search_resident(queries, modes, rank=k, show=n, **kw)
        plain = eng.search_resident(queries, modes, rank=k, **kw)
        same_show(got, expect, n, k, plain)
        assert got.wire_bytes == plain.wire_bytes + wire_bytes_of_show(got)
        spans += got.span_count
        cut += got.cut_lines
    assert spans > 100 and cut > 0
