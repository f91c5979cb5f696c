"""Fuzzy terms on the device (csrc/kernels/fuzzy.hip: the dictionary scan, the scatter, the
verify and the show kernels compiled with the banded matcher of device/fuzzy.hpp beside the
pattern matcher): ``search_file`` / ``Engine.run_search(..., fuzzy=True)`` and ``Engine.run_index``
+ ``search_resident`` against the oracle's full-matrix distance, exactly, ``merged`` included.
The shapes are the smallest at which each part can go wrong: the matcher's edges (edits at the
first and last byte and at the packed words' boundaries, the length filter's edges, bytes of
0x80 and above, the fold's edges, a word of max_key_len bytes), dictionaries around the scan's
tile (256), a term of one word (its list in place), of dozens and of hundreds (merged), fuzzy,
pattern and prefix terms in one phrase and one near query, a plain batch behind a fuzzy one,
and the README's queries over the whole of Hamlet."""
import functools
import os

import pytest

import locust_amd as lc
from tests import fuzzy_cases as fc
from tests.show_cases import same_show

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def check(engine, text, queries, modes, k=None, first_line=0, within=None, exclude=None,
          glob=False, ignore_case=False, wildcard=False, show=None, index_first=False, **okw):
    """run_search (or run_index), then search_resident, both against the oracle; ``merged`` too."""
    expect = fc.want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case,
                     wildcard, **okw)
    x = fc.merged(text, queries, first_line, exclude, glob, ignore_case, wildcard, **okw)
    kw = dict(rank=k, within=within, exclude=exclude, glob=glob, ignore_case=ignore_case,
              wildcard=wildcard, fuzzy=True)
    if index_first:
        engine.run_index(text, first_line)
    else:
        got = engine.run_search(text, queries, modes, first_line, **kw)
        fc.same(got, expect, k)
        assert got.merged == x and got.first_line == first_line
    again = engine.search_resident(queries, modes, **kw)
    fc.same(again, expect, k)
    assert again.merged == x
    if show:
        shown = fc.want_show(text, queries, modes, show, k, first_line, within, exclude, glob,
                             ignore_case, wildcard, **okw)
        same_show(engine.search_resident(queries, modes, show=show, **kw), shown, show, k, again)
    return again


# ------------------------------------------------------------------------------------
# the matcher and the fold
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("k", [None, 3])
def test_matcher_edges(eng, fold, k, tmp_path):
    text = fc.edge_text()
    queries = [[t] for t in fc.edge_terms()]
    expect = fc.want(text, queries, "all", k, ignore_case=fold)
    # through search_file ...
    path = tmp_path / "edges.txt"
    path.write_bytes(text)
    got = lc.search_file(str(path), queries, "all", cfg=gpu_cfg(), rank=k, fuzzy=True,
                         ignore_case=fold)
    fc.same(got, expect, k)
    assert got.merged == fc.merged(text, queries, ignore_case=fold) and got.merged > 0
    assert 0 in got.matches() and max(got.matches()) >= 8
    # ... and through run_index + search_resident
    check(eng, text, queries, "all", k, ignore_case=fold, index_first=True,
          show=None if k else 40)
    if k is None:
        # eight to a query: every term slot; and behind `pad` as phrases and near queries: the
        # verify kernels' matcher sees every key
        terms = list(fc.edge_terms())
        packs = [terms[i:i + 8] for i in range(0, len(terms), 8)]
        check(eng, text, packs, "any", ignore_case=fold)
        two = [[t, b"pad"] for t in terms] + [[b"pod~1", b"pad~1"], [b"pa~1"]]
        check(eng, text, two, "phrase", ignore_case=fold)
        check(eng, text, two, "near", within=2, ignore_case=fold)


def test_matcher_edges_max_key_31():
    engine = lc.Engine(gpu_cfg(max_key_len=31), 1 << 18, 1 << 12)
    text = fc.edge_text(31)
    queries = [[t] for t in fc.edge_terms(31)]
    for fold in (False, True):
        got = check(engine, text, queries, "all", ignore_case=fold, max_key=31)
        assert max(got.hits()) >= 8
    check(engine, text, [[t, b"pad"] for t in fc.edge_terms(31)], "phrase", max_key=31)


# ------------------------------------------------------------------------------------
# fuzz
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz(eng, seed):
    text, queries, modes, within, exclude = fc.fuzz_case(seed)
    assert set(modes) == {"all", "any", "phrase", "near"} and any(exclude)
    for fold in (False, True):
        check(eng, text, queries, modes, None, 3, within, exclude, True, fold, show=16)
        check(eng, text, queries, modes, 3, 3, within, exclude, True, fold)


# ------------------------------------------------------------------------------------
# the dictionary scan: sizes around the tile; one word, dozens, hundreds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_dictionary_sizes(eng, n):
    text = fc.tile_text(n)
    mid = b"w%04d" % min(500, n - 1)
    last = b"w%04d" % (n - 1)
    queries = [[mid + b"~1"], [mid + b"~2"], [b"w0000~1"], [last + b"~1"], [b"x0000~1"],
               [b"w00~2"], [b"zzzzzzz~2"]]
    got = check(eng, text, queries, "all")
    if n == 1:
        # one word: its list in place, nothing merged; and an absent term
        assert got.merged == 0 and got.term_counts(0) == [2] and got.term_counts(4) == [2]
        assert got.term_counts(5) == [2] and got.hits()[6] == 0  # w00 + two bytes; no word
    else:
        assert got.merged > 0 and got.hits()[6] == 0
    if n == 1000:
        # w0500~1: one of the last three digits replaced; w0500~2: two of them
        assert got.term_counts(0) == [2 * (1 + 9 * 3)]
        assert got.term_counts(1) == [2 * (1 + 9 * 3 + 81 * 3)]
    check(eng, text, queries, "any", 4)


# ------------------------------------------------------------------------------------
# all three kinds of term in one query; a plain batch behind a fuzzy one
# ------------------------------------------------------------------------------------
MIX = (b"ham hamlet ham* ha\nhamlet hamlets the\nha ha\nthe ham king\nhamper the hamlet\n"
       b"hum h thy\nHam THE hem\nthe hem kong\nhim tha kin\n")


def test_fuzzy_pattern_and_prefix_terms_in_one_query(eng):
    queries = [[b"the", b"hem~1", b"k?ng"], [b"ha*", b"th?", b"hamlet~2"],
               [b"t?e", b"ham~1", b"ki*"], [b"hamlets~1", b"ham*", b"*e"],
               [b"h?m", b"h*", b"hum~2"], [b"ham~1", b"ham~2", b"ha*", b"h?"]]
    for fold in (False, True):
        kw = dict(glob=True, ignore_case=fold)
        got = check(eng, MIX, queries, "phrase", show=16, **kw)
        near = check(eng, MIX, queries, "near", within=2, show=16, **kw)
        check(eng, MIX, queries, "near", 3, within=2, **kw)
        check(eng, MIX, queries, ["all", "any"] * 3, 3,
              exclude=[[b"hamper~1"], None, [b"k?n"], None, None, [b"thy~1"]], **kw)
    assert got.hits()[0] >= 2 and sum(near.hits()) > sum(got.hits())


def test_a_plain_batch_behind_a_fuzzy_batch(eng):
    plain = [[b"ham"], [b"ha*", b"the"], [b"the", b"ham"], [b"h?m", b"the"]]
    modes = ["all", "all", "phrase", "any"]
    before = eng.run_search(MIX, plain, modes, 11, glob=True, show=16)
    fuzzy = check(eng, MIX, [[b"ham~1"], [b"the", b"hem~1"]], ["all", "phrase"], first_line=11)
    assert fuzzy.merged > 0
    # the fuzzy routing is per batch: the batches behind it answer as before, pattern terms by the
    # pattern kernels, and a batch without patterns without any
    after = eng.search_resident(plain, modes, glob=True, show=16)
    bare = eng.search_resident(plain[:3], modes[:3], wildcard=True)
    assert after.merged == before.merged
    for i in range(4):
        assert after.lines(i) == before.lines(i) and after.term_counts(i) == before.term_counts(i)
        assert after.text(i) == before.text(i) and after.spans(i) == before.spans(i)
    for i in range(3):
        assert bare.lines(i) == before.lines(i) and bare.term_counts(i) == before.term_counts(i)
    # fuzzy=True without a fuzzy term is no fuzzy batch either
    same = eng.search_resident(plain, modes, glob=True, fuzzy=True)
    assert [same.lines(i) for i in range(4)] == [before.lines(i) for i in range(4)]
    # ... and a literal ~1 stays literal without the keyword
    assert eng.search_resident([[b"ham~1"]]).hits() == [0]


# ------------------------------------------------------------------------------------
# the whole of Hamlet: the README's queries
# ------------------------------------------------------------------------------------
HAMLET_TERMS = [[b"Hamlet~1"], [b"lord~1"], [b"be~1"], [b"quene~2"]]


@functools.lru_cache(maxsize=None)
def hamlet_expect(mode, fold):
    text = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    return fc.want(text, HAMLET_TERMS + [[b"hamlet~1"]], mode, ignore_case=fold)


def test_hamlet(hamlet):
    engine = lc.Engine(gpu_cfg(), len(hamlet), hamlet.count(b"\n") + 1)
    got = engine.run_search(hamlet, HAMLET_TERMS + [[b"hamlet~1"]], "all", fuzzy=True)
    fc.same(got, hamlet_expect("all", False))
    assert got.hits()[:4] == [108, 235, 822, 41] and got.merged > 0  # the README's counts
    assert got.term_counts(0) == [113] and got.term_counts(2) == [958]
    fc.same(engine.search_resident(HAMLET_TERMS + [[b"hamlet~1"]], "any", fuzzy=True),
            hamlet_expect("any", False))
    folded = engine.search_resident(HAMLET_TERMS + [[b"hamlet~1"]], "all", fuzzy=True,
                                    ignore_case=True)
    fc.same(folded, hamlet_expect("all", True))
    assert folded.hits()[4] == 112
    # all four in one query, both ways
    both = [sum(HAMLET_TERMS, [])] * 2
    fc.same(engine.search_resident(both, ["all", "any"], fuzzy=True),
            fc.want(hamlet, both, ["all", "any"]))
    # my lord~1 as a phrase, shown
    shown = fc.want_show(hamlet, [[b"my", b"lord~1"]], "phrase", 80)
    got = engine.search_resident([[b"my", b"lord~1"]], "phrase", fuzzy=True, show=80)
    same_show(got, shown, 80)
    assert got.hits()[0] > 100
