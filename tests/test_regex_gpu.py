"""Regex terms on the device (csrc/kernels/regex.hip: the dictionary scan, the scatter, the verify
and the show kernels compiled with the position-automaton matcher of device/regex.hpp beside the
pattern and the fuzzy matcher; the engine's program table): ``search_file`` /
``Engine.run_search(..., regex=True)`` and ``Engine.run_index`` + ``search_resident`` against the
oracle's tree evaluation, exactly, ``merged`` included.  The shapes are the smallest at which each
part can go wrong: the matcher's edges (keys at the packed words' boundaries, bytes of 0x80 and
above, the padding, alternation a greedy matcher gets wrong, nested stars, empty branches, nullable
expressions, 32 positions, the classes' and the fold's edges, max_key_len 31), dictionaries around
the scan's tile (256) with a term of one word (its list in place), of dozens and of hundreds
(merged), eight regex terms in one query, every kind of term in one phrase and one near query,
exclusion and ``expr``, ``show`` with spans, 1,024 distinct programs in one batch and the batches
behind it, and the issue's table over the whole of Hamlet."""
import os

import pytest

import locust_amd as lc
from tests import regex_cases as rc
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
          glob=False, ignore_case=False, wildcard=False, fuzzy=False, show=None, regex=True,
          **okw):
    """Every answer twice, against the oracle, ``merged`` too: through run_search, and again
    through run_index + search_resident (``show`` on the second path)."""
    expect = rc.want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case,
                     wildcard, fuzzy, regex, **okw)
    x = rc.merged(text, queries, modes, first_line, exclude, glob, ignore_case, wildcard, fuzzy,
                  regex, **okw)
    kw = dict(rank=k, within=within, exclude=exclude, glob=glob, ignore_case=ignore_case,
              wildcard=wildcard, fuzzy=fuzzy, regex=regex)
    got = engine.run_search(text, queries, modes, first_line, **kw)
    rc.same(got, expect, k)
    assert got.merged == x and got.first_line == first_line
    engine.run_index(text, first_line)
    again = engine.search_resident(queries, modes, **kw)
    rc.same(again, expect, k)
    assert again.merged == x
    if show:
        shown = rc.want_show(text, queries, modes, show, k, first_line, within, exclude, glob,
                             ignore_case, wildcard, fuzzy, regex, **okw)
        same_show(engine.search_resident(queries, modes, show=show, **kw), shown, show, k, again)
    return again


# ------------------------------------------------------------------------------------
# the matcher and the fold
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("k", [None, 3])
def test_matcher_edges(eng, fold, k, tmp_path):
    text = rc.edge_text()
    queries = [[t] for t in rc.edge_terms()]
    expect = rc.want(text, queries, "all", k, ignore_case=fold)
    # through search_file ...
    path = tmp_path / "edges.txt"
    path.write_bytes(text)
    got = lc.search_file(str(path), queries, "all", cfg=gpu_cfg(), rank=k, regex=True,
                         ignore_case=fold)
    rc.same(got, expect, k)
    assert got.merged == rc.merged(text, queries, ignore_case=fold) and got.merged > 0
    assert 0 in got.matches() and max(got.matches()) >= 8
    # ... and through run_index + search_resident
    check(eng, text, queries, "all", k, ignore_case=fold, show=None if k else 40)
    if k is None:
        # eight to a query: every term slot; and before `pad` as phrases and near queries: the
        # verify kernels' matcher sees every key
        terms = list(rc.edge_terms())
        packs = [terms[i:i + 8] for i in range(0, len(terms), 8)]
        check(eng, text, packs, "any", ignore_case=fold)
        two = [[t, b"pad"] for t in terms]
        check(eng, text, two, "phrase", ignore_case=fold)
        check(eng, text, two, "near", within=2, ignore_case=fold)


def test_matcher_edges_max_key_31():
    engine = lc.Engine(gpu_cfg(max_key_len=31), 1 << 18, 1 << 12)
    text = rc.edge_text(31)
    queries = [[t] for t in rc.edge_terms(31)]
    for fold in (False, True):
        got = check(engine, text, queries, "all", ignore_case=fold, max_key=31)
        assert max(got.hits()) >= 8
        check(engine, text, queries, "all", 3, ignore_case=fold, max_key=31)
    check(engine, text, [[t, b"pad"] for t in rc.edge_terms(31)], "phrase", max_key=31)


def test_patterns_that_fill_their_map_beside_regex_terms():
    """A 31-byte pattern and a 30-byte prefix under the fold use bit 30 of their maps: they are
    pattern slots whatever the batch holds, with and without the keyword."""
    engine = lc.Engine(gpu_cfg(max_key_len=31), 1 << 18, 1 << 12)
    text, _pattern, _prefix, (alone, beside) = rc.full_map_case()
    for fold in (False, True):
        for queries, regex in ((alone, False), (alone, True), (beside, True)):
            got = check(engine, text, queries, "all", glob=True, ignore_case=fold, regex=regex,
                        max_key=31, show=40)
            check(engine, text, queries, "any", 3, glob=True, ignore_case=fold, regex=regex,
                  max_key=31)
            check(engine, text, queries, "phrase", glob=True, ignore_case=fold, regex=regex,
                  max_key=31)
            # kkk...k, kkk...z and the longer word cut to 31 bytes; under the fold KKK...Z too
            assert got.hits()[0] == (4 if fold else 3) and got.hits()[1] >= got.hits()[0]


# ------------------------------------------------------------------------------------
# the dictionary scan: sizes around the tile; one word, dozens, hundreds
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_dictionary_sizes(eng, n):
    text = rc.tile_text(n)
    last = b"w%04d" % (n - 1)
    queries = [[b"/w0003/"], [b"/" + last + b"/"], [b"/w00[0-4]./"], [b"/w0.*/"], [b"/w[0-9]+/"],
               [b"/w0?2[0-9]+/"], [b"/x.*/"], [b"/w0(25[5-9]|51[0-9])/"]]
    got = check(eng, text, queries, "all", first_line=1000)
    # one word: its list in place; dozens and hundreds: merged
    assert got.term_counts(0) == [2] and got.term_counts(1) == [2]
    assert got.term_counts(2) == [100] and got.term_counts(4) == [2 * n] and got.hits()[6] == 0
    assert got.merged == sum(got.term_counts(i)[0] for i in (2, 3, 4, 5, 7)
                             if got.term_counts(i)[0] > 2)
    check(eng, text, queries, "any", 4, first_line=1000)


# ------------------------------------------------------------------------------------
# every slot; every kind of term in one query; exclusion and expr; show
# ------------------------------------------------------------------------------------
MIX = (b"ham hamlet ham* ha\nhamlet hamlets the\nha ha\nthe ham king!\nhamper the hamlet\n"
       b"hum h thy\nHam THE hem\nthe hem kong\nhim tha kin\n(my) lord! the queen?\n"
       b"my lordship a king\n")


def test_eight_regex_terms_in_one_query(eng):
    q = [[b"/ha.*/", b"/the|tha/", b"/h[aeiou]m/", b"/k[io]ng?!?/", b"/(ham)?let.?/", b"/[A-Z]+/",
          b"/.*\\*/", b"/lord(ship)?[!?]*/"]]
    for fold in (False, True):
        got = check(eng, MIX, q * 2, ["any", "all"], ignore_case=fold, show=24)
        check(eng, MIX, q, "any", 3, ignore_case=fold)
    assert got.hits()[0] >= 9


def test_every_kind_of_term_in_one_query(eng):
    queries = [[b"/th[ae]/", b"h?m", b"king~1"], [b"my", b"/lord.*/", b"th*"],
               [b"ha*", b"/ham(let)?s?/", b"the", b"ham~1"], [b"/h.m/", b"t?e", b"hem~1", b"k*", b"the"]]
    for fold in (False, True):
        kw = dict(glob=True, fuzzy=True, ignore_case=fold)
        got = check(eng, MIX, queries, "phrase", show=16, **kw)
        near = check(eng, MIX, queries, "near", within=3, show=16, **kw)
        check(eng, MIX, queries, "near", 3, within=3, **kw)
    assert sum(got.hits()) >= 2 and sum(near.hits()) > sum(got.hits())


def test_exclusion_and_expr(eng):
    queries = [[b"/ham.*/", b"the"], [b"/h.m/"], [b"( /(king|kong)!?/ AND NOT /ham|hem/ ) OR lord!"],
               [b"/(my)|(\\(my\\))/ AND (/lord(ship)?!?/ OR /a|b/)"]]
    modes = ["all", "any", "expr", "expr"]
    exclude = [[b"/ham(per|lets)/"], [b"/th./", b"/H.*/"], None, None]
    for fold in (False, True):
        got = check(eng, MIX, queries, modes, exclude=exclude, ignore_case=fold, show=24)
        check(eng, MIX, queries, modes, 2, exclude=exclude, ignore_case=fold)
    assert got.hits()[2] >= 2 and got.hits()[3] == 2


def test_show_spans_of_a_phrase_with_a_regex(eng):
    text = MIX * 3
    got = check(eng, text, [[b"the", b"/h[ae]m(let)?/"], [b"my", b"/lord(ship)?!?/"]], "phrase",
                show=40, first_line=5)
    assert got.hits() == [9, 6]
    assert all(len(s) >= 2 for s in got.spans(0))


# ------------------------------------------------------------------------------------
# the program table: 1,024 programs, then 3, then batches without one
# ------------------------------------------------------------------------------------
def test_a_full_batch_of_programs_and_the_batches_behind_it(eng):
    text = rc.tile_text(513)
    plain = [[b"w0001"], [b"w00*", b"w0002"], [b"w?003"]]
    before = eng.run_search(text, plain, "any", 3, glob=True, show=16)
    full = [[b"/w%04d?[0-9]?/" % i] for i in range(1024)]  # 1,024 distinct sources
    got = check(eng, text, full, "all", first_line=3)
    assert got.merged > 0 and got.hits()[0] == 20 and got.hits()[1023] == 0
    few = check(eng, text, [[b"/w000[1-3]/"], [b"/w0001/", b"/w0001/"], [b"/w051[0-2]/"]], "any",
                first_line=3)
    assert few.hits() == [6, 2, 6]
    # the regex routing is per batch: the batches behind it answer as before, pattern terms by
    # the pattern kernels, fuzzy terms by the fuzzy kernels, plain terms without any
    after = eng.search_resident(plain, "any", glob=True, show=16)
    assert after.merged == before.merged
    for i in range(3):
        assert after.lines(i) == before.lines(i) and after.term_counts(i) == before.term_counts(i)
        assert after.text(i) == before.text(i) and after.spans(i) == before.spans(i)
    fuzzy = eng.search_resident([[b"w0001~1"]], fuzzy=True)
    assert fuzzy.term_counts(0) == [2 * 24]  # itself; w0[1-5]01, w00[^0]1, w000[^1]: 1 + 5 + 9 + 9
    bare = eng.search_resident([[b"w0001"], [b"/w0001/"]])
    assert bare.hits() == [2, 0]  # without the keyword the slashes are bytes of a word
    # regex=True without a regex term is no regex batch either
    same = eng.search_resident(plain, "any", glob=True, regex=True)
    assert [same.lines(i) for i in range(3)] == [before.lines(i) for i in range(3)]


# ------------------------------------------------------------------------------------
# the whole of Hamlet: the issue's table
# ------------------------------------------------------------------------------------
def test_hamlet(hamlet, tmp_path):
    queries = [[t] for t, _p, _f in rc.HAMLET]
    path = os.path.join(ROOT, "data", "hamlet.txt")
    for fold in (False, True):
        expect = rc.want(hamlet, queries, "all", ignore_case=fold)
        got = lc.search_file(path, queries, "all", cfg=gpu_cfg(), regex=True, ignore_case=fold)
        rc.same(got, expect)
        assert got.merged == rc.merged(hamlet, queries, ignore_case=fold)
        for i, (_t, plain, folded) in enumerate(rc.HAMLET):
            _words, npost, nlines = folded if fold else plain
            assert got.term_counts(i) == [npost] and got.hits()[i] == nlines
    ranked = lc.search_file(path, queries, "all", cfg=gpu_cfg(), regex=True, rank=5)
    rc.same(ranked, rc.want(hamlet, queries, "all", 5), 5)
    # ham* beside /Ham.*/ in one batch, under the fold: equal answers
    both = lc.search_file(path, [[b"ham*"], [b"/Ham.*/"]], "all", cfg=gpu_cfg(), regex=True,
                          wildcard=True, ignore_case=True)
    assert both.lines(0) == both.lines(1) and both.hits() == [470, 470]
    assert both.term_counts(0) == both.term_counts(1) == [476]
