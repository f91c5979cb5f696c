"""Regex terms (``regex``: ``/(king|queen)[!?]?/``) without a GPU: how terms are read and refused,
the compiled program and the shared matcher (through the host evaluation and the CPU engine)
against the oracle's tree evaluation on the edge text, both against the oracle in every mode,
ranked and not, with ``show``, exclusion terms, ``glob``, ``fuzzy`` and ``ignore_case`` beside
them, the oracle itself against Python's ``re`` on seeded random expressions, the CLI's ``--regex
--backend cpu``, and the issue's Hamlet counts.  Every comparison is exact; ``check=True`` runs
``validate_search`` on every result."""
import json
import os
import random
import re
import subprocess

import pytest

import locust_amd as lc
from locust_amd import _C
from locust_amd.utils import oracle
from tests import regex_cases as rc
from tests.show_cases import formatted_show, same_show

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def check(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=False,
          ignore_case=False, wildcard=False, fuzzy=False, show=None, **okw):
    """The CPU engine's run_search, and for all/any/expr the host evaluation over the index."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ckw = {"max_key_len": okw["max_key"]} if "max_key" in okw else {}
    expect = rc.want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case,
                     wildcard, fuzzy, **okw)
    eng = cpu_engine(text, **ckw)
    gkw = dict(rank=k, glob=glob, ignore_case=ignore_case, wildcard=wildcard, fuzzy=fuzzy,
               regex=True)
    got = eng.run_search(text, queries, modes, first_line, within=within, exclude=exclude, **gkw)
    rc.same(got, expect, k)
    assert got.merged == 0  # the host evaluation merges nothing on a device
    keep = [i for i, m in enumerate(modes) if m in ("all", "any", "expr")]
    idx = eng.run_index(text, first_line).search(
        [queries[i] for i in keep], [modes[i] for i in keep],
        exclude=[exclude[i] for i in keep] if exclude else None, **gkw)
    rc.same(idx, [expect[i] for i in keep], k)
    if show:
        shown = rc.want_show(text, queries, modes, show, k, first_line, within, exclude, glob,
                             ignore_case, wildcard, fuzzy, **okw)
        got = eng.run_search(text, queries, modes, first_line, within=within, exclude=exclude,
                             show=show, **gkw)
        same_show(got, shown, show, k)
    return got


# ------------------------------------------------------------------------------------
# reading and refusing
# ------------------------------------------------------------------------------------
def test_reading_a_term():
    read = lambda terms, **kw: _C.make_search_query(terms, **kw)
    assert read([b"/x/"]) == [(b"/x/", "plain")]  # without regex: the literal word
    assert read([b"/x/"], glob=True, fuzzy=True, wildcard=True) == [(b"/x/", "plain")]
    assert read([b"/x/", b"x", b"x/"], regex=True) == [(b"x", "regex"), (b"x", "plain"),
                                                        (b"x/", "plain")]
    # nothing inside the slashes is read by the other readings, and regex implies none of them
    assert read([b"/ab~1/", b"/a*/", b"/h?m/", b"/ham*/"], regex=True, glob=True, fuzzy=True,
                wildcard=True) == [(b"ab~1", "regex"), (b"a*", "regex"), (b"h?m", "regex"),
                                   (b"ham*", "regex")]
    assert read([b"ab~1", b"h?m", b"ha*"], regex=True) == [(b"ab~1", "plain"), (b"h?m", "plain"),
                                                           (b"ha*", "plain")]
    assert read([b"ab~1", b"h?m", b"/a/"], regex=True, glob=True, fuzzy=True) == [
        (b"ab", "fuzzy"), (b"h?m", "pattern"), (b"a", "regex")]
    # an escaped slash is a literal slash; an escaped backslash before the closing slash is not
    assert read([b"/a\\/b/", b"/a\\\\/"], regex=True) == [(b"a\\/b", "regex"), (b"a\\\\", "regex")]
    # the oracle reads the same
    kinds = [t.kind for t in oracle.query_terms([b"/ab~1/", b"ab~1", b"/x/", b"h?m"], glob=True,
                                                fuzzy=True, regex=True)]
    assert kinds == ["regex", "fuzzy", "regex", "pattern"]
    assert oracle.query_terms([b"/x/"])[0].kind == "plain"


@pytest.mark.parametrize("term, msg", rc.REFUSED, ids=[str(i) for i in range(len(rc.REFUSED))])
def test_refusals(term, msg):
    with pytest.raises(lc.LocustError) as e:
        _C.make_search_query([term], regex=True)
    assert msg in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        oracle.query_terms([term], regex=True)
    # the engines refuse it too, whatever else is on
    eng = cpu_engine(b"a b\n")
    with pytest.raises(lc.LocustError) as e:
        eng.run_search(b"a b\n", [[b"a", term]], "any", regex=True, glob=True, fuzzy=True)
    assert msg in str(e.value)


def test_accepted_edges_of_the_syntax():
    for term in rc.ACCEPTED:
        assert _C.make_search_query([term], regex=True) == [(term[1:-1], "regex")], term
        assert oracle.query_terms([term], regex=True)[0].kind == "regex"
    assert _C.kRegexMaxDepth == 32 and _C.kRegexMaxSource == 128 and _C.kRegexMaxPos == 32
    assert (oracle.REGEX_MAX_DEPTH, oracle.REGEX_MAX_SOURCE, oracle.REGEX_MAX_POS) == (32, 128, 32)


def test_the_compiled_program():
    """device/regex.hpp's layout: first, last, nullable, positions, follow[32], B[256]."""
    p = _C.compile_regex(b"(a|ab)(c|bcd)")
    assert len(p) == 292
    first, last, nullable, npos = p[:4]
    follow, B = p[4:36], p[36:]
    # positions: a0 a1 b2 c3 b4 c5 d6
    assert (first, last, nullable, npos) == (0b11, 0b1001000, 0, 7)
    assert follow[:7] == [0b11000, 0b100, 0b11000, 0, 0b100000, 0b1000000, 0]
    assert B[ord("a")] == 0b11 and B[ord("b")] == 0b10100 and B[ord("c")] == 0b101000
    assert B[ord("d")] == 0b1000000 and B[0] == 0 and B[ord("A")] == 0
    assert _C.compile_regex(b"(a|)")[:4] == [1, 1, 1, 1]
    assert _C.compile_regex(b"()")[:4] == [0, 0, 1, 0]
    # the fold is compiled in: a set is closed under the case swap before the negation
    f = _C.compile_regex(b"[^a]b", True)[36:]
    assert f[ord("a")] == 0 and f[ord("A")] == 0 and f[ord("b")] == 0b11 and f[ord("B")] == 0b11
    assert f[ord("@")] == 1 and f[0] == 0
    dot = _C.compile_regex(b".")[36:]
    assert dot[0] == 0 and all(dot[c] == 1 for c in range(1, 256))


# ------------------------------------------------------------------------------------
# the matcher, against the oracle
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_key", [29, 31])
def test_matcher_edges_against_the_oracle(max_key):
    text = rc.edge_text(max_key)
    queries = [[t] for t in rc.edge_terms(max_key)]
    for fold in (False, True):
        got = check(text, queries, "all", ignore_case=fold, max_key=max_key)
        assert 0 in got.hits() and max(got.hits()) >= 8
    check(text, queries, "all", 3, max_key=max_key)
    two = [[t, b"pad"] for t in rc.edge_terms(max_key)]
    check(text, two, "phrase", max_key=max_key, show=40)
    check(text, two, "near", within=2, ignore_case=True, max_key=max_key)


def test_patterns_that_fill_their_map_beside_regex_terms():
    """A 31-byte pattern and a 30-byte prefix under the fold use bit 30 of their maps: they are
    pattern terms whatever the batch holds, with and without the keyword."""
    text, pattern, _prefix, (alone, beside) = rc.full_map_case()
    eng = cpu_engine(text, max_key_len=31)
    for fold in (False, True):
        for queries, regex in ((alone, False), (alone, True), (beside, True)):
            for mode, k in (("all", None), ("any", 3), ("phrase", None)):
                expect = rc.want(text, queries, mode, k, glob=True, ignore_case=fold, regex=regex,
                                 max_key=31)
                got = eng.run_search(text, queries, mode, rank=k, glob=True, ignore_case=fold,
                                     regex=regex)
                rc.same(got, expect, k)
                if mode != "phrase":
                    idx = eng.run_index(text).search(queries, mode, rank=k, glob=True,
                                                     ignore_case=fold, regex=regex)
                    rc.same(idx, expect, k)
            # kkk...k, kkk...z and the longer word cut to 31 bytes; under the fold KKK...Z too
            assert got.matches()[0] == (4 if fold else 3) and got.matches()[1] >= got.matches()[0]
    assert _C.make_search_query([pattern], glob=True, regex=True) == [(pattern, "pattern")]


def test_matcher_edges_by_hand():
    text = rc.edge_text()
    keys = rc.edge_keys()
    eng = cpu_engine(text)

    def words(term, fold=False):
        got = eng.run_search(text, [[term]], "all", regex=True, ignore_case=fold)
        return [keys[l] for l in got.lines(0)]

    assert words(b"/ab./") == [b"abc", b"abd"]  # never the padding: not `ab`
    assert words(b"/(a|ab)(c|bcd)/") == [b"abc", b"abcd", b"ac"]
    assert words(b"/(a*)*b/") == [b"b", b"ab", b"aab", b"aaab"]
    assert words(b"/(a|)b/") == [b"b", b"ab"]
    assert words(b"/a*/") == [b"a", b"aaaa"] and words(b"/()/") == []
    assert words(b"/[a-a]/") == [b"a"] and words(b"/[-a]/") == [b"a"] and words(b"/[a-]/") == [b"a"]
    assert words(b"/[\\]]/") == [b"]"]
    assert b"^" not in words(b"/[^^]/") and b"]" in words(b"/[^^]/")
    assert words(b"/[^a]/", True) == [k for k in keys if len(k) == 1 and k not in (b"a", b"A")]
    assert words(b"/@a\\[/", True) == [b"@a[", b"@A["] and words(b"/`a\\{/", True) == [b"`A{", b"`a{"]
    assert words(b"/[\x80-\xff]+/") == [b"\x80", b"\xff", b"\xff\xff", b"\xc3\xa9"]
    assert words(b"/a[^\x80]b/") == [b"aab", b"a\xffb", b"a/b"]
    # 32 positions: the last one decides
    assert words(b"/" + b"k?" * 31 + b"z/") == [k for k in keys if re.fullmatch(b"k{0,31}z", k[:29])]
    assert words(b"/" + b"k" * 28 + b"./") == [b"k" * 29, b"k" * 28 + b"z", b"k" * 35]


# ------------------------------------------------------------------------------------
# the oracle itself, against Python's re
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dictionaries(hamlet):
    ent, _post = oracle.index(hamlet)
    return [k for k, _v, _c in ent], list(rc.edge_keys())


@pytest.mark.parametrize("fold", [False, True])
def test_oracle_against_re(dictionaries, fold):
    ham, edge = dictionaries
    rng = random.Random(20261 + fold)
    alphabets = [b"abAB", b"kzKZ", b"ab[!", b"a\x80\xffb", b"HamletHl!?[]"]
    done = 0
    for i in range(340):
        alphabet = alphabets[i % len(alphabets)]
        if fold:  # letters and digits only, where both definitions agree by construction
            alphabet = bytes(c for c in alphabet if bytes([c]).isalnum() and c < 0x80) + b"k1"
        src = rc.random_regex(rng, alphabet, fold)
        try:
            tree = oracle.regex_parse(src)
        except ValueError as e:  # (only the position budget: the generator writes legal syntax)
            assert "positions" in str(e), (src, e)
            continue
        rx = re.compile(src, re.DOTALL | (re.IGNORECASE if fold else 0))
        for key in ham[i % 16::16] + edge:  # (every key of Hamlet meets 20 expressions or more)
            assert oracle.regex_fits(tree, key, fold) == (rx.fullmatch(key) is not None), (src, key)
        # ... and the engines' compiled program says the same of the edge keys
        text = b"".join(k + b"\n" for k in edge)
        got = cpu_engine(text).run_search(text, [[b"/" + src.replace(b"/", b"\\/") + b"/"]], "all",
                                          regex=True, ignore_case=fold)
        assert [edge[l] for l in got.lines(0)] == [k for k in edge if rx.fullmatch(k[:29])], src
        done += 1
    assert done >= 300


# ------------------------------------------------------------------------------------
# every mode, exclusion, rank, show, the fold; identity
# ------------------------------------------------------------------------------------
TEXT = (b"the king! and the queen\n"      # 0
        b"King Hamlet, my lord\n"         # 1
        b"[Hamlet Hamlet? Hamlet]\n"      # 2
        b"my lordship! the QUEEN a king\n"  # 3
        b"mylord lord! LORD a\n"          # 4
        b"unseeing and inspired the king\n"  # 5
        b"a /x/ b 42 !?\n")               # 6
QUERIES = [[b"/(king|queen)[!?]?/", b"the"], [b"/\\[?Hamlet[!?\\]]?/"], [b"my", b"/lord(ship)?!?/"],
           [b"/[A-Z][A-Z]+/", b"/[^a-zA-Z]+/"], [b"/(un|in)[a-z]+(ed|ing)/", b"/.*ing/", b"and"],
           [b"/the|a/", b"/(my)?lord/", b"/the|a/"], [b"/x/", b"/\\/x\\//"], [b"/nosuch+/", b"the"]]


@pytest.mark.parametrize("k", [None, 3])
def test_cpu_all_modes(k):
    for fold in (False, True):
        for mode in ("all", "any"):
            check(TEXT, QUERIES, mode, k, first_line=7, ignore_case=fold, show=None if k else 24)
        check(TEXT, QUERIES, "phrase", k, ignore_case=fold, show=40)
        check(TEXT, QUERIES, "near", k, within=3, ignore_case=fold)
    # exclusion terms that are regex terms; a mixed batch of every kind
    check(TEXT, QUERIES[:4], ["all", "any", "all", "any"], k,
          exclude=[[b"/qu.*/"], [b"/\\[.*/"], None, [b"/[0-9]+/", b"the"]], show=24)
    mixed = [[b"/k[a-z]+!?/", b"th?", b"hamlet~1", b"lord*", b"my"], [b"the", b"/quee?n/"]]
    for mode in ("all", "any", "phrase", "near"):
        check(TEXT, mixed, mode, k, within=4 if mode == "near" else None, glob=True, fuzzy=True,
              ignore_case=True, show=30)


def test_expr_mode():
    exprs = [[b"( /(king|queen)[!?]?/ AND NOT /the|a/ ) OR lord"], [b"/a b/ OR (/(my)?lord/ my)"],
             [b"(/[A-Z]+/ OR /(un|in).*/)AND NOT /k.*/"], [b"/the|a/ AND /the|a/ AND NOT /a|the/"]]
    for fold in (False, True):
        check(TEXT, exprs, "expr", ignore_case=fold, show=24)
        check(TEXT, exprs, "expr", 2, ignore_case=fold)
    d = _C.make_search_expr(lc.make_config("cpu"), exprs[0][0], regex=True)
    assert d["terms"] == [b"(king|queen)[!?]?", b"the|a", b"lord"]
    assert d["kinds"] == ["regex", "regex", "plain"] and d["expr"] == exprs[0][0]
    d = _C.make_search_expr(lc.make_config("cpu"), b"  /a  b/   OR\t( /a  b/ x )", regex=True)
    assert d["terms"] == [b"a  b", b"x"] and d["expr"] == b"/a  b/ OR ( /a  b/ x )"
    assert oracle.expr_text(b"  /a  b/   OR\t( /a  b/ x )", True) == d["expr"]
    # without regex the slashes are bytes of a word, and ( ) | split as ever
    d = _C.make_search_expr(lc.make_config("cpu"), b"/a/ OR b")
    assert d["kinds"] == ["plain", "plain"] and d["terms"] == [b"/a/", b"b"]
    for bad, msg in [(b"/ab OR c", "no closing /"), (b"/ab/c OR d", "followed by"),
                     (b"/a**/ OR d", "quantifier")]:
        with pytest.raises(lc.LocustError, match=msg):
            _C.make_search_expr(lc.make_config("cpu"), bad, regex=True)
        with pytest.raises(ValueError):
            oracle.expr_parse(bad, regex=True)


def test_identity_and_scores():
    """Equal sources are one term (counted once in a score, no second list); different sources
    with the same words are two; a regex term is never a term of another kind."""
    text = b"ham ham hem\nham\nhem hem\n"
    eng = cpu_engine(text)
    q = [[b"/ham/", b"/ham/"], [b"/ham/", b"/h[a]m/"], [b"/ham/", b"ham"], [b"/HAM/", b"/ham/"]]
    for fold in (False, True):
        expect = rc.want(text, q, "any", 5, ignore_case=fold)
        got = eng.run_search(text, q, "any", rank=5, regex=True, ignore_case=fold)
        rc.same(got, expect, 5)
    assert got.scores(0)[0] * 2 == got.scores(1)[0] == got.scores(2)[0] == got.scores(3)[0]


# ------------------------------------------------------------------------------------
# the CLI and the Hamlet table
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


@pytest.fixture(scope="module")
def hamlet_index(hamlet):
    return oracle.index(hamlet)


@pytest.mark.parametrize("row", rc.HAMLET, ids=[str(i) for i in range(len(rc.HAMLET))])
def test_hamlet_counts(hamlet, hamlet_index, row):
    term, plain, folded = row
    ent, post = hamlet_index
    eng = cpu_engine(hamlet)
    for fold, (nwords, npost, nlines) in ((False, plain), (True, folded)):
        rx = re.compile(term[1:-1], re.DOTALL | (re.IGNORECASE if fold else 0))
        words = [k for k, _v, _c in ent if rx.fullmatch(k)]
        qt, = oracle.query_terms([term], regex=True, ignore_case=fold)
        assert [k for k, _v, _c in ent if qt.fits(k)] == words and len(words) == nwords
        lines, counts = oracle.search(ent, post, [term], "all", regex=True, ignore_case=fold)
        assert (counts, len(lines)) == ([npost], nlines)
        got = eng.run_search(hamlet, [[term]], "all", regex=True, ignore_case=fold)
        assert got.lines(0) == lines and got.term_counts(0) == [npost]
    if plain[2]:  # the README states the count next to the query
        readme = open(os.path.join(ROOT, "README.md"), "rb").read()
        at = readme.find(b"--search '%s' --regex" % term)
        assert at >= 0, term
        assert (b"%d lines" % plain[2]) in readme[at:at + 300], term


def test_hamlet_equivalences(hamlet):
    eng = cpu_engine(hamlet)
    pairs = [(b"/.*ing/", b"*ing", False), (b"/Ham.*/", b"Ham*", False), (b"/Ham.*/", b"Ham*", True),
             (b"/h.ml.*t/", b"h?ml*t", True), (b"/\\[?Hamlet[!?\\]]?/", b"Hamlet~1", False)]
    for rx, other, fold in pairs:
        got = eng.run_search(hamlet, [[rx], [other]], "all", regex=True, glob=True, fuzzy=True,
                             ignore_case=fold)
        assert got.lines(0) == got.lines(1) and got.hits()[0] > 0, (rx, other)


def test_cli_cpu_regex(cli, hamlet, tmp_path):
    queries = [[b"/\\[?Hamlet[!?\\]]?/", b"my"], [b"/(king|queen)[!?]?/", b"/the|a/"],
               [b"/[A-Z][A-Z]+/"], [b"/a b,c/", b"lord"]]
    exclude = [None, [b"/qu.*/"], None, None]
    args = ["--search", "/\\[?Hamlet[!?\\]]?/ my", "--search", "/(king|queen)[!?]?/,/the|a/",
            "--not", "/qu.*/", "--search", "/[A-Z][A-Z]+/", "--search", "/a b,c/ lord"]
    for mode in ("all", "any", "phrase", "near"):
        extra = ["--within", 3] if mode == "near" else []
        w = 3 if mode == "near" else None
        for fold in (False, True):
            flags = ["--regex"] + (["--ignore-case"] if fold else [])
            p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, *flags,
                    "--check", *extra)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            expect = rc.want(hamlet, queries, mode, within=w, exclude=exclude, ignore_case=fold)
            assert result_lines(p.stdout) == rc.formatted(queries, expect, exclude=exclude)
            assert sum(m for _a, m, _c in expect) > 0
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--regex",
                "--rank", 4, "--check", *extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = rc.want(hamlet, queries, mode, 4, within=w, exclude=exclude)
        assert result_lines(p.stdout) == rc.formatted(queries, expect, 4, exclude)
    # --show --mark: the whole output, by the oracle
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "/\\[?Hamlet[!?\\]]?/ my",
            "--match", "any", "--regex", "--show", 80, "--mark", "--check")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    shown = rc.want_show(hamlet, queries[:1], "any", 80)
    want_out = formatted_show(queries[:1], shown, mark=True)
    assert want_out in p.stdout and b">>[Hamlet<<" in want_out
    # --match expr: the issue's example
    e = b"( /(king|queen)[!?]?/ AND NOT /the|a/ ) OR lord"
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", e.decode(), "--match", "expr",
            "--regex", "--check", "--json", tmp_path / "out.json")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    expect = rc.want(hamlet, [[e]], "expr")
    assert result_lines(p.stdout) == rc.formatted([[e]], expect) and expect[0][1] > 0
    assert json.loads((tmp_path / "out.json").read_text())["regex"] is True
    # without --regex the slashes are literal bytes of a word
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "/x/")
    assert p.returncode == 0
    assert result_lines(p.stdout) == b"print query: /x/ \t hits: 0 \t lines:\n"


@pytest.mark.parametrize("args, msg", [
    (["--regex"], "--search"),
    (["--regex", "--index"], "--search"),
    (["--regex", "--search", "/ab"], "no closing /"),
    (["--regex", "--search", "to /ab/c"], "delimiter or the end"),
    (["--regex", "--search", "//"], "no regex term"),
    (["--regex", "--search", "/a**/"], "quantifier"),
    (["--regex", "--search", "/a{2}/"], "unescaped {"),
    (["--regex", "--search", "/\\d+/"], "reserved"),
    (["--regex", "--search", "/" + "a" * 33 + "/"], "kRegexMaxPos"),
    (["--regex", "--search", "/ham/", "--rank", 2, "--emits-per-line", 8193], "8192"),
    (["--regex", "--match", "expr", "--search", "/ab OR c"], "no closing /"),
])
def test_cli_regex_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr, p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--regex" in p.stdout
