"""Fuzzy terms (``fuzzy``: ``Hamlet~1``, ``quene~2``) without a GPU: how terms are read and
refused, the shared banded matcher (through the host evaluation and the CPU engine) against the
oracle's full-matrix distance on the edge text, both against the oracle in all four modes,
ranked and not, with ``show``, exclusion terms, ``glob`` and ``ignore_case`` beside them, the
CLI's ``--fuzzy --backend cpu``, and the README's counts.  Every comparison is exact;
``check=True`` runs ``validate_search`` on every result."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests import fuzzy_cases as fc
from tests.show_cases import formatted_show, same_show

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def check(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=False,
          ignore_case=False, wildcard=False, show=None, **okw):
    """The CPU engine's run_search, and for all/any the host evaluation over the index."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ckw = {"max_key_len": okw["max_key"]} if "max_key" in okw else {}
    expect = fc.want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case,
                     wildcard, **okw)
    eng = cpu_engine(text, **ckw)
    gkw = dict(rank=k, glob=glob, ignore_case=ignore_case, wildcard=wildcard, fuzzy=True)
    got = eng.run_search(text, queries, modes, first_line, within=within, exclude=exclude, **gkw)
    fc.same(got, expect, k)
    assert got.merged == 0  # the host evaluation merges nothing on a device
    assert got.format() == fc.formatted(queries, expect, k, exclude, glob)
    keep = [i for i, m in enumerate(modes) if m in ("all", "any")]
    idx = eng.run_index(text, first_line).search(
        [queries[i] for i in keep], [modes[i] for i in keep],
        exclude=[exclude[i] for i in keep] if exclude else None, **gkw)
    fc.same(idx, [expect[i] for i in keep], k)
    if show:
        shown = fc.want_show(text, queries, modes, show, k, first_line, within, exclude, glob,
                             ignore_case, wildcard, **okw)
        got = eng.run_search(text, queries, modes, first_line, within=within, exclude=exclude,
                             show=show, **gkw)
        same_show(got, shown, show, k)
    return got


TEXT = (b"ham Hamlet ham~1 ha\n"     # 0
        b"hamlet hamlets HAM\n"      # 1
        b"ha ha sing\n"              # 2
        b"the hem king\n"            # 3
        b"hamper the Hamlet! a*b\n"  # 4
        b"hum h ring [Hamlet\n")     # 5


def test_reading_a_term():
    kinds = lambda terms, **kw: [(t.kind, t.p, t.d) for t in oracle.query_terms(terms, **kw)]
    assert kinds([b"ham~1", b"ham~2", b"ham"], fuzzy=True) == [
        ("fuzzy", b"ham", 1), ("fuzzy", b"ham", 2), ("plain", b"ham", 0)]
    # a ~ anywhere else is a literal byte of its word
    literal = [b"ham~", b"ham~12", b"h~1m", b"~1", b"ham~x", b"~~"]
    assert [k for k, _p, _d in kinds(literal, fuzzy=True)] == ["plain"] * len(literal)
    # without fuzzy, the suffix is literal too
    assert kinds([b"ham~1"]) == [("plain", b"ham~1", 0)]
    # the fuzzy reading comes before the wildcard and glob reading
    assert [k for k, _p, _d in kinds([b"ham~1", b"ha*", b"h?m"], fuzzy=True, glob=True)] == [
        "fuzzy", "prefix", "pattern"]
    # without wildcard or glob a star in the word is a literal byte
    assert kinds([b"a*b~1"], fuzzy=True) == [("fuzzy", b"a*b", 1)]
    eng = cpu_engine(TEXT)
    got = eng.run_search(TEXT, [[b"ham~1"], [b"ham~2"], [b"Hamlet~1"], [b"a*b~1"]], fuzzy=True)
    # ham, ha x 3, hem, hum; not HAM, not h, not ham~1
    assert got.term_counts(0) == [6] and got.lines(0) == [0, 2, 3, 5]
    assert got.term_counts(1) == [8] and got.lines(1) == [0, 2, 3, 5]  # ... and h and ham~1
    # Hamlet, hamlet, Hamlet!, [Hamlet; not hamlets
    assert got.lines(2) == [0, 1, 4, 5] and got.term_counts(2) == [4]
    assert got.lines(3) == [4] and got.term_counts(3) == [1]
    assert got.format().startswith(b"print query: ham~1 \t hits: 4 \t lines: 0 2 3 5\n")
    # without fuzzy, ham~1 is the literal word it has always been
    plain = eng.run_search(TEXT, [[b"ham~1"]])
    assert plain.lines(0) == [0] and plain.term_counts(0) == [1]
    assert plain.format() == b"print query: ham~1 \t hits: 1 \t lines: 0\n"
    lit = eng.run_search(TEXT, [[b"ham~1"]], fuzzy=False, glob=True, ignore_case=True)
    assert lit.lines(0) == [0]
    # ignore_case folds ASCII letters of the word and the key
    got = eng.run_search(TEXT, [[b"ham~1"], [b"HAMLET~1"]], fuzzy=True, ignore_case=True)
    assert got.term_counts(0) == [7] and got.lines(0) == [0, 1, 2, 3, 5]  # ... and HAM
    assert got.term_counts(1) == [5]  # Hamlet hamlet hamlets Hamlet! [Hamlet


def test_refusals():
    eng = cpu_engine(TEXT)
    cases = (([b"ham~0"], "1 or 2"), ([b"ham~3"], "1 or 2"), ([b"ham~9"], "1 or 2"),
             ([b"a~1"], "longer than its budget"), ([b"ab~2"], "longer than its budget"),
             ([b"~~1"], "longer than its budget"),
             ([b"a" * 30 + b"~1"], "never cut"), ([b"a b~1"], "delimiter"),
             ([b"a,b~2"], "delimiter"), ([b"a\nb~1"], "newline"))
    for q, msg in cases:
        for call in (lambda: eng.run_search(TEXT, [q], fuzzy=True),
                     lambda: eng.run_index(TEXT).search([q], fuzzy=True),
                     lambda: lc.search_text(TEXT, [q], backend="cpu", fuzzy=True),
                     lambda: eng.run_search(TEXT, [[b"ham"]], exclude=[q], fuzzy=True)):
            with pytest.raises(lc.LocustError, match=msg):
                call()
        with pytest.raises(ValueError):
            oracle.query_terms(q, fuzzy=True)
    # fuzzy or a pattern, never both: only when wildcard or glob is on
    for kw in (dict(glob=True), dict(wildcard=True), dict(glob=True, wildcard=True)):
        for q in ([b"h*m~1"], [b"h?m~2"], [b"ham*~1"]):
            with pytest.raises(lc.LocustError, match="never both"):
                eng.run_search(TEXT, [q], fuzzy=True, **kw)
            with pytest.raises(ValueError):
                oracle.query_terms(q, fuzzy=True, **kw)
    # a word of exactly max_key_len bytes is legal; a shorter key length refuses sooner
    assert eng.run_search(TEXT, [[b"a" * 29 + b"~2"]], fuzzy=True).hits() == [0]
    short = cpu_engine(TEXT, max_key_len=5)
    assert short.run_search(TEXT, [[b"hamle~1"]], fuzzy=True).term_counts(0) == [5]  # cut keys
    with pytest.raises(lc.LocustError, match="never cut"):
        short.run_search(TEXT, [[b"hamlet~1"]], fuzzy=True)
    # ranked: a fuzzy term is a pattern term -- emits_per_line <= kRankMaxEmits / 8
    big = cpu_engine(TEXT, emits_per_line=8193)
    with pytest.raises(lc.LocustError, match="8192"):
        big.run_search(TEXT, [[b"ham~1"]], rank=3, fuzzy=True)
    with pytest.raises(lc.LocustError, match="8192"):
        big.run_index(TEXT).search([[b"ham~1"]], rank=3, fuzzy=True)
    assert big.run_search(TEXT, [[b"ham~1"]], rank=3).matches() == [1]  # literal: no such limit
    assert big.run_search(TEXT, [[b"ham~1"]], fuzzy=True).hits() == [4]  # unranked: none either
    assert cpu_engine(TEXT, emits_per_line=8192).run_search(
        TEXT, [[b"ham~1"]], rank=3, fuzzy=True).matches() == [4]
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.rank(ent, post, [0], [b"ham~1"], 3, fuzzy=True, emits=8193)
    oracle.rank(ent, post, [0], [b"ham~1"], 3, emits=8193)


@pytest.mark.parametrize("max_key", [29, 31])
def test_matcher_edges_against_the_oracle(max_key):
    text = fc.edge_text(max_key)
    keys, terms = fc.edge_keys(max_key), fc.edge_terms(max_key)
    assert len(keys) == len(set(keys))
    okw = {} if max_key == 29 else {"max_key": max_key}
    queries = [[t] for t in terms]
    for fold in (False, True):
        got = check(text, queries, "all", ignore_case=fold, show=40, **okw)
        hits = got.hits()
        assert 0 not in hits[:2 * len(fc.EDGE_LENGTHS)] and max(hits) >= 8
    # the list is worth its name: every word has keys at exactly d and at exactly d + 1, the
    # length filter's edges among them
    for t in terms[:2 * (len(fc.EDGE_LENGTHS) + (max_key - 29))]:
        w, d = t[:-2], t[-1] - 0x30
        dist = fc.edge_distances(t, max_key)
        assert d in dist and d + 1 in dist, t
        at = {(dd, len(k[:max_key]) - len(w)) for dd, k in zip(dist, keys)}
        edges = {(d, -d), (d + 1, -(d + 1))}  # (no key is longer than max_key)
        edges |= {(dd, dd) for dd in (d, d + 1) if len(w) + dd <= max_key}
        assert edges <= at, t
    # 0x80 and 0xff stand in keys one edit away from a word
    near = [k for k in keys if oracle.levenshtein(fc.edge_word(8), k) == 1]
    assert any(0x80 in k for k in near) or any(0xff in k for k in near)
    assert any(0x80 in k or 0xff in k for k in keys if len(k) == 9 and
               oracle.levenshtein(fc.edge_word(8), k) == 1)
    # fold edges: @ ` [ { do not fold, letters do
    assert oracle.levenshtein(b"@a[", b"`A{") == 3 and oracle.levenshtein(b"@a[", b"`A{", True) == 2
    eng = cpu_engine(text, **({"max_key_len": max_key} if max_key != 29 else {}))
    for fold, n2, nab in ((False, 3, 3), (True, 5, 4)):
        got = eng.run_search(text, [[b"@a[~2"], [b"ab~1"]], fuzzy=True, ignore_case=fold)
        # @a[~2: @a[ a A ... (and, folded, `a{ `A{); ab~1: ab Ab aB a abc ... (folded: AB too)
        ent, _p = oracle.index(text, **okw)
        for i, t in enumerate((b"@a[~2", b"ab~1")):
            qt, = oracle.query_terms([t], fuzzy=True, ignore_case=fold, **okw)
            words = {k for k, _v, _c in ent if qt.fits(k)}
            # (@a[~2 covers the pad word of every line, too)
            assert got.term_counts(i) == [sum(c for k, _v, c in ent if k in words)]
            if i == 0:
                assert ({b"`A{", b"`a{"} <= words) == fold and {b"@a[", b"a"} <= words
            else:
                assert (b"AB" in words) == fold and {b"ab", b"Ab", b"aB", b"a", b"abc"} <= words
    # the long word is matched as its merged key
    got = eng.run_search(text, [[b"m" * (max_key - 1) + b"x~1"]], fuzzy=True)
    assert got.term_counts(0) == [2]  # m * (max_key + 6), cut; and m * (max_key - 1) + n


@pytest.mark.parametrize("k", [None, 3])
def test_cpu_all_modes_by_hand(k):
    queries = [[b"ham~1"], [b"Hamlet~1", b"the"], [b"ham~2", b"h?m*"], [b"the", b"hem~1"],
               [b"hamlet~2", b"ha*"], [b"ham~1", b"ham~1"], [b"ham~1", b"ham~2"], [b"zzz~1"],
               [b"ham", b"zzz~2"], [b"ham~1", b"ham"], [b"ha*", b"hum~1"], [b"ring~2", b"h"]]
    modes = ["all", "all", "any", "phrase", "near", "all", "any", "any", "all", "all",
             "phrase", "near"]
    within = [None, None, None, None, 2, None, None, None, None, None, None, 3]
    exclude = [None, [b"kind~1"], [b"sang~1"], None, None, [b"zzz~2"], None, None, None,
               [b"hamper~2"], None, None]
    for fold in (False, True):
        got = check(TEXT, queries, modes, k, within=within, exclude=exclude, glob=True,
                    ignore_case=fold, show=16)
        assert sum(got.matches()) > 0
        check(TEXT, queries, modes, k, first_line=7, within=within, glob=True, ignore_case=fold)
    check(TEXT, [[b"hamle~1", b"hem~1"], [b"hamle~2"], [b"the", b"hum~1"]],
          ["all", "any", "phrase"], k, ignore_case=True, max_key=5)


def test_identity_and_scores():
    ent, post = oracle.index(TEXT)
    r = lambda terms, lines, **kw: oracle.rank(ent, post, lines, terms, 10, fuzzy=True, **kw)[0]
    once = r([b"ham~1"], [0, 3, 5])
    assert r([b"ham~1", b"ham~1"], [0, 3, 5]) == once              # the same term scores once
    both = dict(r([b"ham~1", b"ham~2"], [0, 3, 5]))
    assert all(both[l] > s for l, s in once)                       # ham~2 is another term
    # never the same as a plain term, even with the same words
    assert dict(r([b"hamper~1", b"hamper"], [4]))[4] == 2 * dict(r([b"hamper"], [4]))[4]
    got = check(TEXT, [[b"ham~1", b"ham~1"], [b"ham~1", b"ham~2"], [b"hamper~1", b"hamper"],
                       [b"HAM~1", b"ham~1"]], "all", 10)
    assert got.term_counts(0)[0] == got.term_counts(0)[1]
    folded = check(TEXT, [[b"HAM~1", b"ham~1"], [b"ham~1"]], "all", 10, ignore_case=True)
    assert folded.scores(0) == folded.scores(1)  # equal after lower-casing: scores once


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [None, 3])
@pytest.mark.parametrize("fold", [False, True])
def test_cpu_fuzz(seed, k, fold):
    text, queries, modes, within, exclude = fc.fuzz_case(seed)
    expect = fc.want(text, queries, modes, k, 3, within, exclude, True, fold)
    assert any(m for (_a, m, _c), mode in zip(expect, modes) if mode == "phrase")
    assert any(m for (_a, m, _c), mode in zip(expect, modes) if mode == "near")
    assert any(m == 0 for _a, m, _c in expect) and any(m > 20 for _a, m, _c in expect)
    assert any(b"ham~1" in q and b"ham~2" in q for q in queries)
    assert any(x and any(t[-2:-1] == b"~" for t in x) for x in exclude)
    check(text, queries, modes, k, 3, within, exclude, True, fold, show=16)


# ------------------------------------------------------------------------------------
# the CLI and the README
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_fuzzy(cli, hamlet):
    queries = [[b"Hamlet~1", b"lord~1"], [b"my", b"lord~1"], [b"quene~2"], [b"nosuchword~2"]]
    exclude = [None, [b"gud~1"], None, None]
    args = ["--search", "Hamlet~1 lord~1", "--search", "my lord~1", "--not", "gud~1",
            "--search", "quene~2", "--search", "nosuchword~2"]
    for mode in ("all", "any", "phrase", "near"):
        extra = ["--within", 3] if mode == "near" else []
        w = 3 if mode == "near" else None
        for fold in (False, True):
            flags = ["--fuzzy"] + (["--ignore-case"] if fold else [])
            p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, *flags,
                    "--check", *extra)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            expect = fc.want(hamlet, queries, mode, within=w, exclude=exclude, ignore_case=fold)
            assert result_lines(p.stdout) == fc.formatted(queries, expect, exclude=exclude)
            assert sum(m for _a, m, _c in expect) > 0
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--fuzzy",
                "--rank", 4, "--check", *extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = fc.want(hamlet, queries, mode, 4, within=w, exclude=exclude)
        assert result_lines(p.stdout) == fc.formatted(queries, expect, 4, exclude)
    # --show --mark: the whole output, by the oracle
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "Hamlet~1 lord~1", "--fuzzy",
            "--show", 40, "--mark", "--check")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    shown = fc.want_show(hamlet, queries[:1], "all", 40)
    want_out = formatted_show(queries[:1], shown, mark=True)
    assert want_out in p.stdout and b">>Hamlet" in want_out
    # without --fuzzy the suffix is two literal bytes of the word
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "Hamlet~1")
    assert p.returncode == 0
    assert result_lines(p.stdout) == b"print query: Hamlet~1 \t hits: 0 \t lines:\n"


def test_tilde_as_a_delimiter_of_the_job():
    """A job that splits text at ``~`` still takes ``word~d``: the suffix is read off before the
    word is held against the delimiter set.  (The CLI splits ``--search`` with the same rule; it
    has no flag that changes the delimiter set, so the engines are asked directly.)"""
    delims = oracle.DEFAULT_DELIMS + b"~"
    text = b"ham~hem him\nhum~1 ham\nxyz~~cot\n"
    eng = lc.Engine(lc.make_config("cpu", check=True, delimiters=delims.decode()), len(text), 1)
    queries = [[b"ham~1", b"him~1"], [b"xyzz~2", b"cot~1"]]
    expect = fc.want(text, queries, "any", delims=delims)
    assert expect[0][0] == [0, 1] and expect[1][0] == [2]
    got = eng.run_search(text, queries, "any", fuzzy=True)
    fc.same(got, expect)
    assert got.format() == fc.formatted(queries, expect)
    fc.same(eng.run_index(text).search(queries, "any", fuzzy=True), expect)
    # without fuzzy the term holds a delimiter, and a ~ inside the word still does
    with pytest.raises(lc.LocustError, match="delimiter"):
        eng.run_search(text, [[b"ham~1"]])
    with pytest.raises(lc.LocustError, match="delimiter"):
        eng.run_search(text, [[b"h~m~1"]], fuzzy=True)


@pytest.mark.parametrize("args, msg", [
    (["--fuzzy"], "--search"),
    (["--fuzzy", "--index"], "--search"),
    (["--fuzzy", "--search", "ham~3"], "1 or 2"),
    (["--fuzzy", "--search", "to a~1"], "longer than its budget"),
    (["--fuzzy", "--search", "a" * 30 + "~1"], "never cut"),
    (["--fuzzy", "--glob", "--search", "h?m~1"], "never both"),
    (["--fuzzy", "--wildcard", "--search", "h*m~2"], "never both"),
    (["--fuzzy", "--search", "ham~1", "--rank", 2, "--emits-per-line", 8193], "8192"),
])
def test_cli_fuzzy_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--fuzzy" in p.stdout


README_COUNTS = [
    # (query, mode, ignore_case, lines the README states)
    ([b"Hamlet~1"], "all", False, 108),
    ([b"hamlet~1"], "all", True, 112),
    ([b"lord~1"], "all", False, 235),
    ([b"quene~2"], "all", False, 41),
    ([b"be~1"], "all", False, 822),
]


def test_readme_counts(hamlet):
    readme = open(os.path.join(ROOT, "README.md"), "rb").read()
    eng = cpu_engine(hamlet)
    for q, mode, fold, stated in README_COUNTS:
        (lines, n, _c), = fc.want(hamlet, [q], mode, ignore_case=fold)
        got = eng.run_search(hamlet, [q], mode, fuzzy=True, ignore_case=fold)
        assert got.lines(0) == lines and n == stated
        # the README states the count next to the query
        flags = b" --fuzzy" + (b" --ignore-case" if fold else b"")
        line = b'--search "%s"%s' % (b" ".join(q), flags)
        at = readme.find(line)
        assert at >= 0, line
        assert (b"the %d lines" % n) in readme[at:at + 400], (line, n)
