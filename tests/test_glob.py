"""Pattern terms (``glob``: ``*ing``, ``h?mlet``) and ``ignore_case`` without a GPU: how
terms are classified and refused, the shared matcher (through the host evaluation) against the
oracle's regular expressions on the edge list, the host evaluation and the CPU engine against
the oracle in all four modes, ranked and not, with exclusion terms and a short key length, the
CLI's ``--glob --ignore-case --backend cpu``, and the README's counts.  Every comparison is
exact; ``check=True`` runs ``validate_search`` on every result."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.glob_cases import (EDGE_KEYS, EDGE_PATTERNS, edge_text, formatted, fuzz_case, same,
                              want)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def check(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=True,
          ignore_case=False, **okw):
    """The CPU engine's run_search, and for all/any the host evaluation over the index."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ckw = {"max_key_len": okw["max_key"]} if "max_key" in okw else {}
    expect = want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case, **okw)
    eng = cpu_engine(text, **ckw)
    gkw = dict(rank=k, glob=glob, ignore_case=ignore_case)
    got = eng.run_search(text, queries, modes, first_line, within=within, exclude=exclude, **gkw)
    same(got, expect, k)
    assert got.merged == 0  # the host evaluation merges nothing on a device
    assert got.format() == formatted(queries, expect, k, exclude, glob)
    keep = [i for i, m in enumerate(modes) if m in ("all", "any")]
    idx = eng.run_index(text, first_line).search(
        [queries[i] for i in keep], [modes[i] for i in keep],
        exclude=[exclude[i] for i in keep] if exclude else None, **gkw)
    same(idx, [expect[i] for i in keep], k)
    return got


TEXT = (b"ham Hamlet ham* ha\n"      # 0
        b"hamlet hamlets HAM\n"      # 1
        b"ha ha sing\n"              # 2
        b"the ham king\n"            # 3
        b"hamper the hamlet a*b\n"   # 4
        b"hum h ring\n")             # 5


def test_classification_and_collapse():
    kinds = lambda terms, **kw: [(t.kind, t.p) for t in oracle.query_terms(terms, glob=True, **kw)]
    assert kinds([b"a**", b"ab", b"a*"]) == [("prefix", b"a"), ("plain", b"ab"), ("prefix", b"a")]
    assert [k for k, _p in kinds([b"a*b", b"*a", b"a?", b"?", b"a**b", b"a?*"])] == ["pattern"] * 6
    assert [k for k, _p in kinds([b"ab", b"a*"], ignore_case=True)] == ["pattern"] * 2
    eng = cpu_engine(TEXT)
    # a** is the prefix a*: it prints collapsed... as the prefix term it is
    got = eng.run_search(TEXT, [[b"ha**"], [b"ha*"], [b"h*t"], [b"*ing"], [b"h?"], [b"?"]],
                         glob=True)
    assert got.lines(0) == got.lines(1) == [0, 1, 2, 3, 4]
    assert got.term_counts(0) == got.term_counts(1)
    assert got.lines(2) == [1, 4] and got.term_counts(2) == [2]       # hamlet x 2, not Hamlet
    assert got.lines(3) == [2, 3, 5] and got.term_counts(3) == [3]    # sing king ring
    assert got.lines(4) == [0, 2] and got.term_counts(4) == [3]       # ha x 3
    assert got.lines(5) == [5] and got.term_counts(5) == [1]          # h
    assert got.format().startswith(b"print query: ha* \t hits: 5")
    assert b"print query: h*t \t hits: 2 \t lines: 1 4\n" in got.format()
    # glob is a superset of wildcard: both together are glob
    both = eng.run_search(TEXT, [[b"ha**"], [b"h*t"]], glob=True, wildcard=True)
    assert both.lines(0) == got.lines(0) and both.lines(1) == got.lines(2)
    # wildcard alone: an inner star and a question mark stay literal
    got = eng.run_search(TEXT, [[b"a*b"], [b"h*t"], [b"h?"]], wildcard=True)
    assert got.hits() == [1, 0, 0] and got.lines(0) == [4]
    # ... and under glob a*b is a pattern: the literal word a*b is one of its words
    got = eng.run_search(TEXT, [[b"a*b"]], glob=True)
    assert got.lines(0) == [4] and got.term_counts(0) == [1]


def test_ignore_case_by_hand():
    eng = cpu_engine(TEXT)
    got = eng.run_search(TEXT, [[b"hamlet"], [b"HAM*"], [b"h?M"], [b"ham*"]], ignore_case=True,
                         wildcard=True)
    assert got.lines(0) == [0, 1, 4] and got.term_counts(0) == [3]
    # ham* under wildcard + ignore_case: ham ham* Hamlet hamlet hamlets HAM hamper
    assert got.lines(1) == got.lines(3) == [0, 1, 3, 4]
    assert got.lines(2) == []  # without glob, ? is literal
    got = eng.run_search(TEXT, [[b"h?M"], [b"ham*"]], ignore_case=True, glob=True)
    assert got.lines(0) == [0, 1, 3, 5] and got.term_counts(0) == [4]   # ham HAM ham hum
    # without wildcard or glob, ham* is the literal word, whatever its case
    got = eng.run_search(TEXT, [[b"HAM*"]], ignore_case=True)
    assert got.lines(0) == [0] and got.term_counts(0) == [1]
    # only ASCII letters fold
    text = b"@a[ `a{\n@A[ `A{\n\xc3\xa9 \xc3\x89\n"
    got = cpu_engine(text).run_search(text, [[b"@a["], [b"`a{"], [b"\xc3\xa9"], [b"@?["]],
                                      ignore_case=True, glob=True)
    assert got.lines(0) == [0, 1] and got.lines(1) == [0, 1]
    assert got.lines(2) == [2] and got.term_counts(2) == [1]
    assert got.lines(3) == [0, 1] and got.term_counts(3) == [2]
    assert cpu_engine(text).run_search(text, [[b"@a["]], glob=True).lines(0) == [0]
    # phrase: to be finds To be
    text = b"To be or\nnot to BE\nto bee\n"
    got = cpu_engine(text).run_search(text, [[b"to", b"be"]], "phrase", ignore_case=True)
    assert got.lines(0) == [0, 1]
    assert cpu_engine(text).run_search(text, [[b"to", b"be"]], "phrase").lines(0) == []


def test_refusals():
    eng = cpu_engine(TEXT)
    for q, msg in (([b"*"], "stars alone"), ([b"**"], "stars alone"), ([b"ham", b"***"], "stars"),
                   ([b"a" * 15 + b"?" + b"a" * 14], "never cut"), ([b"a b?"], "delimiter"),
                   ([b"?,x"], "delimiter"), ([b"a\n*b"], "newline")):
        for call in (lambda: eng.run_search(TEXT, [q], glob=True),
                     lambda: eng.run_index(TEXT).search([q], glob=True),
                     lambda: lc.search_text(TEXT, [q], backend="cpu", glob=True),
                     lambda: eng.run_search(TEXT, [[b"ham"]], exclude=[q], glob=True)):
            with pytest.raises(lc.LocustError, match=msg):
                call()
        with pytest.raises(ValueError):
            oracle.query_terms(q, glob=True)
    # a pattern of exactly max_key_len bytes is legal; a prefix term is cut as ever
    assert eng.run_search(TEXT, [[b"?" * 29], [b"a" * 40 + b"*"]], glob=True).hits() == [0, 0]
    short = cpu_engine(TEXT, max_key_len=5)
    assert short.run_search(TEXT, [[b"h?mle"]], glob=True).term_counts(0) == [3]  # hamlet(s) cut
    with pytest.raises(lc.LocustError, match="never cut"):
        short.run_search(TEXT, [[b"h?mlet"]], glob=True)
    assert short.run_search(TEXT, [[b"hamlets*"]], glob=True).term_counts(0) == [3]  # plain hamle
    # ranked: emits_per_line <= kRankMaxEmits / 8 with a pattern term, kRankMaxEmits without
    big = cpu_engine(TEXT, emits_per_line=8193)
    assert big.run_search(TEXT, [[b"ham*"]], rank=3, glob=True).matches() == [4]
    for kw in (dict(glob=True), dict(ignore_case=True), dict(glob=True, ignore_case=True)):
        q = [[b"h?m"]] if "glob" in kw else [[b"ham"]]
        with pytest.raises(lc.LocustError, match="8192"):
            big.run_search(TEXT, q, rank=3, **kw)
        with pytest.raises(lc.LocustError, match="8192"):
            big.run_index(TEXT).search(q, rank=3, **kw)
        assert cpu_engine(TEXT, emits_per_line=8192).run_search(TEXT, q, rank=3, **kw).matches()[0]
        assert big.run_search(TEXT, q, **kw).hits()[0]  # unranked: no such limit
    ent, post = oracle.index(TEXT)
    with pytest.raises(ValueError):
        oracle.rank(ent, post, [0], [b"h?m"], 3, glob=True, emits=8193)
    oracle.rank(ent, post, [0], [b"ham*"], 3, glob=True, emits=8193)


def test_matcher_edges_against_the_oracle():
    text = edge_text()
    queries = [[p] for p in EDGE_PATTERNS]
    for fold in (False, True):
        got = check(text, queries, "all", glob=True, ignore_case=fold)
        # the list is worth its name: matches, misses and several words per pattern
        hits = got.hits()
        assert 0 in hits and max(hits) >= 8 and sum(1 for h in hits if h == 1) >= 5
        ent, _post = oracle.index(text)
        for p in (b"ab?", b"*ab", b"*ab*ab", b"k" * 28 + b"?"):
            t, = oracle.query_terms([p], glob=True, ignore_case=fold)
            words = {k for k, _v, _c in ent if t.fits(k)}
            if p == b"ab?":
                assert b"ab" not in words and b"abc" in words
            if p == b"*ab":
                assert {b"ab", b"aab", b"abab", b"xab"} <= words and b"abx" not in words
            if p == b"*ab*ab":
                assert {b"abab", b"ababab"} <= words and b"aab" not in words
            if p == b"k" * 28 + b"?":
                assert (b"K" * 28 + b"z" in words) == fold and b"k" * 29 in words
    assert len(EDGE_KEYS) == len(set(EDGE_KEYS))


@pytest.mark.parametrize("k", [None, 3])
def test_cpu_all_modes_by_hand(k):
    queries = [[b"h*t"], [b"*ing", b"the"], [b"h?m*", b"*a"], [b"the", b"*m"], [b"h*", b"*et"],
               [b"*a*", b"*a*"], [b"*a*", b"*m*"], [b"zz?"], [b"ham", b"zz?"], [b"h?m", b"ham"],
               [b"ham*", b"h?m"], [b"?a*", b"hamlet"]]
    modes = ["all", "all", "any", "phrase", "near", "all", "any", "any", "all", "all",
             "phrase", "near"]
    within = [None, None, None, None, 2, None, None, None, None, None, None, 3]
    exclude = [None, [b"k?ng"], [b"*s"], None, None, [b"zz*z"], None, None, None, [b"*per"],
               None, None]
    for fold in (False, True):
        got = check(TEXT, queries, modes, k, within=within, exclude=exclude, ignore_case=fold)
        assert sum(got.matches()) > 0
        check(TEXT, queries, modes, k, first_line=7, within=within, ignore_case=fold)
    check(TEXT, [q for q in queries if all(len(t) <= 5 for t in q)],
          [m for q, m in zip(queries, modes) if all(len(t) <= 5 for t in q)], k,
          within=2, max_key=5)
    check(TEXT, [[b"hamle", b"*mle"], [b"hamlets*"], [b"?amle"]], "all", k, ignore_case=True,
          max_key=5)


def test_identity_and_overlap_scores():
    # N = 21 tokens; *a* and *m* overlap on ham, hamlet, ...: one token feeds both terms
    ent, post = oracle.index(TEXT)
    r = lambda terms, lines, **kw: oracle.rank(ent, post, lines, terms, 10, glob=True, **kw)[0]
    once = r([b"*a*"], [0, 1, 2, 3, 4])
    assert r([b"*a*", b"*a*"], [0, 1, 2, 3, 4]) == once
    both = dict(r([b"*a*", b"*m*"], [0, 1, 2, 3, 4]))
    assert all(both[l] > s for l, s in once if l != 2) and both[2] == dict(once)[2]
    # a pattern term is never the same as a plain or prefix term, even with the same words
    assert dict(r([b"h?mper", b"hamper"], [4]))[4] == 2 * dict(r([b"hamper"], [4]))[4]
    assert dict(r([b"ham*", b"ham?*"], [4]))[4] > dict(r([b"ham*"], [4]))[4]
    got = check(TEXT, [[b"*a*", b"*a*"], [b"*a*", b"*m*"], [b"h?mper", b"hamper"],
                       [b"HAM*", b"ham*"]], "all", 10)
    assert got.term_counts(0)[0] == got.term_counts(0)[1]
    folded = check(TEXT, [[b"HAM*", b"ham*"], [b"ham*"]], "all", 10, ignore_case=True)
    assert folded.scores(0) == folded.scores(1)  # equal after lower-casing: scores once
    # the bound: emits_per_line tokens that all match all eight terms
    text = b" ".join([b"aa"] * 20) + b"\nb\n"
    pats = [b"a?", b"?a", b"*a", b"a*a", b"??", b"*aa", b"?*a", b"a*?"]
    got = check(text, [pats], "all", 1)
    assert got.scores(0) == [20 * 8 * 1] and got.scores(0)[0] <= 32 * 20 * 8
    text = b" ".join([b"aa"] * 20) + b"\n" + b"b c d e f g h i j k l m n o p q r s t u\n" * 40
    got = check(text, [pats], "any", 1)
    assert got.scores(0) == [20 * 8 * 6]  # N = 820, c = 20: weight bit_length(41) = 6


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k", [None, 3])
@pytest.mark.parametrize("fold", [False, True])
def test_cpu_fuzz(seed, k, fold):
    text, queries, modes, within, exclude = fuzz_case(seed)
    expect = want(text, queries, modes, k, 3, within, exclude, True, fold)
    assert any(m for (_a, m, _c), mode in zip(expect, modes) if mode == "phrase")
    assert any(m for (_a, m, _c), mode in zip(expect, modes) if mode == "near")
    assert any(m == 0 for _a, m, _c in expect) and any(m > 20 for _a, m, _c in expect)
    check(text, queries, modes, k, 3, within, exclude, True, fold)


# ------------------------------------------------------------------------------------
# the CLI and the README
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_glob(cli, hamlet):
    queries = [[b"h?ml*t", b"*tio"], [b"my", b"lor*"], [b"*ing"], [b"nosuch?"]]
    exclude = [None, [b"L?RD"], None, None]
    args = ["--search", "h?ml*t *tio", "--search", "my lor*", "--not", "L?RD",
            "--search", "*ing", "--search", "nosuch?"]
    for mode in ("all", "any", "phrase", "near"):
        extra = ["--within", 3] if mode == "near" else []
        w = 3 if mode == "near" else None
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--glob",
                "--ignore-case", "--check", *extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want(hamlet, queries, mode, within=w, exclude=exclude, ignore_case=True)
        assert result_lines(p.stdout) == formatted(queries, expect, exclude=exclude)
        assert sum(m for _a, m, _c in expect) > 0
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--glob",
                "--ignore-case", "--rank", 4, "--check", *extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want(hamlet, queries, mode, 4, within=w, exclude=exclude, ignore_case=True)
        assert result_lines(p.stdout) == formatted(queries, expect, 4, exclude)
    # without --glob the metacharacters are literal bytes of the word
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "*ing")
    assert p.returncode == 0 and result_lines(p.stdout) == b"print query: *ing \t hits: 0 \t lines:\n"


@pytest.mark.parametrize("args, msg", [
    (["--glob"], "--search"),
    (["--ignore-case"], "--search"),
    (["--glob", "--index"], "--search"),
    (["--glob", "--search", "to **"], "stars alone"),
    (["--glob", "--search", "a?" + "b" * 28], "never cut"),
    (["--glob", "--search", "h?m", "--rank", 2, "--emits-per-line", 8193], "8192"),
    (["--ignore-case", "--search", "ham", "--rank", 2, "--emits-per-line", 8193], "8192"),
])
def test_cli_glob_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flags(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--glob" in p.stdout and b"--ignore-case" in p.stdout


README_COUNTS = [
    # (query, mode, glob, ignore_case, lines the README states)
    ([b"*ing"], "all", True, False, 536),
    ([b"h?ml*t"], "all", True, True, 97),
    ([b"to", b"be"], "all", False, True, 60),
    ([b"to", b"be"], "phrase", False, True, 32),
    ([b"to", b"be"], "phrase", False, False, 27),
]


def test_readme_counts(hamlet):
    readme = open(os.path.join(ROOT, "README.md"), "rb").read()
    eng = cpu_engine(hamlet)
    for q, mode, glob, fold, stated in README_COUNTS:
        (lines, n, _c), = want(hamlet, [q], mode, glob=glob, ignore_case=fold)
        got = eng.run_search(hamlet, [q], mode, glob=glob, ignore_case=fold)
        assert got.lines(0) == lines
        if stated is not None:
            assert n == stated
        # the README states the count next to the query
        flags = (b" --glob" if glob else b"") + (b" --ignore-case" if fold else b"")
        match = b" --match phrase" if mode == "phrase" else b""
        line = b'--search "%s"%s%s' % (b" ".join(q), match, flags)
        at = readme.find(line)
        assert at >= 0, line
        assert (b"the %d lines" % n) in readme[at:at + 400], (line, n)
