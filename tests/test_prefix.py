"""Prefix terms (``ham*``) without a GPU: the oracle by hand, the host evaluation
(``IndexResult.search(..., wildcard=True)``) and the CPU engine's ``run_search`` against the
oracle, the helper's reading of the star, the nested-range score rule, and the CLI's
``--wildcard --backend cpu``.  Every comparison is exact; ``check=True`` runs
``validate_search`` on every result."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.prefix_cases import formatted, fuzz_case, same, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cli, *args, **kw):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=300, cwd=ROOT, **kw)


def cpu_engine(text, **kw):
    return lc.Engine(lc.make_config("cpu", check=True, **kw), max(len(text), 1), 1)


def check(text, queries, modes, k=None, first_line=0, **okw):
    """The CPU engine's run_search, and for all/any the host evaluation over the index."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ckw = {"max_key_len": okw["max_key"]} if "max_key" in okw else {}
    expect = want(text, queries, modes, k, first_line, **okw)
    eng = cpu_engine(text, **ckw)
    got = eng.run_search(text, queries, modes, first_line, rank=k, wildcard=True)
    same(got, expect, k)
    assert got.merged == 0  # the host evaluation merges nothing on a device
    assert got.format() == formatted(queries, expect, k)
    keep = [i for i, m in enumerate(modes) if m != "phrase"]
    idx = eng.run_index(text, first_line).search([queries[i] for i in keep],
                                                 [modes[i] for i in keep], rank=k, wildcard=True)
    same(idx, [expect[i] for i in keep], k)
    return got


TEXT = (b"ham hamlet ham* ha\n"      # 0
        b"hamlet hamlets\n"          # 1
        b"ha ha\n"                   # 2
        b"the ham\n"                 # 3
        b"hamper the hamlet\n"       # 4
        b"hum h\n")                  # 5
# keys in order: h ha ham ham* hamlet hamlets hamper hum the; N = 15 tokens


def test_oracle_by_hand():
    ent, post = oracle.index(TEXT)
    assert [k for k, _v, _c in ent] == [b"h", b"ha", b"ham", b"ham*", b"hamlet", b"hamlets",
                                        b"hamper", b"hum", b"the"]
    assert len(post) == 15
    s = lambda terms, mode="all": oracle.search(ent, post, terms, mode, wildcard=True)
    # ham* covers ham (0, 3), ham* (0), hamlet (0, 1, 4), hamlets (1), hamper (4): 8 postings
    assert s([b"ham*"]) == ([0, 1, 3, 4], [8])
    assert s([b"hamlet*"]) == ([0, 1, 4], [4])
    assert s([b"ham*", b"the"]) == ([3, 4], [8, 2])
    assert s([b"hu*", b"hamp*"], "any") == ([4, 5], [1, 1])
    assert s([b"hb*"]) == ([], [0]) and s([b"ham*", b"hb*"]) == ([], [8, 0])
    assert s([b"h*"])[1] == [13] and s([b"z*"]) == ([], [0]) and s([b"A*"]) == ([], [0])
    # an inner star is literal; without wildcard the trailing one is too
    assert s([b"ha*m"]) == ([], [0]) and s([b"ham**"]) == ([0], [1])
    assert oracle.search(ent, post, [b"ham*"]) == ([0], [1])
    with pytest.raises(ValueError):
        s([b"*"])
    with pytest.raises(ValueError):
        s([b"a b*"])
    # a prefix of max_key bytes is the plain term
    assert oracle.prefix_terms([b"abc*", b"ab*", b"abcd*"], True, max_key=3) == [
        (b"abc", False), (b"ab", True), (b"abc", False)]
    # phrase: a token matches when it starts with the prefix; a shorter one does not
    p = lambda terms: oracle.phrase(TEXT, terms, wildcard=True)
    assert p([b"the", b"ham*"]) == ([3, 4], [2, 8])
    assert p([b"ham*", b"ham*"]) == ([0, 1], [8, 8])
    assert p([b"ham*", b"ha"]) == ([0], [8, 3])
    assert p([b"hamle*", b"ha"]) == ([], [4, 3])
    # ranking: N = 15; ham*: c = 8 (weight 1), ha*: c = 11 (weight 1), hamlet: c = 3 (weight 3)
    r = lambda terms, lines: oracle.rank(ent, post, lines, terms, 10, wildcard=True)[0]
    assert r([b"ham*"], [0, 1, 3, 4]) == [(0, 3), (1, 2), (4, 2), (3, 1)]
    # nested: only the outermost range scores; of equal ranges the first
    assert r([b"ha*", b"ham*", b"hamlet"], [0, 1, 4]) == r([b"ha*"], [0, 1, 4]) == [
        (0, 4), (1, 2), (4, 2)]
    assert r([b"ham*", b"ham*"], [0, 1]) == r([b"ham*"], [0, 1])
    assert r([b"hamlet", b"ham*"], [0, 1, 4]) == r([b"ham*"], [0, 1, 4])
    assert r([b"hamlet", b"the"], [4]) == [(4, 3 + 3)]
    assert oracle.merged_elements(ent, [[b"ham*", b"ham*", b"the"], [b"hu*"], [b"ha*", b"ham*"]]) \
        == 8 + 11 + 8


def test_cpu_by_hand():
    queries = [[b"ham*"], [b"ham*", b"the"], [b"hu*", b"hamp*"], [b"hb*"], [b"ham*", b"hb*"],
               [b"h*"], [b"the", b"ham*"], [b"ham*", b"ham*"], [b"hamle*", b"ha"], [b"ha*m"],
               [b"hamlet"], [b"ham**"]]
    modes = ["all", "all", "any", "any", "all", "all", "phrase", "phrase", "phrase", "all",
             "all", "all"]
    got = check(TEXT, queries, modes)
    assert got.lines(0) == [0, 1, 3, 4] and got.term_counts(0) == [8]
    assert got.lines(6) == [3, 4] and got.lines(7) == [0, 1] and got.lines(11) == [0]
    for k in (1, 3, 100):
        check(TEXT, queries, modes, k)
    check(TEXT, queries, modes, 2, first_line=40)
    check(TEXT, queries, modes, None, max_key=3)  # ham* is the plain term ham now
    check(TEXT, queries, modes, 5, max_key=4)


def test_nested_range_score_rule():
    for q in ([b"ha*", b"ham*", b"hamlet"], [b"ham*", b"ham*"], [b"hamlet", b"ham*"]):
        for mode in ("all", "any", "phrase"):
            got = check(TEXT, [q], mode, 10)
            if mode != "phrase":  # the outermost range alone gives the same scores
                outer = check(TEXT, [q[:1] if q[0] != b"hamlet" else q[1:]], mode, 10)
                both = dict(zip(got.lines(0), got.scores(0)))
                alone = dict(zip(outer.lines(0), outer.scores(0)))
                assert all(both[l] == alone[l] for l in both)
    got = check(TEXT, [[b"ha*", b"ham*", b"hamlet"]], "all", 10)
    assert list(zip(got.lines(0), got.scores(0))) == [(0, 4), (1, 2), (4, 2)]
    assert got.term_counts(0) == [11, 8, 3]


def test_star_is_literal_without_wildcard():
    text = b"ham hamlet ham* ha\nhamlet\n"
    eng = cpu_engine(text)
    got = eng.run_search(text, [[b"ham*"]])
    assert got.lines(0) == [0] and got.term_counts(0) == [1]
    assert got.format() == b"print query: ham* \t hits: 1 \t lines: 0\n"
    got = eng.run_index(text).search([[b"ham*"]], wildcard=False)
    assert got.lines(0) == [0] and got.term_counts(0) == [1]
    got = eng.run_search(text, [[b"ham*"]], wildcard=True)
    assert got.lines(0) == [0, 1] and got.term_counts(0) == [4]  # ham, hamlet x 2, ham*; not ha
    assert got.format() == b"print query: ham* \t hits: 2 \t lines: 0 1\n"
    got = eng.run_search(text, [[b"ha*m"], [b"*ham"]], wildcard=True)  # an inner star is literal
    assert got.hits() == [0, 0]
    for call in (lambda: eng.run_search(text, [[b"ham", b"*"]], wildcard=True),
                 lambda: eng.run_index(text).search([[b"*"]], wildcard=True),
                 lambda: lc.search_text(text, [[b"*"]], backend="cpu", wildcard=True)):
        with pytest.raises(lc.LocustError, match="lone"):
            call()
    assert eng.run_search(text, [[b"*"]]).hits() == [0]  # ... and a legal literal without
    with pytest.raises(lc.LocustError, match="search"):
        eng.run_search(text, [[b"a b*"]], wildcard=True)
    # module-level entry points
    got = lc.search_text(text, [[b"ham*"]], backend="cpu", first_line=5, wildcard=True)
    assert got.lines(0) == [5, 6]
    got = lc.search_file(os.path.join(ROOT, "data", "hamlet.txt"), [[b"Haml*"]], "any", 0, 200,
                         backend="cpu", wildcard=True)
    hamlet = open(os.path.join(ROOT, "data", "hamlet.txt"), "rb").read()
    same(got, want(oracle.window(hamlet, 0, 200), [[b"Haml*"]], "any"))
    assert got.hits()[0] > 0


def test_size_refusal_by_arithmetic():
    lc._C.check_search_merge(1024, 2**32 - 1)
    with pytest.raises(lc.LocustError, match=r"merge 4294967296 list elements.*split the batch"):
        lc._C.check_search_merge(7, 2**32)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k", [None, 3])
def test_cpu_fuzz(seed, k):
    text, queries, modes = fuzz_case(seed)
    expect = want(text, queries, modes, k, first_line=3)
    assert any(m for (_a, m, _c), mode in zip(expect, modes) if mode == "phrase")
    assert any(m == 0 for _a, m, _c in expect) and any(m > 20 for _a, m, _c in expect)
    check(text, queries, modes, k, first_line=3)
    check(text, queries, modes, k, max_key=3)


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_cpu_wildcard(cli, hamlet):
    queries = [[b"Haml*", b"Hor*"], [b"my", b"lor*"], [b"nosuch*"]]
    args = ["--search", "Haml* Hor*", "--search", "my lor*", "--search", "nosuch*"]
    for mode in ("all", "any", "phrase"):
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--wildcard",
                "--check")
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        expect = want(hamlet, queries, mode)
        assert result_lines(p.stdout) == formatted(queries, expect)
        assert sum(m for _a, m, _c in expect) > 0
        p = run(cli, "data/hamlet.txt", "--backend", "cpu", *args, "--match", mode, "--wildcard",
                "--rank", 4, "--check")
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert result_lines(p.stdout) == formatted(queries, want(hamlet, queries, mode, 4), 4)
    # without --wildcard the star is a literal byte of the word
    p = run(cli, "data/hamlet.txt", "--backend", "cpu", "--search", "Haml*")
    assert p.returncode == 0 and result_lines(p.stdout) == b"print query: Haml* \t hits: 0 \t lines:\n"


@pytest.mark.parametrize("args, msg", [
    (["--wildcard"], "--search"),
    (["--wildcard", "--index"], "--search"),
    (["--wildcard", "--search", "to *"], "lone"),
])
def test_cli_wildcard_refusals(cli, args, msg, tmp_path):
    for backend in ("cpu", "gpu"):  # (refused while the flags are read: no device is touched)
        p = run(cli, "data/hamlet.txt", *args, "--backend", backend, "--spill-dir", tmp_path)
        assert p.returncode != 0
        assert msg.encode() in p.stderr
        assert b"print query" not in p.stdout and b"print key" not in p.stdout


def test_help_names_the_flag(cli):
    p = run(cli, "--help")
    assert p.returncode == 0 and b"--wildcard" in p.stdout
