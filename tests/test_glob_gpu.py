"""Pattern terms and ``ignore_case`` on the device (the dictionary scan, the scatter and the
glob verify kernels of csrc/kernels/search.hip): ``Engine.run_search(..., glob=True)`` and then
``Engine.search_resident`` against the oracle, exactly, ``merged`` included.  The shapes are the
smallest at which each part can go wrong: the matcher's edges (stars matching nothing,
backtracking, ``?`` at the key's end, the key-word boundaries, bytes of 0x80 and above), the
fold's edges, dictionaries around the scan's wave (64) and tile (256), merged lists around the
wave, the step (256), the gather tile (1024), the sort tile (4096) and the sort's two regimes
(8192), built from two long lists and from that many single postings, one-word and absent
patterns, batches that mix plain, prefix and pattern slots, and every slot of a full batch a
pattern."""
import functools
import os
import subprocess

import pytest

import locust_amd as lc
from tests.glob_cases import (EDGE_PATTERNS, edge_text, formatted, fuzz_case, merged, same,
                              want)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_QUERIES = 1024   # kSearchMaxQueries
TILE = 256           # kSearchBlock: records per workgroup and step of the dictionary scan


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine for the small cases."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


@pytest.fixture(scope="module")
def short():
    """... and one whose keys are cut to 5 bytes."""
    return lc.Engine(gpu_cfg(max_key_len=5), 1 << 16, 1 << 10)


def check(engine, text, queries, modes, k=None, first_line=0, within=None, exclude=None,
          glob=True, ignore_case=False, **okw):
    """run_search, then search_resident, both against the oracle; ``merged`` too."""
    expect = want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case, **okw)
    x = merged(text, queries, first_line, exclude, glob, ignore_case, **okw)
    kw = dict(rank=k, within=within, exclude=exclude, glob=glob, ignore_case=ignore_case)
    got = engine.run_search(text, queries, modes, first_line, **kw)
    same(got, expect, k)
    assert got.merged == x and got.first_line == first_line
    again = engine.search_resident(queries, modes, **kw)
    same(again, expect, k)
    assert again.merged == x
    return got


# ------------------------------------------------------------------------------------
# the matcher and the fold
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
def test_matcher_edges(eng, fold):
    text = edge_text()
    queries = [[p] for p in EDGE_PATTERNS]
    got = check(eng, text, queries, "all", ignore_case=fold)
    hits = got.hits()
    assert 0 in hits and max(hits) >= 8
    check(eng, text, queries, "any", 3, ignore_case=fold)
    # the same patterns, eight to a query: every term slot
    packs = [EDGE_PATTERNS[i:i + 8] for i in range(0, len(EDGE_PATTERNS), 8)]
    check(eng, text, packs, "any", ignore_case=fold)
    check(eng, text, packs, "any", 5, ignore_case=fold)
    # as phrases and near queries behind `pad`: the verify kernels' matcher sees every key
    two = [[p, b"pad"] for p in EDGE_PATTERNS] + [[b"?" * 3, b"p?d"], [b"p*d"]]
    check(eng, text, two, "phrase", ignore_case=fold)
    check(eng, text, two, "near", within=2, ignore_case=fold)


def test_fold_edges(eng, short):
    text = (b"@a[ `a{ Hamlet\n@A[ `A{ HAMLET hamlets\n\xc3\xa9 \xc3\x89 hamlet\n"
            b"To be or\nnot to BE\nto bee Be\n\x80A \x80a \xffz \xffZ\n")
    queries = [[b"@a["], [b"`a{"], [b"\xc3\xa9"], [b"hamlet"], [b"HAM*"], [b"h?ML*"],
               [b"to", b"be"], [b"\x80a"], [b"\xffZ", b"\x80A"], [b"TO", b"b*"], [b"t?", b"B?"]]
    modes = ["all"] * 6 + ["phrase", "all", "any", "phrase", "near"]
    within = [None] * 10 + [2]
    for k in (None, 2):
        got = check(eng, text, queries, modes, k, within=within, ignore_case=True)
        check(eng, text, queries, modes, k, within=within, ignore_case=False)
        check(eng, text, queries, modes, k, within=within, ignore_case=True, glob=False)
    assert got.matches()[0] == 2 and got.matches()[2] == 1 and got.matches()[3] == 3
    assert got.matches()[6] == 2 and got.matches()[7] == 1
    # a plain term with metacharacters stays literal under ignore_case without glob
    lit = b"a*b A*B axb h?m HaM\n"
    got = check(eng, lit, [[b"a*b"], [b"h?m"], [b"a*b*"]], "all", ignore_case=True, glob=False)
    assert got.term_counts(0) == [2] and got.term_counts(1) == [1]
    got = eng.search_resident([[b"a*b*"]], ignore_case=True, wildcard=True)
    assert got.term_counts(0) == [2]
    # ignore_case with max_key_len = 5: terms are cut first
    text5 = b"Hamlet hamlets HAMLE ham\nhamle Hamper\n"
    q5 = [[b"hamlet"], [b"HAMLETS*"], [b"h?mle"], [b"ham*"], [b"hamlet", b"HAM"]]
    check(short, text5, q5, ["all", "all", "all", "all", "phrase"], ignore_case=True, max_key=5)
    check(short, text5, q5, ["all", "all", "all", "all", "near"], 2, within=2, ignore_case=True,
          max_key=5)


# ------------------------------------------------------------------------------------
# the dictionary scan: sizes around the wave and the tile
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_dictionary_sizes(eng, n):
    # words w0000 .. in key order, one posting each, ten to a line
    words = [b"w%04d" % i for i in range(n)]
    text = b"".join(b" ".join(words[i:i + 10]) + b"\n" for i in range(0, n, 10))
    last = b"w%04d" % (n - 1)
    queries = [[b"?0000"],                     # the first word
               [b"?" + last[1:]],              # the last word
               [b"w????"],                     # every word
               [b"w0*5"], [b"*3"],             # scattered over the tiles
               [b"w006?"],                     # ranks 60 .. 69: straddles the wave edge
               [b"w025?"],                     # ranks 250 .. 259: straddles the tile edge
               [b"*9", b"w?2*"]]
    got = check(eng, text, queries, "any")
    assert got.term_counts(0) == [1] and got.term_counts(1) == [1] and got.term_counts(2) == [n]
    check(eng, text, queries, "all", 4)


# ------------------------------------------------------------------------------------
# merged list sizes
# ------------------------------------------------------------------------------------
SIZES = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193]


@functools.lru_cache(maxsize=None)
def two_word_text(x):
    """`wa` and `wb` with x postings together: both on line 0 (tf adds across words), then
    alternating, so the lists interleave; `other` on every third line."""
    lines = [b"wa wb other"]
    lines += [(b"wb" if i % 2 else b"wa") + (b" other" if i % 3 == 0 else b"")
              for i in range(x - 2)]
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("x", SIZES)
def test_merged_sizes_two_long_lists(eng, x):
    text = two_word_text(x)
    queries = [[b"w?"], [b"?a*", b"other"], [b"other", b"*b"], [b"w?", b"*w*"]]
    got = check(eng, text, queries, ["all", "all", "any", "any"])
    # w? merges x; ?a* and *b cover one word each: in place; *w* is another term with w?'s words
    assert got.merged == 3 * x and got.term_counts(0) == [x]
    assert got.lines(0) == list(range(x - 1))
    if x in (65, 1025, 8193):
        check(eng, text, queries, ["all", "all", "any", "any"], 3)


@functools.lru_cache(maxsize=None)
def many_word_text(x):
    """x words of count 1, eight to a line, in an order far from the key order."""
    words = [b"v%05d" % ((i * 7919) % x) for i in range(x)]
    return b"".join(b" ".join(words[i:i + 8]) + b"\n" for i in range(0, x, 8))


@pytest.mark.parametrize("x", SIZES)
def test_merged_sizes_many_words(eng, x):
    text = many_word_text(x)
    got = check(eng, text, [[b"v????*"], [b"*1", b"v*0?"]], ["all", "any"])
    assert got.term_counts(0) == [x] and got.merged >= x


# ------------------------------------------------------------------------------------
# one-word and absent patterns, mixed batches
# ------------------------------------------------------------------------------------
MIX = (b"ham hamlet ham* ha\nhamlet hamlets\nha ha\nthe ham\nhamper the hamlet\nhum h\n"
       b"Ham THE\n")


def test_one_word_and_absent_patterns(eng):
    got = check(eng, MIX, [[b"h?mper"], [b"hampe?", b"the"], [b"*mper", b"h"]],
                ["all", "all", "any"])
    assert got.merged == 0
    plain = eng.search_resident([[b"hamper"], [b"hamper", b"the"], [b"hamper", b"h"]],
                                ["all", "all", "any"])
    assert [got.lines(i) for i in range(3)] == [plain.lines(i) for i in range(3)]
    # an absent pattern: `all` is dead, `any` ignores it, as an exclusion it excludes nothing
    queries = [[b"z?", b"ham"], [b"z?", b"ham"], [b"ham"], [b"zz*z"], [b"the", b"q?"]]
    modes = ["all", "any", "all", "all", "phrase"]
    exclude = [None, None, [b"z?"], None, None]
    got = check(eng, MIX, queries, modes, exclude=exclude)
    assert got.hits() == [0, 2, 2, 0, 0] and got.merged == 0
    check(eng, MIX, queries, modes, 2, exclude=exclude)


def test_mixed_batches_and_a_plain_batch_behind(eng):
    before = eng.run_search(MIX, [[b"ham"], [b"ha*", b"the"], [b"the", b"ham"]],
                            ["all", "all", "phrase"], wildcard=True)
    queries = [[b"ham", b"ha*", b"h?m*"],      # plain, prefix and pattern slots together
               [b"zz?"], [b"h*t"], [b"q*q"],   # empty merged lists between full ones
               [b"*a*"], [b"zq?*"], [b"*m*", b"the"], [b"ha*"], [b"h?"],
               [b"the", b"h?m"], [b"h*", b"*t"], [b"*a*", b"*a*", b"ham"]]
    modes = ["all", "all", "all", "all", "any", "any", "all", "all", "all", "phrase", "near",
             "any"]
    within = [None] * 10 + [3, None]
    exclude = [None, None, [b"*s"], None, [b"h?"], None, None, [b"*per"], None, None, None,
               [b"t?e"]]
    for fold in (False, True):
        for k in (None, 3):
            check(eng, MIX, queries, modes, k, 11, within, exclude, ignore_case=fold)
    # a plain batch straight after a pattern batch: the answer it gave before, no pattern stage
    after = eng.search_resident([[b"ham"], [b"ha*", b"the"], [b"the", b"ham"]],
                                ["all", "all", "phrase"], wildcard=True)
    assert after.merged == before.merged
    assert [[l - 11 for l in after.lines(i)] for i in range(3)] == \
        [before.lines(i) for i in range(3)]
    assert [after.term_counts(i) for i in range(3)] == [before.term_counts(i) for i in range(3)]


def test_full_batch_every_slot_a_pattern(eng):
    text = b"ab ba aa\nbb ab\nba\naa bb ab ba\n\nab\n"
    pats = [b"a?", b"?a", b"?b", b"b?", b"*a", b"*b", b"a*a", b"?*?", b"??", b"a*b", b"b*a",
            b"*ab", b"?a*", b"*b?", b"b*b", b"*aa*"]
    queries = [[pats[(q + 3 * t) % len(pats)] for t in range(8)] for q in range(MAX_QUERIES)]
    modes = ["any" if q % 3 == 0 else "all" for q in range(MAX_QUERIES)]
    check(eng, text, queries, modes)
    check(eng, text, queries, modes, 2)
    with pytest.raises(lc.LocustError, match="kSearchMaxQueries"):
        eng.search_resident(queries + [[b"a?"]], glob=True)


# ------------------------------------------------------------------------------------
# identity and overlap
# ------------------------------------------------------------------------------------
def test_identity_and_overlap(eng):
    queries = [[b"*a*", b"*a*"], [b"*a*"], [b"*a*", b"*m*"], [b"h?mper", b"hamper"],
               [b"HAM*", b"ham*"], [b"ham*", b"ham?*"]]
    got = check(eng, MIX, queries, "all", 10)
    assert got.scores(0) == got.scores(1) and got.term_counts(0)[0] == got.term_counts(0)[1]
    assert got.merged == merged(MIX, queries)
    check(eng, MIX, queries, "any", 10)
    folded = check(eng, MIX, queries, "any", 10, ignore_case=True)
    assert folded.term_counts(4)[0] == folded.term_counts(4)[1]
    # the score bound: emits_per_line tokens, all matching all eight terms
    pats = [b"a?", b"?a", b"*a", b"a*a", b"??", b"*aa", b"?*a", b"a*?"]
    text = b" ".join([b"aa"] * 25) + b"\n" + b"b c d e f g h i j k l m n o p q r s t u\n" * 40
    got = check(eng, text, [pats, pats[:1]], "any", 1)
    assert got.scores(0) == [20 * 8 * 6] and got.scores(1) == [20 * 6]  # N = 820, c = 20
    wide = lc.Engine(gpu_cfg(emits_per_line=8193), 1 << 12, 64)
    with pytest.raises(lc.LocustError, match="8192"):
        wide.run_search(text, [pats], rank=1, glob=True)
    assert wide.run_search(text, [[b"aa"]], rank=1).scores(0) == [25 * 6]  # N = 825, c = 25


# ------------------------------------------------------------------------------------
# phrase and near verification
# ------------------------------------------------------------------------------------
def test_verify_straddles_the_step_and_the_emit_cap(eng):
    lines = []
    for pad in range(56, 70):  # the token `hamlet` starts at bytes 56 .. 69 of the line
        lines.append(b"x" * (pad - 1) + b" hamlet Prince of")
    lines.append(b" ".join([b"y"] * 19) + b" ham prince")   # prince is token 21: past the cap
    lines.append(b" ".join([b"y"] * 18) + b" ham prince")   # ... and token 20: the last one
    text = b"\n".join(lines) + b"\n"
    queries = [[b"h?mlet", b"pr*e"], [b"*let", b"?rince", b"o?"], [b"h*", b"prin??"],
               [b"x*x", b"ham???"], [b"prince", b"h?m"], [b"y", b"*am", b"p*"]]
    for fold in (False, True):
        got = check(eng, text, queries, "phrase", ignore_case=fold)
        check(eng, text, queries, "near", within=2, ignore_case=fold)
        check(eng, text, queries, "near", 3, within=3, ignore_case=fold)
    assert got.hits()[0] == 14 and got.hits()[5] == 1


# ------------------------------------------------------------------------------------
# fuzz, and the CLI
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(eng, seed):
    text, queries, modes, within, exclude = fuzz_case(seed)
    for fold in (False, True):
        for k in (None, 3):
            check(eng, text, queries, modes, k, 3, within, exclude, True, fold)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_gpu_equals_cpu(cli):
    args = ["data/hamlet.txt", "--search", "h?ml*t *tio", "--search", "my lor*", "--not", "L?RD",
            "--search", "*ing", "--search", "to be", "--match", "phrase", "--glob",
            "--ignore-case", "--check"]
    out = {}
    for backend in ("cpu", "gpu"):
        p = subprocess.run([cli, *args, "--backend", backend], capture_output=True, timeout=300,
                           cwd=ROOT)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out[backend] = result_lines(p.stdout)
    assert out["gpu"] == out["cpu"] and out["gpu"].count(b"print query:") == 4
    assert b"hits: 0" not in out["gpu"].split(b"\n")[3]
