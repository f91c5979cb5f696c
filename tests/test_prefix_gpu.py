"""Prefix terms on the device (the lookup's range search and the expand stage of
csrc/kernels/search.hip): ``Engine.run_search(..., wildcard=True)`` and then
``Engine.search_resident`` against the oracle, exactly, ranked and unranked.  The shapes are
the smallest at which each part can go wrong: the ends of the key order for the range search,
keys with 0xff bytes behind the prefix, merged lists around the wave (64), the step (256),
the gather tile (1024), the sort tile (4096) and the sort's two regimes (8192), empty merged
lists between full ones, 13-bit slot numbers, the key-word boundaries (8, 16 bytes) for the
phrase masks, and the cut at max_key_len."""
import functools
import os
import subprocess

import pytest

import locust_amd as lc
from tests.prefix_cases import formatted, fuzz_case, merged, same, want

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_QUERIES = 1024   # kSearchMaxQueries


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


def check(engine, text, queries, modes, k=None, first_line=0, **okw):
    """run_search, then search_resident, both against the oracle; ``merged`` too."""
    expect = want(text, queries, modes, k, first_line, **okw)
    x = merged(text, queries, first_line, **okw)
    got = engine.run_search(text, queries, modes, first_line, rank=k, wildcard=True)
    same(got, expect, k)
    assert got.merged == x and got.first_line == first_line
    again = engine.search_resident(queries, modes, rank=k, wildcard=True)
    same(again, expect, k)
    assert again.merged == x
    return got


# ------------------------------------------------------------------------------------
# the range [lo, hi)
# ------------------------------------------------------------------------------------
EDGES = b"a ab abc b\nab b\nabc abc a\n\nb\n"


def test_range_edges(eng):
    queries = [[b"a*"],            # from the first key, a word that also has extensions
               [b"b*"],            # the last key: one word, in place
               [b"ab*"], [b"abc*"],
               [b"aa*"],           # between keys: absent
               [b"A*"], [b"c*"],   # below and above all keys
               [b"a*", b"b*"], [b"aa*", b"b"], [b"abd*", b"A*", b"c*"]]
    modes = ["all"] * 7 + ["all", "any", "any"]
    got = check(eng, EDGES, queries, modes)
    assert got.lines(0) == [0, 1, 2] and got.term_counts(0) == [7]
    assert got.lines(1) == [0, 1, 4] and got.hits()[4:7] == [0, 0, 0] and got.hits()[9] == 0
    assert got.merged == 7 + 5 + 7  # a*, ab*, a*: b*, abc* and the absent ones merge nothing
    check(eng, EDGES, queries, modes, 3)
    # one word per prefix: nothing is merged, and the answers are the plain terms'
    got = check(eng, EDGES, [[b"b*"], [b"abc*"], [b"b*", b"abc*"]], ["all", "all", "any"])
    assert got.merged == 0
    plain = eng.search_resident([[b"b"], [b"abc"], [b"b", b"abc"]], ["all", "all", "any"])
    assert [got.lines(i) for i in range(3)] == [plain.lines(i) for i in range(3)]


def test_every_word_and_ff_keys(eng):
    text = b"x xa xb\nxa\nx\xff x\xff\xff\nxb x\nx\xffa\n"
    queries = [[b"x*"], [b"x\xff*"], [b"x\xff\xff*"], [b"xb*"], [b"x\xfe*"], [b"x*", b"x\xff*"]]
    got = check(eng, text, queries, ["all"] * 5 + ["any"])
    assert got.lines(0) == [0, 1, 2, 3, 4] and got.term_counts(0) == [9]  # every word
    assert got.lines(1) == [2, 4] and got.term_counts(1) == [3]
    assert got.lines(2) == [2] and got.hits()[4] == 0
    check(eng, text, queries, ["all"] * 5 + ["any"], 2)


def test_prefix_at_and_past_the_key_cut(short):
    text = b"abcdefgh abcdeXYZ abcd\nabcde abc\nabcdX\n"
    # 5 bytes, and longer: cut, and exactly the plain term with its merged long words
    queries = [[b"abcde*"], [b"abcdefg*"], [b"abcde"], [b"abcd*"], [b"abc*"], [b"abcdeQ*", b"abcd"]]
    got = check(short, text, queries, ["all"] * 5 + ["phrase"], max_key=5)
    assert got.lines(0) == got.lines(1) == got.lines(2) == [0, 1]
    assert got.term_counts(0) == got.term_counts(1) == [3] and got.lines(5) == [0]
    assert got.lines(3) == [0, 1, 2] and got.merged == 5 + 6
    check(short, text, queries, ["all"] * 5 + ["phrase"], 2, max_key=5)


# ------------------------------------------------------------------------------------
# merged list sizes
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_word_text(x):
    """`wa` and `wb` with x postings together: both on line 0 (tf adds across words), then
    alternating, so the CSR range is far from sorted; `other` on every third line."""
    lines = [b"wa wb other"]
    lines += [(b"wb" if i % 2 else b"wa") + (b" other" if i % 3 == 0 else b"")
              for i in range(x - 2)]
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("x", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                               8191, 8192, 8193])
def test_merged_list_sizes(eng, x):
    text = two_word_text(x)
    queries = [[b"w*"], [b"w*", b"other"], [b"other", b"w*"]]
    got = check(eng, text, queries, ["all", "all", "any"])
    assert got.merged == 3 * x and got.term_counts(0) == [x]
    assert got.lines(0) == list(range(x - 1))
    got = check(eng, text, queries[:1], "all", 2)
    assert got.merged == x and got.lines(0)[0] == 0 and got.scores(0)[0] == 2 * got.scores(0)[1]


def test_sort_regimes_of_one_list(eng):
    """One merged list on either side of kSmallSortMax: both regimes of the merge's sort."""
    for x in (8192, 8193):
        got = check(eng, two_word_text(x), [[b"w*"]], "all")
        assert got.merged == x and got.hits() == [x - 1]


def test_empty_merged_lists_between_full_ones(eng):
    text = b"va vb wa\nwb va\nua\nwa wb vb\n"
    queries = [[b"w*"], [b"zz*"], [b"w*", b"gone*"], [b"u*"], [b"v*"], [b"q*", b"u*"], [b"v*", b"w*"]]
    modes = ["all", "all", "any", "all", "all", "all", "all"]
    got = check(eng, text, queries, modes)
    assert got.hits() == [3, 0, 3, 1, 3, 0, 3] and got.merged == 4 + 4 + 4 + 4 + 4
    check(eng, text, queries, modes, 2)


def test_full_batch_of_eight_prefix_terms(eng):
    """1024 queries x 8 prefix terms: slots up to 8191 (13 bits), tiny lists."""
    letters = b"abcdefgh"
    lines = [b" ".join(bytes([letters[(i + j) % 8], b"xy"[(i * j) % 2]]) for j in range(i % 5))
             for i in range(40)]
    text = b"\n".join(lines) + b"\n"
    queries = [[bytes([letters[(q + t) % 8]]) + b"*" for t in range(8)] for q in range(MAX_QUERIES)]
    modes = [("all", "any")[q % 2] for q in range(MAX_QUERIES)]
    got = check(eng, text, queries, modes)
    assert got.queries == MAX_QUERIES and got.merged > 8 * MAX_QUERIES and max(got.hits()) > 20
    check(eng, text, queries[-3:], modes[-3:], 4)


# ------------------------------------------------------------------------------------
# modes
# ------------------------------------------------------------------------------------
def test_modes(eng):
    text = (b"ham hamlet the\n" * 3 + b"the the\n" * 20 + b"hamper rare\n" + b"ham\n" * 30 +
            b"rare hamlet ham\n" + b"the hamlets the\n")
    queries = [[b"ham*", b"the"],          # `all`: the merged list is the longer one
               [b"ham*", b"rare"],         # ... the driver is `rare`
               [b"hamle*", b"the"],        # ... the merged list is the driver
               [b"ham*", b"the", b"rare"],  # `any`: merged plus plain lists with overlap
               [b"ham*", b"the", b"ham*"],  # a repeated prefix term
               [b"ha*", b"ham*", b"hamlet"], [b"hamlet", b"ham*", b"h*"],  # nested
               [b"hamlet", b"hamle*"], [b"ham*", b"hamp*", b"rare"]]
    modes = ["all", "all", "all", "any", "all", "all", "any", "any", "any"]
    got = check(eng, text, queries, modes)
    assert got.hits()[0] == 4 and got.lines(1) == [23, 54] and got.hits()[2] == 4
    for k in (1, 5, 100):
        check(eng, text, queries, modes, k)


# ------------------------------------------------------------------------------------
# phrase
# ------------------------------------------------------------------------------------
def test_phrase_token_lengths(eng):
    text = (b"see ham now\n"       # 0: a token equal to the prefix
            b"see hamlet now\n"    # 1: longer
            b"see ha now\n"        # 2: shorter: no match
            b"see now hamlet\n"    # 3: the words, not adjacent
            b"hamper see now\n"    # 4
            b"see hamlets\n")      # 5
    queries = [[b"see", b"ham*", b"now"], [b"ham*", b"see"], [b"see", b"ham*"], [b"ham*", b"now"],
               [b"s*", b"ham*", b"n*"], [b"ham*"], [b"see", b"ha*", b"now"]]
    got = check(eng, text, queries, "phrase")
    assert [got.lines(i) for i in range(4)] == [[0, 1], [4], [0, 1, 5], [0, 1]]
    assert got.lines(6) == [0, 1, 2]
    check(eng, text, queries, "phrase", 3)


@pytest.mark.parametrize("n", [7, 8, 9, 15, 16, 17, 24, 25, 28])
def test_phrase_prefix_at_key_word_boundaries(eng, n):
    p = (b"abcdefghijklmnopqrstuvwxyz0123456789")[:n]
    toks = [p, p + b"X", p + b"XYZ" * 4, p[:-1], p[:-1] + b"X", p[:-1] + b"\xff"]
    text = b"".join(b"go " + t + b" on\n" for t in toks) + b"go on " + p + b"\n"
    queries = [[b"go", p + b"*", b"on"], [p + b"*", b"on"], [b"go", p + b"*"], [p[:-1] + b"*", b"on"]]
    got = check(eng, text, queries, "phrase")
    assert got.lines(0) == [0, 1, 2] == got.lines(1) == got.lines(2)
    assert got.lines(3) == [0, 1, 2, 3, 4, 5]


def test_phrase_at_the_key_cut(short):
    text = b"go abcdefgh on\ngo abcde on\ngo abcd on\ngo abcdX on\n"
    queries = [[b"go", b"abcde*", b"on"], [b"go", b"abcd*", b"on"], [b"go", b"abcdeZZ*"],
               [b"abc*", b"on"]]
    got = check(short, text, queries, "phrase", max_key=5)
    assert got.lines(0) == [0, 1] == got.lines(2) and got.lines(1) == [0, 1, 2, 3] == got.lines(3)


# ------------------------------------------------------------------------------------
# ranked
# ------------------------------------------------------------------------------------
def test_weights_of_merged_counts(eng):
    """N = 64 tokens; a* merges 9 postings (64 // 9 = 7: weight 3), b* 8 (64 // 8 = 8: weight
    4).  Line 0 holds a-words five times (15), line 1 b-words four times (16): line 1 first."""
    lines = [b"a1 a1 a1 a2 a2", b"b1 b1 b2 b2", b"a1 a2 a2 a1", b"b1 b2 b1 b2"]
    fill = 64 - 9 - 8
    lines += [b" ".join(b"f%d" % (i * 20 + j) for j in range(min(20, fill - i * 20)))
              for i in range((fill + 19) // 20)]
    text = b"\n".join(lines) + b"\n"
    got = check(eng, text, [[b"a*", b"b*"], [b"a*"], [b"b*"], [b"a*", b"a1"]], "any", 4)
    assert got.term_counts(0) == [9, 8]
    assert list(zip(got.lines(0), got.scores(0))) == [(1, 16), (3, 16), (0, 15), (2, 12)]
    assert got.scores(1) == [15, 12] == got.scores(3) and got.scores(2) == [16, 16]


def test_more_equal_scores_than_k(eng):
    text = b"".join(b"tie%d x%d\n" % (i % 2, i) for i in range(130)) + b"other\n"
    for k in (63, 64, 65, 129, 130, 131):
        got = check(eng, text, [[b"tie*"]], "all", k)
        assert got.matches() == [130] and got.lines(0) == list(range(min(k, 130)))


# ------------------------------------------------------------------------------------
# the window
# ------------------------------------------------------------------------------------
def test_window(eng):
    text = b"ham hamlet\n\nthe hamper\nhamlet the ham"  # the last line without a newline
    queries = [[b"ham*"], [b"the", b"ham*"], [b"ham*", b"the"]]
    got = check(eng, text, queries, ["all", "phrase", "any"], first_line=1000)
    assert got.lines(0) == [1000, 1002, 1003] and got.lines(1) == [1002, 1003]
    check(eng, text, queries, ["all", "phrase", "any"], 2, first_line=2**32 - 4)


# ------------------------------------------------------------------------------------
# fuzz
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
@pytest.mark.parametrize("k", [None, 4])
def test_fuzz(eng, seed, k):
    text, queries, modes = fuzz_case(seed, nlines=300, nqueries=200)
    assert {"all", "any", "phrase"} == set(modes)
    got = check(eng, text, queries, modes, k, first_line=9)
    assert got.merged > 0 and 0 in got.matches() and max(got.matches()) > 100
    assert any(m for m, mode in zip(got.matches(), modes) if mode == "phrase")


def test_fuzz_short_keys(short):
    text, queries, modes = fuzz_case(5, nlines=200, nqueries=120)
    check(short, text, queries, modes, None, max_key=5)
    check(short, text, queries, modes, 3, max_key=5)


def test_plain_batches_merge_nothing(eng):
    text, queries, modes = fuzz_case(6)
    plain = [[t.rstrip(b"*") or b"x" for t in q] for q in queries]
    got = eng.run_search(text, plain, modes)
    assert got.merged == 0
    assert eng.search_resident(plain, modes, wildcard=True).format() == got.format()


# ------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------
def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print query:"))


def test_cli_wildcard(cli, hamlet):
    queries = [[b"Haml*", b"Hor*"], [b"my", b"lor*"], [b"nosuch*"]]
    args = ["--search", "Haml* Hor*", "--search", "my lor*", "--search", "nosuch*"]
    p = subprocess.run([cli, "data/hamlet.txt", *args, "--match", "any", "--wildcard", "--check"],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == formatted(queries, want(hamlet, queries, "any"))
    p = subprocess.run([cli, "data/hamlet.txt", *args, "--match", "phrase", "--wildcard", "--rank",
                        "5", "--check"], capture_output=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    expect = want(hamlet, queries, "phrase", 5)
    assert expect[1][1] > 5 and result_lines(p.stdout) == formatted(queries, expect, 5)
