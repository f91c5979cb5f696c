"""Dropping the oldest lines of the index on the device (csrc/kernels/drop.hip): after
``drop_index(d)`` the resident index is the index of the remaining lines with their own (global)
numbers -- ``index_resident()`` against the oracle, exactly, after every drop, and every search
feature against ``run_search`` of the window's text on a one-pass engine, field for field.

The shapes are the smallest at which each kernel can go wrong: duplicates of the cut line, every
pattern of vanishing words the compaction can see, a list longer than any postings tile
(``kAppendTile`` = 1024 destination elements) cut at the tile's edges among one-posting
neighbours, kept lists of T - 1, T, T + 1 elements for T = 1024 and 64 at three offsets into their
tile, more distinct words than one scan tile (``kIndexTile`` = 2048), drops of 1, 63, 64 and 65
lines whose statistics the device recounts, a non-zero first line, a sliding window."""
import json
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.test_append import SHAPES, fuzz_text, nlines, text_of, words

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024  # kAppendTile


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine of 1 MiB for every case that needs no other."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def lines_of(text):
    """The text's lines with their newlines (the last one may lack it)."""
    parts = text.split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def stats_of(text, **okw):
    """(overflow_lines, truncated) of the word job over `text`."""
    _e, _t, over, trunc = oracle.wordcount(text, stats=True, **okw)
    return over, trunc


class Window:
    """An engine's resident index and, beside it, the lines it should hold."""

    def __init__(self, engine, text, first_line=0, search=None, **okw):
        self.e, self.first, self.okw = engine, first_line, okw
        self.lines = lines_of(text)
        r = engine.run_search(text, search, "all", first_line) if search else \
            engine.run_index(text, first_line)
        self.tokens, self.unique = r.num_tokens, r.num_unique

    @property
    def text(self):
        return b"".join(self.lines)

    def append(self, text):
        ap = self.e.append_index(text)
        self.lines += lines_of(text)
        self.tokens, self.unique = ap.num_tokens, ap.num_unique
        return ap

    def drop(self, d, compare=True):
        gone = b"".join(self.lines[:d])
        dr = self.e.drop_index(d)
        self.lines = self.lines[d:]
        self.first += d
        assert dr.dropped_lines == d and dr.dropped_bytes == len(gone)
        assert (dr.first_line, dr.num_lines) == (self.first, len(self.lines))
        assert dr.dropped_tokens == self.tokens - dr.num_tokens
        assert dr.dropped_words == self.unique - dr.num_unique
        assert (dr.dropped_overflow_lines, dr.dropped_truncated) == stats_of(gone, **self.okw)
        assert (dr.drop_ms > 0 and dr.store_bytes > 0) if d else dr.drop_ms == 0
        self.tokens, self.unique = dr.num_tokens, dr.num_unique
        return self.compare() if compare else dr

    def compare(self):
        """index_resident() against the oracle's index of the lines that are left."""
        text = self.text
        ent, post = oracle.index(text, first_line=self.first, **self.okw)
        x = self.e.index_resident()
        assert x.entries() == ent
        assert x.postings() == post
        assert x.first_line == self.first and x.num_lines == len(self.lines)
        assert x.num_tokens == len(post) == self.tokens
        assert x.num_unique == len(ent) == self.unique
        assert (x.overflow_lines, x.truncated) == stats_of(text, **self.okw)
        return x

    def same_search(self, queries, mode="all", **kw):
        """search_resident against a one-pass job over the lines that are left."""
        got = self.e.search_resident(queries, mode, **kw)
        want = lc.search_text(self.text, queries, mode, first_line=self.first, **kw)
        assert got.first_line == want.first_line == self.first
        for i in range(len(queries)):
            assert got.lines(i) == want.lines(i)
            assert got.text(i) == want.text(i) and got.spans(i) == want.spans(i)
        assert got.format() == want.format()
        return got


def check(engine, pieces, drops, first_line=0, **okw):
    """The pieces indexed and appended, then every drop checked against the oracle."""
    w = Window(engine, pieces[0], first_line, **okw)
    for p in pieces[1:]:
        w.append(p)
    x = None
    for d in drops:
        x = w.drop(d)
    return w, x


# ---- tiny ----

@pytest.mark.parametrize("pieces, drops", [
    ([b"a b\n", b"b c\n"], [0]),
    ([b"a b\n", b"b c\n"], [1]),
    ([b"a b\n", b"b c\n"], [2]),
    ([b"a b\n", b"b c"], [2]),
    ([b"a b\n", b"b c"], [1, 1]),
    ([b"\n\n", b"\n"], [1, 2]),
    ([b"a b\nb c\nc d\n"], [1]),
    ([b"a b\nb c"], [2]),
    ([b"", b""], [0]),
], ids=["nothing", "one-of-two", "all", "all-no-final-newline", "last-line-alone", "blank-lines",
        "pass-buffers", "pass-buffers-all-no-final-newline", "empty"])
def test_tiny(eng, pieces, drops):
    w, _x = check(eng, pieces, drops)
    if w.lines:  # the text and the line starts are those of one pass
        w.same_search([[b"b"], [b"c"]], "all", show=10)


def test_a_drop_of_nothing_allocates_nothing():
    fresh = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    fresh.run_index(b"a b\nb c\n", 3)
    dr = fresh.drop_index(0)
    assert (dr.first_line, dr.num_lines, dr.num_tokens, dr.num_unique) == (3, 2, 4, 3)
    assert dr.store_bytes == 0 == fresh._eng.stats()["index_store_bytes"]
    assert fresh.drop_index(1).store_bytes == fresh._eng.stats()["index_store_bytes"] > 0


def test_a_drop_behind_a_search_job(eng):
    a, b = SHAPES["all_old"]
    w = Window(eng, a + b, 7, search=[[b"m003"]])
    w.drop(nlines(a))
    w.same_search([[b"m003"], [b"m029"]], "all", show=20)


def test_drop_append_drop(eng):
    w = Window(eng, b"a b\nb c\nc d\n")
    w.drop(1)
    w.append(b"d e\ne a\n")
    x = w.drop(2)
    assert x.postings() == oracle.index(b"d e\ne a\n", first_line=3)[1]
    w.append(b"a")
    w.drop(1)
    w.same_search([[b"a"], [b"e"]], "any", show=5)


def test_drop_everything_then_append(eng):
    w = Window(eng, b"a b\nb c", 5)  # (the last line lacks its newline, and goes too)
    x = w.drop(2)
    assert (x.entries(), x.postings(), x.first_line, x.num_lines) == ([], [], 7, 0)
    assert eng.search_resident([[b"a"]], "all").lines(0) == []
    w.append(b"c a\n")  # an empty resident text counts as ending in a newline
    w.append(b"a\n")
    assert w.compare().postings() == [7, 8, 7]
    w.same_search([[b"a"]], "all", show=5)


# ---- the cut ----

def test_duplicates_at_the_cut(eng):
    text = b"x\nm m\nm m\nm\n"
    w, x = check(eng, [text], [2])
    assert dict((k, c) for k, _v, c in x.entries()) == {b"m": 3}
    assert x.postings() == [2, 2, 3]  # both of line 2's are kept, both of line 1's are gone
    assert w.drop(1).postings() == [3]


VANISH = {
    "none": lambda i: False,
    "all": lambda i: True,
    "first": lambda i: i == 0,
    "last": lambda i: i == 39,
    "every_other": lambda i: i % 2 == 0,
    "runs": lambda i: (i // 5) % 2 == 1,
}


@pytest.mark.parametrize("pattern", sorted(VANISH))
def test_which_words_vanish(eng, pattern):
    ws = words(b"w", 40)
    gone = [w for i, w in enumerate(ws) if VANISH[pattern](i)]
    stay = [w for i, w in enumerate(ws) if not VANISH[pattern](i)]
    old = text_of(gone + stay)            # every word is in the lines that go
    new = text_of(stay) if stay else b"\n\n"  # only the survivors are in the lines that stay
    w, x = check(eng, [old, new], [nlines(old)])
    assert [k for k, _v, _c in x.entries()] == stay
    assert w.unique == len(stay)


# ---- skew and tile edges ----

@pytest.mark.parametrize("cut", [0, 1, TILE - 1, TILE, TILE + 1, 2053, 4999, 5000])
def test_a_cut_inside_a_list_longer_than_any_tile(eng, cut):
    """`the` once on each of 5000 lines, among 300 one-posting words on every 16th line: a drop
    of `cut` lines cuts `cut` elements off the long list, the singles above the cut vanish."""
    singles = words(b"a", 150) + words(b"u", 150)  # below and above "the"
    rows = [b"the"] * 5000
    for i, s in enumerate(singles):
        rows[i * 16] = b"the " + s
    text = b"".join(r + b"\n" for r in rows) + b"zz tail\n"
    _w, x = check(eng, [text], [cut])
    counts = dict((k, c) for k, _v, c in x.entries())
    assert counts.get(b"the", 0) == 5000 - cut
    assert len(counts) == 2 + (5000 - cut > 0) + sum(1 for i in range(300) if i * 16 >= cut)


@pytest.mark.parametrize("length", [63, 64, 65, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("lead", [0, 1, 5])
def test_kept_list_lengths_around_the_tile(eng, length, lead):
    """A kept list of `length` elements that starts `lead` elements into its destination tile,
    with one-posting neighbours behind it; 7 of its elements and 9 whole words are dropped."""
    old = b"m\n" * 7 + b"".join(w + b"\n" for w in words(b"b", 9))
    new = b"".join(w + b"\n" for w in words(b"a", lead)) + b"m\n" * length + \
        b"".join(w + b"\n" for w in words(b"z", 3))
    _w, x = check(eng, [old, new], [nlines(old)])
    assert dict((k, c) for k, _v, c in x.entries())[b"m"] == length
    assert [v for k, v, _c in x.entries() if k == b"m"] == [lead]


def test_more_words_than_one_scan_tile(eng):
    ws = [b"g%04d" % i for i in range(4500)]
    old, new = text_of(ws[:3000], 10), text_of(ws[1500:], 10)
    w, x = check(eng, [old, new], [nlines(old)])
    # the first 1500 words are gone entirely, the next 1500 lists are halved
    assert [k for k, _v, _c in x.entries()] == ws[1500:]
    assert [c for _k, _v, c in x.entries()] == [1] * 3000
    assert w.unique == 3000


# ---- the statistics walk ----

STAT_KW = dict(emits=3, max_key=5)


def stat_rows(n):
    kinds = [
        b"ab cd",                                      # plain
        b"alphabet beta gamma delta",                  # over the cap; one long token in the first 3
        b"x " * 40 + b"longwordhere",                  # > 64 bytes; the long token is past the cap
        b" " * 60 + b"straddles the boundary",         # a long token across the 64-byte step
        b"abcdefg\0hidden tokens after the nul here",  # a NUL ends the line's tokens
        b"." * 130 + b"farawaytoken x",                # > 128 bytes of delimiters first
        b"one two three",                              # exactly the cap: no overflow
        b"ok\0" + b"y " * 50,                          # a NUL before what would overflow
        b"q " * 2 + b"w" * 70,                         # a token longer than a step, inside the cap
        b"",
    ]
    return [kinds[i % len(kinds)] + b"\n" for i in range(n)]


@pytest.fixture(scope="module")
def stat_eng():
    return lc.Engine(gpu_cfg(emits_per_line=3, max_key_len=5), 1 << 16, 1 << 10)


@pytest.mark.parametrize("d", [1, 63, 64, 65])
def test_the_statistics_of_the_dropped_lines(stat_eng, d):
    rows = stat_rows(140)
    rows[0] = b"alphabet beta gamma delta\n"  # a drop of one line has something to count
    text = b"".join(rows)
    w, x = check(stat_eng, [text[:len(b"".join(rows[:70]))], b"".join(rows[70:])], [d], **STAT_KW)
    gone = stats_of(b"".join(rows[:d]), **STAT_KW)
    assert gone[0] > 0 and gone[1] > 0
    got = (x.overflow_lines, x.truncated, x.max_key_len)
    one = stat_eng.run_index(w.text, w.first)  # the one-pass job over the remainder
    assert got[:2] == (one.overflow_lines, one.truncated) and got[2] >= one.max_key_len
    assert one.overflow_lines > 0 and one.truncated > 0


# ---- first line ----

def test_a_first_line_of_1000(eng):
    a, b = SHAPES["interleaved"]
    w, x = check(eng, [a, b, a], [nlines(a) + 3], first_line=1000)
    assert x.first_line == min(x.postings()) == 1000 + nlines(a) + 3
    got = w.same_search([[b"zz"], [b"aa"]], "all", show=20)
    assert got.lines(0) == [1000 + 2 * nlines(a) + nlines(b) - 1]
    assert got.lines(1) == [1000 + nlines(a) + nlines(b) - 1]


# ---- sliding window ----

def hamlet_pieces(hamlet, n):
    lines = hamlet.split(b"\n")[:-1]
    step = (len(lines) + n - 1) // n
    pieces = [b"".join(l + b"\n" for l in lines[i:i + step]) for i in range(0, len(lines), step)]
    assert len(pieces) == n and b"".join(pieces) == hamlet
    return pieces, step


def test_sliding_window_on_hamlet(hamlet):
    pieces, step = hamlet_pieces(hamlet, 12)
    size = max(len(p) for p in pieces)
    sliding, growing = lc.Engine(gpu_cfg(), size, step), lc.Engine(gpu_cfg(), size, step)
    w = Window(sliding, pieces[0])
    growing.run_index(pieces[0])
    for b in range(1, 12):
        w.append(pieces[b])
        last = growing.append_index(pieces[b])
        assert len(w.lines) <= 3 * step  # at most 3 blocks at once
        if b + 1 > 2:
            w.drop(nlines(pieces[b - 2]))
            assert w.text == pieces[b - 1] + pieces[b]
    assert w.first == nlines(b"".join(pieces[:10]))
    # the growing store's halves hold 11 and 12 blocks, the sliding store's never more than 3
    # (half as much again when they were sized): the window's store stays strictly smaller
    assert last.num_lines == nlines(hamlet)
    slid, grown = (e._eng.stats()["index_store_bytes"] for e in (sliding, growing))
    print("index_store_bytes: sliding", slid, "growing", grown)
    assert 0 < slid < grown


# ---- search equivalence ----

BATCHES = [
    ("all", dict(queries=[[b"to", b"be"], [b"Hamlet"]], mode="all")),
    ("any", dict(queries=[[b"to", b"be"], [b"king", b"queen"]], mode="any")),
    ("phrase", dict(queries=[[b"to", b"be"], [b"my", b"lord"]], mode="phrase")),
    ("near", dict(queries=[[b"be", b"to"]], mode="near", within=3)),
    ("expr", dict(queries=[b"( to AND be ) OR ( king AND NOT queen )"], mode="expr")),
    ("rank", dict(queries=[[b"to", b"be"], [b"king"]], mode="any", rank=5)),
    ("wildcard", dict(queries=[[b"Ham*"]], mode="all", wildcard=True)),
    ("glob", dict(queries=[[b"*ing"]], mode="all", glob=True)),
    ("fuzzy", dict(queries=[[b"Hamlet~1"]], mode="all", fuzzy=True)),
    ("regex", dict(queries=[[b"/(king|queen)[!?]?/"]], mode="all", regex=True)),
    ("exclude", dict(queries=[[b"to", b"be"]], mode="all", exclude=[[b"not"]])),
    ("show", dict(queries=[[b"to", b"be"]], mode="phrase", show=80)),
    ("tally", dict(queries=[[b"to", b"be"]], mode="all", tally=6)),
]


@pytest.fixture(scope="module")
def hamlet_engines(hamlet):
    """(an engine built from 6 blocks of Hamlet with the first two blocks' lines dropped -- one
    drop mid-way, one at the end --, a one-pass engine, the window's text and first line)."""
    pieces, step = hamlet_pieces(hamlet, 6)
    windowed = lc.Engine(gpu_cfg(), max(len(p) for p in pieces), step)
    windowed.run_index(pieces[0])
    for b in range(1, 6):
        windowed.append_index(pieces[b])
        if b == 3:
            windowed.drop_index(nlines(pieces[0]))
    windowed.drop_index(nlines(pieces[1]))
    text = b"".join(pieces[2:])
    whole = lc.Engine(gpu_cfg(), len(text), nlines(text))
    return windowed, whole, text, nlines(pieces[0]) + nlines(pieces[1])


@pytest.mark.parametrize("name, batch", BATCHES, ids=[n for n, _b in BATCHES])
def test_search_on_the_window_equals_the_one_pass_run(hamlet_engines, name, batch):
    windowed, whole, text, first = hamlet_engines
    kw = dict(batch)
    queries, mode = kw.pop("queries"), kw.pop("mode")
    want = whole.run_search(text, queries, mode, first, **kw)
    got = windowed.search_resident(queries, mode, **kw)
    assert got.first_line == want.first_line == first
    assert got.hits() == want.hits() and got.matches() == want.matches()
    assert sum(want.hits()) > 0
    for i in range(len(queries)):
        assert got.lines(i) == want.lines(i)
        assert got.term_counts(i) == want.term_counts(i)
        assert got.scores(i) == want.scores(i)
        assert got.text(i) == want.text(i) and got.spans(i) == want.spans(i)
        assert got.tally(i) == want.tally(i)
    assert (got.merged, got.walked) == (want.merged, want.walked)
    assert (got.tally_words(), got.tally_tokens()) == (want.tally_words(), want.tally_tokens())
    assert (got.num_lines, got.num_tokens, got.num_unique, got.overflow_lines, got.truncated) == \
        (want.num_lines, want.num_tokens, want.num_unique, want.overflow_lines, want.truncated)
    assert got.format() == want.format()


def test_the_windows_index_resident(hamlet_engines):
    windowed, whole, text, first = hamlet_engines
    x, one = windowed.index_resident(), whole.run_index(text, first)
    assert x.entries() == one.entries() and x.postings_bytes() == one.postings_bytes()
    assert x.first_line == one.first_line == first and x.format() == one.format()


# ---- fuzz ----

@pytest.mark.parametrize("seed", range(20))
def test_fuzz(eng, seed):
    rng = random.Random(3000 + seed)
    text = fuzz_text(rng) + fuzz_text(rng)
    lines = text.split(b"\n")[:-1]
    nblocks = rng.randrange(2, 6)
    cuts = sorted(rng.randrange(0, len(lines) + 1) for _ in range(nblocks - 1))
    cuts = [0] + cuts + [len(lines)]
    pieces = [b"".join(l + b"\n" for l in lines[i:j]) for i, j in zip(cuts, cuts[1:])]
    if rng.random() < 0.3 and pieces[-1]:
        pieces[-1] = pieces[-1][:-1]

    def some(n):
        return rng.choice([0, n, rng.randrange(0, n + 1), rng.randrange(0, n + 1)])
    w = Window(eng, pieces[0], seed * 7)
    for p in pieces[1:]:
        for _ in range(rng.randrange(0, 3)):
            w.drop(some(len(w.lines)))
        w.append(p)
    w.drop(some(len(w.lines)))
    w.drop(0)
    w.drop(len(w.lines))


# ---- refusals keep the index ----

def test_refused_without_a_resident_index():
    fresh = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    with pytest.raises(lc.LocustError, match="drop_index.*stale"):
        fresh.drop_index(1)
    fresh.run_index(b"a b\n")
    fresh.run(b"c d\n")  # any other job overwrites what the index reads
    with pytest.raises(lc.LocustError, match="drop_index.*stale"):
        fresh.drop_index(0)
    fresh.run_index(b"a b\nb c\n")
    fresh.drop_index(1)
    assert fresh.index_resident().postings() == oracle.index(b"b c\n", first_line=1)[1]


def test_too_many_lines_are_refused_and_the_index_stays():
    small = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    for appended in (False, True):  # in the pass buffers, then in the store
        small.run_index(b"a b\nb c\n", 10)
        if appended:
            small.append_index(b"b\n")
        n = 3 if appended else 2
        before = small.search_resident([[b"b"]], "all").lines(0)
        with pytest.raises(lc.LocustError, match="%d lines to drop.*holds %d" % (n + 1, n)):
            small.drop_index(n + 1)
        assert small.search_resident([[b"b"]], "all").lines(0) == before
        small.append_index(b"b d\n")  # (still appendable)
        assert small.search_resident([[b"b"]], "all").lines(0) == before + [10 + n]
        small.drop_index(n)
        x = small.index_resident()
        assert (x.entries(), x.postings()) == oracle.index(b"b d\n", first_line=10 + n)


# ---- the helpers and the CLI ----

def test_python_helpers_take_keep_blocks(hamlet):
    text = oracle.window(hamlet, 0, 900)
    blocks = lc.split_blocks(text, 8192, 3)
    assert len(blocks) > 3
    off, _n, _l, first = blocks[-2]
    window = text[off:]
    x = lc.index_text(text, block_bytes=8192, keep_blocks=2, first_line=3)
    assert (x.entries(), x.postings()) == oracle.index(window, first_line=first)
    assert x.first_line == first
    one = lc.index_text(window, first_line=first)
    assert (x.num_lines, x.num_tokens, x.num_unique) == (one.num_lines, one.num_tokens, one.num_unique)
    got = lc.search_text(text, [[b"my", b"lord"]], "phrase", show=40, block_bytes=8192,
                         keep_blocks=2, first_line=3)
    want = lc.search_text(window, [[b"my", b"lord"]], "phrase", show=40, first_line=first)
    assert got.lines(0) == want.lines(0) and got.lines(0) and got.format() == want.format()
    assert got.first_line == first


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith((b"print ", b"  ")))


@pytest.mark.parametrize("args", [
    ["--search", "to be", "--match", "phrase", "--show", "80", "--mark"],
    ["--index"],
], ids=["search", "index"])
def test_cli_keep_blocks(cli, hamlet, args, tmp_path):
    j = tmp_path / "k.json"
    blocks = lc.split_blocks(hamlet, 32 << 10)
    assert len(blocks) == 6
    start, total = blocks[-2][3], nlines(hamlet)

    def run(*more):
        return subprocess.run([cli, "data/hamlet.txt", *map(str, more)],
                              capture_output=True, timeout=300, cwd=ROOT)
    want = run(start, total, *args)
    got = run(*args, "--block-kb", 32, "--keep-blocks", 2, "--json", j)
    assert want.returncode == 0 and got.returncode == 0, got.stderr.decode()[-2000:]
    assert result_lines(want.stdout) and result_lines(got.stdout) == result_lines(want.stdout)
    rec = json.load(open(j))
    assert rec["blocks"] == 6 and rec["dropped_blocks"] == 4 and rec["drop_ms"] > 0
    assert rec["first_line"] == start and rec["index_store_bytes"] > 0
