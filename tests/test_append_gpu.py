"""Appending to the index on the device (csrc/kernels/append.hip): after ``run_index(t0)``,
``append_index(t1)``, ..., ``append_index(tk)`` the resident index is the index of
``t0 + t1 + ... + tk`` -- ``index_resident()`` against the oracle, exactly, and every search
feature against ``run_search`` of the whole text on a one-pass engine, field for field.

The shapes are the smallest at which each kernel can go wrong: the five key orders of the
records merge, a list longer than any postings tile (``kAppendTile`` = 1024 source elements)
among one-posting neighbours, lists of T - 1, T, T + 1 elements for T = 1024 and 64, more distinct
words than one scan tile (``kIndexTile`` = 2048) on either side, blocks of 1, 63, 64 and 65 lines,
a store that is reallocated several times, a non-zero first line."""
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


def build(engine, pieces, first_line=0):
    engine.run_index(pieces[0], first_line)
    return [engine.append_index(p) for p in pieces[1:]]


def check(engine, pieces, first_line=0, **okw):
    """The pieces indexed and appended, index_resident() against the oracle's index of their
    concatenation; the appends' own figures."""
    aps = build(engine, pieces, first_line)
    text = b"".join(pieces)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    x = engine.index_resident()
    assert x.entries() == ent
    assert x.postings() == post
    assert x.first_line == first_line and x.num_lines == nlines(text)
    assert x.num_tokens == len(post) and x.num_unique == len(ent)
    lines, seen = nlines(pieces[0]), {k for k, _v, _c in oracle.index(pieces[0], **okw)[0]}
    for ap, p in zip(aps, pieces[1:]):
        mine = oracle.index(p, **okw)
        lines += nlines(p)
        assert (ap.block_lines, ap.block_tokens, ap.block_unique) == \
            (nlines(p), len(mine[1]), len(mine[0]))
        assert ap.fresh_words == len({k for k, _v, _c in mine[0]} - seen)
        seen |= {k for k, _v, _c in mine[0]}
        assert ap.num_lines == lines and ap.num_unique == len(seen)
        assert ap.append_ms > 0 and ap.store_bytes > 0
    if aps:
        assert aps[-1].num_tokens == len(post)
    return x


# ---- tiny ----

@pytest.mark.parametrize("pieces", [
    [b"a b\n", b"b c\n"],
    [b"", b"a b\nb c\n"],
    [b"a b\nb c\n", b""],
    [b"\n\n", b"x\n"],
    [b"a b\n", b"b c"],
    [b"", b""],
    [b"\n", b"\n\n", b"a\n", b"", b"a"],
], ids=["two", "empty-first", "empty-block", "blank-lines", "no-final-newline", "both-empty",
        "mixed"])
def test_tiny(eng, pieces):
    check(eng, pieces)
    text = b"".join(pieces)
    if b"a" in text:  # the text and the line starts are those of one pass
        got = eng.search_resident([[b"a"]], "all", show=10)
        one = lc.search_text(text, [[b"a"]], "all", show=10)
        assert got.lines(0) == one.lines(0) and got.text(0) == one.text(0)


# ---- key order ----

@pytest.mark.parametrize("shape", ["all_new", "all_old", "interleaved", "all_before", "all_after"])
def test_key_orders(eng, shape):
    check(eng, list(SHAPES[shape]))


def test_truncation_and_the_emit_cap():
    a = b"alphabet alpha alphas beta\nbetamax gamma gamma\n"
    b = b"alphanumeric betas delta\ngamma alpha\n"
    small = lc.Engine(gpu_cfg(emits_per_line=2, max_key_len=5), 1 << 16, 1 << 10)
    x = check(small, [a, b], emits=2, max_key=5)
    one = small.run_index(a + b)  # the statistics add up to the one-pass job's
    assert (x.overflow_lines, x.truncated, x.max_key_len) == \
        (one.overflow_lines, one.truncated, one.max_key_len)
    assert x.overflow_lines == 3 and x.truncated > 0


# ---- skew and tile edges ----

def test_a_list_longer_than_any_tile_among_single_postings(eng):
    def side(tag):
        singles = words(tag, 150) + words(b"u" + tag, 150)  # below and above "the"
        rows = [b"the"] * 5000
        for i, w in enumerate(singles):
            rows[i * 16] = b"the " + w
        return b"".join(r + b"\n" for r in rows)
    x = check(eng, [side(b"a"), side(b"b")])
    assert dict((k, c) for k, _v, c in x.entries())[b"the"] == 10000


@pytest.mark.parametrize("length", [63, 64, 65, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("lead", [0, 1, 5])
def test_list_lengths_around_the_tile(eng, length, lead):
    """A list of `length` elements that starts `lead` elements into its tile, with one-posting
    neighbours on either side, in A and in B."""
    def side(tag, n):
        before = b"".join(w + b"\n" for w in words(b"a" + tag, lead))
        after = b"".join(w + b"\n" for w in words(b"z" + tag, 3))
        return before + b"m\n" * n + after
    check(eng, [side(b"p", length), side(b"q", length + 1), side(b"p", 2 * length)])


def test_more_words_than_one_scan_tile_on_either_side(eng):
    ws = [b"g%04d" % i for i in range(4500)]
    a, b = text_of(ws[:3000], 10), text_of(ws[1500:], 10)
    x = check(eng, [a, b])
    assert x.num_unique == 4500
    counts = [c for _k, _v, c in x.entries()]
    assert counts[:1500] == [1] * 1500 and counts[1500:3000] == [2] * 1500


# ---- lines ----

def test_block_line_counts_and_the_text(eng):
    rows = [b"row %d filler w%d" % (i, i % 7) for i in range(1 + 63 + 64 + 65 + 10)]
    cuts = [0, 1, 64, 128, 193, len(rows)]
    rows[64] = b"first line of a block"      # the third block's first line
    rows[63] = b"last line of a block"       # the second block's last line
    rows[150] = b"deep in the fourth block, past the shown bytes"
    pieces = [b"".join(r + b"\n" for r in rows[i:j]) for i, j in zip(cuts, cuts[1:])]
    assert [nlines(p) for p in pieces] == [1, 63, 64, 65, 10]
    check(eng, pieces)
    text = b"".join(pieces)
    queries = [[b"first", b"line", b"of"], [b"last", b"line", b"of"], [b"fourth", b"block"]]
    got = eng.search_resident(queries, "phrase", show=30)
    assert [got.lines(i) for i in range(3)] == [[64], [63], [150]]
    one = lc.search_text(text, queries, "phrase", show=30)
    for i in range(3):
        assert got.text(i) == one.text(i) and got.spans(i) == one.spans(i)
    assert got.text(2) == [rows[150][:30]] and got.cut_lines == one.cut_lines == 1


# ---- growth ----

def test_the_store_grows(hamlet):
    small = lc.Engine(gpu_cfg(), 1 << 16, 1 << 11)
    assert small._eng.stats()["index_store_bytes"] == 0
    lines = hamlet.split(b"\n")
    pieces, at = [b"".join(l + b"\n" for l in lines[:3])], 3
    assert len(pieces[0]) <= 100
    for i in range(8):
        n = 6 << i
        pieces.append(b"".join(l + b"\n" for l in lines[at:at + n]))
        at += n
    aps = build(small, pieces)
    x = small.index_resident()
    assert (x.entries(), x.postings()) == oracle.index(b"".join(pieces))
    sizes = [ap.store_bytes for ap in aps]
    assert sizes == sorted(sizes) and len(set(sizes)) >= 4  # reallocated several times
    assert small._eng.stats()["index_store_bytes"] == sizes[-1] > 0
    # a fresh index on the same engine, and appends to it, reuse the store
    check(small, [pieces[1], pieces[2]])


# ---- first line ----

def test_a_first_line(eng):
    a, b = SHAPES["interleaved"]
    x = check(eng, [a, b, a], first_line=1000)
    assert min(x.postings()) == 1000
    got = eng.search_resident([[b"zz"], [b"aa"]], "all")
    assert got.first_line == 1000
    assert got.lines(0) == [1000 + nlines(a) - 1, 1000 + 2 * nlines(a) + nlines(b) - 1]
    assert got.lines(1) == [1000 + nlines(a) + nlines(b) - 1]


def test_appending_behind_a_search_job(eng):
    a, b = SHAPES["all_old"]
    eng.run_search(a, [[b"m003"]], "all", 7)
    eng.append_index(b)
    x = eng.index_resident()
    assert (x.entries(), x.postings()) == oracle.index(a + b, first_line=7)


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
README_HITS = {"all": 47, "phrase": 27, "near": 31, "wildcard": 464, "glob": 536, "fuzzy": 108}


@pytest.fixture(scope="module")
def hamlet_engines(hamlet):
    """(an engine that holds Hamlet built from 6 blocks, a one-pass engine for the whole)."""
    lines = hamlet.split(b"\n")[:-1]
    step = (len(lines) + 5) // 6
    pieces = [b"".join(l + b"\n" for l in lines[i:i + step]) for i in range(0, len(lines), step)]
    assert len(pieces) == 6 and b"".join(pieces) == hamlet
    blocked = lc.Engine(gpu_cfg(), max(len(p) for p in pieces), step)
    build(blocked, pieces)
    whole = lc.Engine(gpu_cfg(), len(hamlet), len(lines))
    return blocked, whole


@pytest.mark.parametrize("name, batch", BATCHES, ids=[n for n, _b in BATCHES])
def test_search_on_hamlet_equals_the_one_pass_run(hamlet_engines, hamlet, name, batch):
    blocked, whole = hamlet_engines
    kw = dict(batch)
    queries, mode = kw.pop("queries"), kw.pop("mode")
    want = whole.run_search(hamlet, queries, mode, **kw)
    got = blocked.search_resident(queries, mode, **kw)
    assert got.hits() == want.hits() and got.matches() == want.matches()
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
    if name in README_HITS:
        assert got.hits()[0] == README_HITS[name]


def test_hamlet_index_resident(hamlet_engines, hamlet):
    blocked, whole = hamlet_engines
    x, one = blocked.index_resident(), whole.run_index(hamlet)
    assert x.entries() == one.entries() and x.postings_bytes() == one.postings_bytes()
    assert x.format() == one.format()
    # index_resident of an index no append has touched: the pass buffers
    again = whole.index_resident()
    assert again.entries() == one.entries() and again.postings_bytes() == one.postings_bytes()


# ---- fuzz ----

@pytest.mark.parametrize("seed", range(20))
def test_fuzz(eng, seed):
    rng = random.Random(1000 + seed)
    text = fuzz_text(rng) + fuzz_text(rng)
    lines = text.split(b"\n")[:-1]
    nblocks = rng.randrange(2, 6)
    cuts = sorted(rng.randrange(0, len(lines) + 1) for _ in range(nblocks - 1))
    cuts = [0] + cuts + [len(lines)]
    pieces = [b"".join(l + b"\n" for l in lines[i:j]) for i, j in zip(cuts, cuts[1:])]
    if rng.random() < 0.3 and pieces[-1]:
        pieces[-1] = pieces[-1][:-1]
    check(eng, pieces, first_line=seed * 7)


# ---- refusals keep the index ----

def test_refused_without_a_resident_index():
    fresh = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    with pytest.raises(lc.LocustError, match="stale"):
        fresh.append_index(b"a b\n")
    with pytest.raises(lc.LocustError, match="stale"):
        fresh.index_resident()
    fresh.run_index(b"a b\n")
    fresh.run(b"c d\n")  # any other job overwrites what the index reads
    with pytest.raises(lc.LocustError, match="stale"):
        fresh.append_index(b"b c\n")
    fresh.run_index(b"a b\n")
    fresh.append_index(b"b c\n")
    assert fresh.index_resident().postings() == oracle.index(b"a b\nb c\n")[1]


def test_refusals_leave_the_index_searchable():
    small = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    small.run_index(b"a b\nb c\n")
    before = small.search_resident([[b"b"]], "all").lines(0)
    with pytest.raises(lc.LocustError, match="one device pass"):
        small.append_index(b"b too long\n" * 20000)  # larger than the pass
    assert small.search_resident([[b"b"]], "all").lines(0) == before == [0, 1]
    small.append_index(b"b d")  # (still appendable; and now the text lacks its last newline)
    assert small.search_resident([[b"b"]], "all").lines(0) == [0, 1, 2]
    with pytest.raises(lc.LocustError, match="newline"):
        small.append_index(b"e\n")
    got = small.search_resident([[b"b"], [b"d"]], "all", show=8)
    assert got.lines(0) == [0, 1, 2] and got.text(1) == [b"b d"]
    x = small.index_resident()
    assert (x.entries(), x.postings()) == oracle.index(b"a b\nb c\nb d")


def test_a_wrong_first_line_is_refused():
    small = lc.Engine(gpu_cfg(), 1 << 12, 1 << 8)
    small.run_index(b"a b\nb c\n", 10)
    with pytest.raises(lc.LocustError, match="line 12"):
        small._eng.append_index(b"x\n", 11)
    small._eng.append_index(b"x\n", 12)
    assert small.search_resident([[b"x"]], "all").lines(0) == [12]


# ---- the helpers and the CLI ----

def test_python_helpers_take_block_bytes(hamlet):
    text = oracle.window(hamlet, 0, 900)
    x = lc.index_text(text, block_bytes=8192, first_line=3)
    assert (x.entries(), x.postings()) == oracle.index(text, first_line=3)
    got = lc.search_text(text, [[b"to", b"be"]], "phrase", show=40, block_bytes=8192)
    want = lc.search_text(text, [[b"to", b"be"]], "phrase", show=40)
    assert got.format() == want.format()


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith((b"print ", b"  ")))


@pytest.mark.parametrize("args", [
    ["--search", "to be", "--match", "phrase", "--show", "80", "--mark"],
    ["--index"],
], ids=["search", "index"])
def test_cli_block_kb(cli, args, tmp_path):
    j = tmp_path / "b.json"
    def run(*more):
        return subprocess.run([cli, "data/hamlet.txt", *args, *map(str, more)],
                              capture_output=True, timeout=300, cwd=ROOT)
    want, got = run(), run("--block-kb", 32, "--json", j)
    assert want.returncode == 0 and got.returncode == 0, got.stderr.decode()[-2000:]
    assert result_lines(want.stdout) and result_lines(got.stdout) == result_lines(want.stdout)
    rec = json.load(open(j))
    assert rec["blocks"] == 6 and rec["append_ms"] > 0 and rec["index_store_bytes"] > 0
