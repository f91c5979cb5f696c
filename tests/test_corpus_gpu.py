"""Corpus search on the device (csrc/kernels/corpus.hip; engine.hpp "corpus", "file sets"): the
segment table an engine keeps beside its resident index, and the restrict stage that cuts a
batch's hits down to its queries' file sets before anything is sorted or scored.  Every case is
compared with the oracle (oracle.CORPUS_RULES) and, field for field, with the host twin over the
downloaded index.

The shapes are the smallest at which the stage can go wrong: one segment and two with hits on
either side of the boundary, empty files in front, between (two in a row) and behind, a non-zero
first line, more files than two words of a set's bitmap (32 bits each) with hits in the files at
the word edges, no hit at all, sets that keep everything and nothing, ids that are not resident,
63 / 64 / 65 hits (a wave) and T - 1 / T / T + 1 hits for the stage's tile T = kCorpusTile with
the kept pairs in the first and the last line, sets shared between queries, and every mode."""
import random

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.corpus_cases import SMALL, Corpus, hamlet_files, same_result, twin, want

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 1024  # kCorpusTile: pairs per workgroup and step of the restrict kernel, keys per
             # workgroup of the head kernels
LDS_SEGS = 2048  # kCorpusLdsSegs: the longest table the resolve kernel stages in LDS


def gpu_cfg(**kw):
    return lc.make_config("gpu", check=True, **kw)


@pytest.fixture(scope="module")
def eng():
    """One engine of 1 MiB for every case."""
    return lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)


def build(eng, texts, first_line=0, new_file=None):
    """The texts indexed and appended (new_file[i]: text i begins a file; default: every one)."""
    c = Corpus(texts[0], first_line)
    eng.run_index(texts[0], first_line)
    for i, t in enumerate(texts[1:], 1):
        nf = True if new_file is None else new_file[i]
        ap = eng.append_index(t, new_file=nf)
        c.append(t, nf)
        assert ap.files == len(c.table)
    assert eng.segments() == c.table
    return c


def check(eng, c, queries, mode="all", files=None, rank=None, within=None, exclude=None, **kw):
    """One batch against the oracle, query by query, and against the host twin."""
    got = eng.search_resident(queries, mode, rank=rank, within=within, exclude=exclude,
                              files=files, **kw)
    modes = [mode] * len(queries) if isinstance(mode, str) else mode
    text = c.text
    unrestricted = 0
    for i, q in enumerate(queries):
        f = None if files is None else files[i]
        w = within[i] if isinstance(within, list) else within
        x = None if exclude is None else exclude[i]
        okw = dict(first_line=c.first, within=w if modes[i] == "near" else None, exclude=x)
        okw.update({k: v for k, v in kw.items() if k in ("wildcard", "glob", "ignore_case")})
        ref = want(text, c.table, q, modes[i], f, rank=rank, **okw)
        if rank is None:
            assert got.lines(i) == ref, (i, q, f)
        else:
            assert (list(zip(got.lines(i), got.scores(i))), got.matches()[i]) == ref, (i, q, f)
        unrestricted += len(want(text, c.table, q, modes[i], None, **okw))
        if kw.get("by_file"):  # every returned line's file and local number, and the counts
            ids, local, hits = oracle.by_file(c.table, got.lines(i))
            assert (got.files(i), got.local_lines(i), got.file_hits(i)) == (ids, local, hits), i
    assert got.segments() == c.table
    # what the stage removed: the matches without the sets minus the matches with them
    assert got.restricted == unrestricted - sum(got.matches())
    ref = twin(eng.index_resident(), text, queries, mode, files, rank, within, exclude, **kw)
    same_result(got, ref, len(queries))
    return got


# ---- locate ----
def test_one_segment(eng):
    c = build(eng, [b"alpha beta\nbeta\nalpha\n"])
    assert eng.segments() == [(0, 0, 0, 3)]
    got = check(eng, c, [[b"alpha"], [b"alpha"], [b"alpha"]], files=[[0], [1], None])
    assert [got.lines(i) for i in range(3)] == [[0, 2], [], [0, 2]]


def test_two_segments_with_hits_on_either_side_of_the_boundary(eng):
    c = build(eng, [b"x\nalpha\n", b"alpha\nx\n"])
    got = check(eng, c, [[b"alpha"]] * 4, files=[[0], [1], [0, 1], None])
    assert [got.lines(i) for i in range(4)] == [[1], [2], [1, 2], [1, 2]]


@pytest.mark.parametrize("first_line", [0, 4000000000])
def test_empty_files_in_front_between_and_behind(eng, first_line):
    c = build(eng, SMALL, first_line)
    assert [r[3] for r in eng.segments()] == [0, 2, 0, 0, 3, 1, 0]
    qs = [[b"alpha"], [b"beta"], [b"alpha", b"beta"], [b"delta"]]
    for f in ([1], [4], [5], [1, 5], [0, 2, 3, 6], [0, 1, 2, 3, 4, 5, 6]):
        check(eng, c, qs, "all", files=[f] * 4)
    check(eng, c, qs, "any", files=[[0], [4], [3, 4], [6]])


def test_more_files_than_two_bitmap_words(eng):
    # 70 one-line files: ordinals 31 | 32 and 63 | 64 lie in different words of a set
    texts = [b"w f%d\n" % i for i in range(70)]
    c = build(eng, texts)
    assert len(eng.segments()) == 70
    edges = [0, 31, 32, 33, 63, 64, 69]
    got = check(eng, c, [[b"w"]] * 5,
                files=[edges, [31], [32, 64], list(range(70)), list(range(1, 70, 2))])
    assert got.lines(0) == edges and got.restricted == 5 * 70 - (7 + 1 + 2 + 70 + 35)


# ---- restrict ----
def test_no_hit_at_all(eng):
    c = build(eng, [b"alpha\n", b"beta\n"])
    got = check(eng, c, [[b"nothing"], [b"alpha", b"beta"]], files=[[0], [1]])
    assert got.hits() == [0, 0] and got.restricted == 0


def test_sets_that_keep_everything_nothing_and_ids_that_are_not_resident(eng):
    c = build(eng, hamlet_files([30, 30, 30], 2000))
    got = check(eng, c, [[b"the"]] * 5, files=[[0, 1, 2], [7], [1, 7, 4000000000], [], None])
    assert got.lines(0) == got.lines(3) == got.lines(4) and got.lines(1) == []


@pytest.mark.parametrize("n", [63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_hits_around_a_wave_and_around_the_tile(eng, n):
    # n hits; the first and the last line are files of their own, the rest one file
    c = build(eng, [b"w\n", b"w\n" * (n - 2), b"w\n"])
    got = check(eng, c, [[b"w"]] * 4, files=[[0], [2], [0, 2], [1]])
    assert [got.lines(i) for i in range(3)] == [[0], [n - 1], [0, n - 1]]
    assert got.hits()[3] == n - 2 and got.restricted == 4 * n - (1 + 1 + 2 + n - 2)


def test_only_the_middle_query_has_a_set_and_sets_are_shared(eng):
    c = build(eng, hamlet_files([25, 40, 25], 300))
    check(eng, c, [[b"the"], [b"the"], [b"and"]], files=[None, [1], None])
    check(eng, c, [[b"the"], [b"and"], [b"of"]], files=[[0, 2], [0, 2], [1]])


def test_every_mode_under_a_set(eng):
    c = build(eng, hamlet_files([60, 60, 60], 1000))
    # verified candidates that the set then removes: the phrase and the window match in every file
    qs = [[b"of", b"the"], [b"the", b"and"], b"( the AND of ) OR ( and AND NOT to )", [b"the"],
          [b"the", b"to"]]
    modes = ["phrase", "near", "expr", "all", "any"]
    for f in ([1], [0, 2]):
        got = check(eng, c, qs, modes, files=[f] * 5, within=[None, 4, None, None, None],
                    exclude=[None, None, None, [b"of"], [b"and"]])
        assert got.restricted > 0
    check(eng, c, [[b"th*"], [b"*ing"]], "all", files=[[2], [1]], glob=True)


# ---- ranked ----
@pytest.mark.parametrize("k", [2, 1000])
def test_ranked_under_a_set(eng, k):
    c = build(eng, hamlet_files([50, 50, 50], 500))
    qs = [[b"the", b"and"], [b"of"], [b"the"]]
    got = check(eng, c, qs, "any", files=[[1], [0, 2], None], rank=k)
    full = eng.search_resident(qs, "any", rank=1000)  # scores do not change under a set
    for i, f in enumerate([[1], [0, 2]]):
        keep = set(want(c.text, c.table, qs[i], "any", f))
        pairs = [(l, s) for l, s in zip(full.lines(i), full.scores(i)) if l in keep]
        assert list(zip(got.lines(i), got.scores(i))) == pairs[:k]
        assert got.matches()[i] == len(pairs) and (k < len(pairs) or k == 1000)


def test_show_and_tally_over_a_restricted_answer(eng):
    c = build(eng, hamlet_files([40, 40], 100))
    got = check(eng, c, [[b"the"], [b"the"]], files=[[1], None], show=80, tally=5)
    lines = oracle.split_lines(c.text)
    assert got.text(0) == [lines[l][:80] for l in got.lines(0)]
    ent, post = oracle.index(c.text)
    assert got.tally(0) == oracle.tally(ent, post, got.lines(0), 5)[2]


# ---- by file ----
def test_by_file_over_empty_files_and_a_query_without_a_hit_between_two_with_hits(eng):
    c = build(eng, SMALL, 7)
    got = check(eng, c, [[b"alpha"], [b"nothing"], [b"beta"]], by_file=True)
    assert got.file_hits(0) == [(1, 2), (4, 1), (5, 1)] and got.file_hits(1) == []
    assert got.local_lines(2) == [0, 0, 2, 0] and got.files(2) == [1, 4, 4, 5]
    check(eng, c, [[b"alpha"], [b"beta"]], files=[[4, 5], [1]], by_file=True)
    check(eng, c, [[b"nothing"]], by_file=True)  # no returned line at all


def test_one_file_holding_all_hits_and_every_hit_in_its_own_file(eng):
    c = build(eng, [b"x\n", b"w\nw\nw\n", b"x\n"])
    assert check(eng, c, [[b"w"], [b"x"]], by_file=True).file_hits(0) == [(1, 3)]
    c = build(eng, [b"w f%d\n" % i for i in range(70)])
    got = check(eng, c, [[b"w"], [b"w"]], files=[None, [3, 64]], by_file=True)
    assert got.file_hits(0) == [(i, 1) for i in range(70)] and got.local_lines(0) == [0] * 70


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_runs_crossing_the_head_kernels_tile_edges(eng, n):
    # one long file between two one-line files: its run crosses every tile edge, and the second
    # query's runs begin where the first one's end
    c = build(eng, [b"w\n", b"w\n" * (n - 2), b"w\n"])
    got = check(eng, c, [[b"w"], [b"w"], [b"w"]], files=[None, None, [1]], by_file=True)
    assert got.file_hits(0) == got.file_hits(1) == [(0, 1), (1, n - 2), (2, 1)]
    assert got.file_hits(2) == [(1, n - 2)] and got.local_lines(0)[-2:] == [n - 3, 0]


def test_more_one_line_files_than_the_resolve_kernel_stages_in_lds(eng):
    # LDS_SEGS + 1 files: the table is read from global memory; one fewer: from LDS
    texts = [b"w f%d\n" % i for i in range(LDS_SEGS + 1)]
    c = Corpus(texts[0])
    eng.run_index(texts[0])
    for t in texts[1:-1]:
        eng.append_index(t, new_file=True)
        c.append(t, True)
    qs, sets = [[b"w"], [b"f2047"], [b"w"]], [None, None, [0, 31, 32, 2047, 2048]]
    assert len(eng.segments()) == LDS_SEGS
    check(eng, c, qs, files=sets, by_file=True)
    eng.append_index(texts[-1], new_file=True)
    c.append(texts[-1], True)
    assert len(eng.segments()) == LDS_SEGS + 1
    got = check(eng, c, qs + [[b"f2048"]], files=sets + [None], by_file=True)
    assert got.file_hits(3) == [(LDS_SEGS, 1)] and got.lines(2) == [0, 31, 32, 2047, 2048]


def test_ranked_winners_alternating_between_two_files(eng):
    # scores by tf: line 3 (file 1), 0 (file 0), 2 (file 1), 1 (file 0): the keys need the sort
    c = build(eng, [b"w w w\nw\n", b"w w\nw w w w\n"])
    got = check(eng, c, [[b"w"], [b"w"]], rank=4, by_file=True)
    assert got.lines(0) == [3, 0, 2, 1] and got.files(0) == [1, 0, 1, 0]
    assert got.local_lines(0) == [1, 0, 0, 1] and got.file_hits(0) == [(0, 2), (1, 2)]
    got = check(eng, c, [[b"w"], [b"w"]], rank=3, files=[None, [0]], by_file=True)
    assert got.file_hits(0) == [(0, 1), (1, 2)] and got.file_hits(1) == [(0, 2)]  # the winners only
    c = build(eng, hamlet_files([40, 40, 40], 1500))
    check(eng, c, [[b"the", b"and"], [b"of"]], "any", rank=25, files=[None, [0, 2]], by_file=True)


def test_count_only_copies_no_line(eng):
    c = build(eng, hamlet_files([50, 1, 50], 2500))
    qs, sets = [[b"the"], [b"nothing"], [b"and", b"the"]], [None, None, [0, 1]]
    full = check(eng, c, qs, ["all", "all", "any"], files=sets, by_file=True)
    plain = eng.search_resident(qs, ["all", "all", "any"], files=sets)
    got = eng.search_resident(qs, ["all", "all", "any"], files=sets, count_only=True)
    assert got.by_file == 2 and got.matches() == full.matches() and got.hits() == [0, 0, 0]
    for i in range(3):
        assert got.lines(i) == got.files(i) == got.local_lines(i) == []
        assert got.file_hits(i) == full.file_hits(i)
    runs, lines = sum(len(full.file_hits(i)) for i in range(3)), sum(full.hits())
    # exactly what is copied: the counters, the CSR -- and, without count_only, 4 B a line thrice
    assert full.wire_bytes - got.wire_bytes == 12 * lines
    assert got.wire_bytes == plain.wire_bytes - 4 * lines + 20 + 8 * 4 + 8 * runs
    ref = twin(eng.index_resident(), c.text, qs, ["all", "all", "any"], sets, count_only=True)
    same_result(got, ref, 3)
    for kw in ({"rank": 2}, {"show": 10}, {"tally": 3}):
        with pytest.raises(lc.LocustError, match="count_only"):
            eng.search_resident(qs, count_only=True, **kw)
    check(eng, c, qs, ["all", "all", "any"], files=sets, by_file=True)  # the index is intact


def test_show_and_tally_beside_answers_by_file(eng):
    c = build(eng, hamlet_files([40, 40], 100))
    got = check(eng, c, [[b"the"], [b"the"]], files=[[1], None], show=80, tally=5, by_file=True)
    assert got.files(0) == [1] * len(got.lines(0))


# ---- window ----
def window_step(eng, c, queries, sets):
    assert eng.segments() == c.table
    assert eng.index_resident().segments() == c.table
    check(eng, c, queries, "all", files=sets, by_file=True)
    for seg in c.table:  # local numbers stay the file's own
        if seg[3]:
            assert oracle.locate(c.table, seg[1]) == (seg[0], seg[2])


def test_files_block_by_block_and_drops_at_and_inside_files(eng):
    files = hamlet_files([30, 20, 25], 3000)
    whole = {i: oracle.split_lines(t) for i, t in enumerate(files)}
    blocks, flags = [], []
    for t in files:  # two blocks per file: the second extends the file
        ls = oracle.split_lines(t)
        half = len(ls) // 2
        blocks += [b"".join(l + b"\n" for l in ls[:half]), b"".join(l + b"\n" for l in ls[half:])]
        flags += [True, False]
    c = build(eng, blocks, 10, flags)
    assert c.table == oracle.segments_of(files, 10)
    qs, sets = [[b"the"], [b"the"], [b"and"]], [[0], [1, 2], None]
    window_step(eng, c, qs, sets)
    for d, gone in ((7, 0), (23, 1), (5, 0), (15, 1), (0, 0)):  # mid-file, boundary, mid, boundary
        dr = eng.drop_index(d)
        assert c.drop(d) == gone == dr.dropped_files
        window_step(eng, c, qs, sets)
    assert c.table == [(2, 60, 0, 25)]
    got = eng.search_resident([[b"the"]], files=[[0]])  # a set naming a dropped file answers empty
    assert got.lines(0) == [] and got.restricted == len(want(c.text, c.table, [b"the"],
                                                             first_line=c.first))
    for l in eng.search_resident([[b"the"]], files=[[2]]).lines(0):
        i, local = oracle.locate(c.table, l)
        assert b"the" in oracle.tokenize(whole[i][local])[0]
    dr = eng.drop_index(25)  # everything: the last file stays, empty
    assert c.drop(25) == 0 == dr.dropped_files and eng.segments() == [(2, 85, 25, 0)]
    eng.append_index(b"the end\n")
    c.append(b"the end\n")
    window_step(eng, c, [[b"the"]], [[2]])
    assert oracle.locate(eng.segments(), 85) == (2, 25)


def test_fuzz_over_seeded_random_corpora(eng):
    rnd = random.Random(20240607)
    words = [b"a", b"b", b"c", b"dd", b"ee"]

    def text(n):
        return b"".join(b" ".join(rnd.choice(words) for _ in range(rnd.randint(0, 4))) + b"\n"
                        for _ in range(n))

    for _round in range(20):
        c = Corpus(text(rnd.randint(0, 6)), rnd.choice([0, 3, 1 << 20]))
        eng.run_index(c.texts[0], c.first)
        for _ in range(rnd.randint(1, 6)):
            if rnd.random() < 0.7:
                t, nf = text(rnd.randint(0, 5)), rnd.random() < 0.6
                eng.append_index(t, new_file=nf)
                c.append(t, nf)
            else:
                d = rnd.randint(0, sum(s[3] for s in c.table))
                assert eng.drop_index(d).dropped_files == c.drop(d)
        ids = [s[0] for s in c.table] + [99]
        sets = [sorted(rnd.sample(ids, rnd.randint(1, len(ids)))) for _ in range(3)] + [None]
        qs = [[rnd.choice(words)] for _ in range(3)] + [[b"a", b"b"]]
        check(eng, c, qs, ["all", "any", "all", "any"], files=sets, by_file=True)
        check(eng, c, qs[:2], "any", files=sets[:2], rank=2, by_file=True)


# ---- no regression by construction ----
def test_a_batch_without_sets_answers_as_a_single_file_engine(eng):
    files = hamlet_files([50, 50], 700)
    qs = [[b"the", b"of"], [b"th*"], [b"and"]]
    c = build(eng, files)
    got = [eng.search_resident(qs, "all", wildcard=True),
           eng.search_resident(qs, "any", wildcard=True, rank=3)]
    fresh = lc.Engine(gpu_cfg(), 1 << 20, 1 << 15)
    fresh.run_index(c.text)
    ref = [fresh.search_resident(qs, "all", wildcard=True),
           fresh.search_resident(qs, "any", wildcard=True, rank=3)]
    for g, r in zip(got, ref):
        assert (g.walked, g.merged, g.wire_bytes, g.restricted) == (r.walked, r.merged,
                                                                    r.wire_bytes, 0)
        assert g.matches() == r.matches() and g.format() == r.format()
        for i in range(3):
            assert g.lines(i) == r.lines(i) and g.scores(i) == r.scores(i)
            assert g.term_counts(i) == r.term_counts(i)
    assert fresh.segments() == [(0, 0, 0, 100)] and got[0].segments() == c.table
    # ... and a batch with a set copies the counters once more, and nothing else
    more = eng.search_resident(qs, "all", wildcard=True, files=[[0, 1]] * 3)
    assert more.wire_bytes - got[0].wire_bytes in range(1, 256) and more.restricted == 0


def test_cli_answers_by_file_on_the_device_as_on_the_host(tmp_path):
    import subprocess
    paths = []
    for i, t in enumerate(hamlet_files([40, 0, 60], 900)):
        paths.append(str(tmp_path / ("f%d.txt" % i)))
        with open(paths[-1], "wb") as f:
            f.write(t if i != 2 else t[:-1])  # the last file lacks its last newline
    args = [paths[0], "--add", paths[1], "--add", paths[2], "--search", "the", "--search", "and",
            "--in", paths[2], "--block-kb", "1"]
    for extra in (["--by-file"], ["--count"], ["--by-file", "--rank", "5", "--show", "30"]):
        outs = []
        for backend in ("gpu", "cpu"):
            r = subprocess.run([lc.cli_path(), *args, *extra, "--backend", backend],
                               capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr
            outs.append(r.stdout[r.stdout.index(b"print query:"):r.stdout.index(b"\nDone")])
        assert outs[0] == outs[1] and b"  file: " in outs[0]


def test_refusals_leave_the_index_intact(eng):
    c = build(eng, [b"alpha\n", b"beta"])  # the resident text ends without a newline
    with pytest.raises(lc.LocustError, match="does not end in a newline"):
        eng.append_index(b"gamma\n", new_file=True)
    with pytest.raises(lc.LocustError, match="strictly ascending"):
        eng.search_resident([[b"alpha"]], files=[[1, 0]])
    assert eng.segments() == c.table
    check(eng, c, [[b"alpha"], [b"beta"]], files=[[0], [1]])
