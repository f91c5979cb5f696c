"""Corpus search on the host (engine.hpp "corpus", "file sets"; oracle.CORPUS_RULES): the segment
table's arithmetic against a brute-force list of (file, local line) per resident line, the host
twin against the oracle in every mode under file sets, ranked too, the multi-file entry points on
the CPU backend, and every refusal."""
import os
import random
import subprocess

import pytest

import locust_amd as lc
from locust_amd.models.wordcount import _index_corpus
from locust_amd.utils import oracle
from tests.corpus_cases import ROOT, SMALL, hamlet_files, twin, want

C = lc._C


class Brute:
    """Per resident line its (file id, local number), and where every resident file begins."""

    def __init__(self, first, lines):
        self.first = first
        self.lines = [(0, i) for i in range(lines)]
        self.files = [(0, 0)]  # (id, index of its first line in self.lines)
        self.next_id = 1
        self.count = {0: lines}

    def append(self, n, new_file):
        if new_file:
            self.files.append((self.next_id, len(self.lines)))
            self.count[self.next_id] = 0
            self.next_id += 1
        i = self.files[-1][0]
        self.lines += [(i, self.count[i] + j) for j in range(n)]
        self.count[i] += n

    def drop(self, d):
        if d == 0:
            return 0
        before = {i for i, _l in self.lines}
        self.lines = self.lines[d:]
        self.first += d
        moved = [(i, max(at - d, 0)) for i, at in self.files if at - d <= 0]
        later = [(i, at - d) for i, at in self.files if at - d > 0]
        self.files = moved[-1:] + later  # the last file that began at or before the cut stays
        resident = {i for i, _at in self.files}
        return len([i for i in before if i not in resident])

    def check(self, table):
        assert [r[0] for r in table] == [i for i, _at in self.files]
        assert [r[1] for r in table] == [self.first + at for _i, at in self.files]
        assert sum(r[3] for r in table) == len(self.lines)
        for j, (i, local) in enumerate(self.lines):
            assert C.segment_locate(table, self.first + j) == (i, local)
            assert oracle.locate(table, self.first + j) == (i, local)


@pytest.mark.parametrize("seed", range(12))
def test_segment_arithmetic_against_a_list_of_lines(seed):
    rnd = random.Random(seed)
    first, lines = rnd.choice([0, 7, 1000]), rnd.choice([0, 1, 5])
    b = Brute(first, lines)
    table = oracle.segments_of([b"x\n" * lines], first)
    ops = []
    for _ in range(30):
        total = len(b.lines)
        if rnd.random() < 0.6:
            op = ("append", rnd.choice([0, 0, 1, 2, 5]), rnd.random() < 0.6)
        else:
            # a file boundary, everything, or a cut inside a file (twice in a row cuts it twice)
            edges = [at for _i, at in b.files if at <= total]
            op = ("drop", rnd.choice(edges + [total, rnd.randint(0, total), min(1, total)]), False)
        ops.append(op)
        gone = C.segment_ops(first, lines, ops, False)[-1]
        if op[0] == "append":
            b.append(op[1], op[2])
            table = oracle.append_segments(table, op[1], op[2])
            want_gone = 0
        else:
            want_gone = b.drop(op[1])
            table, ogone = oracle.drop_segments(table, op[1])
            assert ogone == want_gone
        assert gone == ([tuple(r) for r in table], want_gone), (ops, table)
        b.check(gone[0])


def test_drop_cases_by_hand():
    # files of 2, 0 and 2 lines from line 5: drop at the boundary, inside a file twice, everything
    ops = [("append", 0, True), ("append", 2, True)]
    t = C.segment_ops(5, 2, ops + [("drop", 2, False)], False)[-1]
    assert t == ([(2, 7, 0, 2)], 1)  # the empty file in front of the first resident line goes too
    t = C.segment_ops(5, 2, ops + [("drop", 1, False)], False)[-1]
    assert t == ([(0, 6, 1, 1), (1, 7, 0, 0), (2, 7, 0, 2)], 0)
    t = C.segment_ops(5, 2, ops + [("drop", 3, False), ("drop", 1, False)], False)[-1]
    assert t == ([(2, 9, 2, 0)], 0)  # d = N: the last file stays, empty, and keeps its numbering
    t = C.segment_ops(5, 2, ops + [("drop", 4, False), ("append", 3, False)], False)[-1]
    assert t == ([(2, 9, 2, 3)], 0)
    assert oracle.segments_of([b"a\nb\n", b"", b"c\nd"], 5, 3) == [(2, 8, 1, 1)]
    assert oracle.by_file(oracle.segments_of([b"a\nb\n", b"", b"c\nd"], 5), [5, 7, 8]) == \
        ([0, 2, 2], [0, 0, 1], [(0, 1), (2, 2)])


def test_more_than_the_most_files_is_refused_with_the_table_intact():
    ops = [("append", 0, True)] * (C.kCorpusMaxFiles - 1)
    table, _ = C.segment_ops(0, 1, ops, False)[-1]
    assert len(table) == C.kCorpusMaxFiles == oracle.CORPUS_MAX_FILES
    with pytest.raises(C.LocustError, match="kCorpusMaxFiles"):
        C.segment_ops(0, 1, ops + [("append", 1, True)], False)
    # without new_file the block still extends the last file
    assert C.segment_ops(0, 1, ops + [("append", 4, False)], False)[-1][0][-1] == \
        (C.kCorpusMaxFiles - 1, 1, 0, 4)


@pytest.fixture(scope="module")
def small():
    """The SMALL corpus on the CPU backend: (IndexResult, its text, the oracle's table)."""
    cfg = lc.make_config("cpu", check=True)
    _eng, x, text = _index_corpus(cfg, SMALL, None, None)
    return x, text, oracle.segments_of(SMALL)


def test_merge_and_trim_carry_the_table(small):
    x, text, table = small
    assert x.segments() == table
    assert text == b"".join(SMALL) and x.num_lines == 6
    cfg = lc.make_config("cpu", check=True)
    one = C.cpu_run_index(cfg, text, 0)
    assert one.segments() == [(0, 0, 0, 6)]  # a single-file user sees nothing new
    for d in (0, 2, 3, 6):
        assert lc.trim_index(x, d).segments() == oracle.drop_segments(table, d)[0]
    more = C.cpu_run_index(cfg, b"eps\n", 6)
    assert lc.merge_index(x, more).segments()[-1] == (6, 6, 0, 1)  # extends the empty last file
    assert lc.merge_index(x, more, new_file=True).segments()[-1] == (7, 6, 0, 1)


SETS = [None, [1], [4], [1, 4], [5], [1, 4, 5], [0, 2, 6], [9], [4, 99]]
QUERIES = [([b"alpha"], "all", {}), ([b"alpha", b"beta"], "all", {}),
           ([b"alpha", b"delta"], "any", {}), ([b"alpha", b"beta"], "phrase", {}),
           ([b"beta", b"alpha"], "near", {"within": 2}),
           ([b"beta"], "all", {"exclude": [b"gamma"]}),
           (b"( alpha AND beta ) OR delta", "expr", {})]


@pytest.mark.parametrize("files", SETS)
def test_host_twin_against_the_oracle_under_file_sets(small, files):
    x, text, table = small
    for terms, mode, kw in QUERIES:
        ref = want(text, table, terms, mode, files, **kw)
        tw = {k: [v] if k == "exclude" else v for k, v in kw.items()}
        got = twin(x, text, [terms], mode, None if files is None else [files], **tw)
        assert got.lines(0) == ref, (terms, mode, files)
        assert got.matches() == [len(ref)] and got.segments() == table
        assert got.restricted == 0  # (the device's counter)
    # a batch in which only the middle query has a set
    got = twin(x, text, [[b"alpha"], [b"alpha"], [b"beta"]], "all", [None, files, None])
    assert got.lines(0) == want(text, table, [b"alpha"])
    assert got.lines(1) == want(text, table, [b"alpha"], files=files)
    assert got.lines(2) == want(text, table, [b"beta"])


@pytest.mark.parametrize("k", [1, 2, 100])
def test_ranked_under_a_set_is_the_unrestricted_ranking_filtered(small, k):
    x, text, table = small
    for files in ([4], [1, 5], [9]):
        for terms, mode in (([b"alpha", b"beta"], "any"), ([b"beta"], "all")):
            top, matches = want(text, table, terms, mode, files, rank=k)
            got = twin(x, text, [terms], mode, [files], rank=k)
            assert list(zip(got.lines(0), got.scores(0))) == top and got.matches() == [matches]
            # scores do not change: the whole ranking, filtered to the set, cut to K
            full = twin(x, text, [terms], mode, rank=100)
            keep = set(want(text, table, terms, mode, files))
            pairs = [(l, s) for l, s in zip(full.lines(0), full.scores(0)) if l in keep]
            assert top == pairs[:k]


def test_show_and_tally_see_the_restricted_answer(small):
    x, text, table = small
    got = twin(x, text, [[b"alpha"]], "all", [[4, 5]], show=64, tally=3)
    lines = want(text, table, [b"alpha"], files=[4, 5])
    assert got.lines(0) == lines == [3, 5]
    all_lines = oracle.split_lines(text)
    assert got.text(0) == [all_lines[l] for l in lines]
    ent, post = oracle.index(text)
    words, tokens, top = oracle.tally(ent, post, lines, 3)
    assert got.tally(0) == top and got.tally_words() == [words]


def test_host_twin_answers_by_file(small):
    x, text, table = small
    for files in SETS:
        for terms, mode, kw in QUERIES:
            tw = {k: [v] if k == "exclude" else v for k, v in kw.items()}
            fs = None if files is None else [files]
            got = twin(x, text, [terms], mode, fs, by_file=True, **tw)
            lines = want(text, table, terms, mode, files, **kw)
            assert got.lines(0) == lines
            assert (got.files(0), got.local_lines(0), got.file_hits(0)) == \
                oracle.by_file(table, lines)
            cnt = twin(x, text, [terms], mode, fs, count_only=True, **tw)
            assert cnt.lines(0) == cnt.files(0) == [] and cnt.matches() == [len(lines)]
            assert cnt.file_hits(0) == got.file_hits(0) and cnt.by_file == 2
    # ranked: the counts are over the winners, in rank order the files alternate
    top, _m = want(text, table, [b"alpha", b"beta"], "any", rank=3)
    got = twin(x, text, [[b"alpha", b"beta"]], "any", rank=3, by_file=True)
    assert (got.files(0), got.local_lines(0), got.file_hits(0)) == \
        oracle.by_file(table, [l for l, _s in top])
    plain = twin(x, text, [[b"alpha"]])
    assert plain.by_file == 0 and plain.files(0) == plain.local_lines(0) == plain.file_hits(0) == []
    for kw in ({"rank": 2}, {"show": 10}, {"tally": 3}):
        with pytest.raises(C.LocustError, match="count_only"):
            twin(x, text, [[b"alpha"]], count_only=True, **kw)


def test_search_files_and_index_files_on_the_cpu(tmp_path):
    texts = [b"alpha beta\ngamma", b"", b"beta\nalpha gamma\n"]  # one without its last newline
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("f%d.txt" % i)))
        with open(paths[-1], "wb") as f:
            f.write(t)
    fixed = [texts[0] + b"\n", texts[1], texts[2]]
    table = oracle.segments_of(fixed)
    x = lc.index_files(paths, backend="cpu", check=True)
    assert x.paths == paths and x.segments() == table == [(0, 0, 0, 2), (1, 2, 0, 0), (2, 2, 0, 2)]
    ent, post = oracle.index(b"".join(fixed))
    assert x.entries() == ent and x.postings() == post  # the added byte makes no new line
    r = lc.search_files(paths, [[b"gamma"], [b"gamma"], [b"alpha"]], backend="cpu", check=True,
                        files=[None, [2], [0, 1]])
    assert r.paths == paths and r.segments() == table
    assert [r.lines(i) for i in range(3)] == [[1, 3], [3], [0]]
    assert r.files(0) == [0, 2] and r.local_lines(0) == [1, 1]  # by_file is search_files' default
    assert [r.file_hits(i) for i in range(3)] == [[(0, 1), (2, 1)], [(2, 1)], [(0, 1)]]
    cnt = lc.search_files(paths, [[b"gamma"]], backend="cpu", check=True, count_only=True)
    assert cnt.lines(0) == [] and cnt.file_hits(0) == [(0, 1), (2, 1)] and cnt.matches() == [2]
    assert [oracle.locate(table, l) for l in r.lines(0)] == [(0, 1), (2, 1)]
    # block by block, and a window of the last two blocks: file 0 has left, its id selects nothing
    r = lc.search_files(paths, [[b"alpha"], [b"alpha"]], backend="cpu", check=True, block_bytes=12,
                        keep_blocks=2, files=[[0], [2]])
    assert r.segments() == [(2, 2, 0, 2)] and [r.lines(i) for i in range(2)] == [[], [3]]
    assert r.format() == oracle.format_search([[b"alpha"], [b"alpha"]], [[], [3]])


def run_cli(*args):
    r = subprocess.run([lc.cli_path(), *args], capture_output=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def result_lines(stdout):
    """The CLI's result lines: from the first query's line to the blank line before Done."""
    at = stdout.index(b"print query:")
    return stdout[at:stdout.index(b"\nDone")]


def test_cli_on_three_files_against_the_oracle(tmp_path):
    texts = [b"alpha beta\ngamma alpha", b"", b"beta\nalpha gamma\nalpha\n"]
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("f%d.txt" % i)))
        with open(paths[-1], "wb") as f:
            f.write(t)
    text = texts[0] + b"\n" + texts[2]
    table = oracle.segments_of([texts[0] + b"\n", texts[1], texts[2]])
    ent, post = oracle.index(text)
    base = [paths[0], "--backend", "cpu", "--add", paths[1], "--add", paths[2]]
    qs = [[b"alpha"], [b"gamma"], [b"alpha"]]
    ans = [oracle.search(ent, post, q, files=f, table=table)[0]
           for q, f in zip(qs, (None, None, [2]))]
    search = ["--search", "alpha", "--search", "gamma", "--search", "alpha", "--in", paths[2]]
    js = str(tmp_path / "out.json")
    rc, out, err = run_cli(*base, *search, "--by-file", "--json", js)
    assert rc == 0, err
    assert result_lines(out) == oracle.format_search(qs, ans, by_file=(table, paths))
    assert ans[2] == [3, 4] and b"  file: %s \t hits: 2 \t lines: 1 2\n" % paths[2].encode() in out
    import json
    j = json.load(open(js))
    assert j["files"] == [{"path": p, "id": i, "first_line": t[1], "base": t[2], "lines": t[3]}
                          for i, (p, t) in enumerate(zip(paths, table))]
    assert j["dropped_files"] == 0 and j["restricted"] == 0 and j["hits"] == sum(map(len, ans))
    # without --by-file the lines are what they always were
    rc, out, err = run_cli(*base, *search)
    assert rc == 0 and result_lines(out) == oracle.format_search(qs, ans)
    rc, out, err = run_cli(*base, *search, "--count")
    assert rc == 0, err
    assert result_lines(out) == oracle.format_search(qs, ans, by_file=(table, paths), count=True)
    # ranked, block by block
    tops = [oracle.rank(ent, post, a, q, 2) for q, a in zip(qs, ans)]
    rc, out, err = run_cli(*base, *search, "--by-file", "--rank", "2", "--block-kb", "1")
    assert rc == 0, err
    assert result_lines(out) == oracle.format_ranked(qs, [t for t, _m in tops],
                                                     [m for _t, m in tops],
                                                     by_file=(table, paths))
    # --show: the prefix names the file and its own line
    rc, out, err = run_cli(*base, "--search", "gamma", "--by-file", "--show", "40")
    assert rc == 0 and b"  %s:1: gamma alpha\n" % paths[0].encode() in out
    assert b"  %s:1: alpha gamma\n" % paths[2].encode() in out
    # --index over the corpus
    rc, out, err = run_cli(*base, "--index", "--json", js)
    assert rc == 0 and oracle.format_index(ent, post) in out
    assert [f["lines"] for f in json.load(open(js))["files"]] == [2, 0, 3]
    # refusals, each with its reason, before anything starts
    for extra, why in ((["--search", "alpha", "--in", "nope.txt"], b"none of the files"),
                       (["--search", "alpha", "--top", "3"], b"--top"),
                       (["--search", "alpha", "--gpus", "2"], b"--gpus"),
                       (["--search", "alpha", "--chunk-mb", "1"], b"--chunk-mb"),
                       (["--search", "alpha", "--count", "--rank", "2"], b"count_only"),
                       ([], b"--index or --search"), (["--by-file", "--index"], b"--search")):
        rc, out, err = run_cli(*base, *extra)
        assert rc != 0 and why in err, (extra, err)
    rc, out, err = run_cli(paths[0], "0", "1", "--backend", "cpu", "--add", paths[1], "--search",
                           "alpha")
    assert rc != 0 and b"line window" in err


def test_refusals(small):
    x, text, _table = small
    for bad in ([2, 1], [1, 1], [0, 5, 3]):
        with pytest.raises(C.LocustError, match="strictly ascending"):
            twin(x, text, [[b"alpha"]], "all", [bad])
        with pytest.raises(ValueError):
            oracle.search(*oracle.index(text), [b"alpha"], files=bad, table=oracle.segments_of(SMALL))
    with pytest.raises(C.LocustError, match="one file set"):
        x._search([[b"alpha"], [b"beta"]], [0, 0], files=[[1]])
    with pytest.raises(ValueError, match="one entry per query"):
        x.search([[b"alpha"], [b"beta"]], files=[1, 2])
    with pytest.raises(ValueError):
        oracle.search(*oracle.index(text), [b"alpha"], files=[1])  # a set needs the table
    cpu = lc.Engine(lc.make_config("cpu"))
    for call in (cpu.segments, lambda: cpu.append_index(b"x\n", new_file=True)):
        with pytest.raises(C.LocustError, match="needs a GPU engine"):
            call()
    with pytest.raises(ValueError):
        lc.search_files([], [[b"alpha"]], backend="cpu")
    with pytest.raises(ValueError):
        oracle.drop_segments(oracle.segments_of(SMALL), 7)


def test_hamlet_files_every_mode(tmp_path):
    files = hamlet_files([40, 1, 70, 33], start=1000)
    cfg = lc.make_config("cpu", check=True)
    _e, x, text = _index_corpus(cfg, files, 1 << 10, None)
    table = oracle.segments_of(files)
    assert x.segments() == table and text == b"".join(files)
    for sets in ([0, 2], [1], [3]):
        for terms, mode, kw in (([b"the"], "all", {}), ([b"the", b"of"], "any", {}),
                                ([b"of", b"the"], "phrase", {}),
                                ([b"the", b"and"], "near", {"within": 4})):
            got = twin(x, text, [terms], mode, [sets], **kw)
            assert got.lines(0) == want(text, table, terms, mode, sets, **kw), (terms, mode, sets)


def test_the_host_only_sanitizer_build_still_links():
    r = subprocess.run(["make", "-C", ROOT, "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(os.path.join(ROOT, "build", "asan", "MapReduce"))
