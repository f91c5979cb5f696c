"""Shared texts and helpers of the corpus tests (tests/test_corpus.py, tests/test_corpus_gpu.py):
files cut from data/hamlet.txt and tiny synthetic lines, a corpus kept beside an engine as plain
file texts, the oracle's answer of a query under a file set, and the host twin's."""
import os

import locust_amd as lc
from locust_amd.models.wordcount import _by_file, _search_args, _search_files
from locust_amd.utils import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hamlet():
    with open(os.path.join(ROOT, "data", "hamlet.txt"), "rb") as f:
        return f.read()


def hamlet_files(sizes, start=0):
    """Consecutive slices of Hamlet of these many lines, each ending in a newline."""
    lines = hamlet().split(b"\n")
    out = []
    for n in sizes:
        out.append(b"".join(l + b"\n" for l in lines[start:start + n]))
        start += n
    return out


# six small files: an empty one in front, between (two in a row) and behind
SMALL = [b"", b"alpha beta\ngamma alpha\n", b"", b"", b"beta gamma delta\nalpha\nbeta beta\n",
         b"delta alpha beta\n", b""]


class Corpus:
    """The files of an index as texts, and the table the oracle derives from what happened."""

    def __init__(self, first_text, first_line=0):
        self.first = first_line
        self.texts = {0: first_text}  # id -> what of the file is resident
        self.table = oracle.segments_of([first_text], first_line)

    def append(self, text, new_file=False):
        n = len(oracle.split_lines(text))
        self.table = oracle.append_segments(self.table, n, new_file)
        i = self.table[-1][0]
        self.texts[i] = self.texts.get(i, b"") + text
        return n

    def drop(self, d):
        left = d
        for seg in self.table:
            i, take = seg[0], min(left, seg[3])
            self.texts[i] = b"".join(l + b"\n" for l in oracle.split_lines(self.texts[i])[take:])
            left -= take
        self.table, gone = oracle.drop_segments(self.table, d)
        self.first += d
        self.texts = {s[0]: self.texts[s[0]] for s in self.table}
        return gone

    @property
    def text(self):
        return b"".join(self.texts[s[0]] for s in self.table)


def want(text, table, terms, mode="all", files=None, first_line=0, within=None, exclude=None,
         rank=None, **okw):
    """The oracle's answer of one query: its lines, or its (line, score) winners and matches."""
    ent, post = oracle.index(text, first_line=first_line)
    kw = dict(files=files, table=table, exclude=exclude, **okw)
    if mode == "phrase":
        lines, _c = oracle.phrase(text, terms, first_line=first_line, **kw)
    elif mode == "near":
        lines, _c = oracle.near(text, terms, within, first_line=first_line, **kw)
    elif mode == "expr":
        lines, _c, terms = oracle.expr_search(ent, post, terms, files=files, table=table, **okw)
        terms = [t for t in terms]
    else:
        lines, _c = oracle.search(ent, post, terms, mode, **kw)
    if rank is None:
        return lines
    if mode == "expr":
        raise ValueError("the helper ranks no expr query")
    return oracle.rank(ent, post, lines, terms, rank, exclude=exclude, **okw)


def twin(x, text, queries, mode="all", files=None, rank=None, within=None, exclude=None, **kw):
    """The host twin over an IndexResult and the text it covers (search_index with the text)."""
    queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
    return lc._C.search_index_text(x, text, queries, flags, rank, bool(kw.get("wildcard")),
                                   windows, exclude, bool(kw.get("glob")),
                                   bool(kw.get("ignore_case")), kw.get("show"),
                                   bool(kw.get("fuzzy")), bool(kw.get("regex")), kw.get("tally"),
                                   _search_files(files, len(queries)),
                                   _by_file(kw.get("by_file"), kw.get("count_only")))


def same_result(got, ref, nq):
    """Two SearchResults field for field (what both evaluations fill)."""
    assert got.matches() == ref.matches() and got.hits() == ref.hits()
    assert got.segments() == ref.segments()
    for i in range(nq):
        assert got.lines(i) == ref.lines(i), i
        assert got.scores(i) == ref.scores(i), i
        assert got.term_counts(i) == ref.term_counts(i), i
        assert got.text(i) == ref.text(i) and got.spans(i) == ref.spans(i), i
        assert got.tally(i) == ref.tally(i), i
        assert got.files(i) == ref.files(i) and got.local_lines(i) == ref.local_lines(i), i
        assert got.file_hits(i) == ref.file_hits(i), i
    assert got.by_file == ref.by_file
    assert got.format() == ref.format()
