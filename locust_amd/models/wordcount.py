"""WordCount -- the reference's one job (README.md:26-62), as a reusable job object.

``Engine`` keeps a preallocated device pipeline (HBM arena, pinned staging, stream,
events) alive across runs, so repeated jobs pay no allocation.  ``WordCount`` is the
user-facing job: load a file or a text window, run on one GPU, many GPUs (loopback in
one process) or the CPU reference path, and format the reference's output.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from .._native import load
from ..config import make_config, make_dist_config

_C = load()


_SEARCH_MODES = {"all": 0, "any": 1, "phrase": 2, "near": 3, "expr": 4}


def _search_exclude(exclude, n):
    """One list of exclusion terms per query (``[]``: none) from ``exclude``: ``None``, or a
    list with one entry per query, each ``None`` or a list of byte-string terms."""
    if exclude is None:
        return []
    if isinstance(exclude, (bytes, str)) or len(exclude) != n:
        raise ValueError("search: exclude takes one entry per query, each None or a list of "
                         "terms")
    out = []
    for x in exclude:
        if isinstance(x, (bytes, str)):
            raise ValueError("search: an entry of exclude is None or a list of terms, not the "
                             "term %r itself" % (x,))
        out.append([] if x is None else list(x))
    return out


def _search_files(files, n):
    """One file set per query (``[]``: every file) from ``files``: ``None``, or a list with one
    entry per query, each ``None`` or a list of file ids (``Engine.segments``)."""
    if files is None:
        return []
    files = list(files)
    if len(files) != n or any(isinstance(f, int) for f in files):
        raise ValueError("search: files takes one entry per query, each None or a list of "
                         "file ids")
    return [[] if f is None else [int(i) for i in f] for f in files]


def _by_file(by_file, count_only):
    """The native entry points' by_file flag: 0 none, 1 by_file, 2 count_only (which implies
    by_file)."""
    return 2 if count_only else 1 if by_file else 0


def _search_args(queries, mode, within=None, exclude=None):
    """(term lists, one mode flag per query: 0 all, 1 any, 2 phrase, 3 near, 4 expr, one window per
    query: 0 none, one list of exclusion terms per query or none at all) for the native search
    entry points."""
    queries = list(queries)
    modes = [mode] * len(queries) if isinstance(mode, str) else list(mode)
    if len(modes) != len(queries):
        raise ValueError("search: one mode per query")
    # (an 'expr' query may be given as the expression itself: bytes, not a list of terms)
    queries = [[q] if m == "expr" and isinstance(q, (bytes, str)) else list(q)
               for q, m in zip(queries, modes)]
    exclude = _search_exclude(exclude, len(queries))
    for m in modes:
        if m not in _SEARCH_MODES:
            raise ValueError("search: mode must be 'all', 'any', 'phrase', 'near' or 'expr', "
                             "not %r" % (m,))
    for q, m, x in zip(queries, modes, exclude or [[]] * len(queries)):
        if m != "expr":
            continue
        if len(q) != 1:
            raise ValueError("search: an 'expr' query is one expression (bytes, or a "
                             "one-element list), not %d terms" % len(q))
        if x:
            raise ValueError("search: an 'expr' query takes no exclusion terms (exclude): "
                             "write NOT in the expression instead")
    if not isinstance(within, (list, tuple)):  # one window for the batch's near queries
        windows = [within if m == "near" else None for m in modes]
        if within is not None and "near" not in modes:
            raise ValueError("search: within is the window of a 'near' query; no query of "
                             "this batch is one")
    else:
        windows = list(within)
        if len(windows) != len(queries):
            raise ValueError("search: one window (within) per query, None for a query that "
                             "is not 'near'")
    for m, w in zip(modes, windows):
        if m != "near":
            if w is not None:
                raise ValueError("search: within=%r on a %r query; only a 'near' query takes "
                                 "a window" % (w, m))
        elif isinstance(w, bool) or not isinstance(w, int) or not 1 <= w < 1 << 32:
            raise ValueError("search: a 'near' query takes within=W, an integer with "
                             "1 <= W < 2^32, not %r" % (w,))
    return queries, [_SEARCH_MODES[m] for m in modes], [w or 0 for w in windows], exclude


def _index_search(self, queries, mode="all", rank=None, wildcard=False, within=None,
                  exclude=None, glob=False, ignore_case=False, show=None, fuzzy=False, regex=False,
                  tally=None, files=None, by_file=False, count_only=False):
    """All/any word queries over this index, evaluated on the host (``SearchResult``):
    ``queries``, ``mode``, ``rank``, ``within`` and ``exclude`` as ``Engine.run_search`` takes
    them, any number of queries.  A ``"phrase"`` query, and a ``"near"`` query of two or more
    positive terms, is refused: the index holds no positions, so they need the text
    (``Engine.run_search``, ``search_text``).  ``glob``, ``fuzzy`` and ``ignore_case`` as
    there.
    ``show=N`` is refused like a phrase: the shown lines come from the text.
    ``tally=K`` is answered here too (``Engine.run_search``): the rule needs no text.
    ``files`` as there, over this index's ``segments()``."""
    queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
    return self._search(queries, flags, rank, bool(wildcard), windows, exclude, bool(glob),
                        bool(ignore_case), show, bool(fuzzy), bool(regex), tally,
                        _search_files(files, len(queries)), _by_file(by_file, count_only))


_C.IndexResult.search = _index_search


class Engine:
    """Single-device engine with fixed capacity (bytes, lines)."""

    def __init__(self, cfg=None, max_bytes: int = 1 << 20, max_lines: int = 1 << 15):
        self.cfg = cfg if cfg is not None else make_config()
        self.cpu = self.cfg.backend == _C.Backend.cpu
        self._eng = None if self.cpu else _C.GpuEngine(self.cfg, max_bytes, max_lines)
        self._next_line = 0  # the line behind the resident index (append_index)

    @property
    def capacity(self) -> int:
        return 0 if self.cpu else self._eng.capacity

    def run(self, text: bytes):
        if self.cpu:
            return _C.cpu_run(self.cfg, text)
        return self._eng.run(text)

    def run_top(self, text: bytes, k: int):
        """WordCount of ``text``, then its ``k`` most frequent words (count descending,
        ties by key ascending) as a ``TopResult``.  On the GPU the selection runs on the
        device and only the winners cross PCIe (``k <= _C.kTopKMax``; for a larger ``k``
        take ``run(text).top(k)``, the host selection)."""
        if self.cpu:
            return _C.cpu_run_top(self.cfg, text, k)
        return self._eng.run_top(text, k)

    def run_index(self, text: bytes, first_line: int = 0):
        """WordCount of ``text`` and its inverted index (``IndexResult``): for every word
        the lines it occurs on, one posting per occurrence, numbered from ``first_line``.
        ``entries()`` are the word job's; entry ``(key, val, count)`` owns
        ``postings()[val:val + count]``.  On the GPU the index is built on the device behind
        the word job (one pass, dictionary engine, fast map, word keys)."""
        if self.cpu:
            return _C.cpu_run_index(self.cfg, text, first_line)
        res = self._eng.run_index(text, first_line)
        self._next_line = first_line + res.num_lines
        return res

    def run_search(self, text: bytes, queries, mode="all", first_line: int = 0, rank=None,
                   wildcard=False, within=None, exclude=None, glob=False, ignore_case=False,
                   show=None, fuzzy=False, regex=False, tally=None, files=None, by_file=False,
                   count_only=False):
        """WordCount of ``text``, its inverted index, and a batch of word queries answered
        from it (``SearchResult``).  ``queries`` is a list of term lists (1 to 8 byte-string
        terms each); ``mode`` is ``"all"`` (lines that hold every term), ``"any"`` (lines
        that hold at least one), ``"phrase"`` (lines on which the terms are consecutive
        tokens, in order: ``oracle.phrase`` states the rules) or ``"near"`` (lines on which
        some ``within`` consecutive tokens match every term, in any order: ``oracle.near``
        states the rules), or a list with one mode per query.  ``within`` is the window of
        the ``"near"`` queries, which need one: an int ``W`` with ``1 <= W < 2**32`` for all
        of them, or a list with one entry per query, ``None`` for a query that is not
        ``"near"``.  ``"expr"`` answers a Boolean expression: the query is one bytes
        expression (or a one-element list) such as ``b"( to AND be ) OR ( Ham* AND NOT
        Hamlet )"`` -- ``AND``, ``OR``, ``NOT`` in upper case, parentheses, side-by-side operands
        joined by ``AND``, at most 8 distinct terms read under ``wildcard`` / ``glob`` /
        ``fuzzy`` as any term is (``oracle.EXPR_RULES`` states the rules).  An expression that
        is true of a line with none of its words (``NOT a``) is refused, and so are
        ``exclude`` and ``within`` on such a query.  It may share a batch with queries of the
        other modes.  On the GPU the query walks only a covering set of its terms' lists;
        ``walked`` is the number of list elements the batch's hit stage walked.
        ``lines(i)`` are query
        ``i``'s global line numbers, ascending, each once.  On the GPU the index stays in
        device memory and only the answers cross PCIe (at most ``_C.kSearchMaxQueries``
        queries per batch; ``run_index(text).search(...)`` evaluates any number of all/any
        queries on the host).  A phrase or a near query is verified on the device against
        the engine's own copy of the text; the CPU engine answers them at any size.

        ``rank=K`` (``K >= 1``, one per batch) answers every query's best ``K`` lines, best
        first (``oracle.rank`` states the score): ``lines(i)`` are in the order (score
        descending, line ascending), ``scores(i)`` are their scores and ``matches()`` counts
        every query's matching lines, of which ``min(K, matches)`` are returned.  On the GPU
        the lines are scored and selected on the device and only the winners cross PCIe.
        ``rank=None`` is the unranked answer (``scores(i)`` empty, ``matches() == hits()``).

        ``wildcard=True`` reads a term that ends in ``*`` (and is longer than one byte) as a
        prefix term: ``ham*`` stands for every word that starts with ``ham``, and behaves as
        one word whose list is the merged lists of them all (``oracle.search`` with
        ``wildcard=True`` states the rules).  A lone ``*`` is refused and a ``*`` anywhere
        else is literal; without ``wildcard`` every ``*`` is.  On the GPU the lists are merged
        on the device; ``merged`` is the number of list elements the batch merged.

        ``exclude`` gives exclusion terms: a list with one entry per query, each ``None`` or
        a list of byte-string terms (``oracle.search(..., exclude=)`` states the rules).  A
        query answers what its mode answers for its own terms, minus every line that holds an
        exclusion term; an absent exclusion term takes nothing away.  Own and exclusion terms
        together number at most 8, ``wildcard`` applies to both, ``term_counts(i)`` lists the
        own terms first and then the exclusion terms, and a ranked query scores by its own
        terms only.  On the GPU the lines are dropped on the device, before verification,
        scoring and the sort.

        ``glob=True`` reads ``*`` (any run of bytes, the empty one too) and ``?`` (exactly one
        byte) anywhere in a term: ``*ing``, ``h?mlet``, ``*aml*``.  Runs of ``*`` collapse;
        ``p*`` stays the prefix term of ``wildcard`` (``glob`` is a superset of it); any other
        term with a ``*`` or ``?`` is a pattern term, which stands for every word the whole
        pattern matches and behaves as one word with their merged lists (``oracle.search``
        with ``glob=True`` states the rules).  A pattern is never cut: one longer than
        ``max_key_len`` is refused, and so is one of stars alone.  ``ignore_case=True`` (a
        property of the whole batch) lets the ASCII letters of every term match either case:
        ``to be`` finds ``To be``.  On the GPU a scan of the dictionary finds a pattern's
        words -- (pattern terms) x (dictionary words) matcher calls per batch -- and their
        lists are merged on the device, counted in ``merged``.  A ranked batch with a pattern
        term takes ``emits_per_line <= 8192``: its lists may overlap, and a score reaches
        ``32 * emits_per_line * 8``.

        ``fuzzy=True`` reads a term that ends in ``~1`` or ``~2`` as a fuzzy term: ``Hamlet~1``
        stands for every word within one byte edit (an insertion, a deletion or a substitution;
        no transposition) of ``Hamlet`` -- ``Hamlet!`` and ``[Hamlet`` among them -- and
        ``quene~2`` finds ``queen``.  It behaves as one word with their merged lists, exactly as
        a pattern term does (``oracle.search`` with ``fuzzy=True`` states the rules), under
        ``ignore_case`` too.  The word is never cut and must be longer than its budget; a digit
        other than 1 or 2 is refused, and so is a ``*`` or ``?`` in the word when ``wildcard``
        or ``glob`` is on.  A ``~`` anywhere else is literal, and without ``fuzzy`` every ``~``
        is.  On the GPU the dictionary scan finds the words with a banded edit-distance matcher.

        ``regex=True`` reads a term written ``/re/`` as a regular expression that a whole word
        must match: ``/(king|queen)[!?]?/``, ``/[A-Z][A-Z]+/``, ``/\\[?Hamlet[!?\\]]?/``.  The
        syntax is literals, ``\\x`` escapes of non-alphanumeric bytes, ``.``, classes ``[a-z]``
        and ``[^...]``, groups, ``|``, ``*``, ``+`` and ``?``, over bytes; at most 32 positions
        and 128 source bytes; ``{m,n}``, anchors, ``\\d`` and ``\\w`` are refused
        (``oracle.REGEX_RULES`` states the rules).  It behaves as one word with its words' merged
        lists, exactly as a pattern term does, under ``ignore_case`` too, and is read before the
        fuzzy, wildcard and glob readings.  Without ``regex`` a ``/x/`` is a literal word.  On
        the GPU the dictionary scan runs the compiled position automaton, one key per lane.

        ``show=N`` (``1 <= N <= 65536``; ``None`` or ``0``: no show) also returns, for every
        returned line, its first ``N`` bytes and the spans of its tokens that match one of the
        query's own terms (``oracle.show`` states the rules): ``text(i)`` is the list of query
        ``i``'s shown lines, ``spans(i)`` per line a list of ``(start, len, mask)`` with bit
        ``j`` of ``mask`` set when the token matches term ``j``; ``cut_lines`` counts the lines
        longer than ``N`` and ``format(mark=True)`` prints the lines with the spans between
        ``>>`` and ``<<``.  On the GPU the lines and spans are gathered on the device from the
        resident text (``show_ms``), and only they cross PCIe.

        ``tally=K`` (``1 <= K <= 4096``; ``None`` or ``0``: no tally) also counts, for every
        query, the index's words over the lines it returns -- ranked: its winners -- however
        they were found (``oracle.TALLY_RULES`` states the rules): ``tally(i)`` is query
        ``i``'s ``K`` most frequent words as ``[(key, count)]``, count descending and key
        ascending; ``tally_words()`` and ``tally_tokens()`` give per query the distinct words
        and the tokens of those lines.  Keys are counted as the index holds them (``To`` and
        ``to`` apart, under ``ignore_case`` too).  On the GPU the returned lines are tokenised,
        sorted and counted on the device (``tally_ms``; ``tallied`` pair words), and only the
        winners cross PCIe.

        ``files`` gives file sets: a list with one entry per query, each ``None`` (every file)
        or a list of distinct file ids in ascending order (``segments()``: ``run_search`` begins
        file 0, ``append_index(text, new_file=True)`` the next).  A query then answers what it
        answers without the set, intersected with the lines of those files
        (``oracle.CORPUS_RULES`` states the rules): after exclusion, in every mode; a ranked
        query's scores do not change, so its answer is the unrestricted ranking filtered to the
        set and cut to ``K``.  An id that is not resident selects nothing.  On the GPU the hits
        outside the sets are removed on the device before anything is sorted or scored;
        ``restricted`` counts them.

        ``by_file=True`` also answers by file: ``files(i)`` and ``local_lines(i)`` give, parallel
        to ``lines(i)``, every returned line's file id and its number inside that file, and
        ``file_hits(i)`` is ``[(id, count)]`` over the files with a returned line, ids ascending
        (ranked: over the winners).  ``count_only=True`` implies it and returns the counts alone,
        as ``grep -c`` does: ``lines(i)`` is empty, ``matches()`` and ``file_hits(i)`` are
        filled, and on the GPU the lines never cross PCIe.  It is refused with ``rank``, ``show``
        or ``tally``.  On the GPU the files are resolved and counted on the device behind the
        search (``by_file_ms``)."""
        queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
        files = _search_files(files, len(queries))
        if self.cpu:
            return _C.cpu_run_search(self.cfg, text, queries, flags, first_line, rank,
                                     bool(wildcard), windows, exclude, bool(glob),
                                     bool(ignore_case), show, bool(fuzzy), bool(regex), tally,
                                     files, _by_file(by_file, count_only))
        res = self._eng.run_search(text, queries, flags, first_line, rank, bool(wildcard),
                                   windows, exclude, bool(glob), bool(ignore_case), show,
                                   bool(fuzzy), bool(regex), tally, files,
                                   _by_file(by_file, count_only))
        self._next_line = first_line + res.num_lines
        return res

    def search_resident(self, queries, mode="all", rank=None, wildcard=False, within=None,
                        exclude=None, glob=False, ignore_case=False, show=None, fuzzy=False,
                        regex=False, tally=None, files=None, by_file=False, count_only=False):
        """Another batch from the index this engine's last job left on the device; that
        job must have been a ``run_index`` or a ``run_search`` (GPU engines only).  Every
        mode of ``run_search``: the job's text is resident too, so phrases and near queries
        are answered.  ``rank``, ``within``, ``exclude``, ``glob``, ``ignore_case``, ``show``,
        ``fuzzy``, ``tally``, ``files``, ``by_file`` and ``count_only`` as ``run_search`` takes
        them."""
        if self.cpu:
            raise _C.LocustError("search_resident needs a GPU engine: the CPU engine keeps "
                                 "no index (use run_index(text).search(...))")
        queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
        return self._eng.search_resident(queries, flags, rank, bool(wildcard), windows, exclude,
                                         bool(glob), bool(ignore_case), show, bool(fuzzy),
                                         bool(regex), tally, _search_files(files, len(queries)),
                                         _by_file(by_file, count_only))

    def segments(self):
        """The files of the index this engine holds on the device: ``[(id, first_line, base,
        lines)]``, consecutive line ranges in order.  ``id`` numbers the files in the order they
        were begun, ``first_line`` is the global number of the file's first resident line and
        ``base`` that line's number inside the file (0 until a drop has cut into it): global
        line ``l`` of the file is its line ``l - first_line + base`` (GPU engines only)."""
        if self.cpu:
            raise _C.LocustError("segments needs a GPU engine: the CPU engine keeps no index "
                                 "(use IndexResult.segments())")
        return self._eng.segments()

    def append_index(self, text: bytes, new_file: bool = False):
        """One more block of whole lines into the index this engine holds on the device
        (``IndexAppend``): afterwards the resident index is the index of everything indexed and
        appended so far, one text after the other, and ``search_resident`` answers from it.
        The block's lines are numbered behind the resident ones; it is indexed in one pass of
        this engine and merged on the device.  Refused with the resident index intact: no
        resident index, a block larger than the engine's pass, a resident text that does not
        end in a newline (GPU engines only).  ``new_file=True`` begins a file with the next id
        at the block's first line (``segments()``); otherwise the block extends the last file.
        At most 65536 files are resident at a time."""
        if self.cpu:
            raise _C.LocustError("append_index needs a GPU engine: the CPU engine keeps no "
                                 "index (use merge_index(a, b) on two IndexResults)")
        res = self._eng.append_index(text, self._next_line, bool(new_file))
        self._next_line += res.block_lines
        return res

    def drop_index(self, lines: int):
        """The oldest ``lines`` lines out of the index this engine holds on the device
        (``IndexDrop``): afterwards the resident index is the index of the remaining lines,
        numbered as before, so its ``first_line`` moves up by ``lines`` and every search
        answers over the window.  The postings below the cut, the words whose lists empty out,
        the text and the line starts go; the rest is compacted on the device.  ``lines == 0`` is
        a no-op, all lines leave an empty index that ``append_index`` goes on from.  Refused
        with the resident index intact: no resident index, more lines than it holds (GPU
        engines only)."""
        if self.cpu:
            raise _C.LocustError("drop_index needs a GPU engine: the CPU engine keeps no "
                                 "index (use trim_index(x, lines) on an IndexResult)")
        return self._eng.drop_index(lines)

    def index_resident(self):
        """The index this engine holds on the device, downloaded (``IndexResult``), whatever it
        was built from: a ``run_index``, a ``run_search``, or those and appends."""
        if self.cpu:
            raise _C.LocustError("index_resident needs a GPU engine: the CPU engine keeps no "
                                 "index (use run_index(text))")
        return self._eng.index_resident()

    def top_counts(self, records: list[tuple[bytes, int]], k: int):
        """The selection alone over (key, count) records sorted by key with distinct
        keys: a ``TopResult`` on the GPU, the plain (key, val, count) list on the CPU."""
        if self.cpu:
            out, pos = [], 0
            for key, count in records:
                out.append((key, pos, count))
                pos += count
            return sorted(out, key=lambda e: (-e[2], e[0]))[:k]
        return self._eng.top_counts(records, k)

    def map_stage(self, text: bytes) -> list[bytes]:
        """Map + sort only (stage 1): the sorted token list of ``text``."""
        if self.cpu:
            return _C.cpu_map_stage(self.cfg, text)
        return self._eng.map_stage(text)

    def reduce_stage(self, keys: list[bytes]):
        """Reduce only (stage 2) over tokens in any order."""
        if self.cpu:
            text = b"\n".join(keys)
            return _C.cpu_run(self.cfg, text)
        return self._eng.reduce_stage(keys)

    def sort_keys(self, keys: list[bytes], counts: list[int] | None = None):
        """Device radix sort of byte-string keys: (sorted keys, permutation).  With
        ``counts`` (one u64 per key) they travel with their keys through the sort's fused
        gather: (sorted keys, permutation, sorted counts)."""
        if counts is not None and len(counts) != len(keys):
            raise ValueError("sort_keys: one count per key")
        if self.cpu:
            perm = sorted(range(len(keys)), key=lambda i: keys[i])
            if counts is not None:
                return [keys[i] for i in perm], perm, [counts[i] for i in perm]
            return [keys[i] for i in perm], perm
        return self._eng.sort_keys(keys, counts)

    def compact_slots(self, line_counts: list[int], slot_keys: list[bytes]) -> list[bytes]:
        """Stable compaction of fixed [line * emits_per_line + k] slots (compat engine):
        the first ``line_counts[l]`` slots of each line, in order."""
        return self._eng.compact_slots(line_counts, slot_keys)

    def reduce_sorted(self, keys: list[bytes]):
        """Boundary mark + head compaction + adjacent difference over sorted keys."""
        return self._eng.reduce_sorted(keys)

    def merge_runs(self, runs: list[list[tuple[bytes, int]]]):
        """Root merge of the gather strategy: runs of (key, count), each sorted with
        distinct keys -> merged (key, val, count) entries."""
        return self._eng.merge_runs(runs)


def wordcount_text(text: bytes, backend: str = "gpu", cfg=None, **kw):
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    nlines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run(text)


def wordcount_file(path: str, line_start: int = -1, line_end: int = -1, backend: str = "gpu",
                   cfg=None, **kw):
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    text, nlines, _first, _total = _C.load_lines(path, line_start, line_end, cfg.ref_compat)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run(text)


def top_words_text(text: bytes, k: int, backend: str = "gpu", cfg=None, **kw):
    """The ``k`` most frequent words of ``text`` (``TopResult``: rank-ordered
    ``(key, val, count)`` entries, ``val`` as in the full output)."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    nlines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_top(text, k)


def top_words_file(path: str, k: int, line_start: int = -1, line_end: int = -1,
                   backend: str = "gpu", cfg=None, **kw):
    """The ``k`` most frequent words of a file or of its line window."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    text, nlines, _first, _total = _C.load_lines(path, line_start, line_end, cfg.ref_compat)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_top(text, k)


def merge_index(a, b, new_file: bool = False):
    """The index of ``a``'s text followed by ``b``'s, from the two ``IndexResult`` alone: the
    host twin of the device merge.  ``b.first_line`` must be ``a.first_line + a.num_lines``.
    ``new_file=True``: ``b`` begins a file of the merged index (``segments()``)."""
    return _C.merge_index(a, b, bool(new_file))


def trim_index(x, lines: int, overflow_lines: int = 0, truncated: int = 0):
    """The index of ``x``'s text without its first ``lines`` lines, from the ``IndexResult``
    alone: the host twin of the device drop.  An index holds no text, so the dropped lines'
    ``overflow_lines`` and ``truncated`` are the caller's to supply (the dropped block's own
    index has them); ``max_key_len`` stays, the longest the index has held."""
    return _C.trim_index(x, lines, overflow_lines, truncated)


def split_blocks(text: bytes, block_bytes: int, first_line: int = 0):
    """``text`` cut into line-aligned blocks of at most ``block_bytes`` bytes:
    ``[(offset, bytes, lines, first_line)]``.  Every block but the last ends in a newline; a
    line longer than a block is refused."""
    return _C.split_blocks(text, block_bytes, first_line)


def _blocks(text, block_bytes, first_line):
    return [(text[o:o + n], lines, first) for o, n, lines, first in
            _C.split_blocks(text, block_bytes, first_line)]


def _index_blocks(cfg, text, first_line, block_bytes, keep_blocks=None):
    """(engine holding the index of ``text`` built block by block, or None on the CPU; the CPU
    backend's merged IndexResult, or None; the text the index covers).  ``keep_blocks=M``: once
    more than M blocks are in the index, the oldest block's lines are dropped from it."""
    if keep_blocks is not None and keep_blocks < 1:
        raise ValueError("keep_blocks must be >= 1")
    blocks = _blocks(text, block_bytes, first_line)
    oldest = 0  # the first block still in the index
    if cfg.backend == _C.Backend.cpu:
        parts = [_C.cpu_run_index(cfg, blocks[0][0], first_line)]
        x = parts[0]
        for b, (piece, _lines, first) in enumerate(blocks[1:], 1):
            parts.append(_C.cpu_run_index(cfg, piece, first))
            x = _C.merge_index(x, parts[b])
            if keep_blocks is not None and b + 1 - oldest > keep_blocks:
                x = _C.trim_index(x, blocks[oldest][1], parts[oldest].overflow_lines,
                                  parts[oldest].truncated)
                oldest += 1
        return None, x, b"".join(b[0] for b in blocks[oldest:])
    eng = Engine(cfg, max(max(len(b[0]) for b in blocks), 1), max(max(b[1] for b in blocks), 1))
    eng.run_index(blocks[0][0], first_line)
    for b, (piece, _lines, _first) in enumerate(blocks[1:], 1):
        eng.append_index(piece)
        if keep_blocks is not None and b + 1 - oldest > keep_blocks:
            eng.drop_index(blocks[oldest][1])
            oldest += 1
    return eng, None, b"".join(b[0] for b in blocks[oldest:])


def index_text(text: bytes, backend: str = "gpu", cfg=None, first_line: int = 0,
               block_bytes=None, keep_blocks=None, **kw):
    """The inverted index of ``text`` (``IndexResult``); lines are numbered from
    ``first_line``.  ``block_bytes=N``: built block by block (``split_blocks``), the first
    block indexed and the rest appended, so the engine is sized to one block.
    ``keep_blocks=M`` beside it: a sliding window -- whenever more than ``M`` blocks are in the
    index the oldest block's lines are dropped (``Engine.drop_index``; ``trim_index`` on the
    CPU), and the result is the index of the last ``M`` blocks with their own (global) line
    numbers and ``first_line``."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    if keep_blocks is not None and block_bytes is None:
        raise ValueError("keep_blocks needs block_bytes")
    if block_bytes is not None:
        eng, x, _window = _index_blocks(cfg, text, first_line, block_bytes, keep_blocks)
        return x if eng is None else eng.index_resident()
    nlines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_index(text, first_line)


def index_file(path: str, line_start: int = -1, line_end: int = -1, backend: str = "gpu",
               cfg=None, block_bytes=None, keep_blocks=None, **kw):
    """The inverted index of a file or of its line window, with the file's own (global)
    line numbers.  ``block_bytes`` and ``keep_blocks`` as ``index_text`` takes them."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    text, nlines, first, _total = _C.load_lines(path, line_start, line_end, cfg.ref_compat)
    if keep_blocks is not None and block_bytes is None:
        raise ValueError("keep_blocks needs block_bytes")
    if block_bytes is not None:
        return index_text(text, cfg=cfg, first_line=first, block_bytes=block_bytes,
                          keep_blocks=keep_blocks)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_index(text, first)


def search_text(text: bytes, queries, mode="all", backend: str = "gpu", cfg=None,
                first_line: int = 0, rank=None, wildcard=False, within=None, exclude=None,
                glob=False, ignore_case=False, show=None, fuzzy=False, regex=False, tally=None,
                block_bytes=None, keep_blocks=None, **kw):
    """All/any/phrase/near word queries over ``text`` (``SearchResult``); see
    ``Engine.run_search``.  ``block_bytes=N``: the index is built block by block
    (``index_text``) and the batch answered from it (on the CPU: from the merged index and the
    text it covers).  ``keep_blocks=M`` beside it: the batch is answered over the last ``M``
    blocks only, with their own (global) line numbers."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    if keep_blocks is not None and block_bytes is None:
        raise ValueError("keep_blocks needs block_bytes")
    if block_bytes is not None:
        eng, x, text = _index_blocks(cfg, text, first_line, block_bytes, keep_blocks)
        if eng is not None:
            return eng.search_resident(queries, mode, rank, wildcard, within, exclude, glob,
                                       ignore_case, show, fuzzy, regex, tally)
        queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
        return _C.search_index_text(x, text, queries, flags, rank, bool(wildcard), windows,
                                    exclude, bool(glob), bool(ignore_case), show, bool(fuzzy),
                                    bool(regex), tally, [], 0)
    nlines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_search(
        text, queries, mode, first_line, rank, wildcard, within, exclude, glob, ignore_case,
        show, fuzzy, regex, tally)


def search_file(path: str, queries, mode="all", line_start: int = -1, line_end: int = -1,
                backend: str = "gpu", cfg=None, rank=None, wildcard=False, within=None,
                exclude=None, glob=False, ignore_case=False, show=None, fuzzy=False, regex=False,
                tally=None, block_bytes=None, keep_blocks=None, **kw):
    """All/any/phrase/near word queries over a file or its line window, answered with the file's
    own (global) line numbers.  ``block_bytes`` and ``keep_blocks`` as ``search_text`` takes
    them."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    text, nlines, first, _total = _C.load_lines(path, line_start, line_end, cfg.ref_compat)
    if keep_blocks is not None and block_bytes is None:
        raise ValueError("keep_blocks needs block_bytes")
    if block_bytes is not None:
        return search_text(text, queries, mode, cfg=cfg, first_line=first, rank=rank,
                           wildcard=wildcard, within=within, exclude=exclude, glob=glob,
                           ignore_case=ignore_case, show=show, fuzzy=fuzzy, regex=regex,
                           tally=tally, block_bytes=block_bytes, keep_blocks=keep_blocks)
    return Engine(cfg, max(len(text), 1), max(nlines, 1)).run_search(
        text, queries, mode, first, rank, wildcard, within, exclude, glob, ignore_case, show,
        fuzzy, regex, tally)


def _corpus_blocks(texts, block_bytes):
    """The files' blocks in order, [(piece, lines, first_line, new_file)]: a file that lacks its
    last newline gets one when another follows (the byte makes no new line), every file but the
    first begins a segment, and a file is cut into line-aligned blocks when ``block_bytes`` is
    given (an empty file is one empty block)."""
    out, line = [], 0
    for i, t in enumerate(texts):
        if t and not t.endswith(b"\n") and i + 1 < len(texts):
            t += b"\n"
        nlines = t.count(b"\n") + (1 if t and not t.endswith(b"\n") else 0)
        pieces = ([(t, nlines, line)] if block_bytes is None else _blocks(t, block_bytes, line))
        for j, (piece, lines, first) in enumerate(pieces):
            out.append((piece, lines, first, i > 0 and j == 0))
        line += nlines
    return out


def _index_corpus(cfg, texts, block_bytes, keep_blocks):
    """``_index_blocks`` over several files: (engine or None, the CPU backend's IndexResult or
    None, the text the index covers)."""
    if not texts:
        raise ValueError("a corpus is one file or more")
    if keep_blocks is not None and (block_bytes is None or keep_blocks < 1):
        raise ValueError("keep_blocks needs block_bytes, and must be >= 1")
    blocks = _corpus_blocks(texts, block_bytes)
    oldest = 0
    if cfg.backend == _C.Backend.cpu:
        parts = [_C.cpu_run_index(cfg, blocks[0][0], 0)]
        x = parts[0]
        for b, (piece, _lines, first, new_file) in enumerate(blocks[1:], 1):
            parts.append(_C.cpu_run_index(cfg, piece, first))
            x = _C.merge_index(x, parts[b], new_file)
            if keep_blocks is not None and b + 1 - oldest > keep_blocks:
                x = _C.trim_index(x, blocks[oldest][1], parts[oldest].overflow_lines,
                                  parts[oldest].truncated)
                oldest += 1
        return None, x, b"".join(b[0] for b in blocks[oldest:])
    eng = Engine(cfg, max(max(len(b[0]) for b in blocks), 1), max(max(b[1] for b in blocks), 1))
    eng.run_index(blocks[0][0], 0)
    for b, (piece, _lines, _first, new_file) in enumerate(blocks[1:], 1):
        eng.append_index(piece, new_file)
        if keep_blocks is not None and b + 1 - oldest > keep_blocks:
            eng.drop_index(blocks[oldest][1])
            oldest += 1
    return eng, None, b"".join(b[0] for b in blocks[oldest:])


def _read_files(paths):
    texts = []
    for p in paths:
        with open(p, "rb") as f:
            texts.append(f.read())
    return texts


def index_files(paths, backend: str = "gpu", cfg=None, block_bytes=None, keep_blocks=None, **kw):
    """One inverted index over several files (``IndexResult``): the first file is indexed and
    the others appended, each beginning a file of the index (``segments()``), so lines are
    numbered through the corpus.  A file that lacks its last newline gets one when another
    follows.  ``block_bytes`` cuts every file into blocks and ``keep_blocks`` slides a window
    over them, as ``index_text`` does.  The result carries ``paths``."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    paths = list(paths)
    eng, x, _text = _index_corpus(cfg, _read_files(paths), block_bytes, keep_blocks)
    res = x if eng is None else eng.index_resident()
    res.paths = paths
    return res


def search_files(paths, queries, mode="all", backend: str = "gpu", cfg=None, rank=None,
                 wildcard=False, within=None, exclude=None, glob=False, ignore_case=False,
                 show=None, fuzzy=False, regex=False, tally=None, block_bytes=None,
                 keep_blocks=None, files=None, by_file=True, count_only=False, **kw):
    """Word queries over several files in one index (``SearchResult``; ``index_files`` builds
    it).  ``files`` restricts each query to some of the files, by their ids -- file ``i`` of
    ``paths`` has id ``i`` -- as ``Engine.run_search`` takes them; the lines of the answer are
    global, and ``segments()`` of the result gives each file's ``first_line`` and ``base``.
    ``by_file`` (the default here) and ``count_only`` as ``Engine.run_search`` takes them.  The
    result carries ``paths``."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    paths = list(paths)
    eng, x, text = _index_corpus(cfg, _read_files(paths), block_bytes, keep_blocks)
    if eng is not None:
        res = eng.search_resident(queries, mode, rank, wildcard, within, exclude, glob,
                                  ignore_case, show, fuzzy, regex, tally, files, by_file,
                                  count_only)
    else:
        queries, flags, windows, exclude = _search_args(queries, mode, within, exclude)
        res = _C.search_index_text(x, text, queries, flags, rank, bool(wildcard), windows,
                                   exclude, bool(glob), bool(ignore_case), show, bool(fuzzy),
                                   bool(regex), tally, _search_files(files, len(queries)),
                                   _by_file(by_file, count_only))
    res.paths = paths
    return res


def map_stage(path: str, spill: str, line_start: int = -1, line_end: int = -1,
              backend: str = "gpu", fmt: str = "binary", cfg=None, **kw) -> dict:
    """Stage 1 of the reference's split job (main.cu:421-433), count-carrying: the line
    window's combined (key, count) records -> ``spill`` (+ ``spill + ".idx"``); returns
    the counts, spill size and stage times.  ``fmt``: text | binary | kiv."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    return _C.map_stage(cfg, path, line_start, line_end, spill, fmt)


def reduce_stage(spills: list[str], reducer: int = 0, reducers: int = 1,
                 backend: str = "gpu", cfg=None, **kw):
    """Stage 2: key range ``reducer`` of ``reducers`` over the spills, merged with counts
    summed (the device merge on the GPU); returns (result, stats).  The result's entries
    carry the global val; concatenating reducers 0..R-1 gives the single-stage result."""
    cfg = cfg if cfg is not None else make_config(backend, **kw)
    return _C.reduce_spills(cfg, list(spills), reducer, reducers)


def run_multi(text: bytes, world: int, backend: str = "gpu", combine: bool = True,
              samples_per_rank: int = 64, strategy: str | None = None, comm: str = "auto",
              **kw):
    """Multi-rank WordCount in this process, one thread per rank.  comm="auto" (and
    "loopback"): the loopback communicator -- ranks exchange by peer-to-peer device copies
    (over xGMI when the ranks' GPUs differ; rehearses N ranks on fewer GPUs).  comm="rccl":
    an RCCL clique (ncclCommInitAll), one GPU per rank -- opt-in until a run with real RCCL
    peers has been recorded (csrc/engine/dist_runner.hip resolve_local_comm)."""
    dcfg = make_dist_config(world, make_config(backend, combine=combine, **kw),
                            samples_per_rank=samples_per_rank, strategy=strategy)
    return _C.run_multi(text, dcfg, comm)


@dataclass
class WordCount:
    """A WordCount job description (the reference's only job)."""

    path: str | None = None
    line_start: int = -1
    line_end: int = -1
    backend: str = "gpu"
    gpus: int = 1
    options: dict = field(default_factory=dict)

    def load(self):
        cfg = make_config(self.backend, **self.options)
        return _C.load_lines(self.path, self.line_start, self.line_end, cfg.ref_compat)

    def run(self):
        text, _n, _first, _total = self.load()
        if self.gpus > 1:
            return run_multi(text, self.gpus, self.backend, **self.options)
        return wordcount_text(text, self.backend, **self.options)
