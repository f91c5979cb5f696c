"""Independent pure-Python WordCount oracle.

Shares no code with the native engine: tokenization is a direct re-statement of BSD
``strtok_r`` semantics over the reference's delimiter set (main.cu:138), with the
20-emit cap (main.cu:141) and key truncation at 29 bytes.  Sorting is Python's bytes
order == unsigned-byte lexicographic == the reference's KIVComparator (KeyValue.h:20-33).
Word n-grams (``ngrams``, ``wordcount(..., ngram=N)``) are stated here once; every engine
matches them exactly.
"""
from __future__ import annotations

import functools
import re

from collections import Counter

DEFAULT_DELIMS = b" ,.-;:'()\"\t"


def split_lines(text: bytes) -> list[bytes]:
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def tokenize(line: bytes, delims: bytes = DEFAULT_DELIMS, emits: int = 20,
             max_key: int = 29) -> tuple[list[bytes], bool]:
    """Tokens of one line and whether the emit cap dropped any."""
    line = line.split(b"\0", 1)[0]  # strtok_r stops at NUL
    dset = set(delims)
    out: list[bytes] = []
    cur = bytearray()
    for c in line:
        if c in dset:
            if cur:
                out.append(bytes(cur))
                cur = bytearray()
        else:
            cur.append(c)
    if cur:
        out.append(bytes(cur))
    dropped = len(out) > emits
    return [t[:max_key] for t in out[:emits]], dropped


def ngrams(line: bytes, n: int, delims: bytes = DEFAULT_DELIMS, emits: int = 20,
           max_key: int = 29) -> tuple[list[bytes], bool, int]:
    """The word n-grams of one line: (keys, overflow, truncated).

    The line's tokens t0 .. t(T-1) are taken uncapped and untruncated; the n-grams are
    g_i = t_i + b" " + ... + b" " + t_(i+n-1) for i = 0 .. T-n (none if T < n), always
    joined by one 0x20 byte whatever stood between the tokens.  The first ``emits`` of
    them are emitted, each as the first ``max_key`` bytes of g_i; ``overflow`` says the
    line had more, ``truncated`` counts the emitted n-grams longer than ``max_key``.
    n = 1 gives the tokens themselves."""
    if not 1 <= n <= 3:
        raise ValueError("ngram must be in [1, 3]")
    toks, _ = tokenize(line, delims, emits=len(line) + 1, max_key=len(line) + 1)
    grams = [b" ".join(toks[i:i + n]) for i in range(len(toks) - n + 1)]
    emitted = grams[:emits]
    return ([g[:max_key] for g in emitted], len(grams) > emits,
            sum(len(g) > max_key for g in emitted))


def wordcount(text: bytes, delims: bytes = DEFAULT_DELIMS, emits: int = 20, max_key: int = 29,
              ngram: int = 1, stats: bool = False):
    """Returns (entries, num_tokens, overflow_lines): entries = [(key, val, count)] sorted.
    ``ngram`` = 2, 3: one record per word n-gram of a line (see ``ngrams``); num_tokens then
    counts the emitted n-grams.  ``stats=True`` appends the number of truncated records:
    (entries, num_tokens, overflow_lines, truncated)."""
    counter: Counter = Counter()
    overflow = 0
    truncated = 0
    for line in split_lines(text):
        toks, dropped, trunc = ngrams(line, ngram, delims, emits, max_key)
        counter.update(toks)
        overflow += dropped
        truncated += trunc
    entries = []
    pos = 0
    for key in sorted(counter):
        entries.append((key, pos, counter[key]))
        pos += counter[key]
    if stats:
        return entries, pos, overflow, truncated
    return entries, pos, overflow


def top(entries, k: int):
    """The k entries with the largest count: count descending, ties by key ascending."""
    return sorted(entries, key=lambda e: (-e[2], e[0]))[:k]


def index(text: bytes, delims: bytes = DEFAULT_DELIMS, emits: int = 20, max_key: int = 29,
          first_line: int = 0):
    """The inverted index of ``text``: ``(entries, postings)``.

    Every token a line emits under the word job's rules (``tokenize``: the delimiter set, a
    NUL ends the line's tokens, the first ``emits`` tokens only, keys cut to ``max_key``
    bytes) yields one pair (key, line), ``line`` being the global 0-based line number
    ``first_line + i``.  The pairs are sorted by (key in unsigned-byte order, line).
    ``entries`` are exactly ``wordcount``'s ``(key, val, count)``; ``postings`` holds one
    line number per emitted token in sorted pair order, so word i's list is
    ``postings[val_i : val_i + count_i]``, non-decreasing, one posting per occurrence (a
    word twice on a line has that line twice).  Keys that merge under truncation merge
    their lists."""
    pairs = []
    for i, line in enumerate(split_lines(text)):
        toks, _dropped = tokenize(line, delims, emits, max_key)
        pairs.extend((t, first_line + i) for t in toks)
    pairs.sort()
    entries = []
    for pos, (key, _line) in enumerate(pairs):
        if entries and entries[-1][0] == key:
            entries[-1][2] += 1
        else:
            entries.append([key, pos, 1])
    return [tuple(e) for e in entries], [line for _key, line in pairs]


def index_lines(entries, postings, key: bytes, unique: bool = False) -> list[int]:
    """The lines of ``key`` in an index (``unique``: each line once); [] if absent."""
    for k, val, count in entries:
        if k == key:
            lines = postings[val:val + count]
            return sorted(set(lines)) if unique else list(lines)
    return []


def format_index(entries, postings) -> bytes:
    """The CLI's ``--index`` result lines, in key order."""
    return b"".join(
        b"print key: %s \t count: %d \t lines: %s\n"
        % (k, c, b" ".join(b"%d" % l for l in postings[v:v + c]))
        for k, v, c in entries)


CORPUS_RULES = """
Several files in one index.  An index over the lines [F, F + N) is cut into S >= 1 segments,
the files of a corpus: consecutive, possibly empty line ranges that cover [F, F + N) in order.
A segment is (id, first_line, base, lines): id numbers the files in the order they were begun
(the first text indexed is file 0; a dropped file never frees its id), first_line is the global
number of the file's first line that is still in the index, base is that line's number inside
the file (0 until lines of the file have been dropped), lines is how many of its lines the index
holds.  A global line l belongs to the LAST segment with first_line <= l, so an empty file
between two others owns no line; inside its file the line has the number l - first_line + base,
counted from 0.

Dropping the d oldest lines, 0 < d <= N, moves F to F + d.  The first segment that stays is the
last one that begins at or before line F + d: it keeps its id, its first_line becomes F + d and
its base grows by the lines it lost.  Every segment in front of it leaves the table, the empty
ones too; the non-empty ones among them are the dropped files.  d == N therefore leaves the last
file, empty, and a text appended without beginning a new file continues its numbering.  d == 0
changes nothing.

A file that lacks its last newline is given one before the next file begins; the byte makes no
new line, so every file keeps its own numbering.

File sets.  A query may name a set of file ids, distinct and ascending; no set means every file.
Its matching set is what its mode answers -- all, any, phrase, near or expr, after the exclusion
terms -- intersected with the lines whose segment's id is in the set.  An id that is not in the
table selects nothing and is no error.  The set selects lines only: a ranked query's N and
counts stay those of the whole index, so its answer is the unrestricted ranking filtered to the
set and cut to K, and matches counts the restricted set.  A set whose ids are not strictly
ascending is refused.

Answers by file.  A batch may ask, beside each query's lines, for every returned line's file id
and local number (``locate``), in the order of the lines (ranked: rank order), and per query for
the files with at least one returned line, ids ascending, each with its number of returned lines
(``by_file``); the counts of a query add up to its returned lines -- unranked every match, ranked
the min(K, matches) winners.  Count only answers those counts and the matches alone, no line; it
is refused together with a ranking, shown lines or a tally.
"""

CORPUS_MAX_FILES = 65536


def segments_of(file_texts, first_line: int = 0, drop: int = 0):
    """The table of a corpus (``CORPUS_RULES``): ``[(id, first_line, base, lines)]`` for the
    files ``file_texts`` indexed one after the other from ``first_line``, after the ``drop``
    oldest lines have been dropped.  Written from the files' own line counts; a file that lacks
    its last newline counts that line."""
    counts = [len(split_lines(t)) for t in file_texts]
    if not counts:
        raise ValueError("a corpus is one file or more")
    total = sum(counts)
    if not 0 <= drop <= total:
        raise ValueError("drop takes 0 <= d <= %d lines" % total)
    starts, at = [], first_line
    for c in counts:
        starts.append(at)
        at += c
    end = first_line + total
    if drop == 0:
        return [(i, starts[i], 0, counts[i]) for i in range(len(counts))]
    cut = first_line + drop
    keep = max(i for i in range(len(counts)) if starts[i] <= cut)
    out = [(keep, cut, cut - starts[keep], starts[keep] + counts[keep] - cut)]
    out += [(i, starts[i], 0, counts[i]) for i in range(keep + 1, len(counts))]
    assert sum(r[3] for r in out) == end - cut
    return out


def append_segments(table, lines: int, new_file: bool = False):
    """``table`` after ``lines`` more lines behind it (``CORPUS_RULES``): a new file with the
    next id (one more than the last file's), or more lines of the last file."""
    table = [tuple(s) for s in table]
    if new_file:
        if len(table) >= CORPUS_MAX_FILES:
            raise ValueError("an index holds at most %d files" % CORPUS_MAX_FILES)
        last = table[-1]
        return table + [(last[0] + 1, last[1] + last[3], 0, lines)]
    i, first, base, n = table[-1]
    return table[:-1] + [(i, first, base, n + lines)]


def drop_segments(table, d: int):
    """``(table, dropped files)`` after the ``d`` oldest lines have left (``CORPUS_RULES``)."""
    table = [tuple(s) for s in table]
    total = sum(s[3] for s in table)
    if not 0 <= d <= total:
        raise ValueError("drop takes 0 <= d <= %d lines" % total)
    if d == 0:
        return table, 0
    cut = table[0][1] + d
    keep = max(j for j, s in enumerate(table) if s[1] <= cut)
    i, first, base, n = table[keep]
    gone = sum(1 for s in table[:keep] if s[3])
    return [(i, cut, base + cut - first, first + n - cut)] + table[keep + 1:], gone


def locate(table, line: int):
    """``(id, local line)`` of global ``line`` under ``table`` (``CORPUS_RULES``): the last
    segment that begins at or before it."""
    at = None
    for seg in table:
        if seg[1] <= line:
            at = seg
    if at is None or line >= table[-1][1] + table[-1][3]:
        raise ValueError("line %d outside the table's lines" % line)
    return at[0], line - at[1] + at[2]


def by_file(table, lines):
    """``lines`` by file: ``(ids, locals, hits)`` -- parallel to ``lines`` the file id and local
    number of each, and ``[(id, count)]`` ascending by id over the files with a line."""
    where = [locate(table, l) for l in lines]
    counts = {}
    for i, _local in where:
        counts[i] = counts.get(i, 0) + 1
    return [w[0] for w in where], [w[1] for w in where], sorted(counts.items())


def _check_files(files):
    files = list(files)
    if any(not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < 1 << 32 for f in files) \
            or any(a >= b for a, b in zip(files, files[1:])):
        raise ValueError("a file set is distinct file ids in ascending order, not %r" % (files,))
    return set(files)


def in_files(table, lines, files):
    """The ``lines`` whose file is in the set ``files`` (``CORPUS_RULES``; ``None``: all)."""
    if files is None:
        return list(lines)
    if table is None:
        raise ValueError("a file set needs the table (segments_of)")
    want = _check_files(files)
    return [l for l in lines if locate(table, l)[0] in want] if want else list(lines)


MAX_SEARCH_TERMS = 8


def prefix_terms(terms, wildcard: bool, delims: bytes = DEFAULT_DELIMS, max_key: int = 29):
    """The terms of a query as ``(p, is_prefix)`` pairs, validated and cut.

    Without ``wildcard`` every term is literal.  With it, a term that ends in ``*`` and is
    longer than one byte is a prefix term of what precedes the star, a lone ``*`` is an
    error and a ``*`` anywhere else is literal.  ``p`` is non-empty and validated exactly
    as a term is (no NUL, newline or byte of ``delims``: ``ValueError``), and cut to
    ``max_key`` bytes as a term is.  A prefix of ``max_key`` bytes (after the cut) is
    exactly the plain term ``p``: it comes back with ``is_prefix`` False."""
    bad = set(delims) | {0, 0x0A}
    out = []
    for t in terms:
        if wildcard and t == b"*":
            raise ValueError("a lone * is no prefix term")
        pre = bool(wildcard) and len(t) > 1 and t.endswith(b"*")
        p = t[:-1] if pre else t
        if not p or any(c in bad for c in p):
            raise ValueError("invalid term %r" % (t,))
        p = p[:max_key]
        out.append((p, pre and len(p) < max_key))
    return out


PATTERN_RULES = """
    Pattern terms (``glob=True``) and ``ignore_case=True``.

    - With ``glob``, runs of ``*`` in a term collapse to one ``*`` first.  A term without ``*``
      or ``?`` is then a plain term; ``p*`` with ``p`` non-empty and free of metacharacters is
      the prefix term of ``wildcard`` (its cut rule included: ``glob`` is a superset of
      ``wildcard``, and both together are ``glob``); anything else that holds a ``*`` or ``?``
      is a pattern term.  There is no escape character.
    - A pattern's bytes other than ``*`` and ``?`` are validated as a term's are.  Refused
      (``ValueError``): a pattern longer than ``max_key`` bytes after the collapse (a pattern
      is never cut), and one with no byte other than ``*``.  ``???`` is legal.
    - A pattern term's words are the index keys (cut to ``max_key`` as the index holds them)
      that the whole pattern matches: ``*`` any run of bytes, the empty run included; ``?``
      exactly one byte; every other byte itself.  Its list is the multiset union of its words'
      postings, its count the sum of their counts; without a word it is absent.  In phrase and
      near verification a token matches when its cut key matches the pattern.
    - ``ignore_case`` holds for all terms of a query, positive and exclusion: each is cut
      exactly as without it and then evaluated as a pattern whose bytes A-Z and a-z match
      either case -- plain ``hamlet`` as the pattern ``hamlet`` (a ``*`` or ``?`` in it stays
      literal), prefix ``ham*`` as ``ham*``.  Only ASCII letters fold.
    - Identity: two pattern terms are the same term when their collapsed pattern bytes are
      equal (under ``ignore_case``: after lower-casing ASCII).  The later one repeats the
      earlier one: same count, not merged again, scores once.  A pattern term is never the
      same as a plain or prefix term, never inside another term's range, and no term is
      inside it; the nesting rule applies to plain and prefix terms among themselves.
    - Ranked: weight and tf as for a prefix term.  Lists of pattern terms may overlap, so a
      score is at most 32 * emits_per_line * 8; a ranked query with a pattern term is refused
      when emits_per_line > RANK_MAX_EMITS / 8.
    - ``merged`` adds the count of every pattern term that covers two or more words and
      repeats no earlier term of its query.

    The matching here is independent of the engines' matcher: the pattern is translated to a
    bytes regular expression (``re.escape``, ``*`` -> ``.*``, ``?`` -> ``.``, DOTALL,
    ``fullmatch``), a folding letter to a two-byte class.
"""


FUZZY_RULES = """
    Fuzzy terms (``fuzzy=True``): ``Hamlet~1``, ``quene~2``.

    - Syntax.  With ``fuzzy``, a term ``t`` with ``len(t) >= 3``, ``t[-2] == '~'`` and ``t[-1]``
      a decimal digit is a fuzzy term of the word ``w = t[:-2]`` with budget ``d = t[-1]``.
      ``d`` must be 1 or 2 (``ValueError`` otherwise).  A ``~`` anywhere else is a literal byte
      of its word: no digit behind it, two digits behind it, or ``~1`` in the middle of a word.
      Without ``fuzzy``, ``Hamlet~1`` is the literal word.  This reading comes before the
      wildcard and glob reading of the term.
    - The word.  ``w`` is validated byte for byte as a term is.  It is never cut: ``len(w) >
      max_key`` is refused.  It must be longer than its budget: ``len(w) <= d`` is refused.
      With ``glob`` or ``wildcard`` also on, a ``w`` that holds ``*`` or ``?`` is refused.
      ``fuzzy`` implies neither and combines with both and with ``ignore_case``.
    - Words.  A fuzzy term's words are the index keys ``k`` (cut to ``max_key`` as the index
      holds them) with ``lev(w, k) <= d``: the Levenshtein distance over bytes, one insertion,
      deletion or substitution costing 1, no transposition, no UTF-8 awareness.  Under
      ``ignore_case`` ASCII letters match either case and nothing else folds.
    - Everything else is a pattern term's rule (``PATTERN_RULES``) with this matcher: the list,
      the count, absence, the modes, phrase / near verification and show spans (a token matches
      when its cut key is within ``d`` of ``w``), the ranked bound and refusal, ``merged``.
    - Identity.  Two fuzzy terms are the same term when their ``w`` bytes (under ``ignore_case``:
      after lower-casing ASCII) and their budget are equal; ``ham~1`` and ``ham~2`` differ.  A
      fuzzy term is never the same as a plain, prefix or pattern term and takes no part in the
      nesting rule.
    - Output prints the term as asked: ``Hamlet~1``.

    The matching here is independent of the engines' banded matcher: a plain full-matrix
    dynamic program over the two byte strings.
"""


REGEX_RULES = r"""
    Regex terms (``regex=True``): ``/\[?Hamlet[!?\]]?/``, ``/(king|queen)[!?]?/``.

    - Reading.  With ``regex`` a term that starts with ``/`` is a regex term: at least three
      bytes, ending in a ``/`` that an odd run of backslashes does not escape; the source is what
      stands between the slashes.  ``/``, ``//`` and ``/ab`` are refused.  The reading comes
      before the fuzzy, wildcard and glob readings; nothing inside the slashes is read by them.
      Without ``regex`` the term is the literal word.
    - Syntax, over bytes.  A literal byte; ``\x`` for a byte ``x`` that is no ASCII letter or
      digit (a letter or digit behind a backslash is refused); ``.`` any one byte; ``[...]`` and
      ``[^...]`` with single bytes and ranges ``a-z``, ``\`` escapes, ``]`` escaped, ``-`` first
      or last literal, ``^`` special only first; ``( )`` groups, ``|`` alternates, ``*``, ``+``,
      ``?`` repeat the atom before them; an empty branch or group matches the empty string.
      Refused: the empty source; a quantifier with nothing to repeat or directly behind another;
      an unescaped ``{``, ``}``, ``^``, ``$`` outside a class; unbalanced parentheses; a range
      with lo > hi, an empty or unterminated class; a NUL or newline; nesting deeper than 32; a
      source longer than 128 bytes; more than 32 positions (literals, dots, classes).
      Delimiter bytes are legal in the source and match no key.  A regex is never cut.
    - Words.  The index keys (cut to ``max_key``) that the whole expression matches, anchored at
      both ends.  Nothing matches beyond the key's bytes.
    - ``ignore_case``.  A position's byte set -- a literal's byte, a class's members before its
      negation -- is closed under the ASCII case swap, then negated: ``[^a]`` matches neither
      ``a`` nor ``A``.
    - Identity.  Two regex terms are the same term when their sources are equal byte for byte,
      also under ``ignore_case``; never the same as a term of another kind; outside the nesting.
    - Everything else is a pattern term's rule (``PATTERN_RULES``).

    The evaluation here is independent of the engines' position automaton: the source is parsed
    into a tree, and a token matches when the set of offsets reachable through the tree from
    offset 0 holds its length.
"""

REGEX_MAX_DEPTH = 32
REGEX_MAX_SOURCE = 128
REGEX_MAX_POS = 32


def regex_source(term: bytes) -> bytes:
    """The source of the regex term ``/source/`` (``REGEX_RULES``, reading)."""
    back = len(term) - len(term[:-1].rstrip(b"\\")) - 1 if len(term) >= 3 else 0
    if len(term) < 3 or term[-1] != 0x2F or back % 2:
        raise ValueError("the term %r starts with / but is no /source/" % (term,))
    return term[1:-1]


def regex_parse(src: bytes):
    """The tree of a regex source: ``("set", frozenset, negated)``, ``("cat", (..))``,
    ``("alt", (..))``, ``("rep", node, lo, unbounded)``.  ``ValueError`` for every refusal."""
    if not src:
        raise ValueError("an empty regex source")
    if len(src) > REGEX_MAX_SOURCE:
        raise ValueError("a regex source longer than %d bytes" % REGEX_MAX_SOURCE)
    if 0 in src or 0x0A in src:
        raise ValueError("a regex source holds a NUL or a newline")
    pos, count = 0, 0

    def escape():
        nonlocal pos
        if pos + 1 >= len(src):
            raise ValueError("a trailing backslash")
        c = src[pos + 1]
        if bytes([c]).isalnum() and c < 0x80:
            raise ValueError("a backslash before a letter or digit is reserved")
        pos += 2
        return c

    def leaf(members, negated=False):
        nonlocal count
        count += 1
        if count > REGEX_MAX_POS:
            raise ValueError("more than %d positions" % REGEX_MAX_POS)
        return ("set", frozenset(members), negated)

    def klass():
        nonlocal pos
        negated = pos < len(src) and src[pos] == 0x5E
        pos += negated
        members = set()
        while True:
            if pos >= len(src):
                raise ValueError("an unterminated class")
            if src[pos] == 0x5D:
                pos += 1
                break
            if src[pos] == 0x5C:
                lo = escape()
            else:
                lo, pos = src[pos], pos + 1
            hi = lo
            if pos + 1 < len(src) and src[pos] == 0x2D and src[pos + 1] != 0x5D:
                pos += 1
                if src[pos] == 0x5C:
                    hi = escape()
                else:
                    hi, pos = src[pos], pos + 1
                if lo > hi:
                    raise ValueError("a range with lo > hi")
            members.update(range(lo, hi + 1))
        if not members:
            raise ValueError("an empty class")
        return leaf(members, negated)

    def atom(depth):
        nonlocal pos
        c = src[pos]
        if c == 0x28:
            if depth >= REGEX_MAX_DEPTH:
                raise ValueError("nesting deeper than %d" % REGEX_MAX_DEPTH)
            pos += 1
            x = alt(depth + 1)
            if pos >= len(src) or src[pos] != 0x29:
                raise ValueError("unbalanced parentheses")
            pos += 1
            return x
        if c == 0x5B:
            pos += 1
            return klass()
        if c == 0x2E:
            pos += 1
            return leaf(range(256))
        if c in b"{}^$":
            raise ValueError("an unescaped %r outside a class" % chr(c))
        if c in b"*+?":
            raise ValueError("a quantifier with nothing to repeat")
        if c == 0x5C:
            return leaf([escape()])
        pos += 1
        return leaf([c])

    def cat(depth):
        nonlocal pos
        parts = []
        while pos < len(src) and src[pos] not in b"|)":
            x = atom(depth)
            if pos < len(src) and src[pos] in b"*+?":
                q = src[pos]
                pos += 1
                x = ("rep", x, 1 if q == 0x2B else 0, q != 0x3F)
                if pos < len(src) and src[pos] in b"*+?":
                    raise ValueError("a quantifier directly after another quantifier")
            parts.append(x)
        return ("cat", parts)

    def alt(depth):
        nonlocal pos
        branches = [cat(depth)]
        while pos < len(src) and src[pos] == 0x7C:
            pos += 1
            branches.append(cat(depth))
        return ("alt", branches)

    tree = alt(0)
    if pos != len(src):
        raise ValueError("unbalanced parentheses")
    return _freeze(tree)


def _freeze(node):
    """The tree with tuples for lists: hashable, so a (tree, token) verdict can be cached."""
    if node[0] in ("cat", "alt"):
        return (node[0], tuple(_freeze(x) for x in node[1]))
    if node[0] == "rep":
        return ("rep", _freeze(node[1]), node[2], node[3])
    return node


def _swap_case(c: int) -> int:
    return c ^ 0x20 if 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A else c


def _regex_ends(node, tok: bytes, starts: frozenset, fold: bool) -> frozenset:
    """The offsets behind a match of ``node`` that starts at one of ``starts``."""
    kind = node[0]
    if kind == "set":
        _k, members, negated = node
        out = set()
        for o in starts:
            if o < len(tok):
                c = tok[o]
                inside = c in members or (fold and _swap_case(c) in members)
                if inside != negated:
                    out.add(o + 1)
        return frozenset(out)
    if kind == "cat":
        for part in node[1]:
            starts = _regex_ends(part, tok, starts, fold)
            if not starts:
                break
        return starts
    if kind == "alt":
        out = set()
        for branch in node[1]:
            out |= _regex_ends(branch, tok, starts, fold)
        return frozenset(out)
    _k, inner, lo, unbounded = node  # "rep"
    once = _regex_ends(inner, tok, starts, fold)
    if not unbounded:  # `?`
        return starts | once
    reached, frontier = set(once), once
    while frontier:  # the offsets behind one, two, ... rounds
        frontier = _regex_ends(inner, tok, frozenset(frontier), fold) - reached
        reached |= frontier
    return frozenset(reached) | (starts if lo == 0 else frozenset())


@functools.lru_cache(maxsize=1 << 16)
def regex_fits(tree, tok: bytes, fold: bool = False) -> bool:
    """Does the whole token match the tree (``regex_parse``)?  (Cached: a text's tokens repeat.)"""
    return len(tok) in _regex_ends(tree, tok, frozenset([0]), fold)


def _fold(c: int) -> int:
    return c | 0x20 if 0x41 <= c <= 0x5A else c


@functools.lru_cache(maxsize=1 << 16)
def levenshtein(a: bytes, b: bytes, fold: bool = False) -> int:
    """The edit distance of two byte strings, the whole matrix row by row.  (Cached: a text's
    tokens repeat.)"""
    if fold:
        a, b = bytes(map(_fold, a)), bytes(map(_fold, b))
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        row = [i]
        for j, cb in enumerate(b, 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = row
    return prev[-1]


class QueryTerm:
    """One term as it is evaluated: ``kind`` is ``"plain"``, ``"prefix"``, ``"pattern"`` or
    ``"fuzzy"``; ``p`` the cut bytes of a plain or prefix term, a fuzzy term's word; ``rx`` a
    pattern's compiled expression; ``d`` and ``fold`` a fuzzy term's budget and fold; ``ident``
    what makes two pattern terms, or two fuzzy terms, the same term."""

    def __init__(self, kind, p=b"", rx=None, ident=None, d=0, fold=False):
        self.kind, self.p, self.rx, self.ident, self.d, self.fold = kind, p, rx, ident, d, fold

    @property
    def scattered(self) -> bool:
        """A term whose words are no key range: told apart by ``ident``, outside the nesting."""
        return self.kind in ("pattern", "fuzzy", "regex")

    def fits(self, tok: bytes) -> bool:
        if self.kind == "regex":
            return regex_fits(self.rx, tok, self.fold)
        if self.kind == "fuzzy":
            return levenshtein(self.p, tok, self.fold) <= self.d
        if self.kind == "pattern":
            return self.rx.fullmatch(tok) is not None
        return tok[:len(self.p)] == self.p if self.kind == "prefix" else tok == self.p


def _fuzzy_term(w: bytes, d: int, fold: bool) -> QueryTerm:
    ident = ("fuzzy", bytes(map(_fold, w)) if fold else w, d)
    return QueryTerm("fuzzy", p=w, ident=ident, d=d, fold=fold)


def _pattern_term(cells, fold: bool) -> QueryTerm:
    """The pattern term of ``cells``: (byte, is_meta) pairs."""
    out = []
    for c, meta in cells:
        if meta:
            out.append(b".*" if c == 0x2A else b".")
        elif fold and (0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A):
            out.append(b"[" + bytes([c & ~0x20]) + bytes([c | 0x20]) + b"]")
        else:
            out.append(re.escape(bytes([c])))
    ident = tuple((c | 0x20 if fold and not meta and 0x41 <= c <= 0x5A else c, meta)
                  for c, meta in cells)
    return QueryTerm("pattern", rx=re.compile(b"".join(out), re.DOTALL), ident=ident)


def query_terms(terms, wildcard: bool = False, glob: bool = False, ignore_case: bool = False,
                delims: bytes = DEFAULT_DELIMS, max_key: int = 29, *, fuzzy: bool = False, regex: bool = False):
    """The terms of a query as ``QueryTerm`` objects, validated and cut: ``prefix_terms``'
    sibling for ``glob`` and ``ignore_case`` (``PATTERN_RULES``) and ``fuzzy``
    (``FUZZY_RULES``)."""
    bad = set(delims) | {0, 0x0A}
    out = []
    for t in terms:
        if regex and t[:1] == b"/":  # (read before every other reading: REGEX_RULES)
            src = regex_source(t)
            out.append(QueryTerm("regex", p=src, rx=regex_parse(src), ident=("regex", src),
                                 fold=ignore_case))
            continue
        if fuzzy and len(t) >= 3 and t[-2] == 0x7E and 0x30 <= t[-1] <= 0x39:
            w, d = t[:-2], t[-1] - 0x30  # (read before the wildcard and glob reading)
            if d not in (1, 2):
                raise ValueError("the fuzzy term %r: a budget is 1 or 2" % (t,))
            if len(w) <= d:
                raise ValueError("the fuzzy term %r: its word is no longer than its budget" % (t,))
            if len(w) > max_key:
                raise ValueError("the fuzzy term %r: its word is longer than max_key" % (t,))
            if (glob or wildcard) and any(c in b"*?" for c in w):
                raise ValueError("the fuzzy term %r holds a * or ?: fuzzy or a pattern, never "
                                 "both" % (t,))
            if any(c in bad for c in w):
                raise ValueError("invalid term %r" % (t,))
            out.append(_fuzzy_term(w, d, ignore_case))
            continue
        cells = None  # a pattern term's (byte, is_meta) pairs
        if glob:
            t = re.sub(rb"\*+", b"*", t)
            if t == b"*":
                raise ValueError("a pattern of stars alone is no term")
            metas = [i for i, c in enumerate(t) if c in b"*?"]
            if metas and not (metas == [len(t) - 1] and t.endswith(b"*")):
                if len(t) > max_key:
                    raise ValueError("the pattern %r is longer than max_key" % (t,))
                cells = [(c, c in b"*?") for c in t]
                if any(c in bad for c, meta in cells if not meta):
                    raise ValueError("invalid term %r" % (t,))
        if cells is None:
            (p, pre), = prefix_terms([t], wildcard or glob, delims, max_key)
            if not ignore_case:
                out.append(QueryTerm("prefix" if pre else "plain", p))
                continue
            cells = [(c, False) for c in p] + ([(0x2A, True)] if pre else [])
        out.append(_pattern_term(cells, ignore_case))
    return out


def _qt_words(entries, term: QueryTerm):
    return [i for i, (k, _v, _c) in enumerate(entries) if term.fits(k)]


def _term_words(entries, p: bytes, pre: bool):
    """The indices of a term's words among ``entries``: the keys that start with ``p``
    (a word equal to ``p`` among them) for a prefix term, the key ``p`` for a plain one."""
    return [i for i, (k, _v, _c) in enumerate(entries)
            if (k[:len(p)] == p if pre else k == p)]


def _term_list(entries, postings, words):
    """The merged list of the words: the multiset union of their postings, non-decreasing."""
    return sorted(l for i in words for l in postings[entries[i][1]:entries[i][1] + entries[i][2]])


EXCLUDE_RULES = """
    Exclusion terms.  A query has 1 or more positive terms and 0 or more exclusion terms
    (``exclude``); together they number at most 8.  An exclusion term is validated, cut to
    max_key_len and, with wildcards, read as a prefix term exactly as a positive term is.

    - Excluded lines.  A term's lines are the distinct lines of its postings list, as for
      `all`; a prefix term's list is its merged list.  A query's excluded lines are the union
      of its exclusion terms' lines.  An absent exclusion term excludes nothing: it does not
      empty the answer, unlike an absent positive term in `all`.
    - Matching set.  The matching set is what the mode answers for the positive terms alone,
      minus the excluded lines.  The mode, the `near` window, the repetition rules and the
      one-term shortcuts apply to the positive terms only: the `near` shortcut "W >=
      emits_per_line answers as `all`" and the shortcut "one distinct term answers as `all`"
      count distinct positive terms, and phrase and `near` verification sees only the
      positive terms.  [alpha beta] not gamma as a phrase matches the line `alpha beta delta`
      and does not match `alpha beta gamma`: the second line is excluded because it holds
      gamma anywhere among its emitted tokens.
    - Pure function of the index.  Exclusion depends only on the index, so a token past the
      emit cap excludes nothing: the rule every other mode follows.
    - Overlap with a positive term.  An exclusion term whose words equal or contain a
      positive term's words empties `all`, `phrase` and `near`; in `any` it removes that
      term's lines from the union.  This is legal, not an error.
    - Ranked.  `matches` counts the matching set after exclusion.  Exclusion terms take no
      part in the score, in the "distinct present terms" or in the nesting rule: in Ham* not
      Hamlet, Ham* still scores with its full merged count.  The bound score <= 32 *
      emits_per_line is unchanged.
    - term_counts report every term, positive terms first and then the exclusion terms in
      the order given; an exclusion term reports its word's count, or its merged count.
    - `merged`: the rule is unchanged and runs over all of the query's terms: the sum of the
      counts over the query's terms that cover two or more words, a term whose words repeat
      an earlier term's left out.  An exclusion prefix term covering two or more words is
      therefore merged and counted; one covering a single word uses that word's list in
      place.
    - Refused (``ValueError``): a query with no positive term, more than 8 terms in total,
      an invalid exclusion term, a lone `*` with wildcards.
"""


def _check_exclude(terms, exclude):
    """The exclusion terms as a list (``None``: none), the term budget checked."""
    exclude = [] if exclude is None else list(exclude)
    if isinstance(terms, (bytes, str)) or any(not isinstance(t, bytes) for t in exclude):
        raise ValueError("exclusion terms are byte strings")
    if len(terms) < 1:
        raise ValueError("a query takes at least one positive term")
    if len(terms) + len(exclude) > MAX_SEARCH_TERMS:
        raise ValueError("a query takes at most %d terms, positive and exclusion terms "
                         "together" % MAX_SEARCH_TERMS)
    return exclude


def _excluded_by_index(entries, postings, exclude, wildcard, delims, max_key, glob=False,
                       ignore_case=False, fuzzy=False, regex=False):
    """``(lines, counts)`` of exclusion terms over an index: the union of the terms' lines as
    a set, and every term's count (its word's, or its merged count; 0: absent)."""
    out, counts = set(), []
    for term in query_terms(exclude, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex):
        lines = _term_list(entries, postings, _qt_words(entries, term))
        counts.append(len(lines))
        out.update(lines)
    return out, counts


def _excluded_by_text(text, exclude, wildcard, delims, emits, max_key, first_line, glob=False,
                      ignore_case=False, fuzzy=False, regex=False):
    """The same from the text: a line is excluded when one of its emitted tokens (the index
    holds no other) matches an exclusion term; a term's count is its matching tokens."""
    want = query_terms(exclude, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex)
    out, counts = set(), [0] * len(want)
    for i, line in enumerate(split_lines(text)):
        toks, _dropped = tokenize(line, delims, emits, max_key)
        for j, term in enumerate(want):
            n = sum(term.fits(tok) for tok in toks)
            counts[j] += n
            if n:
                out.add(first_line + i)
    return out, counts


def merged_elements(entries, queries, delims: bytes = DEFAULT_DELIMS, max_key: int = 29, *,
                    exclude=None, glob: bool = False, ignore_case: bool = False,
                    fuzzy: bool = False, regex: bool = False,
                    wildcard: bool = True) -> int:
    """``SearchResult.merged`` of a device batch of wildcard ``queries`` (term lists): over
    the batch's prefix terms that cover two or more words, a term whose words repeat an
    earlier term's of its query left out, the sum of their counts.  (A term that covers one
    word uses that word's list in place: nothing is merged.)

    ``exclude``: one entry per query, ``None`` or its exclusion terms, which stand behind the
    query's own terms (``EXCLUDE_RULES``: the rule runs over all of the query's terms).

    ``glob`` / ``ignore_case`` (``PATTERN_RULES``): a pattern term that covers two or more
    words and repeats no earlier pattern term of its query adds its count.  ``wildcard=False``
    with them: the batch was asked without wildcards (a trailing ``*`` is literal unless
    ``glob`` reads it)."""
    total = 0
    if exclude is not None:
        if len(exclude) != len(queries):
            raise ValueError("exclude takes one entry per query")
        queries = [list(q) + _check_exclude(list(q), x) for q, x in zip(queries, exclude)]
    for terms in queries:
        seen = []
        for term in query_terms(terms, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex):
            words = _qt_words(entries, term)
            # what a later term must repeat: a pattern term's pattern, another term's words
            same = term.ident if term.scattered else words
            if len(words) >= 2 and same not in seen:
                total += sum(entries[i][2] for i in words)
            seen.append(same)
    return total


def search(entries, postings, terms, mode: str = "all", delims: bytes = DEFAULT_DELIMS,
           max_key: int = 29, *, wildcard: bool = False, exclude=None, glob: bool = False,
           ignore_case: bool = False, fuzzy: bool = False, regex: bool = False, files=None,
           table=None):
    """One all/any word query over an index: ``(lines, counts)``.

    ``files`` / ``table``: the query's file set under the corpus's table (``CORPUS_RULES``):
    the answer below, intersected with the lines of those files.

    ``entries`` and ``postings`` are ``index``'s output.  A query is 1 to 8 ``terms`` and a
    ``mode``.  A term is a non-empty byte string without NUL, newline or a byte of
    ``delims`` (``ValueError`` otherwise); one longer than ``max_key`` is cut to its first
    ``max_key`` bytes, as the map cuts keys, so it matches the merged list of every long
    word with that prefix.  A term's lines are the distinct lines of its postings list; an
    absent word has none.  ``"all"`` is the intersection of the terms' lines (empty as soon
    as one term is absent), ``"any"`` their union; a repeated term changes nothing.
    ``lines`` are global line numbers, ascending, each once; ``counts[t]`` is the count of
    term ``t``'s word, 0 when it is absent.

    ``wildcard=True``: a term may be a prefix term (``prefix_terms``).  Its words are the
    index keys ``k`` with ``k[:len(p)] == p``, a word equal to ``p`` among them; its list is
    the multiset union of those words' postings, non-decreasing; its count is the sum of
    their counts; if no word matches, the term is absent.  In ``"all"`` and ``"any"`` it
    behaves as a word with that list.

    ``exclude``: the query's exclusion terms (``EXCLUDE_RULES``).  The answer is the one
    above for ``terms`` alone minus the excluded lines, and ``counts`` lists the terms'
    counts first and then the exclusion terms'."""
    if mode not in ("all", "any"):
        raise ValueError("mode must be 'all' or 'any'")
    terms = list(terms)
    if files is not None:
        lines, counts = search(entries, postings, terms, mode, delims, max_key,
                               wildcard=wildcard, exclude=exclude, glob=glob,
                               ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        return in_files(table, lines, files), counts
    if exclude is not None:
        exclude = _check_exclude(terms, exclude)
        lines, counts = search(entries, postings, terms, mode, delims, max_key,
                               wildcard=wildcard, glob=glob, ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        gone, xcounts = _excluded_by_index(entries, postings, exclude, wildcard, delims,
                                           max_key, glob, ignore_case, fuzzy, regex)
        return [l for l in lines if l not in gone], counts + xcounts
    if not 1 <= len(terms) <= MAX_SEARCH_TERMS:
        raise ValueError("a query takes 1 to %d terms" % MAX_SEARCH_TERMS)
    if wildcard or glob or ignore_case or fuzzy or regex:  # (``glob`` / ``ignore_case``: PATTERN_RULES)
        sets, counts = [], []
        for term in query_terms(terms, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex):
            lines = _term_list(entries, postings, _qt_words(entries, term))
            counts.append(len(lines))
            sets.append(set(lines))
        hit = set.intersection(*sets) if mode == "all" else set.union(*sets)
        return sorted(hit), counts
    bad = set(delims) | {0, 0x0A}
    for t in terms:
        if not t or any(c in bad for c in t):
            raise ValueError("invalid term %r" % (t,))
    by_key = {k: (v, c) for k, v, c in entries}
    sets, counts = [], []
    for t in terms:
        v, c = by_key.get(t[:max_key], (0, 0))
        counts.append(c)
        sets.append(set(postings[v:v + c]))
    hit = set.intersection(*sets) if mode == "all" else set.union(*sets)
    return sorted(hit), counts


def phrase(text: bytes, terms, delims: bytes = DEFAULT_DELIMS, emits: int = 20,
           max_key: int = 29, first_line: int = 0, *, wildcard: bool = False, exclude=None,
           glob: bool = False, ignore_case: bool = False, fuzzy: bool = False, regex: bool = False,
           files=None, table=None):
    """One phrase query over ``text``: ``(lines, counts)``, as ``search`` answers
    (``files`` / ``table`` too).

    `phrase` answers the lines on which the terms occur as consecutive tokens, in order.
    A line's token sequence is exactly what the word job emits for it, in order: the job's
    delimiter set, a NUL ends the line's tokens, only the first emits_per_line tokens, each
    token cut to max_key_len bytes.  A line with tokens k_0 .. k_(n-1) matches the terms
    t_0 .. t_(m-1), each cut to max_key_len bytes, when some o exists with k_(o+j) == t_j
    for every j in [0, m).  Tokens past the emit cap do not exist for this purpose, a phrase
    never crosses a line end, and what stood between two consecutive tokens does not matter:
    any run of delimiters, of any length, counts.  Repeated terms are significant here:
    [bye, bye] matches only a line with two consecutive bye tokens.  A one-term phrase
    answers as `all` does, an absent term gives an empty answer, and long tokens that merge
    under truncation match as their merged key, the rule the index uses.  The answer and the
    per-term counts have the shape of the other modes'; repeated terms report the same count.

    Terms are validated as ``search`` validates them (``ValueError``).  Written straight from
    the paragraph above: every line is tokenised and every window compared; no index.

    ``wildcard=True``: a term may be a prefix term (``prefix_terms``).  A token matches a
    prefix term when the token's key (cut to ``max_key``) starts with ``p``; a token shorter
    than ``p`` does not match.  Its count is the number of emitted tokens that match it.  A
    one-term phrase answers the lines that hold a matching token, as `all` does.

    ``exclude``: the query's exclusion terms (``EXCLUDE_RULES``).  The answer is the one
    above for ``terms`` alone minus the lines with an emitted token that matches an exclusion
    term, and ``counts`` lists the terms' counts first and then the exclusion terms'."""
    terms = list(terms)
    if files is not None:
        lines, counts = phrase(text, terms, delims, emits, max_key, first_line,
                               wildcard=wildcard, exclude=exclude, glob=glob,
                               ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        return in_files(table, lines, files), counts
    if exclude is not None:
        exclude = _check_exclude(terms, exclude)
        lines, counts = phrase(text, terms, delims, emits, max_key, first_line,
                               wildcard=wildcard, glob=glob, ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        gone, xcounts = _excluded_by_text(text, exclude, wildcard, delims, emits, max_key,
                                          first_line, glob, ignore_case, fuzzy, regex)
        return [l for l in lines if l not in gone], counts + xcounts
    if not 1 <= len(terms) <= MAX_SEARCH_TERMS:
        raise ValueError("a query takes 1 to %d terms" % MAX_SEARCH_TERMS)
    if wildcard or glob or ignore_case or fuzzy or regex:  # (``glob`` / ``ignore_case``: PATTERN_RULES)
        want = query_terms(terms, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex)
        m = len(want)

        def fits(tok, term):
            return term.fits(tok)

        lines = []
        counts = [0] * m
        for i, line in enumerate(split_lines(text)):
            toks, _dropped = tokenize(line, delims, emits, max_key)
            for j, term in enumerate(want):
                counts[j] += sum(fits(tok, term) for tok in toks)
            if any(all(fits(toks[o + j], want[j]) for j in range(m))
                   for o in range(len(toks) - m + 1)):
                lines.append(first_line + i)
        return lines, counts
    bad = set(delims) | {0, 0x0A}
    for t in terms:
        if not t or any(c in bad for c in t):
            raise ValueError("invalid term %r" % (t,))
    want = [t[:max_key] for t in terms]
    m = len(want)
    lines = []
    counts = [0] * m
    for i, line in enumerate(split_lines(text)):
        toks, _dropped = tokenize(line, delims, emits, max_key)
        for j, t in enumerate(want):
            counts[j] += toks.count(t)
        if any(toks[o:o + m] == want for o in range(len(toks) - m + 1)):
            lines.append(first_line + i)
    return lines, counts


MAX_SEARCH_WITHIN = (1 << 32) - 1


def near(text: bytes, terms, within: int, delims: bytes = DEFAULT_DELIMS, emits: int = 20,
         max_key: int = 29, first_line: int = 0, *, wildcard: bool = False, exclude=None,
         glob: bool = False, ignore_case: bool = False, fuzzy: bool = False, regex: bool = False,
         files=None, table=None):
    """One proximity query over ``text``: ``(lines, counts)``, as ``search`` answers
    (``files`` / ``table`` too).

    `near` answers the lines on which the terms occur within ``within`` = W tokens of one
    another, in any order; W is an integer with 1 <= W <= 2^32 - 1 (``ValueError``
    otherwise).  A line's token sequence is exactly the phrase mode's: the job's delimiter
    set, a NUL ends the line's tokens, only the first emits_per_line tokens exist, each
    token cut to max_key_len bytes.  A line with tokens k_0 .. k_(n-1) matches when
    positions a <= b exist with b - a + 1 <= W such that every term is matched by at least
    one token k_i, a <= i <= b.  A plain term, cut to max_key_len bytes, matches a token by
    equality; with ``wildcard=True`` a prefix term (``prefix_terms``) matches a token whose
    key starts with ``p``.  Order does not matter, a repeated term changes nothing (set
    semantics, as in `all`), one token may satisfy several terms, a window never crosses a
    line end, and an absent term gives an empty answer.  A one-term query and every
    W >= emits_per_line answer as `all` does.  ``counts[t]`` is the number of emitted tokens
    that match term ``t``, as `all` reports it.

    Terms are validated as ``search`` validates them (``ValueError``).  Written straight from
    the paragraph above: every line is tokenised and every window of W consecutive tokens
    tested; no index.

    ``exclude``: the query's exclusion terms (``EXCLUDE_RULES``).  The answer is the one
    above for ``terms`` alone minus the lines with an emitted token that matches an exclusion
    term, and ``counts`` lists the terms' counts first and then the exclusion terms'."""
    terms = list(terms)
    if files is not None:
        lines, counts = near(text, terms, within, delims, emits, max_key, first_line,
                             wildcard=wildcard, exclude=exclude, glob=glob,
                             ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        return in_files(table, lines, files), counts
    if exclude is not None:
        exclude = _check_exclude(terms, exclude)
        lines, counts = near(text, terms, within, delims, emits, max_key, first_line,
                             wildcard=wildcard, glob=glob, ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
        gone, xcounts = _excluded_by_text(text, exclude, wildcard, delims, emits, max_key,
                                          first_line, glob, ignore_case, fuzzy, regex)
        return [l for l in lines if l not in gone], counts + xcounts
    if not 1 <= len(terms) <= MAX_SEARCH_TERMS:
        raise ValueError("a query takes 1 to %d terms" % MAX_SEARCH_TERMS)
    if isinstance(within, bool) or not isinstance(within, int) or \
            not 1 <= within <= MAX_SEARCH_WITHIN:
        raise ValueError("a near query takes a window 1 <= W < 2^32, not %r" % (within,))
    # (``glob`` / ``ignore_case``: PATTERN_RULES)
    want = query_terms(terms, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex)

    def fits(tok, term):
        return term.fits(tok)

    lines = []
    counts = [0] * len(want)
    for i, line in enumerate(split_lines(text)):
        toks, _dropped = tokenize(line, delims, emits, max_key)
        for j, term in enumerate(want):
            counts[j] += sum(fits(tok, term) for tok in toks)
        # the windows of W consecutive tokens (a shorter line: the one window it has)
        for a in range(max(len(toks) - within, 0) + 1):
            win = toks[a:a + within]
            if all(any(fits(tok, term) for tok in win) for term in want):
                lines.append(first_line + i)
                break
    return lines, counts


EXPR_RULES = """
    Boolean expressions (``mode="expr"``): ``( to AND be ) OR ( Ham* AND NOT Hamlet )``.

    - Syntax.  An expression is a byte string.  Blanks and tabs separate tokens; ``(`` and ``)``
      are grouping tokens by themselves wherever they stand.  The tokens ``AND``, ``OR`` and
      ``NOT``, exactly these upper-case bytes, are operators; every other token is a term.
      ``NOT`` binds tighter than ``AND``, ``AND`` tighter than ``OR``; ``AND`` and ``OR``
      associate to the left; two operands side by side are joined by ``AND``.  ``and``, ``or``
      and ``not`` in lower case are words; the word ``AND`` cannot be asked for.
    - Terms.  A term is read exactly as a term of any query is (``query_terms``: ``wildcard``,
      ``glob``, ``fuzzy``, ``ignore_case``, the cut to ``max_key``) and with the same errors; one
      that holds a NUL, a newline or a delimiter is refused.  Two operands are the same term when
      they read to the same bytes and the same kind.  A query has 1 to 8 distinct terms, numbered
      in order of first occurrence.
    - Meaning.  A term's lines are the distinct lines of its (merged) list; an absent term has
      none and does not empty the answer.  A line matches when the expression holds with every
      term replaced by "the line is among the term's lines".  Ascending line numbers, each once.
      ``counts`` are in term order.
    - Refused (``ValueError``): an empty expression, unbalanced parentheses, ``()``, a dangling
      operator, more than 8 distinct terms, parentheses nested deeper than ``EXPR_MAX_DEPTH``, and
      an expression that holds for a line with none of its words (``NOT a``, ``a OR NOT b``).
      ``a AND NOT a`` is legal and answers nothing.
    - Ranked: the matching set as above, the score ``any``'s over the expression's terms (``rank``
      with these terms), under a ``NOT`` or not.  Show: ``show`` with these terms.
    - Output: the result line prints the expression, runs of blanks collapsed to one space and
      the ends trimmed (``expr_text``), where the other modes print the joined terms.
    - The walked set (``expr_walked``).  P: the present terms.  A set S of terms covers when every
      set m of terms inside P for which the expression holds (exactly the terms of m holding)
      meets S.  Greedy: S = P; the terms by list length descending, of equal lengths the higher
      term number first; a term is dropped when the rest still covers.  If the expression holds
      for no m inside P, S is empty.  The device walks the summed lengths of S's lists.

    The evaluation here shares nothing with the engines' truth table: the parsed tree is
    evaluated per line with set membership.
"""

EXPR_MAX_DEPTH = 64


def _regex_token_end(expr: bytes, i: int) -> int:
    """The index of the slash that closes the regex token starting at ``expr[i] == '/'``."""
    j = i + 1
    while j < len(expr) and expr[j] != 0x2F:
        j += 2 if expr[j] == 0x5C else 1
    if j >= len(expr):
        raise ValueError("a regex term without its closing /")
    if j + 1 < len(expr) and expr[j + 1] not in b" \t()":
        raise ValueError("a regex term's closing / is followed by a blank, a parenthesis or the end")
    return j


def expr_tokens(expr: bytes, regex: bool = False):
    out, cur = [], bytearray()
    skip = -1
    for i, c in enumerate(expr):
        if i <= skip:
            continue
        if regex and c == 0x2F and not cur:  # a regex token: blanks and parentheses belong to it
            skip = _regex_token_end(expr, i)
            out.append(expr[i:skip + 1])
            continue
        if c in b" \t()":
            if cur:
                out.append(bytes(cur))
                cur = bytearray()
            if c in b"()":
                out.append(bytes([c]))
        else:
            cur.append(c)
    if cur:
        out.append(bytes(cur))
    return out


def expr_text(expr: bytes, regex: bool = False) -> bytes:
    """The expression as a result line prints it (a regex token's blanks are its own)."""
    if not regex:
        return b" ".join(p for p in re.split(rb"[ \t]+", expr) if p)
    out, gap, skip, start = bytearray(), False, -1, True
    for i, c in enumerate(expr):
        if i <= skip:
            continue
        if c in b" \t":
            gap, start = bool(out), True
            continue
        if gap:
            out.append(0x20)
        gap = False
        if c == 0x2F and start:
            skip = _regex_token_end(expr, i)
            out += expr[i:skip + 1]
            start = False
            continue
        out.append(c)
        start = c in b"()"
    return bytes(out)


def expr_parse(expr: bytes, delims: bytes = DEFAULT_DELIMS, max_key: int = 29, *,
               wildcard: bool = False, glob: bool = False, fuzzy: bool = False, regex: bool = False):
    """``(tree, terms)`` of an expression (``EXPR_RULES``): ``terms`` are its distinct terms as
    asked, in order of first occurrence; ``tree`` is ``("term", t)``, ``("not", x)``,
    ``("and", x, y)`` or ``("or", x, y)``.  ``ValueError`` for every refused expression, the one
    that holds for no word among them."""
    toks = expr_tokens(expr, regex)
    if not toks:
        raise ValueError("an empty expression")
    terms, idents = [], []
    pos = 0

    def number(tok):
        query_terms([tok], wildcard, glob, False, delims, max_key, fuzzy=fuzzy, regex=regex)  # its errors
        t, = query_terms([tok], wildcard, glob, False, delims, 1 << 30, fuzzy=fuzzy, regex=regex)
        ident = (t.kind, t.ident if t.scattered else t.p)
        if ident in idents:
            return idents.index(ident)
        if len(terms) == MAX_SEARCH_TERMS:
            raise ValueError("more than %d distinct terms" % MAX_SEARCH_TERMS)
        terms.append(tok)
        idents.append(ident)
        return len(terms) - 1

    def atom(depth):
        nonlocal pos
        neg = False
        while pos < len(toks) and toks[pos] == b"NOT":
            neg, pos = not neg, pos + 1
        if pos == len(toks) or toks[pos] in (b"AND", b"OR"):
            raise ValueError("a dangling operator")
        if toks[pos] == b")":
            raise ValueError("() holds no operand" if pos and toks[pos - 1] == b"("
                             else "a dangling operator before )")
        if toks[pos] == b"(":
            if depth >= EXPR_MAX_DEPTH:
                raise ValueError("parentheses nested deeper than %d" % EXPR_MAX_DEPTH)
            pos += 1
            x = either(depth + 1)
            if pos == len(toks) or toks[pos] != b")":
                raise ValueError("unbalanced parentheses")
            pos += 1
        else:
            x = ("term", number(toks[pos]))
            pos += 1
        return ("not", x) if neg else x

    def both(depth):
        nonlocal pos
        x = atom(depth)
        while pos < len(toks) and toks[pos] not in (b")", b"OR"):
            if toks[pos] == b"AND":
                pos += 1
            x = ("and", x, atom(depth))
        return x

    def either(depth):
        nonlocal pos
        x = both(depth)
        while pos < len(toks) and toks[pos] == b"OR":
            pos += 1
            x = ("or", x, both(depth))
        return x

    tree = either(0)
    if pos != len(toks):
        raise ValueError("unbalanced parentheses")
    if expr_holds(tree, set()):
        raise ValueError("the expression holds for a line with none of its words")
    return tree, terms


def expr_holds(tree, have) -> bool:
    """The tree's value when exactly the terms in the set ``have`` hold."""
    stack, todo = [], [tree]  # (iterative post-order: a left-deep chain may be long)
    while todo:
        n = todo.pop()
        if isinstance(n, str):
            if n == "not":
                stack.append(not stack.pop())
            else:
                b, a = stack.pop(), stack.pop()
                stack.append((a and b) if n == "and" else (a or b))
        elif n[0] == "term":
            stack.append(n[1] in have)
        else:
            todo.append(n[0])
            todo.extend(reversed(n[1:]))
    return stack[0]


def _expr_lists(entries, postings, terms, delims, max_key, wildcard, glob, ignore_case, fuzzy, regex):
    return [_term_list(entries, postings, _qt_words(entries, t))
            for t in query_terms(terms, wildcard, glob, ignore_case, delims, max_key, fuzzy=fuzzy, regex=regex)]


def expr_search(entries, postings, expr: bytes, delims: bytes = DEFAULT_DELIMS,
                max_key: int = 29, *, wildcard: bool = False, glob: bool = False,
                ignore_case: bool = False, fuzzy: bool = False, regex: bool = False,
                files=None, table=None):
    """One ``expr`` query over an index: ``(lines, counts, terms)`` (``EXPR_RULES``);
    ``files`` / ``table``: its file set (``CORPUS_RULES``)."""
    tree, terms = expr_parse(expr, delims, max_key, wildcard=wildcard, glob=glob, fuzzy=fuzzy, regex=regex)
    lists = _expr_lists(entries, postings, terms, delims, max_key, wildcard, glob, ignore_case,
                        fuzzy, regex)
    sets = [set(l) for l in lists]
    lines = [line for line in sorted(set().union(*sets))
             if expr_holds(tree, {t for t, s in enumerate(sets) if line in s})]
    return in_files(table, lines, files), [len(l) for l in lists], terms


def expr_walked(entries, postings, expr: bytes, delims: bytes = DEFAULT_DELIMS,
                max_key: int = 29, *, wildcard: bool = False, glob: bool = False,
                ignore_case: bool = False, fuzzy: bool = False, regex: bool = False) -> int:
    """The list elements the device walks for one ``expr`` query: the summed list lengths of
    the greedy covering set (``EXPR_RULES``, the walked set)."""
    tree, terms = expr_parse(expr, delims, max_key, wildcard=wildcard, glob=glob, fuzzy=fuzzy, regex=regex)
    lens = [len(l) for l in _expr_lists(entries, postings, terms, delims, max_key, wildcard, glob,
                                        ignore_case, fuzzy, regex)]
    present = [t for t, n in enumerate(lens) if n]
    true_sets = []  # the sets of present terms for which the expression holds
    for bits in range(1, 1 << len(present)):
        m = {present[i] for i in range(len(present)) if bits >> i & 1}
        if expr_holds(tree, m):
            true_sets.append(m)
    if not true_sets:
        return 0
    keep = set(present)
    for t in sorted(present, key=lambda t: (-lens[t], -t)):
        rest = keep - {t}
        if all(m & rest for m in true_sets):
            keep = rest
    return sum(lens[t] for t in keep)


def _query_text(queries, exclude):
    """Each query's text in a result line: its terms joined by one space and, when it has
    exclusion terms, `` \t not: `` and those joined by one space."""
    if exclude is None:
        exclude = [None] * len(queries)
    if len(exclude) != len(queries):
        raise ValueError("exclude takes one entry per query")
    return [b" ".join(q) + (b" \t not: " + b" ".join(x) if x else b"")
            for q, x in zip(queries, exclude)]


TALLY_MAX_K = 4096

TALLY_RULES = """
    Tally (``tally=K``): the most frequent words of the lines a query returns.

    - ``K`` is an integer with 1 <= K <= 4096 (``ValueError`` otherwise), and a tally goes with
      a search only.
    - The returned lines of a query are the entries ``show`` would print: unranked, every
      matching line; ranked, the ``min(rank, matches)`` winners.  A line returned for two queries
      counts for each.
    - ``count(q, w)`` is the number of postings of index word ``w`` on a returned line of ``q``:
      what the word job would count over those lines alone, with its delimiters, its emit cap
      (a token past it does not exist) and its key cut (long tokens that merge under the cut
      count as the merged key).  A word twice on a line counts twice.
    - How the lines were found changes nothing: mode, window, exclusion, prefix, pattern, fuzzy
      and regex terms and ``ignore_case`` select lines only.  Keys are the index's own bytes, so
      ``To`` and ``to`` are two words under ``ignore_case`` too; the query's words count like any.
    - Per query: ``words`` = the words with a count above 0, ``tokens`` = the sum of the counts,
      and the first ``min(K, words)`` words by (count descending, key ascending in unsigned-byte
      order) -- ``top``'s order -- each as ``(key, count)``.  No word with count 0 is returned; a
      query without a returned line has ``(0, 0, [])``.
"""


def tally(entries, postings, lines, k: int):
    """One query's tally over an index (``TALLY_RULES``): ``(words, tokens, top)`` for the
    returned ``lines`` (global numbers, any order, each once).  The index is turned round --
    per line the keys of its postings -- and the returned lines' keys are counted."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TALLY_MAX_K:
        raise ValueError("tally takes 1 <= K <= %d, not %r" % (TALLY_MAX_K, k))
    on_line = {}
    for key, val, count in entries:
        for l in postings[val:val + count]:
            on_line.setdefault(l, []).append(key)
    counts = {}
    for l in lines:
        for key in on_line.get(l, ()):
            counts[key] = counts.get(key, 0) + 1
    ordered = sorted(counts.items(), key=lambda kc: (-kc[1], kc[0]))
    return len(counts), sum(counts.values()), ordered[:k]


def format_tally(words: int, tokens: int, top) -> bytes:
    """One query's tally lines in the CLI's ``--search ... --tally K`` output, which stand under
    its ``print query:`` line and its shown lines."""
    return b"  words: %d \t tokens: %d\n" % (words, tokens) + b"".join(
        b"  word: %s \t count: %d\n" % (key, c) for key, c in top)


def _tally_lines(tallies, n):
    if tallies is None:
        return [b""] * n
    if len(tallies) != n:
        raise ValueError("tallies takes one (words, tokens, top) per query")
    return [format_tally(*t) for t in tallies]


def _file_lines(by_file, lines, scores=None, count=False):
    """The CLI's ``--by-file`` lines of one query: per file of its lines, ids ascending,
    ``  file: <path> \t hits: <n> \t lines: <local> ...`` (ranked: ``top:`` and
    ``<local>:<score>`` in rank order; ``count``: the line ends behind its hits).  ``by_file``
    is ``(table, paths)``, ``paths[id]`` the file's path."""
    if by_file is None:
        return b""
    table, paths = by_file
    ids, local, hits = globals()["by_file"](table, lines)
    out = b""
    for i, n in hits:
        path = paths[i] if isinstance(paths[i], bytes) else paths[i].encode()
        out += b"  file: %s \t hits: %d" % (path, n)
        if not count:
            out += b" \t top:" if scores is not None else b" \t lines:"
            for j, l in enumerate(local):
                if ids[j] == i:
                    out += b" %d" % l + (b":%d" % scores[j] if scores is not None else b"")
        out += b"\n"
    return out


def format_search(queries, answers, *, exclude=None, tallies=None, by_file=None,
                  count=False) -> bytes:
    """The CLI's ``--search`` result lines: one per query, ``queries[i]`` its terms and
    ``answers[i]`` its lines (every line number after one space; none after "lines:" when
    the query has no hit).

    ``exclude``: one entry per query, ``None`` or its exclusion terms; a query with exclusion
    terms prints `` \t not: <terms joined by one space>`` between its text and ``hits:``
    (terms as they were asked: a prefix term with its star).
    ``tallies``: one ``tally`` answer per query, printed under its line (``format_tally``).
    ``by_file=(table, paths)``: the CLI's ``--by-file`` lines under each query's line and above
    its tally lines (``_file_lines``); ``count`` beside it: ``--count`` -- the query's line ends
    behind its hits with `` \t files: <f>``, the file lines behind theirs."""
    if count:
        return b"".join(
            b"print query: %s \t hits: %d \t files: %d\n"
            % (q, len(a), len(globals()["by_file"](by_file[0], a)[2])) +
            _file_lines(by_file, a, count=True)
            for q, a in zip(_query_text(queries, exclude), answers))
    return b"".join(
        b"print query: %s \t hits: %d \t lines:%s\n"
        % (q, len(a), b"".join(b" %d" % l for l in a)) + _file_lines(by_file, a) + t
        for q, a, t in zip(_query_text(queries, exclude), answers,
                           _tally_lines(tallies, len(queries))))


RANK_MAX_EMITS = 65536


def rank(entries, postings, lines, terms, k: int, max_key: int = 29, *,
         wildcard: bool = False, delims: bytes = DEFAULT_DELIMS, exclude=None,
         glob: bool = False, ignore_case: bool = False, fuzzy: bool = False, regex: bool = False, emits=None,
         files=None, table=None):
    """The ranked answer of one query: ``(top, matches)``.

    ``files`` / ``table``: the query's file set (``CORPUS_RULES``).  The matching set is
    ``lines`` (before or after the set was applied) intersected with the set's lines; N and the
    counts, and so every score, stay those of the whole index.

    ``lines`` is the query's matching set, as ``search`` or ``phrase`` answered it; ranking
    never changes which lines match, only their order and how many are returned.  N is
    ``len(postings)``.  The distinct present terms are the ``terms``, each cut to
    ``max_key`` bytes, a repeated cut key counted once and an absent word left out.  A
    term's weight is ``bit_length(N // c)`` with ``c`` its word's count (a rarer word weighs
    more); ``tf`` is how often the line occurs in the term's postings list; a line's score
    is the sum of ``weight * tf`` over the distinct present terms.  ``top`` is the first
    ``min(k, matches)`` matching lines in the order (score descending, line ascending) as
    ``(line, score)`` pairs, ``matches`` is ``len(lines)``.  ``k >= 1``.

    ``wildcard=True``: a term may be a prefix term (``prefix_terms``).  Its ``c`` is its
    merged count (the sum of its words' counts; the weight is still ``bit_length(N // c)``)
    and its ``tf`` the line's multiplicity in its merged list.  Every present term has a
    key range, the set of its words; prefix ranges and single words form a laminar family:
    two ranges are nested or disjoint.  A present term whose range lies inside the range of
    another present term of the query contributes nothing to the score; of equal ranges the
    first occurrence counts (for plain terms: a repeated key counts once).

    ``exclude``: the query's exclusion terms (``EXCLUDE_RULES``).  The matching set is
    ``lines`` minus the excluded lines (``lines`` may be the answer before or after the
    exclusion) and ``matches`` counts it; the exclusion terms take no part in the score, in
    the distinct present terms or in the nesting rule.

    ``glob`` / ``ignore_case`` (``PATTERN_RULES``): a pattern term scores as a prefix term
    does, once per distinct pattern, outside the nesting rule.  ``emits`` (the job's
    emits_per_line), when given, is held against the limit of a ranked search: RANK_MAX_EMITS,
    or an eighth of it for a query with a pattern term (``ValueError``)."""
    if k < 1:
        raise ValueError("rank takes k >= 1")
    lines = in_files(table, lines, files)
    if emits is not None:
        pat = any(t.scattered for t in query_terms(
            list(terms) + list(exclude or []), wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex))
        if emits > (RANK_MAX_EMITS // MAX_SEARCH_TERMS if pat else RANK_MAX_EMITS):
            raise ValueError("a ranked search takes emits_per_line <= %d"
                             % (RANK_MAX_EMITS // MAX_SEARCH_TERMS if pat else RANK_MAX_EMITS))
    if exclude is not None:
        exclude = _check_exclude(list(terms), exclude)
        gone, _counts = _excluded_by_index(entries, postings, exclude, wildcard, delims,
                                           max_key, glob, ignore_case, fuzzy, regex)
        return rank(entries, postings, [l for l in lines if l not in gone], terms, k,
                    max_key, wildcard=wildcard, delims=delims, glob=glob,
                    ignore_case=ignore_case, fuzzy=fuzzy, regex=regex)
    if wildcard or glob or ignore_case or fuzzy or regex:
        n = len(postings)
        want = query_terms(terms, wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex)
        ranges = [set(_qt_words(entries, t)) for t in want]
        lists = []
        for j, rj in enumerate(ranges):
            if not rj:  # absent
                continue
            if want[j].scattered:  # once per distinct pattern; no nesting rule
                if any(want[i].scattered and want[i].ident == want[j].ident
                       for i in range(j)):
                    continue
            elif any(ri and i != j and not want[i].scattered and rj <= ri and
                     (rj != ri or i < j) for i, ri in enumerate(ranges)):
                continue
            merged = _term_list(entries, postings, sorted(rj))
            tf = {}
            for line in merged:
                tf[line] = tf.get(line, 0) + 1
            lists.append(((n // len(merged)).bit_length(), tf))
        scored = [(sum(w * tf.get(line, 0) for w, tf in lists), line) for line in lines]
        scored.sort(key=lambda sl: (-sl[0], sl[1]))
        return [(line, score) for score, line in scored[:k]], len(lines)
    n = len(postings)
    by_key = {key: (v, c) for key, v, c in entries}
    lists = []
    seen = set()
    for t in terms:
        key = t[:max_key]
        if key in seen or key not in by_key:
            continue
        seen.add(key)
        v, c = by_key[key]
        lists.append(((n // c).bit_length(), list(postings[v:v + c])))
    scored = [(sum(w * l.count(line) for w, l in lists), line) for line in lines]
    scored.sort(key=lambda sl: (-sl[0], sl[1]))
    return [(line, score) for score, line in scored[:k]], len(lines)


def format_ranked(queries, tops, matches, *, exclude=None, tallies=None, by_file=None) -> bytes:
    """The CLI's ``--search ... --rank K`` result lines: one per query, ``queries[i]`` its
    terms, ``tops[i]`` its ``(line, score)`` pairs and ``matches[i]`` its number of matching
    lines (nothing after "top:" when nothing matched).  ``exclude`` and ``tallies`` as
    ``format_search`` takes them; ``by_file=(table, paths)`` too, over the winners."""
    return b"".join(
        b"print query: %s \t hits: %d \t top:%s\n"
        % (q, m, b"".join(b" %d:%d" % (l, s) for l, s in t)) +
        _file_lines(by_file, [l for l, _s in t], [s for _l, s in t]) + ta
        for q, t, m, ta in zip(_query_text(queries, exclude), tops, matches,
                               _tally_lines(tallies, len(queries))))


SHOW_MAX_BYTES = 65536

SHOW_RULES = """
    Show (``show=N``): the returned lines' text and match spans.

    - ``N`` is an integer with 1 <= N <= 65536 (``ValueError`` otherwise).  Every returned line
      of a query, in result order (unranked ascending; ranked the winners in rank order), is
      one entry; the same line returned for two queries is two entries.
    - text: the line's bytes from its start to its end -- the newline, the end of the input or
      a NUL, where the tokeniser stops -- cut to the first ``N`` bytes.  ``cut`` counts the
      entries whose line was longer than ``N``.
    - spans: one ``(start, len, mask)`` for every emitted token of the line (one of its first
      ``emits`` tokens) that matches at least one of the query's own terms, in token order.
      ``start`` is the byte offset from the line's start, ``len`` the token's full length up to
      the next delimiter or the line's end (cut neither to ``max_key`` nor to ``N``), ``mask``
      bit ``j`` is set when the token matches term ``j``: the token's key, cut to ``max_key``,
      equals a plain term, starts with a prefix term's bytes, or is matched by a pattern term,
      with ``ignore_case`` folding ASCII letters.  A repeated term sets its own bit too.
    - Exclusion terms never produce a span, a token past the emit cap produces nothing, and the
      rule is the same in every mode: in a phrase or near query every token that matches a term
      is a span, not only those of an occurrence or a window.
"""


def line_tokens(line: bytes, delims: bytes = DEFAULT_DELIMS, emits: int = 20):
    """``(start, token)`` of the first ``emits`` tokens of one line, uncut; a NUL ends them."""
    dset = set(delims)
    out, at = [], None
    for i, c in enumerate(line + b"\0"):
        if c == 0 or c in dset:
            if at is not None:
                out.append((at, line[at:i]))
                at = None
            if c == 0:
                break
        elif at is None:
            at = i
    return out[:emits]


def show(text: bytes, lines, terms, n: int, delims: bytes = DEFAULT_DELIMS, emits: int = 20,
         max_key: int = 29, first_line: int = 0, *, wildcard: bool = False, glob: bool = False,
         ignore_case: bool = False, fuzzy: bool = False, regex: bool = False):
    """What ``show=n`` adds to one query's answer ``lines`` (global numbers, in result order):
    ``(texts, spans, cut)`` -- per entry the shown bytes and the ``(start, len, mask)`` list,
    and the number of entries whose line was longer than ``n`` (``SHOW_RULES``).  ``terms`` are
    the query's own terms, without its exclusion terms."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= SHOW_MAX_BYTES:
        raise ValueError("show takes 1 <= N <= %d, not %r" % (SHOW_MAX_BYTES, n))
    if len(text) >= 1 << 32:
        raise ValueError("show takes a text of less than 2^32 bytes")
    want = query_terms(list(terms), wildcard, glob, ignore_case, delims, max_key,
                       fuzzy=fuzzy, regex=regex)
    all_lines = split_lines(text)
    texts, spans, cut = [], [], 0
    for l in lines:
        line = all_lines[l - first_line].split(b"\0", 1)[0]
        cut += len(line) > n
        texts.append(line[:n])
        one = []
        for start, tok in line_tokens(line, delims, emits):
            mask = sum(1 << j for j, term in enumerate(want) if term.fits(tok[:max_key]))
            if mask:
                one.append((start, len(tok), mask))
        spans.append(one)
    return texts, spans, cut


def format_show(first: bytes, lines, texts, spans=None, mark: bool = False) -> bytes:
    """One query's part of the CLI's ``--search ... --show N`` output: ``first``, its
    ``print query:`` line (``format_search`` / ``format_ranked`` of the query alone), then per
    entry two spaces, the global line number, ``: `` and the shown bytes.  ``mark``: the part of
    every span that lies inside the shown bytes stands between ``>>`` and ``<<``."""
    out = [first]
    for i, (l, t) in enumerate(zip(lines, texts)):
        if mark:
            parts, done = [], 0
            for start, ln, _mask in spans[i]:
                if start >= len(t):
                    break
                end = min(start + ln, len(t))
                parts += [t[done:start], b">>", t[start:end], b"<<"]
                done = end
            t = b"".join(parts) + t[done:]
        out.append(b"  %d: %s\n" % (l, t))
    return b"".join(out)


def format_gpu(entries) -> bytes:
    """The reference GPU build's result lines (main.cu:132)."""
    return b"".join(b"print key: %s \t val: %d \t count: %d\n" % (k, v, c) for k, v, c in entries)


def format_cpu(entries) -> bytes:
    """The reference CPU build's result lines (main.cu:286)."""
    return b"".join(b"print key: %s \t value: %d\n" % (k, c) for k, _v, c in entries)


def window(text: bytes, line_start: int = -1, line_end: int = -1, ref_compat: bool = False) -> bytes:
    """Lines [line_start, line_end) of text, with the reference's last-line quirk if asked."""
    lines = split_lines(text)
    total = len(lines)
    if line_start < 0:
        first, last = 0, total - (1 if ref_compat and total else 0)
    else:
        first = min(line_start, total)
        last = total if line_end < 0 else min(max(line_end, line_start), total)
        if ref_compat and 0 <= line_end and line_end >= total and last > first:
            last -= 1
    sel = lines[first:last]
    return b"".join(l + b"\n" for l in sel)
