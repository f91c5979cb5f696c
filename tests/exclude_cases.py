"""The cases tests/test_exclude.py (CPU) and tests/test_exclude_gpu.py share: the hand-written
text with one line per rule of the exclusion semantics (``oracle.EXCLUDE_RULES``), the
oracle's answers for a mixed batch, the comparison of a ``SearchResult`` with them, and the
fuzz generator."""
import functools
import random

from locust_amd.utils import oracle

W_MAX = (1 << 32) - 1

TEXT = (b"alpha beta delta\n"          # 0: the phrase, no gamma
        b"alpha beta gamma\n"          # 1: the phrase, and gamma behind it
        b"beta alpha gamma gamma\n"    # 2: both words, gamma twice
        b"alpha x beta\n"              # 3: both words, one token between
        b"gamma\n"                     # 4: the exclusion word alone
        b"alpha\n"                     # 5
        b"bye bye now\n"               # 6: a repeated word
        b"bye now x\n"                 # 7
        b"ab abc abd\n"                # 8: three words of the range ab*
        b"abc alpha\n"                 # 9
        b"ab alpha beta\n"             # 10
        b"Ham Hamlet alpha\n"          # 11
        b"Hamlet\n"                    # 12
        b"Ham alpha\n"                 # 13
        b"alpha\0 gamma beta\n"        # 14: a NUL ends the line's tokens: no gamma, no beta
        b"gamma gamma gamma")          # 15: the last line, without its newline

# (terms, exclusion terms, mode, W, wildcard, the lines by hand)
BY_HAND = [
    ([b"alpha", b"beta"], [b"gamma"], "all", None, False, [0, 3, 10]),
    ([b"alpha", b"beta"], [], "all", None, False, [0, 1, 2, 3, 10]),
    ([b"alpha", b"beta"], [b"gamma"], "phrase", None, False, [0, 10]),
    ([b"alpha", b"beta"], [b"delta"], "phrase", None, False, [1, 10]),
    ([b"alpha", b"beta"], [b"gamma"], "near", 2, False, [0, 10]),
    ([b"beta", b"alpha"], [b"gamma"], "near", 3, False, [0, 3, 10]),
    ([b"beta", b"alpha"], [b"gamma"], "near", 20, False, [0, 3, 10]),   # W >= the cap: `all`
    ([b"alpha", b"beta"], [b"gamma"], "any", None, False, [0, 3, 5, 9, 10, 11, 13, 14]),
    # an absent exclusion term excludes nothing, and nothing goes dead
    ([b"alpha", b"beta"], [b"gone"], "all", None, False, [0, 1, 2, 3, 10]),
    ([b"alpha", b"beta"], [b"gone", b"gamma", b"away"], "all", None, False, [0, 3, 10]),
    # an absent positive term still empties `all`
    ([b"alpha", b"gone"], [b"gamma"], "all", None, False, []),
    ([b"alpha", b"gone"], [b"gamma"], "any", None, False, [0, 3, 5, 9, 10, 11, 13, 14]),
    # the union of several exclusion terms; a repeated one changes nothing
    ([b"alpha"], [b"gamma", b"beta"], "all", None, False, [5, 9, 11, 13, 14]),
    ([b"alpha"], [b"gamma", b"gamma", b"beta", b"gamma"], "all", None, False, [5, 9, 11, 13, 14]),
    # an exclusion term that repeats a positive term
    ([b"alpha", b"beta"], [b"alpha"], "all", None, False, []),
    ([b"alpha", b"beta"], [b"beta"], "phrase", None, False, []),
    ([b"alpha", b"beta"], [b"beta"], "near", 2, False, []),
    ([b"alpha", b"beta"], [b"beta"], "any", None, False, [5, 9, 11, 13, 14]),
    ([b"alpha"], [b"alpha"], "any", None, False, []),
    # the repetition rules are the positive terms' own
    ([b"bye", b"bye"], [b"x"], "phrase", None, False, [6]),
    ([b"bye", b"bye"], [b"x"], "all", None, False, [6]),
    ([b"bye", b"bye"], [b"x"], "near", 1, False, [6]),     # one distinct term: `all`
    ([b"bye", b"now"], [b"x"], "phrase", None, False, [6]),
    ([b"bye"], [b"bye"], "phrase", None, False, []),
    # the NUL: what stands behind it is not in the index, so it excludes nothing
    ([b"alpha"], [b"gamma", b"delta", b"x", b"ab*", b"Ham"], "all", None, False,
     [5, 9, 10, 14]),                                      # `ab*` is a literal token here
    # prefix exclusions: 0, 1 and 3 words
    ([b"alpha"], [b"zz*"], "all", None, True, [0, 1, 2, 3, 5, 9, 10, 11, 13, 14]),
    ([b"alpha"], [b"gam*"], "all", None, True, [0, 3, 5, 9, 10, 11, 13, 14]),
    ([b"alpha"], [b"ab*"], "all", None, True, [0, 1, 2, 3, 5, 11, 13, 14]),
    ([b"abc"], [b"ab*"], "all", None, True, []),           # the range holds the positive word
    ([b"ab*"], [b"abc"], "all", None, True, [10]),         # ... and the other way round
    ([b"ab*"], [b"ab*"], "any", None, True, []),
    ([b"Ham*"], [b"Hamlet"], "all", None, True, [13]),
    ([b"Ham*", b"alpha"], [b"Hamlet"], "phrase", None, True, [13]),
    ([b"Ham*", b"alpha"], [b"gamma"], "phrase", None, True, [11, 13]),
    ([b"Ham*", b"alpha"], [b"Haml*"], "near", 2, True, [13]),
    ([b"alpha", b"b*"], [b"g*", b"ab"], "all", None, True, [0, 3]),
]


@functools.lru_cache(maxsize=16)
def _index(text, first_line, okw):
    return oracle.index(text, first_line=first_line, **dict(okw))


def norm(exclude, n):
    """``exclude`` as one list per query."""
    if exclude is None:
        return [[] for _ in range(n)]
    assert len(exclude) == n
    return [list(x or []) for x in exclude]


def want(text, queries, modes, within=None, exclude=None, first_line=0, wildcard=False, **okw):
    """[(lines, counts)] of every query by the oracle, each distinct query computed once:
    ``near`` and ``phrase`` from the text, the other modes from the index.  A query without
    exclusion terms goes through the oracle's calls as they were before ``exclude=``."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if within is None or isinstance(within, int):
        within = [within if m == "near" else None for m in modes]
    exclude = norm(exclude, len(queries))
    skw = {k: v for k, v in okw.items() if k in ("delims", "max_key")}
    memo, out = {}, []
    for q, m, w, x in zip(queries, modes, within, exclude):
        key = (tuple(q), m, w, tuple(x))
        if key not in memo:
            xkw = {"exclude": x} if x else {}
            if m == "near":
                memo[key] = oracle.near(text, q, w, first_line=first_line, wildcard=wildcard,
                                        **okw, **xkw)
            elif m == "phrase":
                memo[key] = oracle.phrase(text, q, first_line=first_line, wildcard=wildcard,
                                          **okw, **xkw)
            else:
                ent, post = _index(text, first_line, tuple(sorted(okw.items())))
                memo[key] = oracle.search(ent, post, q, m, wildcard=wildcard, **skw, **xkw)
        out.append(memo[key])
    return out


def same(got, expect):
    assert got.queries == len(expect)
    assert got.hits() == [len(l) for l, _c in expect]
    for i, (lines, counts) in enumerate(expect):
        assert got.lines(i) == lines, i
        assert got.term_counts(i) == counts, i


def same_ranked(got, text, queries, exclude, expect, k, first_line=0, wildcard=False, **okw):
    """A ranked answer against ``oracle.rank`` over the oracle's matching lines (``expect``:
    the answers after exclusion)."""
    ent, post = _index(text, first_line, tuple(sorted(okw.items())))
    rkw = {k_: v for k_, v in okw.items() if k_ in ("delims", "max_key")}
    exclude = norm(exclude, len(queries))
    assert got.rank_k == k and got.queries == len(expect)
    for i, (lines, counts) in enumerate(expect):
        top, matches = oracle.rank(ent, post, lines, queries[i], k, wildcard=wildcard,
                                   exclude=exclude[i], **rkw)
        assert got.matches()[i] == matches == len(lines), i
        assert got.lines(i) == [l for l, _s in top], i
        assert got.scores(i) == [s for _l, s in top], i
        assert got.term_counts(i) == counts, i


@functools.lru_cache(maxsize=8)
def fuzz_case(seed, nlines=300, nvocab=28, nqueries=200, wildcard=False):
    """``(text, queries, modes, within, exclude)``: 28 words of vocabulary (short ones, so
    that prefixes cover several, and long stems that merge under truncation), 0-12 tokens per
    line, so a word stands on about a fifth of the lines.  A query's positive terms (1 to 4)
    mostly come from a short stretch of one of the text's own lines, so that most queries
    have an answer; two thirds of the queries get 1 to 4 exclusion terms from the vocabulary,
    now and then an absent word or one of the query's own terms.  ``wildcard``: every fourth
    term, of either kind, becomes a prefix term of its first bytes.

    Asserted here, on the oracle alone: of the queries with exclusion terms, at least a
    quarter answer something else than their positive terms alone, and at least a quarter
    still answer some line."""
    rng = random.Random(seed)
    stem = b"q" * 29
    vocab = [bytes(rng.choice(b"abcXY") for _ in range(rng.randrange(1, 5)))
             for _ in range(nvocab - 4)]
    vocab += [stem, stem + b"A", stem + b"B" * 11, b"r" * 28 + b"s"]
    seps = [b" ", b" ", b", ", b"  ", b"-", b";\t"]
    lines = []
    for _ in range(nlines):
        words = [rng.choice(vocab) for _ in range(rng.randrange(0, 13))]
        lines.append(b"".join(w + rng.choice(seps) for w in words))
    text = b"\n".join(lines) + b"\n"
    extra = [b"absent", stem + b"C", b"q" * 40, b"q" * 28]
    queries, modes, within, exclude = [], [], [], []

    def star(t):
        return t[:rng.randrange(1, len(t) + 1)] + b"*" if wildcard and rng.random() < 0.25 else t

    for _ in range(nqueries):
        toks = oracle.tokenize(rng.choice(lines), emits=99, max_key=99)[0]
        n = rng.randrange(1, 5)
        if len(toks) >= 2 and rng.random() < 0.8:
            o = rng.randrange(len(toks) - 1)
            stretch = toks[o:o + rng.randrange(2, 6)]
            q = [rng.choice(stretch) for _ in range(min(n, len(stretch)))]
        else:
            q = [rng.choice(vocab + extra) for _ in range(n)]
        x = []
        if rng.random() < 0.67:
            x = [rng.choice(vocab) for _ in range(rng.randrange(1, 5))]
            if rng.random() < 0.15:
                x[rng.randrange(len(x))] = rng.choice(extra + q)
        m = rng.choice(["all", "all", "any", "phrase", "phrase", "near", "near"])
        queries.append([star(t) for t in q])
        exclude.append([star(t) for t in x])
        modes.append(m)
        within.append((W_MAX if rng.random() < 0.05 else rng.randrange(1, 6))
                      if m == "near" else None)
    with_x = [i for i, x in enumerate(exclude) if x]
    after = want(text, queries, modes, within, exclude, wildcard=wildcard)
    before = want(text, queries, modes, within, None, wildcard=wildcard)
    differ = sum(after[i][0] != before[i][0] for i in with_x)
    alive = sum(bool(after[i][0]) for i in with_x)
    assert len(with_x) >= nqueries // 2, len(with_x)
    assert 4 * differ >= len(with_x) and 4 * alive >= len(with_x), (differ, alive, len(with_x))
    return text, queries, modes, within, exclude
