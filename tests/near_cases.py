"""The cases tests/test_near.py (CPU) and tests/test_near_gpu.py share: the hand-written
text with one line per rule of the `near` semantics, the oracle's answers for a mixed batch,
the comparison of a ``SearchResult`` with them, and the fuzz generator."""
import functools
import random

from locust_amd.utils import oracle

W_MAX = (1 << 32) - 1

TEXT = (b"to be or not to be\n"        # 0: neighbours, twice
        b"be x to\n"                   # 1: the other order, one token between: W = 3
        b"to x y be\n"                 # 2: two tokens between: W = 4
        b"to\n"                        # 3: | the two words on two lines: never
        b"be\n"                        # 4: |
        b"bye now\n"                   # 5: one bye
        b"Hamlet speaks\n"             # 6
        b"Ham and Hamlet\n"            # 7
        b"to\0 be\n"                   # 8: a NUL ends the line's tokens
        b"a b c d e to f g h be\n")    # 9: tokens 5 and 9: W = 5

# (terms, W, wildcard, the lines by hand)
BY_HAND = [
    ([b"to", b"be"], 1, False, []),             # one token cannot be both words
    ([b"to", b"be"], 2, False, [0]),
    ([b"to", b"be"], 3, False, [0, 1]),         # distance W - 1 matches ...
    ([b"to", b"be"], 4, False, [0, 1, 2]),
    ([b"to", b"be"], 5, False, [0, 1, 2, 9]),
    ([b"be", b"to"], 2, False, [0]),            # both orders
    ([b"be", b"to"], 4, False, [0, 1, 2]),      # ... W does not: line 9 needs 5
    ([b"be", b"to"], 20, False, [0, 1, 2, 9]),  # W >= the emit cap: `all`
    ([b"to", b"be"], W_MAX, False, [0, 1, 2, 9]),
    ([b"bye", b"bye"], 1, False, [5]),          # a repeated term changes nothing
    ([b"now", b"bye", b"bye"], 2, False, [5]),
    ([b"Ham*", b"Hamlet"], 1, True, [6, 7]),    # one token for two terms
    ([b"Ham*", b"Hamlet"], 1, False, []),       # `Ham*` is a literal token without wildcard
    ([b"Ham", b"Hamlet"], 2, False, []),
    ([b"Ham", b"Hamlet"], 3, False, [7]),
    ([b"Ham*", b"and"], 2, True, [7]),
    ([b"to"], 1, False, [0, 1, 2, 3, 8, 9]),    # one term: `all`
    ([b"to", b"gone"], 9, False, []),           # an absent term
    ([b"e", b"f", b"to"], 3, False, [9]),
    ([b"e", b"f", b"to", b"be"], 5, False, []),
    ([b"e", b"f", b"to", b"be"], 6, False, [9]),
]


@functools.lru_cache(maxsize=16)
def _index(text, first_line, okw):
    return oracle.index(text, first_line=first_line, **dict(okw))


def want(text, queries, modes, within, first_line=0, wildcard=False, **okw):
    """[(lines, counts)] of every query by the oracle, each distinct query computed once:
    ``near`` and ``phrase`` from the text, the other modes from the index."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if within is None or isinstance(within, int):
        within = [within if m == "near" else None for m in modes]
    skw = {k: v for k, v in okw.items() if k in ("delims", "max_key")}
    memo, out = {}, []
    for q, m, w in zip(queries, modes, within):
        key = (tuple(q), m, w)
        if key not in memo:
            if m == "near":
                memo[key] = oracle.near(text, q, w, first_line=first_line, wildcard=wildcard,
                                        **okw)
            elif m == "phrase":
                memo[key] = oracle.phrase(text, q, first_line=first_line, wildcard=wildcard,
                                          **okw)
            else:
                ent, post = _index(text, first_line, tuple(sorted(okw.items())))
                memo[key] = oracle.search(ent, post, q, m, wildcard=wildcard, **skw)
        out.append(memo[key])
    return out


def same(got, expect):
    assert got.queries == len(expect)
    assert got.hits() == [len(l) for l, _c in expect]
    for i, (lines, counts) in enumerate(expect):
        assert got.lines(i) == lines, i
        assert got.term_counts(i) == counts, i


def same_ranked(got, text, queries, expect, k, first_line=0, wildcard=False, **okw):
    """A ranked answer against ``oracle.rank`` over the oracle's matching lines."""
    ent, post = _index(text, first_line, tuple(sorted(okw.items())))
    rkw = {k_: v for k_, v in okw.items() if k_ in ("delims", "max_key")}
    assert got.rank_k == k and got.queries == len(expect)
    for i, (lines, counts) in enumerate(expect):
        top, matches = oracle.rank(ent, post, lines, queries[i], k, wildcard=wildcard, **rkw)
        assert got.matches()[i] == matches == len(lines), i
        assert got.lines(i) == [l for l, _s in top], i
        assert got.scores(i) == [s for _l, s in top], i
        assert got.term_counts(i) == counts, i


def fuzz_case(seed, nlines=300, nvocab=50, nqueries=200, wildcard=False):
    """``(text, queries, modes, within)``: 50 words of vocabulary, some of them long stems
    that merge under truncation, 0-12 tokens per line; most queries pick their terms, in any
    order, from a short stretch of one of the text's own lines, so that the window decides.
    W is drawn from 1..8, now and then 2^32 - 1.  ``wildcard``: every fourth term becomes a
    prefix term of its first bytes."""
    rng = random.Random(seed)
    stem = b"q" * 29
    vocab = [bytes(rng.choice(b"abcdeXYZ") for _ in range(rng.randrange(1, 7)))
             for _ in range(nvocab - 4)]
    vocab += [stem, stem + b"A", stem + b"B" * 11, b"r" * 28 + b"s"]
    seps = [b" ", b" ", b", ", b"  ", b"-", b";\t"]
    lines = []
    for _ in range(nlines):
        words = [rng.choice(vocab) for _ in range(rng.randrange(0, 13))]
        lines.append(b"".join(w + rng.choice(seps) for w in words))
    text = b"\n".join(lines) + b"\n"
    extra = [b"absent", stem + b"C", b"q" * 40, b"q" * 28]
    queries, modes, within = [], [], []
    for _ in range(nqueries):
        toks = oracle.tokenize(rng.choice(lines), emits=99, max_key=99)[0]
        n = rng.randrange(1, 9)
        if len(toks) >= 2 and rng.random() < 0.75:
            o = rng.randrange(len(toks) - 1)
            stretch = toks[o:o + rng.randrange(2, 9)]
            q = [rng.choice(stretch) for _ in range(min(n, len(stretch) + 1))]
            if rng.random() < 0.2:
                q[rng.randrange(len(q))] = rng.choice(vocab + extra)
        else:
            q = [rng.choice(vocab + extra) for _ in range(n)]
        if wildcard:
            q = [t[:rng.randrange(1, len(t) + 1)] + b"*" if rng.random() < 0.25 else t for t in q]
        m = rng.choice(["near"] * 5 + ["all", "any", "phrase"])
        queries.append(q)
        modes.append(m)
        within.append((W_MAX if rng.random() < 0.05 else rng.randrange(1, 9))
                      if m == "near" else None)
    return text, queries, modes, within
