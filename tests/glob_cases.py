"""What tests/test_glob.py and tests/test_glob_gpu.py share: the oracle's answer of a batch
with pattern terms (``glob`` and ``ignore_case``, engine.hpp "pattern terms") and its exact
comparison with a ``SearchResult``, ranked or not."""
import random
import re

from locust_amd.utils import oracle


def want(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=True,
         ignore_case=False, **okw):
    """[(answer, matches, counts)] of every query by the oracle; ``answer`` is the ascending
    lines (``k`` None) or the ``(line, score)`` pairs of the best ``k``.  ``within``: one
    window for every near query, or a list; ``exclude``: None or one entry per query."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if not isinstance(within, list):
        within = [within] * len(queries)
    exclude = exclude or [None] * len(queries)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    gkw = {"glob": glob, "ignore_case": ignore_case}
    out = []
    for q, m, w, x in zip(queries, modes, within, exclude):
        if m == "phrase":
            lines, counts = oracle.phrase(text, q, first_line=first_line, exclude=x, **gkw, **okw)
        elif m == "near":
            lines, counts = oracle.near(text, q, w, first_line=first_line, exclude=x, **gkw, **okw)
        else:
            lines, counts = oracle.search(ent, post, q, m, exclude=x, **gkw, **skw)
        if k is None:
            out.append((lines, len(lines), counts))
        else:
            top, matches = oracle.rank(ent, post, lines, q, k, exclude=x, **gkw, **skw)
            out.append((top, matches, counts))
    return out


def merged(text, queries, first_line=0, exclude=None, glob=True, ignore_case=False, **okw):
    """``SearchResult.merged`` of the batch on the device, by the oracle."""
    ent, _post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    return oracle.merged_elements(ent, queries, exclude=exclude, glob=glob,
                                  ignore_case=ignore_case, wildcard=False, **skw)


def same(got, expect, k=None):
    assert got.queries == len(expect) and got.rank_k == (k or 0)
    assert got.matches() == [m for _a, m, _c in expect]
    assert got.hits() == [m if k is None else min(k, m) for _a, m, _c in expect]
    for i, (answer, _m, counts) in enumerate(expect):
        if k is None:
            assert got.lines(i) == answer and got.scores(i) == [], i
        else:
            assert list(zip(got.lines(i), got.scores(i))) == answer, i
        assert got.term_counts(i) == counts, i


def formatted(queries, expect, k=None, exclude=None, glob=True):
    """The CLI's result lines of the batch, the queries as asked (``glob``: runs of stars
    collapsed, as the terms are read)."""
    if glob:
        star = lambda terms: [re.sub(rb"\*+", b"*", t) for t in terms]
        queries = [star(q) for q in queries]
        exclude = [star(x) if x else x for x in exclude] if exclude else exclude
    if k is None:
        return oracle.format_search(queries, [a for a, _m, _c in expect], exclude=exclude)
    return oracle.format_ranked(queries, [a for a, _m, _c in expect],
                                [m for _a, m, _c in expect], exclude=exclude)


# The matcher's edges: (pattern, keys it must be tried on).  Every key is one word of the text
# edge_text() builds, one per line; the oracle says which of them a pattern matches.
EDGE_KEYS = [
    b"ab", b"aab", b"abab", b"ababab", b"a", b"b", b"abc", b"ba", b"xaby", b"abx", b"xab",
    b"\x80", b"\xff", b"a\x80b", b"a\xffb", b"\xff\xff", b"@a[", b"`a{", b"@A[", b"`A{",
    b"AB", b"Ab", b"aB", b"\xc3\xa9", b"\xc3\x89",
] + [b"k" * n for n in (7, 8, 9, 15, 16, 17, 24, 29)] \
  + [b"k" * (n - 1) + b"z" for n in (7, 8, 9, 15, 16, 17, 24, 29)] \
  + [b"K" * 28 + b"z"]
EDGE_PATTERNS = [
    b"*ab", b"ab*c", b"a*b", b"*a*b*", b"ab*?", b"?b", b"a?", b"ab?", b"?", b"??", b"???",
    b"*ab*ab", b"*ab*", b"a*", b"*b", b"a**b", b"?*", b"*?", b"*?*", b"x*y", b"*\x80*",
    b"\xff*\xff", b"?\xff?", b"a?b", b"@a[", b"`a{", b"@?[", b"`*{", b"AB", b"a*B", b"\xc3?", b"q?", b"ab?ab?ab",
] + [b"k" * (n - 1) + b"?" for n in (7, 8, 9, 15, 16, 17, 24, 29)] \
  + [b"*" + b"k" * (n - 2) + b"z" for n in (7, 8, 9, 15, 16, 17, 24, 29)] \
  + [b"k" * 8 + b"*" + b"k" * 8 + b"?", b"?" * 29, b"k" * 28 + b"*", b"*" + b"k" * 28,
     b"k*k*k*k*z", b"*k*k*k*kz"]


def edge_text():
    return b"".join(k + b" pad\n" for k in EDGE_KEYS)


def fuzz_case(seed, nlines=120, nqueries=60):
    """A text of `nlines` lines over a small alphabet in both cases (so that patterns hit and
    folding matters; words of 29, 30 and 35 bytes that merge, keys with 0x80 and 0xff bytes)
    and `nqueries` random queries mixing plain, prefix and pattern terms in all four modes,
    some with exclusion terms: (text, queries, modes, within, exclude)."""
    rng = random.Random(seed)
    alphabet = b"abAB" if seed % 2 else b"abcA"
    vocab = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 6))) for _ in range(50)]
    vocab += [b"a" * 29, b"a" * 29 + b"X", b"A" * 35, b"b\xff", b"b\x80a", b"b", b"@a[", b"`A{"]
    lines = [b" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 10)))
             for _ in range(nlines)]
    text = b"\n".join(lines) + b"\n"

    def term():
        w = bytearray(rng.choice(vocab + [b"zz", b"ab", b"BA"]))[:rng.randrange(1, 8)]
        r = rng.random()
        if r < 0.25:
            return bytes(w)
        if r < 0.4:
            return bytes(w) + b"*"
        for _ in range(rng.randrange(1, 3)):  # a pattern: stars and question marks anywhere
            at = rng.randrange(len(w) + 1)
            if rng.random() < 0.5:
                w[at:at] = b"*"
            elif at < len(w):
                w[at] = 0x3F
            else:
                w[at:at] = b"?"
        return bytes(w)

    queries, modes, within, exclude = [], [], [], []
    for _ in range(nqueries):
        mode = rng.choice(["all", "any", "phrase", "near"])
        q = [term() for _t in range(rng.randrange(1, 4 if mode in ("phrase", "near") else 7))]
        if rng.random() < 0.3:
            q[rng.randrange(len(q))] = q[0]  # a repeated term
        x = [term() for _t in range(rng.randrange(1, 3))] if rng.random() < 0.3 else None
        queries.append(q)
        modes.append(mode)
        within.append(rng.randrange(1, 5) if mode == "near" else None)
        exclude.append(x)
    return text, queries, modes, within, exclude
