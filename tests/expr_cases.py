"""What tests/test_expr.py and tests/test_expr_gpu.py share: the oracle's answer of a batch
with ``expr`` queries (engine.hpp "boolean expressions", ``oracle.EXPR_RULES`` -- the oracle
parses the expression itself and evaluates the tree per line with set membership, no truth
table), its exact comparison with a ``SearchResult``, ranked or not and with ``show``, the
256-line text on which every mask of eight words occurs once, and the seeded generator of
random expressions."""
import functools
import random

from locust_amd.utils import oracle
from tests.glob_cases import same  # noqa: F401  (the comparison is every search test's)

WORDS = [b"w%d" % t for t in range(8)]


@functools.lru_cache(maxsize=None)
def mask_text(repeat=1):
    """256 lines: line i holds word w_t exactly when bit t of i is set (line 0 holds only a
    filler), so every mask of the eight words occurs once.  ``repeat`` > 1 writes every word
    that many times (adjacent duplicates in the lists, tf > 1)."""
    return b"".join(b" ".join([b"zz"] + [w for t, w in enumerate(WORDS) if i >> t & 1] * repeat)
                    + b"\n" for i in range(256))


def random_tree(rng, depth, nterms):
    if depth == 0 or rng.random() < 0.25:
        return rng.randrange(nterms)
    op = rng.choice(("and", "and", "or", "or", "not", "side"))
    if op == "not":
        return ("not", random_tree(rng, depth - 1, nterms))
    return (op, random_tree(rng, depth - 1, nterms), random_tree(rng, depth - 1, nterms))


def tree_text(tree, words, rng):
    """The tree as an expression: every inner node in parentheses, glued to the words or not;
    "side": two operands side by side (the implicit AND)."""
    if isinstance(tree, int):
        return words[tree]
    open_, close = rng.choice(((b"( ", b" )"), (b"(", b")"), (b" (  ", b"\t) ")))
    if tree[0] == "not":
        return b"NOT " + open_ + tree_text(tree[1], words, rng) + close
    op = {"and": b" AND ", "or": b" OR ", "side": b" "}[tree[0]]
    return open_ + tree_text(tree[1], words, rng) + op + tree_text(tree[2], words, rng) + close


def random_exprs(seed, count, words=WORDS, depth=4):
    """``count`` seeded random expressions of depth <= ``depth`` over up to ``len(words)``
    terms; about a third hold for the empty mask and must be refused."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(1, len(words))
        out.append(tree_text(random_tree(rng, rng.randint(1, depth), n), words, rng))
    return out


def refused(expr, **gkw):
    """Does the oracle refuse the expression?"""
    gkw = {k: v for k, v in gkw.items() if k in ("wildcard", "glob", "fuzzy")}
    try:
        oracle.expr_parse(expr, **gkw)
    except ValueError:
        return True
    return False


def want(text, exprs, k=None, first_line=0, **gkw):
    """[(answer, matches, counts)] of every ``expr`` query by the oracle, as
    ``glob_cases.want``'s; gkw: wildcard, glob, fuzzy, ignore_case."""
    ent, post = oracle.index(text, first_line=first_line)
    out = []
    for e in exprs:
        lines, counts, terms = oracle.expr_search(ent, post, e, **gkw)
        if k is None:
            out.append((lines, len(lines), counts))
        else:
            top, matches = oracle.rank(ent, post, lines, terms, k, **gkw)
            out.append((top, matches, counts))
    return out


def terms_of(exprs, **gkw):
    gkw = {k: v for k, v in gkw.items() if k in ("wildcard", "glob", "fuzzy")}
    return [oracle.expr_parse(e, **gkw)[1] for e in exprs]


def want_show(text, exprs, n, k=None, first_line=0, **gkw):
    """``(base, shown)`` as ``show_cases.want_show``: spans for every token that matches one of
    the expression's terms, bit t for term t."""
    base = want(text, exprs, k, first_line, **gkw)
    shown = []
    for terms, (answer, _m, _c) in zip(terms_of(exprs, **gkw), base):
        lines = answer if k is None else [l for l, _s in answer]
        shown.append(oracle.show(text, lines, terms, n, first_line=first_line, **gkw))
    return base, shown


def walked(text, exprs, first_line=0, **gkw):
    """``SearchResult.walked`` of a device batch made only of these ``expr`` queries."""
    ent, post = oracle.index(text, first_line=first_line)
    return sum(oracle.expr_walked(ent, post, e, **gkw) for e in exprs)


def merged(text, exprs, first_line=0, **gkw):
    """``SearchResult.merged`` of the batch on the device: the existing rule over the terms."""
    ent, _post = oracle.index(text, first_line=first_line)
    mkw = {k: gkw.get(k, False) for k in ("wildcard", "glob", "fuzzy", "ignore_case")}
    return oracle.merged_elements(ent, terms_of(exprs, **gkw), **mkw)


def formatted(exprs, expect, k=None):
    """The CLI's result lines: the expression, blanks collapsed, where other modes print terms."""
    queries = [[oracle.expr_text(e)] for e in exprs]
    if k is None:
        return oracle.format_search(queries, [a for a, _m, _c in expect])
    return oracle.format_ranked(queries, [a for a, _m, _c in expect], [m for _a, m, _c in expect])


def formatted_show(exprs, expect, k=None, mark=False):
    base, shown = expect
    out = []
    for e, one, (texts, spans, _cut) in zip(exprs, base, shown):
        lines = one[0] if k is None else [l for l, _s in one[0]]
        out.append(oracle.format_show(formatted([e], [one], k), lines, texts, spans, mark))
    return b"".join(out)
