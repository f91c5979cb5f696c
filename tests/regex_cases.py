"""What tests/test_regex.py and tests/test_regex_gpu.py share: the oracle's answer of a batch with
regex terms (``regex``, engine.hpp "regex terms", ``oracle.REGEX_RULES`` -- the oracle parses the
source into a tree and tracks reachable offsets, no position automaton), alone or beside ``glob``,
``fuzzy``, ``wildcard`` and ``ignore_case``, its exact comparison with a ``SearchResult``, ranked
or not and with ``show``, the matcher's edge text, the issue's Hamlet table and the seeded
generator of random expressions."""
import functools
import random

from locust_amd.utils import oracle
from tests.glob_cases import same  # noqa: F401  (the comparison is every search test's)


def want(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=False,
         ignore_case=False, wildcard=False, fuzzy=False, regex=True, **okw):
    """[(answer, matches, counts)] of every query by the oracle, as ``glob_cases.want``; a query
    of mode ``"expr"`` is a one-element list, its expression."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if not isinstance(within, list):
        within = [within] * len(queries)
    exclude = exclude or [None] * len(queries)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    gkw = {"glob": glob, "ignore_case": ignore_case, "wildcard": wildcard, "fuzzy": fuzzy,
           "regex": regex}
    out = []
    for q, m, w, x in zip(queries, modes, within, exclude):
        terms = q
        if m == "expr":
            lines, counts, terms = oracle.expr_search(ent, post, q[0], **gkw, **skw)
        elif m == "phrase":
            lines, counts = oracle.phrase(text, q, first_line=first_line, exclude=x, **gkw, **okw)
        elif m == "near":
            lines, counts = oracle.near(text, q, w, first_line=first_line, exclude=x, **gkw, **okw)
        else:
            lines, counts = oracle.search(ent, post, q, m, exclude=x, **gkw, **skw)
        if k is None:
            out.append((lines, len(lines), counts))
        else:
            top, matches = oracle.rank(ent, post, lines, terms, k, exclude=x, **gkw, **skw)
            out.append((top, matches, counts))
    return out


def terms_of(queries, modes, **gkw):
    """Every query's terms: its own, or the distinct terms of its expression."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    pkw = {k: v for k, v in gkw.items() if k in ("wildcard", "glob", "fuzzy", "regex")}
    return [oracle.expr_parse(q[0], **pkw)[1] if m == "expr" else q
            for q, m in zip(queries, modes)]


def want_show(text, queries, modes, n, k=None, first_line=0, within=None, exclude=None,
              glob=False, ignore_case=False, wildcard=False, fuzzy=False, regex=True, **okw):
    """``(base, shown)`` as ``show_cases.want_show``: ``want``'s list, and per query ``(texts,
    spans, cut)`` of its returned lines by ``oracle.show``."""
    base = want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case, wildcard,
                fuzzy, regex, **okw)
    gkw = dict(glob=glob, wildcard=wildcard, fuzzy=fuzzy, regex=regex)
    shown = []
    for q, (answer, _m, _c) in zip(terms_of(queries, modes, **gkw), base):
        lines = answer if k is None else [l for l, _s in answer]
        shown.append(oracle.show(text, lines, q, n, first_line=first_line,
                                 ignore_case=ignore_case, **gkw, **okw))
    return base, shown


def merged(text, queries, modes="all", first_line=0, exclude=None, glob=False, ignore_case=False,
           wildcard=False, fuzzy=False, regex=True, **okw):
    """``SearchResult.merged`` of the batch on the device, by the oracle."""
    ent, _post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    gkw = dict(glob=glob, wildcard=wildcard, fuzzy=fuzzy, regex=regex)
    return oracle.merged_elements(ent, terms_of(queries, modes, **gkw), exclude=exclude,
                                  ignore_case=ignore_case, **gkw, **skw)


def formatted(queries, expect, k=None, exclude=None):
    """The CLI's result lines of the batch, the queries as asked: a regex term with its slashes."""
    if k is None:
        return oracle.format_search(queries, [a for a, _m, _c in expect], exclude=exclude)
    return oracle.format_ranked(queries, [a for a, _m, _c in expect],
                                [m for _a, m, _c in expect], exclude=exclude)


# ---- the refusals (engine.hpp "regex terms"): the term, and a piece of the error's text ----
REFUSED = [
    (b"/", "no regex term"), (b"//", "no regex term"), (b"/ab", "no regex term"),
    (b"/ab\\/", "no regex term"),
    (b"/a**/", "directly after the quantifier"), (b"/a*?/", "directly after the quantifier"),
    (b"/a+?/", "directly after the quantifier"), (b"/(?/", "nothing to repeat"),
    (b"/*a/", "nothing to repeat"), (b"/a|+/", "nothing to repeat"),
    (b"/a{2}/", "unescaped {"), (b"/a}/", "unescaped }"), (b"/^a/", "unescaped ^"),
    (b"/a$/", "unescaped $"),
    (b"/(a/", "never closed"), (b"/a)/", "closes nothing"), (b"/((a)/", "never closed"),
    (b"/a\x00b/", "NUL or a newline"), (b"/a\nb/", "NUL or a newline"),
    (b"/\\d/", "reserved"), (b"/\\w+/", "reserved"), (b"/[\\d]/", "reserved"),
    (b"/[z-a]/", "lo > hi"), (b"/[]/", "empty class"), (b"/[^]/", "empty class"),
    (b"/[ab/", "unterminated class"), (b"/[a\\]/", "unterminated class"),
    (b"/" + b"(" * 33 + b"a" + b")" * 33 + b"/", "kRegexMaxDepth"),
    (b"/" + b"a" * 129 + b"/", "kRegexMaxSource"),
    (b"/" + b"a" * 33 + b"/", "kRegexMaxPos"),
    (b"/" + b"[ab]" * 16 + b"." * 17 + b"/", "kRegexMaxPos"),
]
ACCEPTED = [b"/(a|)/", b"/()/", b"/a|/", b"/" + b"(" * 32 + b"a" + b")" * 32 + b"/",
            b"/" + b"a" * 32 + b"/", b"/" + b"(a|b)*" * 16 + b"/", b"/a\\/b/", b"/\\\\/",
            b"/a.b-c(d)/", b"/[a\\]]/", b"/]/", b"/a b/"]


# ---- the matcher's edges ----
# Every key is one word of edge_text(), one per line before the word `pad`; the oracle says which
# of them a term covers.  Keys of 1, 7, 8, 9, 16, 17 and max_key bytes (the packed words'
# boundaries), a longer word that the index cuts, bytes 0x80 and 0xff, and the fold's edges.
EDGE_LENGTHS = (1, 7, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def edge_keys(max_key=29):
    keys = []
    for n in EDGE_LENGTHS + (max_key,):
        keys += [b"k" * n, b"k" * (n - 1) + b"z", b"K" * (n - 1) + b"Z"]
    keys += [b"k" * (max_key + 6), b"k" * (max_key - 2) + b"zz"]
    keys += [b"a", b"A", b"b", b"B", b"ab", b"AB", b"aB", b"abc", b"abcd", b"abd", b"abcbcd", b"ac",
             b"aab", b"aaab", b"aaaa", b"ba", b"abab", b"c", b"bcd"]
    keys += [b"\x80", b"\xff", b"a\x80b", b"a\xffb", b"\xff\xff", b"\x7f", b"a\x80", b"\xc3\xa9"]
    keys += [b"@a[", b"`A{", b"`a{", b"@A[", b"^", b"]", b"[", b"a]", b"a^", b"{", b"a/b", b"/"]
    seen, out = set(), []
    for key in keys:
        if key not in seen:
            seen.add(key)
            out.append(key)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_terms(max_key=29):
    terms = []
    for n in EDGE_LENGTHS + (max_key,):
        terms += [b"/" + b"k" * (n - 1) + b"./", b"/" + b"k" * (n - 1) + b"[^k]/"]
    terms += [b"/k+/", b"/k*z/", b"/k+zz?/", b"/.*z/", b"/[kK]+[zZ]/", b"/k" + b"." * 16 + b"/",
              b"/" + b"." * 8 + b"/", b"/" + b"." * 9 + b"/", b"/" + b"." * max_key + b"/",
              b"/" + b"." * (max_key - 1) + b"z/"]
    # 0x80 and 0xff against `.`, classes and negated classes
    terms += [b"/./", b"/../", b"/[\x80-\xff]+/", b"/[^\x80]/", b"/a.b/", b"/a[^\x80]b/",
              b"/a[\x80\xff]b/", b"/[^a-z]+/", b"/\xff+/", b"/[\x01-\x7f]/"]
    # the padding, alternation that a greedy matcher gets wrong, nested stars, empty branches,
    # nullable expressions
    terms += [b"/ab./", b"/ab.?/", b"/(a|ab)(c|bcd)/", b"/(a|ab)(c|bcd)*/", b"/(a*)*b/",
              b"/(a*)*/", b"/(a|)b/", b"/(|a)(|b)/", b"/a*/", b"/(ab)?/", b"/()/", b"/(a|b)*/",
              b"/(a+b?)+/", b"/((a|b)(c|d)?)+/", b"/a|b|c|abcd/"]
    # exactly 32 positions; the last position alone decides
    terms += [b"/" + b"k?" * 31 + b"z/", b"/" + b"k?" * 31 + b"k/", b"/" + b"k" * 28 + b"[a-z]?z?.?.?/",
              b"/(k|K)" + b"k?" * 29 + b"[zZ]/"]
    # classes
    terms += [b"/[a-a]/", b"/[-a]/", b"/[a-]/", b"/[\\]]/", b"/[^^]/", b"/[\\^a]/", b"/a[\\]^]/",
              b"/[a-c]+/", b"/[^a-c]/", b"/a\\/b/", b"/\\//", b"/[\\/]/"]
    # the fold's edges: @ [ ` { do not fold; a negated class under the fold
    terms += [b"/@a\\[/", b"/`a\\{/", b"/`A\\{/", b"/[@-\\[]a./", b"/[^a]/", b"/[^A]/", b"/[^a]b/",
              b"/[A-Z]+/", b"/[a-z]+/", b"/aB/", b"/AB/", b"/\xc3\xa9/", b"/\xc3\x89/", b"/[`-\\{]+/"]
    return tuple(terms)


def edge_text(max_key=29):
    return b"".join(k + b" pad\n" for k in edge_keys(max_key))


def full_map_case(max_key=31):
    """``(text, pattern, prefix, batches)`` at ``max_key`` 31: a pattern of 31 bytes whose last byte
    is ``?`` and a prefix of 30 bytes (under ``ignore_case`` the pattern ``p*``) set bit 30 of
    their metacharacter maps, the highest a map has.  No bit of a map may mean anything else: the
    batches hold them alone (to be asked with and without the ``regex`` keyword) and beside
    regex terms, in one query and in queries of their own; to be read with ``glob=True``."""
    n = max_key - 1
    keys = [b"k" * max_key, b"k" * n + b"z", b"K" * n + b"Z", b"k" * n, b"k" * (n - 1) + b"z",
            b"k" * (max_key + 1) + b"q", b"kz"]
    text = b"".join(k + b" pad\n" for k in keys)
    pattern, prefix = b"k" * n + b"?", b"k" * n + b"*"
    alone = [[pattern], [prefix], [prefix, pattern], [pattern, b"pad"]]
    beside = alone + [[b"/k+z/"], [pattern, b"/K+Z?/"], [prefix, b"/k+./"], [b"/k+[a-z]/", b"pad"]]
    return text, pattern, prefix, (alone, beside)


def tile_text(nwords):
    """``nwords`` distinct words w0000, w0001, ... one per line, each on a second line again: a
    dictionary of exactly ``nwords`` keys."""
    words = [b"w%04d" % i for i in range(nwords)]
    return b"".join(w + b"\n" for w in words + words)


# ---- the issue's Hamlet table: term -> ((words, postings, lines), the same with ignore_case) ----
HAMLET = [
    (rb"/.*ing/", (212, 566, 536), (212, 566, 536)),
    (rb"/Ham.*/", (5, 470, 464), (8, 476, 470)),
    (rb"/\[?Hamlet[!?\]]?/", (5, 113, 108), (6, 117, 112)),
    (rb"/(king|queen)[!?]?/", (5, 41, 40), (10, 323, 305)),
    (rb"/[A-Z][A-Z]+/", (14, 33, 24), (5010, 29908, 4148)),
    (rb"/(my)?lord(ship)?[!?]*/", (6, 213, 210), (7, 234, 229)),
    (rb"/[^a-zA-Z]+/", (4, 62, 62), (4, 62, 62)),
    (rb"/(un|in)[a-z]+(ed|ing)/", (24, 46, 46), (27, 57, 55)),
    (rb"/h.ml.*t/", (0, 0, 0), (2, 100, 97)),
]


# ---- random expressions in the accepted subset, for the oracle's cross-check with `re` ----
def random_regex(rng, alphabet, fold):
    """One source, at most 32 positions and 128 bytes: literals, dots, classes, groups,
    alternation and quantifiers over ``alphabet``.  Under the fold classes hold letters and
    digits only, where the rule's definition and ``re.IGNORECASE`` agree by construction.  No
    ``*`` or ``+`` stands on a group that holds one: ``re`` backtracks exponentially there (the
    edge terms hold such expressions, checked by the oracle alone)."""
    budget = [rng.randrange(1, 12)]

    def member(c):
        return (b"" if bytes([c]).isalnum() and c < 0x80 or c >= 0x80 else b"\\") + bytes([c])

    def klass():
        members = rng.sample(list(alphabet), rng.randrange(1, min(4, len(alphabet)) + 1))
        body = b"".join(member(c) for c in members)
        if rng.random() < 0.4:
            lo, hi = sorted(rng.sample(list(alphabet), 2))
            if bytes([lo]).isalnum() and bytes([hi]).isalnum() and hi < 0x80:
                body += bytes([lo]) + b"-" + bytes([hi])
        if not fold and rng.random() < 0.2:
            body += rng.choice([b"\\]", b"\\^", b"!", b"\\\\"])
        return b"[" + (b"^" if rng.random() < 0.3 else b"") + body + b"]"

    def atom(depth):
        """(source, holds an unbounded quantifier)"""
        r = rng.random()
        if depth < 3 and r < 0.25:
            inner, loops = alt(depth + 1)
            return b"(" + inner + b")", loops
        budget[0] -= 1
        if r < 0.4:
            return b".", False
        if r < 0.6:
            return klass(), False
        return member(rng.choice(list(alphabet))), False

    def cat(depth):
        out, loops = b"", False
        for _ in range(rng.randrange(0 if depth else 1, 4)):
            if budget[0] <= 0:
                break
            a, inner = atom(depth)
            out += a
            loops |= inner
            if rng.random() < 0.4:
                q = rng.choice([b"?"] if inner else [b"*", b"+", b"?"])
                out += q
                loops |= q != b"?"
        return out, loops

    def alt(depth):
        parts = [cat(depth) for _ in range(rng.choice([1, 1, 2, 3]))]
        return b"|".join(p for p, _l in parts), any(l for _p, l in parts)

    while True:
        src, _loops = alt(0)
        if src and len(src) <= 128:
            return src
