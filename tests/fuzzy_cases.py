"""What tests/test_fuzzy.py and tests/test_fuzzy_gpu.py share: the oracle's answer of a batch
with fuzzy terms (``fuzzy``, engine.hpp "fuzzy terms", ``oracle.FUZZY_RULES``), alone or beside
``glob``, ``wildcard`` and ``ignore_case``, its exact comparison with a ``SearchResult``, ranked
or not and with ``show``, the matcher's edge text and the fuzz generator."""
import functools
import random

from locust_amd.utils import oracle
from tests import glob_cases
from tests.glob_cases import same  # noqa: F401  (the comparison is the pattern terms')


def want(text, queries, modes, k=None, first_line=0, within=None, exclude=None, glob=False,
         ignore_case=False, wildcard=False, fuzzy=True, **okw):
    """[(answer, matches, counts)] of every query by the oracle, as ``glob_cases.want``."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if not isinstance(within, list):
        within = [within] * len(queries)
    exclude = exclude or [None] * len(queries)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    gkw = {"glob": glob, "ignore_case": ignore_case, "wildcard": wildcard, "fuzzy": fuzzy}
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


def want_show(text, queries, modes, n, k=None, first_line=0, within=None, exclude=None,
              glob=False, ignore_case=False, wildcard=False, fuzzy=True, **okw):
    """``(base, shown)`` as ``show_cases.want_show``: ``want``'s list, and per query ``(texts,
    spans, cut)`` of its returned lines by ``oracle.show``."""
    base = want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case, wildcard,
                fuzzy, **okw)
    shown = []
    for q, (answer, _m, _c) in zip(queries, base):
        lines = answer if k is None else [l for l, _s in answer]
        shown.append(oracle.show(text, lines, q, n, first_line=first_line, glob=glob,
                                 ignore_case=ignore_case, wildcard=wildcard, fuzzy=fuzzy, **okw))
    return base, shown


def merged(text, queries, first_line=0, exclude=None, glob=False, ignore_case=False,
           wildcard=False, fuzzy=True, **okw):
    """``SearchResult.merged`` of the batch on the device, by the oracle."""
    ent, _post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    return oracle.merged_elements(ent, queries, exclude=exclude, glob=glob, fuzzy=fuzzy,
                                  ignore_case=ignore_case, wildcard=wildcard, **skw)


def formatted(queries, expect, k=None, exclude=None, glob=False):
    """The CLI's result lines of the batch, the queries as asked: a fuzzy term with its ``~d``
    (``glob``: runs of stars collapsed, as the terms are read)."""
    return glob_cases.formatted(queries, expect, k, exclude, glob)


# ---- the matcher's edges ----
# One word per length, and around each the keys one, two and three edits away: substitutions,
# insertions and deletions at the first byte, at the last byte and on both sides of the packed
# words' boundaries (bytes 7/8, 15/16, 23/24).  Every key is one word of edge_text(), one per
# line; the oracle says which of them a term covers.
EDGE_LENGTHS = (7, 8, 9, 15, 16, 17, 24, 28, 29)
FILL = b"ZY\x80\xffXW"  # what substitutions and insertions put in: 0x80 and 0xff among them


def edge_word(n):
    """The word of ``n`` bytes: lower-case letters, no two adjacent ones equal, and different
    words at different lengths."""
    return bytes(0x61 + (5 * i + 3 * n) % 26 for i in range(n))


def edge_positions(n):
    return sorted({0, n - 1} | {p for p in (7, 8, 15, 16, 23, 24) if p < n})


def _edits(w, kind, at):
    """``w`` with one edit of ``kind`` at each position of ``at``, in descending order so that
    the positions stay those of ``w``."""
    w = bytearray(w)
    for i, p in enumerate(sorted(at, reverse=True)):
        f = FILL[(p + i + len(w)) % len(FILL)]
        if kind == "sub":
            w[p] = f
        elif kind == "ins":
            w[p:p] = bytes([f])
        else:
            del w[p]
    return bytes(w)


@functools.lru_cache(maxsize=None)
def edge_keys(max_key=29):
    lengths = EDGE_LENGTHS + tuple(n for n in (30, 31) if n <= max_key)
    keys = []
    for n in lengths:
        w = edge_word(n)
        pos = edge_positions(n)
        keys.append(w)
        for p in pos:  # one edit
            keys += [_edits(w, kind, [p]) for kind in ("sub", "ins", "del")]
        for a, b in zip(pos, pos[1:] + pos[:1]):  # two and three edits of one kind
            for kind in ("sub", "ins", "del"):
                if a != b:
                    keys.append(_edits(w, kind, [a, b]))
                third = [p for p in pos if p not in (a, b)] or [(a + 2) % n]
                if len({a, b, third[0]}) == 3:
                    keys.append(_edits(w, kind, [a, b, third[0]]))
        # mixed kinds: a substitution at the front and a deletion at the back (length - 1)
        keys.append(_edits(_edits(w, "del", [n - 1]), "sub", [0]))
    # a long word, cut to max_key and matched as its merged key; a word one byte off its cut
    keys += [b"m" * (max_key + 6), b"m" * (max_key - 1) + b"n"]
    # fold edges: only ASCII letters fold
    keys += [b"@a[", b"`A{", b"`a{", b"a", b"A", b"AB", b"ab", b"Ab", b"aB", b"abc", b"ABC", b"aBd"]
    # a `~` that is no suffix is a literal byte of its word
    keys += [b"ab~0x", b"ab~12", b"a~b", b"a~c", b"a~~b"]
    seen, out = set(), []
    for k in keys:  # (as asked: a key longer than max_key is a word of the text, cut by the index)
        if k and k not in seen and not any(c in b" \n\t" for c in k):
            seen.add(k)
            out.append(k)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_terms(max_key=29):
    lengths = EDGE_LENGTHS + tuple(n for n in (30, 31) if n <= max_key)
    terms = []
    for n in lengths:
        terms += [edge_word(n) + b"~1", edge_word(n) + b"~2"]
    terms += [b"m" * max_key + b"~1", b"m" * (max_key - 1) + b"x~1", b"m" * (max_key - 2) + b"~2"]
    terms += [b"@a[~1", b"@a[~2", b"`A{~2", b"ab~1", b"AB~1", b"abc~2", b"Abd~2"]
    terms += [b"ab~0x", b"ab~12", b"a~b~1", b"a~1b"]  # a ~ elsewhere is a literal byte
    return tuple(terms)


def edge_text(max_key=29):
    return b"".join(k + b" pad\n" for k in edge_keys(max_key))


def edge_distances(term, max_key=29, fold=False):
    """The distances from a fuzzy term's word to every key of the edge text, as the index holds
    them (cut to ``max_key``)."""
    return [oracle.levenshtein(term[:-2], k[:max_key], fold) for k in edge_keys(max_key)]


# ---- fuzz ----
def fuzz_case(seed, nlines=120, nqueries=60):
    """``glob_cases.fuzz_case``'s shape over a 3-4 letter alphabet in both cases, so that words
    one and two edits apart abound: a text of ``nlines`` lines and ``nqueries`` random queries
    mixing plain, prefix, pattern and fuzzy terms in all four modes, with repeated terms, the
    same word under both budgets in one query, and exclusion terms that are fuzzy: ``(text,
    queries, modes, within, exclude)``, to be read with ``glob=True, fuzzy=True``."""
    rng = random.Random(seed * 31 + 7)
    alphabet = b"abAB" if seed % 2 else b"abcA"
    vocab = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 6))) for _ in range(50)]
    vocab += [b"a" * 29, b"a" * 29 + b"X", b"A" * 35, b"b\xff", b"b\x80a", b"b", b"@a[", b"`A{",
              b"ham", b"hem", b"hams", b"Ham", b"hm"]
    lines = [b" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 10)))
             for _ in range(nlines)]
    text = b"\n".join(lines) + b"\n"

    def fuzzy_term(d=None):
        d = d or rng.randrange(1, 3)
        w = rng.choice([v for v in vocab + [b"zzz", b"abab", b"BAb"] if d < len(v) <= 29])
        if rng.random() < 0.3:  # an edit of our own: the word itself may be no key
            at = rng.randrange(len(w))
            w = w[:at] + bytes([rng.choice(alphabet)]) + w[at + rng.randrange(2):]
        w = w[:29]
        return (w if len(w) > d else w + b"ab") + b"~%d" % d

    def term():
        r = rng.random()
        if r < 0.45:
            return fuzzy_term()
        w = bytearray(rng.choice(vocab + [b"zz", b"ab", b"BA"]))[:rng.randrange(1, 8)]
        if r < 0.6:
            return bytes(w)
        if r < 0.7:
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
    for i in range(nqueries):
        mode = rng.choice(["all", "any", "phrase", "near"])
        q = [term() for _t in range(rng.randrange(1, 4 if mode in ("phrase", "near") else 7))]
        if rng.random() < 0.3:
            q[rng.randrange(len(q))] = q[0]  # a repeated term
        if i % 6 == 0:  # the same word under both budgets: two terms, not one
            q = q[:5] + [b"ham~1", b"ham~2"]
            rng.shuffle(q)
        x = None
        if rng.random() < 0.35:
            x = [fuzzy_term() if rng.random() < 0.6 else term()
                 for _t in range(rng.randrange(1, 3))][:8 - len(q)] or None
        queries.append(q)
        modes.append(mode)
        within.append(rng.randrange(1, 5) if mode == "near" else None)
        exclude.append(x)
    return text, queries, modes, within, exclude


def tile_text(nwords):
    """``nwords`` distinct words w0000, w0001, ... one per line, each on a second line again: a
    dictionary of exactly ``nwords`` keys."""
    words = [b"w%04d" % i for i in range(nwords)]
    return b"".join(w + b"\n" for w in words + words)
