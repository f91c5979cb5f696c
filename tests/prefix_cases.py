"""What tests/test_prefix.py and tests/test_prefix_gpu.py share: the oracle's answer of a
batch with prefix terms (``wildcard=True`` throughout) and its exact comparison with a
``SearchResult``, ranked or not."""
import random

from locust_amd.utils import oracle


def want(text, queries, modes, k=None, first_line=0, **okw):
    """[(answer, matches, counts)] of every query by the oracle; ``answer`` is the ascending
    lines (``k`` None) or the ``(line, score)`` pairs of the best ``k``."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    ent, post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    out = []
    for q, m in zip(queries, modes):
        if m == "phrase":
            lines, counts = oracle.phrase(text, q, first_line=first_line, wildcard=True, **okw)
        else:
            lines, counts = oracle.search(ent, post, q, m, wildcard=True, **skw)
        if k is None:
            out.append((lines, len(lines), counts))
        else:
            top, matches = oracle.rank(ent, post, lines, q, k, wildcard=True, **skw)
            out.append((top, matches, counts))
    return out


def merged(text, queries, first_line=0, **okw):
    """``SearchResult.merged`` of the batch on the device, by the oracle."""
    ent, _post = oracle.index(text, first_line=first_line, **okw)
    skw = {key: v for key, v in okw.items() if key in ("delims", "max_key")}
    return oracle.merged_elements(ent, queries, **skw)


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


def formatted(queries, expect, k=None):
    """The CLI's result lines of the batch, the queries as asked (with their stars)."""
    if k is None:
        return oracle.format_search(queries, [a for a, _m, _c in expect])
    return oracle.format_ranked(queries, [a for a, _m, _c in expect], [m for _a, m, _c in expect])


def fuzz_case(seed, nlines=150, nqueries=80):
    """A text of `nlines` lines over a 3-4 letter alphabet, so that prefixes cover many
    words (and words of 29, 30 and 35 bytes that merge, and keys with 0xff bytes), and
    `nqueries` random queries mixing plain and prefix terms in all three modes."""
    rng = random.Random(seed)
    alphabet = b"abc" if seed % 2 else b"abcd"
    vocab = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 6))) for _ in range(60)]
    vocab += [b"a" * 29, b"a" * 29 + b"X", b"a" * 35, b"b\xff", b"b\xff\xff", b"b"]
    lines = [b" ".join(rng.choice(vocab) for _ in range(rng.randrange(0, 10)))
             for _ in range(nlines)]
    text = b"\n".join(lines) + b"\n"
    queries, modes = [], []
    for _ in range(nqueries):
        q = []
        for _t in range(rng.randrange(1, 9)):
            w = rng.choice(vocab + [b"zz", b"d", b"ab"])
            if rng.random() < 0.5:
                w = w[:rng.randrange(1, len(w) + 1)] + b"*"
            q.append(w)
        if rng.random() < 0.3:
            q[rng.randrange(len(q))] = q[0]  # a repeated term
        mode = rng.choice(["all", "any", "phrase"])
        if mode == "phrase":
            q = q[:rng.randrange(1, 4)]
        queries.append(q)
        modes.append(mode)
    return text, queries, modes
