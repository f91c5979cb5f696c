"""What tests/test_tally.py and tests/test_tally_gpu.py share: the oracle's answer of a batch
with ``tally=K`` (engine.hpp "tally: the words of the returned lines", ``oracle.TALLY_RULES``),
its exact comparison with a ``SearchResult``, the CLI's output by the oracle, the brute-force
count over the returned lines' text, and the text builders of the device stage's edges."""
import collections
import functools
import random

from locust_amd.utils import oracle

OPTS = ("wildcard", "glob", "ignore_case", "fuzzy", "regex")


def want(text, queries, modes, tally, k=None, first_line=0, within=None, exclude=None, **okw):
    """``(base, tallies)``: ``base`` is [(answer, matches, counts)] of every query by the oracle
    -- ``answer`` the ascending lines (``k`` None) or the ``(line, score)`` pairs of the best
    ``k`` -- and ``tallies`` per query ``oracle.tally``'s ``(words, tokens, top)`` over its
    returned lines.  ``okw``: the readings (OPTS) and the job's delims / emits / max_key."""
    if isinstance(modes, str):
        modes = [modes] * len(queries)
    if not isinstance(within, list):
        within = [within] * len(queries)
    exclude = exclude or [None] * len(queries)
    opts = {key: v for key, v in okw.items() if key in OPTS}
    job = {key: v for key, v in okw.items() if key not in OPTS}
    ent, post = oracle.index(text, first_line=first_line, **job)
    skw = {key: v for key, v in job.items() if key in ("delims", "max_key")}
    base, tallies = [], []
    for q, m, w, x in zip(queries, modes, within, exclude):
        if m == "phrase":
            lines, counts = oracle.phrase(text, q, first_line=first_line, exclude=x, **opts, **job)
        elif m == "near":
            lines, counts = oracle.near(text, q, w, first_line=first_line, exclude=x, **opts, **job)
        else:
            lines, counts = oracle.search(ent, post, q, m, exclude=x, **opts, **skw)
        if k is None:
            base.append((lines, len(lines), counts))
        else:
            top, matches = oracle.rank(ent, post, lines, q, k, exclude=x, **opts, **skw)
            base.append((top, matches, counts))
            lines = [l for l, _s in top]
        tallies.append(oracle.tally(ent, post, lines, tally))
    return base, tallies


def same_base(got, base, k=None):
    assert got.queries == len(base) and got.rank_k == (k or 0)
    assert got.matches() == [m for _a, m, _c in base]
    assert got.hits() == [m if k is None else min(k, m) for _a, m, _c in base]
    for i, (answer, _m, counts) in enumerate(base):
        if k is None:
            assert got.lines(i) == answer and got.scores(i) == [], i
        else:
            assert list(zip(got.lines(i), got.scores(i))) == answer, i
        assert got.term_counts(i) == counts, i


def same(got, expect, tally, k=None, device=False):
    """``got`` (a ``SearchResult`` with tally) against ``expect`` = ``want``'s pair, exactly:
    the search's own answer, tally_words, tally_tokens and every query's words.  ``device``:
    ``tallied`` is the batch's pair words; the host evaluation reports 0."""
    base, tallies = expect
    same_base(got, base, k)
    assert got.tally_k == tally
    assert got.tally_words() == [w for w, _t, _top in tallies]
    assert got.tally_tokens() == [t for _w, t, _top in tallies]
    for i, (words, _tokens, top) in enumerate(tallies):
        assert got.tally(i) == top, i
        assert len(top) == min(tally, words)
    assert got.tallied == (sum(t for _w, t, _top in tallies) if device else 0)


def formatted(queries, expect, k=None, exclude=None, shown=None, mark=False):
    """The CLI's ``--search ... --tally K`` output of the batch, by the oracle.  ``shown``: per
    query ``oracle.show``'s ``(texts, spans, cut)``, for a batch with ``--show`` too."""
    base, tallies = expect
    out = []
    for i, (q, one, t) in enumerate(zip(queries, base, tallies)):
        x = [exclude[i]] if exclude else None
        if k is None:
            first = oracle.format_search([q], [one[0]], exclude=x)
            lines = one[0]
        else:
            first = oracle.format_ranked([q], [one[0]], [one[1]], exclude=x)
            lines = [l for l, _s in one[0]]
        if shown is not None:
            first = oracle.format_show(first, lines, shown[i][0], shown[i][1], mark)
        out.append(first + oracle.format_tally(*t))
    return b"".join(out)


def brute(text, lines, k, first_line=0, **job):
    """``oracle.tally``'s answer without an index: a ``Counter`` over ``oracle.tokenize`` of the
    returned lines' text."""
    all_lines = oracle.split_lines(text)
    counts = collections.Counter()
    for l in lines:
        counts.update(oracle.tokenize(all_lines[l - first_line], **job)[0])
    ordered = sorted(counts.items(), key=lambda kc: (-kc[1], kc[0]))
    return len(counts), sum(counts.values()), ordered[:k]


def wire_bytes_of_tally(got):
    """What the tally stage is documented to copy (docs/ARCHITECTURE.md 2k): the 64-byte counters
    at the sizing readback; then, when the lines hold a token, the counters and the per-query
    word counts (u32), the three per-query u64 arrays (Q, Q, Q + 1), the winners' 40-byte records
    and the counters once more."""
    if sum(got.hits()) == 0:
        return 0
    if got.tallied == 0:
        return 64
    q = got.queries
    records = sum(len(got.tally(i)) for i in range(q))
    return 64 + (64 + 4 * q) + (3 * q + 1) * 8 + 40 * records + 64


@functools.lru_cache(maxsize=None)
def fuzz_text(seed, nlines=60):
    """A small text over a small vocabulary in both cases: keys past 29 bytes that merge, runs of
    delimiters, NULs inside lines, empty lines, lines past the emit cap; every third seed ends
    without a newline."""
    rng = random.Random(seed)
    vocab = [bytes(rng.choice(b"abAB") for _ in range(rng.randrange(1, 4))) for _ in range(12)]
    vocab += [b"a" * 29, b"a" * 29 + b"X", b"a" * 40, b"To", b"to", b"b\xff", b"b\x80a"]
    seps = [b" ", b" ", b"  ", b", ", b".-", b"\t"]
    lines = []
    for _ in range(rng.randrange(nlines // 2, nlines + 1)):
        words = [rng.choice(vocab) for _ in range(rng.choice([0, 1, 2, 3, 5, 8, 13, 24, 40]))]
        line = b"".join(w + rng.choice(seps) for w in words)
        if line and rng.random() < 0.1:
            at = rng.randrange(len(line))
            line = line[:at] + b"\0" + line[at:]
        lines.append(line)
    text = b"\n".join(lines)
    return text if seed % 3 == 0 else text + b"\n"


def word(i):
    """Distinct words of letters only: word(0) = `a`, ... in key order within a length."""
    out = b""
    i += 1
    while i:
        i, d = divmod(i - 1, 26)
        out = bytes([97 + d]) + out
    return b"w" + out


def lines_of_words(nwords, per_line, marker=b"hit"):
    """``nwords`` distinct words, ``per_line`` to a line, every line starting with ``marker``."""
    rows = [b" ".join([marker] + [word(i) for i in range(at, min(at + per_line, nwords))])
            for at in range(0, nwords, per_line)]
    return b"\n".join(rows) + b"\n"
