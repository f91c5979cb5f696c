"""What tests/test_show.py, tests/test_show_gpu.py and tests/test_show_cli_gpu.py share: the
oracle's answer of a batch with ``show=N`` (engine.hpp "show", ``oracle.SHOW_RULES``), its exact
comparison with a ``SearchResult``, the CLI's output by the oracle, and the fuzz generator."""
import functools
import random

from locust_amd.utils import oracle
from tests.glob_cases import formatted, same, want


def want_show(text, queries, modes, n, k=None, first_line=0, within=None, exclude=None,
              glob=False, ignore_case=False, **okw):
    """``(base, shown)``: ``base`` is ``glob_cases.want``'s [(answer, matches, counts)], and
    ``shown`` per query ``(texts, spans, cut)`` of its returned lines by ``oracle.show``."""
    base = want(text, queries, modes, k, first_line, within, exclude, glob, ignore_case, **okw)
    shown = []
    for q, (answer, _m, _c) in zip(queries, base):
        lines = answer if k is None else [l for l, _s in answer]
        shown.append(oracle.show(text, lines, q, n, first_line=first_line, glob=glob,
                                 ignore_case=ignore_case, **okw))
    return base, shown


def same_show(got, expect, n, k=None, plain=None):
    """``got`` (a ``SearchResult`` with show) against ``expect`` = ``want_show``'s pair: text,
    text_off, spans, span_off and cut_lines exactly; ``plain``: the ``show=0`` run of the same
    batch, whose lines, hits, scores, matches and counts must be ``got``'s."""
    base, shown = expect
    same(got, base, k)
    assert got.show_bytes == n
    text_off, span_off = [0], [0]
    for i, (texts, spans, _cut) in enumerate(shown):
        assert got.text(i) == texts, i
        assert got.spans(i) == spans, i
        for t, s in zip(texts, spans):
            assert len(t) <= n
            text_off.append(text_off[-1] + len(t))
            span_off.append(span_off[-1] + len(s))
    assert got.text_off() == text_off
    assert got.span_off() == span_off
    assert got.span_count == span_off[-1]
    assert got.cut_lines == sum(cut for _t, _s, cut in shown)
    if plain is not None:
        assert plain.show_bytes == 0 and plain.text_off() == [] and plain.span_off() == []
        assert plain.cut_lines == 0 and plain.show_ms == 0
        assert plain.hits() == got.hits() and plain.matches() == got.matches()
        for i in range(got.queries):
            assert plain.lines(i) == got.lines(i) and plain.scores(i) == got.scores(i), i
            assert plain.term_counts(i) == got.term_counts(i), i
            assert plain.text(i) == [] and plain.spans(i) == []


def formatted_show(queries, expect, k=None, exclude=None, glob=False, mark=False):
    """The CLI's ``--show N [--mark]`` output of the batch, by the oracle."""
    base, shown = expect
    out = []
    for i, (q, one, (texts, spans, _cut)) in enumerate(zip(queries, base, shown)):
        first = formatted([q], [one], k, [exclude[i]] if exclude else None, glob)
        lines = one[0] if k is None else [l for l, _s in one[0]]
        out.append(oracle.format_show(first, lines, texts, spans, mark))
    return b"".join(out)


def wire_bytes_of_show(got):
    """What the show stage is documented to copy (docs/ARCHITECTURE.md 2h): both offset arrays,
    the span triples, the text, and its 32-byte counters twice."""
    entries = sum(got.hits())
    if entries == 0:
        return 0
    return 2 * (entries + 1) * 8 + 12 * got.span_count + got.text_off()[-1] + 2 * 32


LONG = [b"a" * 29, b"a" * 29 + b"X", b"b" * 70, b"ab" * 65, b"A" * 35]


@functools.lru_cache(maxsize=None)
def fuzz_text(seed, nlines=300):
    """A text of at most ``nlines`` lines over a small alphabet in both cases: short tokens,
    tokens of 29 to 130 bytes, runs of delimiters, NULs, empty lines, lines up to a few hundred
    bytes; every third seed ends without a newline."""
    rng = random.Random(seed)
    alphabet = b"abAB" if seed % 2 else b"abcA"
    vocab = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 6))) for _ in range(40)]
    vocab += LONG + [b"b\xff", b"b\x80a", b"@a["]
    seps = [b" ", b" ", b" ", b"  ", b", ", b".-", b"\t"]
    lines = []
    for _ in range(rng.randrange(nlines // 2, nlines + 1)):
        words = [rng.choice(vocab) for _ in range(rng.choice([0, 1, 2, 3, 5, 8, 13, 24, 40]))]
        line = b"".join(w + rng.choice(seps) for w in words)
        if rng.random() < 0.3:
            line = line.rstrip(b" \t")
        if rng.random() < 0.2:
            line = rng.choice(seps) + line
        if line and rng.random() < 0.05:
            at = rng.randrange(len(line))
            line = line[:at] + b"\0" + line[at:]
        lines.append(line)
    text = b"\n".join(lines)
    return text if seed % 3 == 0 else text + b"\n"


def fuzz_batch(seed, text_seed):
    """One random batch over ``fuzz_text(text_seed)``: ``(queries, modes, kwargs)`` with
    ``kwargs`` holding within, exclude, glob, ignore_case, rank and show."""
    rng = random.Random(seed * 7919 + text_seed)
    alphabet = b"abAB" if text_seed % 2 else b"abcA"
    glob = rng.random() < 0.5
    words = [bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 4))) for _ in range(6)]
    words += LONG + [b"zz", b"b\xff"]

    def term():
        w = bytearray(rng.choice(words))[:29]
        if not glob or rng.random() < 0.4:
            return bytes(w)
        w = w[:rng.randrange(1, 8)]
        if rng.random() < 0.4:
            return bytes(w) + b"*"
        at = rng.randrange(len(w) + 1)
        if rng.random() < 0.5:
            w[at:at] = b"*"
        elif at < len(w):
            w[at] = 0x3F
        else:
            w[at:at] = b"?"
        return bytes(w)

    queries, modes, within, exclude = [], [], [], []
    for _ in range(rng.randrange(1, 7)):
        mode = rng.choice(["all", "any", "any", "phrase", "near"])
        q = [term() for _t in range(rng.randrange(1, 4 if mode in ("phrase", "near") else 9))]
        if len(q) > 1 and rng.random() < 0.3:
            q[rng.randrange(1, len(q))] = q[0]  # a repeated term
        x = None
        if len(q) < 8 and rng.random() < 0.25:
            x = [term() for _t in range(rng.randrange(1, min(3, 9 - len(q))))]
        queries.append(q)
        modes.append(mode)
        within.append(rng.randrange(1, 5) if mode == "near" else None)
        exclude.append(x)
    kw = dict(within=within, exclude=exclude, glob=glob, ignore_case=rng.random() < 0.3,
              rank=rng.choice([None, None, 1, 3, 50]),
              show=rng.choice([1, 5, 63, 64, 65, 80, 200, 4096, 65536]))
    return queries, modes, kw


FUZZ_TEXTS = range(8)
FUZZ_BATCHES = 30  # per text: 240 batches in all


@functools.lru_cache(maxsize=None)
def fuzz_expect(text_seed, seed, first_line=0):
    """The oracle's answer of one fuzz batch (shared by the CPU and the GPU test)."""
    queries, modes, kw = fuzz_batch(seed, text_seed)
    return want_show(fuzz_text(text_seed), queries, modes, kw["show"], kw["rank"], first_line,
                     kw["within"], kw["exclude"], kw["glob"], kw["ignore_case"])
