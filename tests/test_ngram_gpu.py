"""Word n-grams on the device (csrc/kernels/ngram.hip): the n-gram map through both tile
shapes and every consumer of its output -- the ordered dictionary build, psort / radix,
streaming, top-K, the multi-rank exchange -- and the CLI.  Every comparison is exact against
``oracle.wordcount(text, ngram=N)`` (entries, num_tokens, num_unique, overflow_lines,
truncated); the 8 MiB text is compared with the CPU engine, which tests/test_ngram.py ties
to the oracle.  Shapes are the smallest at which the kernel can go wrong: the last word of
an n-gram on either side of a 64-byte segment edge, a 1 KiB tile edge and the staged
overhang, delimiter runs up to 300 bytes, the end of the text."""
import os
import subprocess

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from tests.ngram_texts import got, num_lines, random_text, want

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_DELIMS = b" ,;.-\t:'"


def engine(n, max_bytes=8 << 10, max_lines=1 << 10, **kw):
    return lc.Engine(lc.make_config("gpu", check=True, ngram=n, **kw), max_bytes, max_lines)


@pytest.fixture(scope="module")
def small_engines():
    """One engine per N for every small case (one config per engine)."""
    return {n: engine(n) for n in (2, 3)}


def check(eng, text, n, **kw):
    assert got(eng.run(text)) == want(text, n, **kw), (n, len(text), text[:80])


# ---------------- boundary sweep: 1 KiB tiles ----------------
def boundary_text(n: int, target: int, run: int, final_newline: bool) -> bytes:
    """A text whose last line has n tokens, the first byte of the last one at offset
    `target`, a delimiter run of `run` bytes before it; the text ends with that token, or
    with a newline and one more line."""
    delims = bytes(RUN_DELIMS[i % len(RUN_DELIMS)] for i in range(run))
    head = (b"alpha" if n == 2 else b"alpha, beta") + delims
    start = target - len(head)
    filler = bytearray()
    line = b"the quick brown fox jumps over\n"
    while len(filler) + len(line) + 60 <= start:
        filler += line
    while len(filler) < start:  # pad lines of at most 60 bytes up to the line's start
        m = min(start - len(filler), 60)
        filler += b"p" * (m - 1) + b"\n"
    text = bytes(filler) + head + b"omega"
    assert text.index(b"omega") == target and len(filler) == start
    return text + (b"\nnext words follow here\n" if final_newline else b"")


@pytest.mark.parametrize("run", [1, 63, 64, 65, 130, 300])
@pytest.mark.parametrize("n", [2, 3])
def test_boundary_sweep(small_engines, n, run):
    eng = small_engines[n]
    for d in range(-70, 71):
        for final_newline in (True, False):
            text = boundary_text(n, 2048 + d, run, final_newline)
            assert 1900 < len(text) <= 3072  # three 1 KiB tiles
            w = want(text, n)
            gram = b"alpha omega" if n == 2 else b"alpha beta omega"
            assert gram in [k for k, _v, _c in w[0]]
            assert got(eng.run(text)) == w, (n, run, d, final_newline)


# ---------------- line rules ----------------
def line_rule_texts(n: int) -> list[bytes]:
    E = 20
    tok = lambda i: b"t%d" % i
    line = lambda t: b" ".join(tok(i) for i in range(t))
    texts = [line(t) + b"\n" for t in (0, 1, n - 1, n, n + 1)]
    texts += [b"\n\n\n", b"a b c\r\nd e f\r\n", b"\n a b c\n\n\nd e\n",
              b"caf\xc3\xa9 na\xefve \xff\x80 z\n",
              b"a b\0c d e\nf g h\n",          # a NUL between the words of a would-be n-gram
              b"a b c\0 d e f\nf g h\n",        # ... and after an n-gram
              b"a\0\nb c d\n", b"\0a b c\nd e f",
              line(E + n - 1) + b"\n",          # exactly E n-grams: no overflow
              line(E + n) + b"\n",              # E + 1: overflow 1
              line(E + n + 7) + b"\n" + line(3) + b"\n"]
    for ln in (24, 25, 26, 27, 28, 29, 30, 31):  # joined 29 / 30: the truncation edge
        texts.append(b"x" * ln + b" yz w\n" + b"x" * ln + b" y\n" + b"k " + b"x" * ln + b"\n")
    texts.append(b"m" * 40 + b" " + b"n" * 40 + b" o\n")
    return texts


@pytest.mark.parametrize("n", [2, 3])
def test_line_rules(small_engines, n):
    eng = small_engines[n]
    texts = line_rule_texts(n)
    for text in texts:
        check(eng, text, n)
    check(eng, b"".join(texts), n)
    whole = want(b"".join(texts), n)
    assert whole[3] >= 2 and whole[4] >= 4  # overflow and truncation really occur


@pytest.mark.parametrize("n", [2, 3])
def test_delimiters_and_emit_cap(n):
    text = b"".join(line_rule_texts(n)) + random_text(3, 3000)
    eng = engine(n, delimiters="ae ")
    check(eng, text, n, delims=b"ae ")
    eng = engine(n, emits_per_line=1)
    check(eng, text, n, emits=1)
    eng = engine(n, max_key_len=8)
    check(eng, text, n, max_key=8)


# ---------------- seeded random texts ----------------
@pytest.mark.parametrize("sort", ["dict", "radix"])
@pytest.mark.parametrize("n", [2, 3])
def test_random_texts(n, sort):
    eng = engine(n, sort=sort)
    for seed in range(120):
        text = random_text(seed)
        assert got(eng.run(text)) == want(text, n), (seed, len(text))


# ---------------- Hamlet ----------------
@pytest.mark.parametrize("sort", ["dict", "radix"])
@pytest.mark.parametrize("n", [2, 3])
def test_hamlet(hamlet, n, sort):
    win = oracle.window(hamlet, 0, 700)
    eng = engine(n, len(hamlet), num_lines(hamlet), sort=sort)
    w_whole, w_win = want(hamlet, n), want(win, n)
    other = random_text(11, 5120)
    # the second and third job run on the partition map retuned from the first output
    for text, w in ((hamlet, w_whole), (win, w_win), (hamlet, w_whole), (other, want(other, n)),
                    (hamlet, w_whole)):
        assert got(eng.run(text)) == w
    print("ngram", n, sort, "stats", eng._eng.stats())


# ---------------- large tiles, piecewise upload ----------------
def test_large_tiles_bigrams():
    """Just above kMapLargeInput (8 MiB, also the piecewise upload's threshold): 4 KiB tiles,
    the token list's two sweeps, per-tile combining.  A stress block of 130-byte delimiter
    runs in lines of varying length lies across many 4 KiB tile edges."""
    base = lc._C.gen_text(bytes=1 << 20, seed=5)
    stress = bytearray()
    i = 0
    while len(stress) < (64 << 10):
        a, b, c = b"s" * (1 + i % 9), b"u" * (1 + i % 31), b"v" * (1 + i % 5)
        run = bytes(RUN_DELIMS[(i + j) % len(RUN_DELIMS)] for j in range(130))
        stress += a + run + b + b" " + c + b"\n"
        i += 1
    block = base + bytes(stress)
    text = block * (((8 << 20) // len(block)) + 1)
    assert (8 << 20) < len(text) < (10 << 20)
    w = got(lc._C.cpu_run(lc.make_config("cpu", ngram=2), text))
    eng = lc.Engine(lc.make_config("gpu", check=True, ngram=2), len(text), num_lines(text))
    for _ in range(2):
        assert got(eng.run(text)) == w
    print("large bigrams: stats", eng._eng.stats(), "unique", w[2])


# ---------------- streaming, top-K, multi-rank ----------------
def test_streaming(hamlet):
    cfg = lc.make_config("gpu", check=True, ngram=2, chunk_bytes=16 << 10)
    eng = lc._C.GpuEngine(cfg, 1 << 30, 1 << 30)
    w = want(hamlet, 2)
    st = eng.stats()
    assert st["streaming"] and st["chunk_bytes"] < len(hamlet) // 2  # several chunks
    assert got(eng.run(hamlet)) == w
    t = eng.run_top(hamlet, 10)
    assert t.chunks > 1 and t.entries() == oracle.top(w[0], 10)
    assert (t.num_tokens, t.num_unique, t.overflow_lines, t.truncated) == w[1:]


@pytest.mark.parametrize("k", [1, 10, 1000])
def test_top_k(hamlet, k):
    w = want(hamlet, 2)
    t = lc.top_words_text(hamlet, k, check=True, ngram=2)
    assert t.entries() == oracle.top(w[0], k)
    assert (t.num_tokens, t.num_unique, t.overflow_lines, t.truncated) == w[1:]


@pytest.mark.parametrize("strategy", ["gather", "shuffle"])
def test_multi_rank_loopback(hamlet, strategy):
    w = want(hamlet, 2)
    one = lc.wordcount_text(hamlet, check=True, ngram=2)
    r = lc.run_multi(hamlet, 3, check=True, ngram=2, strategy=strategy, comm="loopback")
    assert r.entries() == one.entries() == w[0]
    assert r.num_tokens == w[1] and r.num_unique == w[2]


# ---------------- refusals ----------------
def test_compat_map_refused():
    with pytest.raises(lc.LocustError, match="map_path fast"):
        lc.Engine(lc.make_config("gpu", map_path="compat", ngram=2), 1 << 12, 64)
    for n in (0, 4):
        with pytest.raises(lc.LocustError, match="ngram"):
            lc.Engine(lc.make_config("gpu", ngram=n), 1 << 12, 64)


# ---------------- the CLI ----------------
def run_cli(cli, *args):
    return subprocess.run([cli, *map(str, args)], capture_output=True, timeout=100, cwd=ROOT)


def result_lines(out: bytes) -> bytes:
    return b"".join(l + b"\n" for l in out.split(b"\n") if l.startswith(b"print key:"))


@pytest.mark.parametrize("extra", [(), ("--sort", "radix"), ("--check", "--gpus", 2, "--comm", "loopback")])
def test_cli_ngram(cli, hamlet, extra):
    p = run_cli(cli, "data/hamlet.txt", "--ngram", 2, *extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_gpu(want(hamlet, 2)[0])


def test_cli_ngram_top(cli, hamlet):
    p = run_cli(cli, "data/hamlet.txt", "--ngram", 2, "--top", 10)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert result_lines(p.stdout) == oracle.format_gpu(oracle.top(want(hamlet, 2)[0], 10))
