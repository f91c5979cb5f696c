"""Randomised differential tests: seeded random byte texts -- delimiters, digits, letters,
'\\r', embedded NULs, bytes >= 0x80, over-long tokens, lines past the 20-emit cap, empty
lines -- through every engine path, against the independent Python oracle.  The CPU
engine is checked here on every run; the GPU paths (lean dictionary job, radix path,
reference-layout map, stage-split and graph modes) on the GPU box.  The word job, the
inverted index (``run_index``) and the top-K selection (``run_top``) all see the same texts;
every comparison is exact."""
import functools
import random

import pytest

import locust_amd as lc
from locust_amd.utils import oracle
from test_index import TEXTS as INDEX_TEXTS, random_text as index_random_text

LETTERS = b"abcdefghijklmnopqrstuvwxyzABCDEFGH0123456789"
DELIMS = b" ,.-;:'()\"\t"
ODD = b"\r\x00\x80\xc3\xa9\xff\x7f"


def random_text(rng: random.Random, size: int, fresh: float = 0.4) -> bytes:
    """fresh: share of words drawn at random (the rest from a 300-word vocabulary)."""
    out = bytearray()
    while len(out) < size:
        r = rng.random()
        if r < 0.06:
            out += b"\n"
        elif r < 0.30:
            out += bytes([rng.choice(DELIMS)]) * rng.randint(1, 3)
        elif r < 0.33:
            out += bytes([rng.choice(ODD)])
        elif r < 0.35:  # an over-long token (truncated at the key width)
            out += bytes(rng.choice(LETTERS) for _ in range(rng.randint(30, 80)))
        elif r < 0.37:  # a long line: more than 20 tokens
            out += b" ".join(bytes([rng.choice(LETTERS)]) * rng.randint(1, 3)
                             for _ in range(rng.randint(21, 60)))
        else:  # a word from a small vocabulary (repeats) or a random one
            if rng.random() >= fresh:
                out += b"w%d" % rng.randint(0, 300)
            else:
                out += bytes(rng.choice(LETTERS) for _ in range(rng.randint(1, 12)))
    return bytes(out[:size])


SIZES = [1, 2, 17, 300, 4095, 4096, 4097, 65536, 200_000]


def cases(n_seeds):
    for seed in range(n_seeds):
        rng = random.Random(1000 + seed)
        for size in SIZES:
            yield seed, size, random_text(rng, size)


@pytest.mark.parametrize("seed", range(4))
def test_cpu_engine_matches_oracle(seed):
    rng = random.Random(1000 + seed)
    for size in SIZES[:-1]:
        text = random_text(rng, size)
        ent, ntok, _ = oracle.wordcount(text)
        r = lc.wordcount_text(text, backend="cpu")
        assert r.num_tokens == ntok, (seed, size)
        assert r.entries() == ent, (seed, size)


# ------------------------------------------------------------------------------------
# inverted index and top-K: the same texts, and test_index.py's line generator (a 40-word
# vocabulary with keys up to 35 bytes, delimiter runs, NULs; with and without a final newline)
# ------------------------------------------------------------------------------------
TOP_KS = (1, 10, 1000)


def oracle_kw(kw):
    """The oracle's names for a configuration's job parameters."""
    names = {"emits_per_line": "emits", "max_key_len": "max_key"}
    out = {names[k]: v for k, v in kw.items() if k in names}
    if "delimiters" in kw:
        out["delims"] = kw["delimiters"].encode()
    return out


def cfg_id(kw):
    return "-".join(f"{k}={v!r}" for k, v in kw.items()) or "default"


def index_texts():
    for seed, final_newline in INDEX_TEXTS:
        yield seed, ("lines", final_newline), index_random_text(seed, 120, final_newline)


@functools.lru_cache(maxsize=None)
def all_texts(n_seeds):
    """[(seed, size, text)]: cases(n_seeds) and the 12 line texts, built once per session."""
    return tuple(cases(n_seeds)) + tuple(index_texts())


@functools.lru_cache(maxsize=None)
def cpu_texts(seed):
    rng = random.Random(1000 + seed)
    out = [(seed, size, random_text(rng, size)) for size in SIZES[:-1]]
    return tuple(out) + tuple(t for t in index_texts() if t[0] % 4 == seed)


def check_index(got, text, first_line, okw, ident):
    """An IndexResult against oracle.index and the counters of oracle.wordcount."""
    ent, post = oracle.index(text, first_line=first_line, **okw)
    _e, ntok, over, trunc = oracle.wordcount(text, stats=True, **okw)
    assert got.entries() == ent, ident
    assert got.postings() == post, ident
    assert (got.num_tokens, got.num_unique) == (len(post), len(ent)), ident
    assert ntok == len(post), ident
    assert got.first_line == first_line, ident
    assert (got.overflow_lines, got.truncated) == (over, trunc), ident
    return ent


CPU_CONFIGS = [dict(), dict(emits_per_line=3, max_key_len=5, delimiters="ae \t")]


@pytest.mark.parametrize("kw", CPU_CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("seed", range(4))
def test_cpu_index_and_top_match_oracle(seed, kw):
    cfg = lc.make_config("cpu", check=True, **kw)
    okw = oracle_kw(kw)
    for i, (s, size, text) in enumerate(cpu_texts(seed)):
        ident = (s, size, kw)
        first_line = 7 * (i & 1)
        ent = check_index(lc._C.cpu_run_index(cfg, text, first_line), text, first_line, okw, ident)
        assert ent == oracle.wordcount(text, **okw)[0], ident
        for k in TOP_KS:
            assert lc._C.cpu_run_top(cfg, text, k).entries() == oracle.top(ent, k), ident + (k,)


GPU_PATHS = [
    dict(),                                           # lean dictionary job
    dict(graph=0),                                    # stage events
    dict(graph=1),                                    # graph replay
    dict(sort="radix"),                               # the reference's algorithm
    dict(sort="radix", reduce_path="global"),
    dict(map_path="compat", sort="dict"),             # the reference's map layout
]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", GPU_PATHS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_gpu_paths_match_oracle(opts):
    for seed, size, text in cases(3):
        ent, ntok, _ = oracle.wordcount(text)
        r = lc.wordcount_text(text, backend="gpu", check=True, **opts)
        assert r.num_tokens == ntok, (seed, size, opts)
        assert r.entries() == ent, (seed, size, opts)


@pytest.mark.gpu
def test_gpu_engine_reused_across_random_texts():
    """One engine, many different texts back to back (buffer pool, self-cleaning scratch,
    partition-map retunes between unrelated inputs)."""
    rng = random.Random(77)
    eng = lc._C.GpuEngine(lc.make_config("gpu", check=True), 300_000, 300_000)
    for _ in range(30):
        text = random_text(rng, rng.choice([100, 5000, 60_000, 250_000]))
        assert eng.run(text).entries() == oracle.wordcount(text)[0]


INDEX_CONFIGS = [
    dict(),
    dict(delimiters="ae \t"),                         # letters as delimiters
    dict(emits_per_line=1),
    dict(emits_per_line=3, max_key_len=5),
    dict(emits_per_line=100),                         # the cap is (almost) never reached
] + [dict(max_key_len=m) for m in (1, 8, 9, 16, 24, 31)]  # the key words' edges; 31: the longest


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kw", INDEX_CONFIGS, ids=cfg_id)
def test_gpu_index_matches_oracle(kw):
    """The index stage's own tokenizer (index_map_kernel) against the oracle, and so against
    the map's: one engine per configuration, every text through it back to back."""
    eng = lc.Engine(lc.make_config("gpu", check=True, **kw), 300_000, 300_000)
    okw = oracle_kw(kw)
    for i, (seed, size, text) in enumerate(all_texts(3)):
        first_line = 7 * (i & 1)
        check_index(eng.run_index(text, first_line), text, first_line, okw, (seed, size, kw))


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kw", [dict(), dict(emits_per_line=3, max_key_len=5)], ids=cfg_id)
def test_gpu_top_matches_oracle(kw):
    eng = lc.Engine(lc.make_config("gpu", check=True, **kw), 300_000, 300_000)
    okw = oracle_kw(kw)
    for seed, size, text in all_texts(3):
        ent, ntok, _ = oracle.wordcount(text, **okw)
        for k in TOP_KS:
            t = eng.run_top(text, k)
            assert t.entries() == oracle.top(ent, k), (seed, size, kw, k)
            assert (t.num_tokens, t.num_unique) == (ntok, len(ent)), (seed, size, kw, k)


@pytest.mark.gpu
def test_gpu_large_random_pass_matches_cpu_engine():
    """A ~12 MB random text with a bounded vocabulary: upload pieces, per-piece partials and
    the two-kernel ordered build (first job on the default partition map, then retuned),
    against the CPU engine (itself checked against the oracle above)."""
    rng = random.Random(5)
    parts, size = [], 0
    while size < 12 << 20:
        chunk = random_text(rng, 256 << 10, fresh=0.002)
        chunk = chunk[: chunk.rfind(b"\n") + 1] or b"x\n"
        parts.append(chunk)
        size += len(chunk)
    text = b"".join(parts)
    want = lc._C.cpu_run(lc.make_config("cpu"), text).entries()
    eng = lc._C.GpuEngine(lc.make_config("gpu", check=True), len(text), text.count(b"\n") + 1)
    for _ in range(3):
        assert eng.run(text).entries() == want
    # the same through the distributed shuffle on one RCCL rank (asynchronous map)
    dcfg = lc.make_dist_config(1, lc.make_config("gpu", combine=True), strategy="shuffle")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dr = lc._C.DistRank(dcfg, 0, "rccl", "127.0.0.1", port, len(text), text.count(b"\n") + 1,
                        60.0)
    for _ in range(3):
        res, _info = dr.run(text, 0)
        assert res.entries() == want
