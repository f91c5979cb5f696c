"""The lean job's epilogue (dict.hip ordered_partition, psort.hip reduce_tail): every wave
waits for its stores, the workgroup releases them and counts itself done, and the workgroup
whose count is last tells the host with a relaxed store -- nothing orders that store behind
the other workgroups' records but their own waited-for write-backs.  (Written with the
fence-free, write-through form of that epilogue, which these tests passed and the benchmark
did not: docs/PERFORMANCE.md, "Write-through tail".)  A word that is not out when the host
is told shows up as a wrong, missing or left-over entry, so every job here is compared
entry by entry with the independent oracle, at the smallest shapes where that can happen:

  minimal    one token: 255 empty partitions and one single-word record -- the workgroup
             that tells the host is almost never the one with data
  widths     256 distinct keys of 1..32 bytes: compact records of every width (1-5 words),
             records straddling 64-byte lines, >= 200 partitions of the default map in use
  hot        4,000 copies of one 9-byte word + 50 words sharing its first two bytes: one
             partition finishes far behind the other 255 (uneven load)
  stale      400 back-to-back jobs alternating two texts of different token and key
             totals, each result held until the next returns (the two output buffers
             alternate): anything left over from the previous job is a mismatch

each on the dictionary path (the ordered kernel) and with sort="radix" (the fused
partitioned sort)."""
import bisect

import pytest

import locust_amd as lc
from locust_amd.utils import oracle

pytestmark = pytest.mark.gpu

SORTS = ["dict", "radix"]


def _default_map_cuts():
    """The (first byte, second byte) lower bounds of the default partition map's ranges
    (csrc/engine/partmap.cpp part_map_default), restated to count the partitions in use."""
    cuts = [(0x00, 0)] + [(d, 0) for d in range(ord("0"), ord("9") + 1)] + [(0x3A, 0)]
    for c in range(ord("A"), ord("Z") + 1):
        cuts += [(c, 0), (c, ord("a")), (c, ord("n"))]
    cuts.append((0x5B, 0))
    for c in range(ord("a"), ord("z") + 1):
        cuts += [(c, 0), (c, ord("g")), (c, ord("n")), (c, ord("t"))]
    cuts.append((0x7B, 0))
    cuts += [(b, 0) for b in range(0xC2, 0xF5)] + [(0xF5, 0)]
    assert len(cuts) == 248 and cuts == sorted(cuts)
    return cuts


def _partition(cuts, key: bytes) -> int:
    return bisect.bisect_right(cuts, (key[0], key[1] if len(key) > 1 else 0)) - 1


def _widths_text() -> bytes:
    cuts = _default_map_cuts()
    # one two-byte prefix inside each range that a key can start with (no delimiter, NUL or
    # newline: the first range, controls and punctuation, is left out; ':' ';' -> '<')
    prefixes = [bytes([b0 + 2 if b0 == 0x3A else b0, b1 if b1 else ord("0")])
                for b0, b1 in cuts[1:]]
    assert not any(c in oracle.DEFAULT_DELIMS + b"\n\0" for p in prefixes for c in p)
    keys = []
    for i in range(256):
        n = i % 32 + 1  # 1 .. 32 bytes (the engine keeps the first 29)
        keys.append((prefixes[i % len(prefixes)] + b"%03d" % i + b"x" * 32)[:n])
    assert len({k[:29] for k in keys}) == 256  # distinct after truncation too
    assert len({_partition(cuts, k) for k in keys}) >= 200
    return b"".join(k + b"\n" for k in keys)


def _hot_text() -> bytes:
    hot = b"thundered"  # 9 bytes
    near = [b"th" + b"%c%c" % (97 + i // 26, 97 + i % 26) + b"q" * (i % 7) for i in range(50)]
    assert len(set(near)) == 50 and hot not in near
    words = [hot] * 4000 + near
    # the distinct words spread through the text, ten words a line
    words = [w for i in range(81) for w in words[i::81]]
    return b"".join(b" ".join(words[i:i + 10]) + b"\n" for i in range(0, len(words), 10))


def _texts():
    return {"minimal": b"a\n", "widths": _widths_text(), "hot": _hot_text()}


@pytest.fixture(scope="module")
def expected():
    """Each text's oracle result, computed once: (entries, tokens)."""
    out = {}
    for name, text in {**_texts(), **dict(zip("AB", _stale_texts()))}.items():
        ent, ntok, _ = oracle.wordcount(text)
        out[name] = (ent, ntok)
    return out


def _stale_texts():
    a = b"".join(b"alpha beta gamma delta w%03d x%02d\n" % (i, i % 37) for i in range(300))
    b = b"".join(b"beta delta epsilon w%03d yy%03d z%d zeta eta\n" % (i, 2 * i, i % 11)
                 for i in range(170))
    return a, b


def _engine(sort: str, nbytes: int, nlines: int):
    return lc._C.GpuEngine(lc.make_config("gpu", sort=sort), nbytes, nlines)


def _check(r, want, what):
    ent, ntok = want
    assert r.num_tokens == ntok, what
    assert r.num_unique == len(ent), what
    got = r.entries()
    assert len(got) == len(ent), what
    for i, (g, w) in enumerate(zip(got, ent)):
        assert g == w, f"{what}: entry {i} is {g!r}, the oracle has {w!r}"


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("name", ["minimal", "widths", "hot"])
def test_shape_matches_oracle(expected, name, sort):
    text = _texts()[name]
    eng = _engine(sort, len(text) + 1, text.count(b"\n") + 1)
    for j in range(4):  # the first job plans / tunes, later ones run on the retuned map
        r = eng.run(text)
        _check(r, expected[name], f"{name}, sort={sort}, job {j}")
    assert r.times()["graph"] is False  # the lean job: the kernel tells the host itself


@pytest.mark.parametrize("sort", SORTS)
def test_alternating_jobs_leave_nothing_behind(expected, sort):
    a, b = _stale_texts()
    ea, eb = expected["A"], expected["B"]
    assert ea[1] != eb[1] and len(ea[0]) != len(eb[0])  # token and key totals differ
    eng = _engine(sort, max(len(a), len(b)) + 1, max(a.count(b"\n"), b.count(b"\n")) + 1)
    held = None  # the previous result stays alive: its output buffer is not reused yet
    for j in range(400):
        r = eng.run(b if j & 1 else a)
        _check(r, eb if j & 1 else ea, f"sort={sort}, job {j} ({'AB'[j & 1]})")
        held = r
    assert held is not None and held.times()["graph"] is False
