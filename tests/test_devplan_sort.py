"""The device-planned radix sort (radix_sort.hip with sync_plan=False) and its pass schedule.

With ``sync_plan=False`` the sort never learns n or the live digit positions on the host:
it launches the single-workgroup kernel, the histogram and plan kernels, all four word
gathers, all 32 passes over a grid sized for the engine's capacity, and the final gather;
every kernel then decides on the device whether it is live and which ping-pong buffer it
reads (``pass_src`` / ``word_src`` / ``final_src``, locust/device/radix_sched.hpp).

* CPU: the three parity functions against a Python model of the documented pass order
  (words 3..0, bytes 7..0, buffer 0 first, buffer 2 = identity), and a self-check of the
  key generator below.
* GPU: ``sort_keys`` (with counts, so the fused count gathers run too) on engines built
  with ``sync_plan=False``, compared exactly with Python's stable sort: every combination
  of {dead, odd, even} live-byte counts over the four key words, sizes around the
  single-workgroup threshold, the look-back batch and the engine's exact capacity, stale
  plans on a reused engine, agreement with the host planner, and ``reduce_stage``.

Every GPU test asserts ``stats()["process_path"]``, so none can pass on another path."""
import functools
import itertools
import random

import pytest

import locust_amd as lc

gpu = pytest.mark.gpu

DEV, HOST = "radix-device-plan", "radix-host-plan"

# cap = 2^17 / 2 + 1 = 65,537 records = 16 tiles of 4,096 keys + 1 key
ENG_BYTES, ENG_LINES, ENG_CAP = 1 << 17, 1 << 13, 65537


# ---------------------------------------------------------------------------------------
# The pass schedule (CPU)
# ---------------------------------------------------------------------------------------
def check_schedule(act):
    """The documented pass order, replayed: which buffer each live step must read."""
    word_src, pass_src, final_src = lc._C.radix_schedule(act)
    assert len(word_src) == 4 and len(pass_src) == 32
    holder = 2  # the identity permutation
    for w in (3, 2, 1, 0):
        if not (act >> (8 * w)) & 0xff:
            continue
        assert word_src[w] == holder, (hex(act), w)
        cur = 0  # the word's gather writes buffer 0
        for b in range(7, -1, -1):
            if (act >> (8 * w + b)) & 1:
                assert pass_src[8 * w + b] == cur, (hex(act), w, b)
                cur ^= 1
        holder = cur
    assert final_src == holder, hex(act)


OTHERS = (0x00, 0x10, 0x81, 0x07, 0xff)


@pytest.mark.parametrize("w", range(4))
def test_schedule_matches_pass_order_model(w):
    """All 256 live patterns of word w, crossed with the other three words from OTHERS
    (dead, one pass, two, three, eight): 32,000 masks per word."""
    rest = [v for v in range(4) if v != w]
    for pat in range(256):
        for others in itertools.product(OTHERS, repeat=3):
            act = pat << (8 * w)
            for v, o in zip(rest, others):
                act |= o << (8 * v)
            check_schedule(act)


def test_schedule_no_live_and_all_live():
    check_schedule(0)
    assert lc._C.radix_schedule(0)[2] == 2  # nothing to sort: the identity permutation
    check_schedule(0xffffffff)
    word_src, pass_src, final_src = lc._C.radix_schedule(0xffffffff)
    # eight passes end in the buffer they began in, 0; word 3 starts from the identity
    assert word_src == [0, 0, 0, 2] and final_src == 0
    assert pass_src == [1, 0] * 16


# ---------------------------------------------------------------------------------------
# Key families by live mask
# ---------------------------------------------------------------------------------------
KINDS = ("dead", "odd", "even")
COMBOS = [c for c in itertools.product(KINDS, repeat=4) if any(k != "dead" for k in c)]
assert len(COMBOS) == 80
FAMILY_NS = (8193, 9000, 12289, 16384)
LIVE_BYTES = b"\x01a\x80\xff"  # no NUL, both sides of 0x80; four values: many equal keys


def combo_id(combo):
    return "".join(k[0] for k in combo)  # word 0 first: d / o / e


def family_mask(idx):
    """Live key-byte positions (= digit positions: bit 8w + b is byte b of word w) of
    family idx: per word none, 1 or 3 (odd), or 2 or 4 (even) of its eight bytes."""
    rng = random.Random(1000 + idx)
    mask = set()
    for w, kind in enumerate(COMBOS[idx]):
        if kind == "dead":
            continue
        cnt = rng.choice((1, 3) if kind == "odd" else (2, 4))
        mask |= {8 * w + b for b in rng.sample(range(8), cnt)}
    return mask


@functools.lru_cache(maxsize=4)
def family(idx, full):
    """(keys, mask, n) of family idx.  Short form: keys end with their highest live word, so
    the words above it are zero (the histogram's zero-word branch).  full: every key is 32
    bytes.  Dead bytes are a constant 'm'; live bytes are drawn from LIVE_BYTES."""
    mask = family_mask(idx)
    n = 8193 if full else FAMILY_NS[idx % 4]
    length = 32 if full else 8 * (max(mask) // 8 + 1)
    live = sorted(mask)
    rng = random.Random(5000 + idx)
    keys = []
    for _ in range(n):
        k = bytearray(b"m" * length)
        bits = rng.getrandbits(2 * len(live))
        for j, p in enumerate(live):
            k[p] = LIVE_BYTES[(bits >> (2 * j)) & 3]
        keys.append(bytes(k))
    return keys, mask, n


@pytest.mark.parametrize("full", [False, True], ids=["short", "full"])
def test_families_have_their_masks(full):
    """Generator self-check: in every family exactly the intended positions hold more than
    one byte value (so the plan kernel finds exactly that live mask), every combination
    is what it says, and equal keys abound (so stability is tested)."""
    for idx, combo in enumerate(COMBOS):
        keys, mask, n = family(idx, full)
        assert len(keys) == n
        length = 32 if full else 8 * (max(mask) // 8 + 1)
        assert all(len(k) == length and 0 not in k for k in keys)
        varying = {p for p in range(length) if len({k[p] for k in keys}) > 1}
        assert varying == mask, (idx, combo)
        for w, kind in enumerate(combo):
            cnt = sum(1 for p in mask if p // 8 == w)
            assert {"dead": cnt == 0, "odd": cnt in (1, 3), "even": cnt in (2, 4)}[kind]
        if len(mask) <= 6:
            assert len(set(keys)) < n


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def make_engine(sync_plan, **kw):
    kw.setdefault("sort", "radix")
    eng = lc.Engine(lc.make_config("gpu", sync_plan=sync_plan, **kw), ENG_BYTES, ENG_LINES)
    assert eng.capacity == ENG_CAP
    return eng


@pytest.fixture(scope="module")
def dev_eng():
    return make_engine(False)


@pytest.fixture(scope="module")
def host_eng():
    return make_engine(True)


def counts_for(n):
    """Distinct per index, all 64 bits in use (an odd multiplier permutes Z / 2^64)."""
    return [(i * 0x9E3779B97F4A7C15 + 0x0123456789ABCDEF) & (2 ** 64 - 1) for i in range(n)]


def check_sort(eng, keys, path, ref=None, with_counts=True):
    """One sort_keys call against Python's stable sort (the one right permutation)."""
    n = len(keys)
    if ref is None:
        ref = sorted(range(n), key=keys.__getitem__)
    if with_counts:
        counts = counts_for(n)
        got, perm, got_counts = eng.sort_keys(keys, counts)
    else:
        got, perm = eng.sort_keys(keys)
    assert eng._eng.stats()["process_path"] == path
    assert list(perm) == ref
    assert got == [keys[i] for i in ref]
    if with_counts:
        assert list(got_counts) == [counts[i] for i in ref]
    return got, list(perm)


@gpu
@pytest.mark.parametrize("idx", range(80), ids=[combo_id(c) for c in COMBOS])
def test_live_mask_families(dev_eng, idx):
    """Every parity of live passes per word, with dead and zero words between."""
    keys, _mask, _n = family(idx, False)
    check_sort(dev_eng, keys, DEV)


@gpu
@pytest.mark.parametrize("idx", range(80), ids=[combo_id(c) for c in COMBOS])
def test_live_mask_families_full_length(dev_eng, idx):
    """The same masks with no zero word: dead words are constant and non-zero."""
    keys, _mask, _n = family(idx, True)
    check_sort(dev_eng, keys, DEV)


def random_keys(n, seed):
    rng = random.Random(seed)
    return [bytes(rng.choice(b"aZ09\x80\xff~") for _ in range(rng.randint(1, 32)))
            for _ in range(n)]


@functools.lru_cache(maxsize=None)
def big_case():
    """36,865 keys (nine tiles + 1: the look-back runs past one batch of 8) and their
    reference permutation, shared by the tests that need them and never modified."""
    keys = random_keys(36865, 36865)
    return keys, sorted(range(len(keys)), key=keys.__getitem__)


@gpu
@pytest.mark.parametrize("n", [0, 1, 2, 8191, 8192, 8193, 36865, 65537])
def test_sizes_under_device_plan(dev_eng, n):
    """Through 8,192 the single-workgroup kernel sorts and every launched multi-tile kernel
    must leave its output alone; 65,537 is the engine's exact capacity (every launched tile
    live, one key in the last)."""
    keys, ref = big_case() if n == 36865 else (random_keys(n, n), None)
    check_sort(dev_eng, keys, DEV, ref)
    check_sort(dev_eng, keys, DEV, ref, with_counts=False)


@gpu
def test_all_equal_keys_are_identity(dev_eng):
    """No live position at all: the final gather reads the identity (final_src = 2)."""
    _got, perm = check_sort(dev_eng, [b"same"] * 9000, DEV)
    assert perm == list(range(9000))


@gpu
def test_descending_keys(dev_eng):
    keys = sorted((b"k%08d" % i for i in range(8193)), reverse=True)
    _got, perm = check_sort(dev_eng, keys, DEV)
    assert perm == list(range(8192, -1, -1))


@gpu
def test_stale_plan_on_reused_engine():
    """One engine, four sorts: a small sort leaves the previous large sort's plan->pass[]
    in place, and a large one after another mask must read only its own."""
    eng = make_engine(False)
    big, big_ref = big_case()
    check_sort(eng, big, DEV, big_ref)
    keys, _mask, n = family(44, False)  # another live mask, two tiles + 1 key
    assert n == 8193
    check_sort(eng, keys, DEV)
    check_sort(eng, random_keys(5000, 5), DEV)  # single workgroup: plan->pass[] untouched
    check_sort(eng, big, DEV, big_ref)


@gpu
def test_both_planners_agree(dev_eng, host_eng):
    big, big_ref = big_case()
    cases = [(family(i, False)[0], None) for i in (7, 40, 79)] + [(big, big_ref)]
    for keys, ref in cases:
        a = check_sort(dev_eng, keys, DEV, ref)
        b = check_sort(host_eng, keys, HOST, ref)
        assert a == b, len(keys)


@gpu
@pytest.mark.parametrize("reduce_path", ["lds", "global"])
@pytest.mark.parametrize("n", [8193, 36865])
def test_reduce_stage_device_plan(reduce_path, n):
    """reduce_stage sorts its (shuffled) input with the device-planned sort first."""
    from test_kernels import runs_reference

    rng = random.Random(n)
    pool = [bytes(rng.choice(b"abcdefghij\x80\xfe") for _ in range(rng.randint(1, 29)))
            for _ in range(n // 7)]
    keys = [rng.choice(pool) for _ in range(n)]
    eng = make_engine(False, reduce_path=reduce_path)
    r = eng.reduce_stage(keys)
    assert eng._eng.stats()["process_path"] == DEV
    want = runs_reference(sorted(keys))
    assert r.entries() == want
    assert r.num_unique == len(set(keys)) == len(want)
    assert r.num_tokens == n
