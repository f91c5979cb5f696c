"""The reference of the dictionary stage tests (tests/dict_ref.py) against brute force, the
conditions its inputs must meet (computed here, never measured on the device), and the
refusals of the stage entry points, which all come before any device call.  No GPU."""
import random

import pytest

import locust_amd as lc

import dict_ref as ref

C = lc._C
K = ref.K
pad = ref.pad


def small_keys(rng, n, alphabet=b"ab\x80\xff", maxlen=3):
    return [pad(bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, maxlen + 1))))
            for _ in range(n)]


# ---------------------------------------------------------------------------------------
# the reference against brute force
# ---------------------------------------------------------------------------------------

def test_constants_are_the_kernels():
    assert K["kLdsSlots"] == 1024 and K["kLdsProbes"] == 8
    assert K["kPartSlots"] == 2048 and K["kPartProbes"] == 512 and K["kPartWindow"] == 16384
    assert K["kPlanSamples"] == 8192 and K["kSingletonWeight"] == 9
    assert K["kRankI"] == 256 and K["kPackTile"] == 2048 and K["kRankSortMax"] == 32768
    assert K["kWordMagic"] == 0x0000FFFF0000FFFF and K["kDictParts"] == 256
    assert K["kCtrDictOverflow"] == C.ctr_dict_overflow_flag()


@pytest.mark.parametrize("seed", range(5))
def test_aggregate_and_ranks_brute_force(seed):
    rng = random.Random(seed)
    keys = small_keys(rng, 60) + [ref.ZERO_KEY] * 3
    rng.shuffle(keys)
    counts = [rng.choice((0, 1, 2, 1 << 40)) for _ in keys]
    want = {}
    for k, c in zip(keys, counts):
        if k != ref.ZERO_KEY and c:
            want[k] = want.get(k, 0) + c
    assert ref.aggregate(keys, counts) == want
    assert ref.aggregate(keys) == {k: keys.count(k) for k in set(keys) if k != ref.ZERO_KEY}
    rank, val = ref.ranks(keys, counts)
    for i, k in enumerate(keys):
        smaller = [j for j in range(len(keys)) if ref.words(keys[j]) < ref.words(k)]
        assert rank[i] == len(smaller)
        assert val[i] == sum(counts[j] for j in smaller)
    assert ref.ranks(keys)[1] == [0] * len(keys)


def test_byte_order_is_word_order_unsigned():
    keys = [pad(b"a"), pad(b"a\x7f"), pad(b"a\x80"), pad(b"a\xff"), pad(b"b"), pad(b"\x80")]
    assert sorted(keys) == sorted(keys, key=ref.words)
    assert ref.ranks(keys)[0] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("seed", range(4))
def test_emit_scatter_scan_pack_brute_force(seed):
    rng = random.Random(seed)
    keys = list(dict.fromkeys(small_keys(rng, 40)))
    counts = [rng.randrange(1, 1 << 40) for _ in keys]
    u = len(keys)
    rank, val = ref.ranks(keys, counts)
    ctr = {f: 10 + i for i, f in enumerate(ref.CTR_FIELDS)}
    ctr["num_unique"] = u
    recs, out = ref.emit(keys, counts, rank, val, ctr, u + 2)
    assert recs == sorted(zip(keys, counts))
    assert out["total_count"] == sum(counts) and out["num_unique"] == u
    assert all(out[f] == ctr[f] for f in ref.CTR_FIELDS if f not in ("num_unique", "total_count"))
    skeys, scounts = ref.scatter(keys, counts, rank, u, u + 2)
    assert list(zip(skeys[:u], scounts[:u])) == recs
    assert skeys[u:] == [ref.PATTERN_KEY] * 2 and scounts[u:] == [ref.PATTERN_U64] * 2
    recs2, total, out2 = ref.scan_pack(skeys, scounts, u, u)
    assert recs2 == recs and total == sum(counts) and out2["total_count"] == total
    recs3, total3, out3 = ref.scan_pack(skeys, scounts, u, u - 1, {"flags": 4})
    assert recs3 is None and total3 is None
    assert out3["flags"] == 4 | ref.NOT_EMITTED and out3["total_count"] == ref.PATTERN_U64
    assert ref.scan_pack([], [], 0, 0)[1:] == (None, ref.ctr_out_of({}, 0, 0, 0))
    # clamp, empty, and above the rank sort's limit
    assert ref.emit(keys, counts, rank, val, dict(ctr, num_unique=u + 9), u)[1]["num_unique"] == u
    assert ref.emit([], [], [], [], {"num_unique": 0}, 0)[1]["total_count"] == 0
    none, out4 = ref.emit([], [], [], [], {"num_unique": ref.RANK_MAX + 1}, ref.RANK_MAX + 1)
    assert none is None and out4["flags"] == ref.NOT_EMITTED
    assert out4["total_count"] == ref.PATTERN_U64


def plan_brute_force(w0, counts, d_u, ucap):
    """Range q starts at the first sample (in first-word order) whose inclusive weight
    prefix reaches past the quantile: the smallest e with (pre_e + w_e) * 256 // W >= q."""
    U = min(d_u, ucap)
    S = min(U, K["kPlanSamples"])
    smp = sorted((w0[i * U // S], K["kSingletonWeight"] if counts[i * U // S] == 1 else 1)
                 for i in range(S))
    W = sum(w for _, w in smp)
    lo = [0] + [q << 56 for q in range(1, 256)] + [ref.M64]
    if W:
        for q in range(1, 256):
            acc = 0
            for k, w in smp:
                acc += w
                if acc * 256 // W >= q:
                    lo[q] = k
                    break
    return lo


@pytest.mark.parametrize("U", [0, 1, 2, 3, 200, 255, 256, 257, 700])
@pytest.mark.parametrize("kind", ["ones", "twos", "zipf"])
def test_part_plan_brute_force(U, kind):
    w0, counts = ref.plan_input(U, kind)
    lo = ref.part_plan(w0, counts, U, U)
    assert lo == plan_brute_force(w0, counts, U, U)
    assert lo[0] == 0 and lo[256] == ref.M64 and lo == sorted(lo)
    if U == 0:
        assert lo[1:256] == [q << 56 for q in range(1, 256)]


def test_part_plan_stride_and_clamp():
    w0, counts = ref.plan_input(20000, "zipf")
    lo = ref.part_plan(w0, counts, 20000, 20000)
    assert lo == sorted(lo)
    # the samples are elements i * U // S: every other one or so, not the first 8,192
    assert lo != ref.part_plan(w0[:8192], counts[:8192], 8192, 8192)
    assert ref.part_plan(w0, counts, 20009, 20000) == lo
    assert ref.part_plan(w0, counts, 20000, 9000) == ref.part_plan(w0[:9000], counts[:9000], 9000, 9000)


@pytest.mark.parametrize("U", [0, 1, 2, 255, 256, 257, 8191, 8192, 8193, 20000])
def test_part_plan_ascends_and_ignores_tie_order(U):
    for kind in ("ones", "twos", "zipf"):
        w0, counts = ref.plan_input(U, kind)
        # ties: every first word four times, with different counts
        w0t = [w0[i // 4] for i in range(U)]
        lo = ref.part_plan(w0t, counts, U, U)
        assert lo == sorted(lo)
        for seed in range(3):
            assert ref.part_plan(w0t, counts, U, U, tie_rng=random.Random(seed)) == lo
        assert ref.part_plan(w0, counts, U, U) == sorted(ref.part_plan(w0, counts, U, U))


def test_part_plan_weights_matter():
    """All counts 1 and all counts 2 give the same plan (equal weights); a mix does not: the
    singleton weight moves the cuts."""
    w0, _ = ref.plan_input(2000, "ones")
    ones = ref.part_plan(w0, [1] * 2000, 2000, 2000)
    assert ones == ref.part_plan(w0, [2] * 2000, 2000, 2000)
    order = sorted(range(2000), key=lambda i: w0[i])
    mixed = [0] * 2000
    for r, i in enumerate(order):
        mixed[i] = 1 if r < 1000 else 2
    assert ref.part_plan(w0, mixed, 2000, 2000) != ones


def test_hash_port_table_rules():
    rng = random.Random(5)
    for slots in (4, 64):
        for _ in range(50):
            homes = [rng.randrange(slots) for _ in range(rng.randrange(0, slots + 1))]
            occ = ref.occupied(homes, slots)
            assert len(occ) == len(homes)
            for seed in range(3):  # any arrival order: the same slots
                sh = homes[:]
                random.Random(seed).shuffle(sh)
                assert ref.occupied(sh, slots) == occ
            runs = "".join("x" if s in occ else "." for s in range(slots))
            want = max(map(len, (runs + runs).split("."))) if len(occ) < slots else slots
            assert ref.longest_cluster(occ, slots) == min(want, slots)
    assert ref.occupied([3, 3, 3], 4) == {3, 0, 1}
    # mix64 is the 64-bit finaliser of MurmurHash3: its published fixed points
    assert ref.mix64(0) == 0 and ref.mix64(1) == 0xB456BCFC34C2CB2C


# ---------------------------------------------------------------------------------------
# the inputs of test_dict_stage_kernels.py
# ---------------------------------------------------------------------------------------

def test_families_are_valid_distinct_keys_with_high_bytes():
    for f in ref.FAMILIES:
        for m in (1, 2, 255, 256, 257, 511, 513, 4097):
            keys = ref.family(f, m)
            assert len(set(keys)) == m
            assert all(ref.valid_key(k) and C.dict_valid_key(k) for k in keys[:300])
    assert any(b >= 0x80 for k in ref.family("edges", 600) for b in k)
    for f in ("tie8", "tie16", "tie24"):  # equal in word 0, and up to the word they name
        n = int(f[3:])
        assert len({k[:n] for k in ref.family(f, 600)}) == 1
    assert len(set(ref.family("short", 32769, b"w"))) == 32769
    for m in (1500, 2049, 5000):
        assert len(set(ref.part_keys(m))) == m
        assert {k[:1] for k in ref.part_keys(m)} == {b"p"}


def test_valid_key_rule():
    good = [ref.ZERO_KEY, pad(b"a"), pad(b"a" * 8), pad(b"a" * 9), b"\xa5" * 32, pad(b"\xff" * 31)]
    bad = [b"a\0b" + bytes(29), bytes(8) + b"a" + bytes(23), b"a" * 8 + bytes(8) + b"b" + bytes(15),
           bytes(31) + b"x", pad(b"a" * 8) [:8] + (K["kWordMagic"]).to_bytes(8, "big") + bytes(16)]
    for k in good:
        assert ref.valid_key(k) and C.dict_valid_key(k), k
    for k in bad:
        assert not ref.valid_key(k) and not C.dict_valid_key(k), k
    # no word of a valid key equals kWordMagic (a NUL, then non-NUL bytes)
    assert not ref.valid_key(bytes(8) + K["kWordMagic"].to_bytes(8, "big") + bytes(16))


def test_equal_hash_pairs_hash_identically():
    keys = ref.equal_hash_pairs()
    assert len(set(keys)) == len(keys) == 80
    for a, b in zip(keys[::2], keys[1::2]):
        assert a != b and ref.key_hash(a) == ref.key_hash(b)
        assert [x ^ y for x, y in zip(a, b)] == [0] * 24 + [0x80] + [0] * 7
        assert ref.words(a)[:3] == ref.words(b)[:3]


def test_wrap_keys_cross_the_table_end():
    keys = ref.wrap_keys()
    homes = [ref.hbm_slot(k, ref.WRAP_SLOTS) for k in keys]
    assert len(set(keys)) == len(keys) == 14 and all(60 <= h <= 63 for h in homes)
    occ = ref.occupied(homes, ref.WRAP_SLOTS)
    assert len(occ) == 14 and 63 in occ and {0, 1, 2, 3} <= occ  # behind the end: slots 0..


def test_lds_collide_keys_share_one_cache_slot():
    keys = ref.lds_collide_keys()
    assert len(set(keys)) == len(keys) == K["kLdsProbes"] + 4
    assert len({ref.lds_slot(k) for k in keys}) == 1
    # and they do not all share their HBM slot: the spill is told from a stuck probe
    assert len({ref.hbm_slot(k, 64) for k in keys}) > 1


def test_part_capacity_conditions():
    # 1,500 keys of one partition: no cluster of its 2,048-slot table is longer than the
    # probe limit, so every key is placed whatever the arrival order
    assert ref.part_cluster(ref.part_keys(1500)) <= K["kPartProbes"]
    assert len(ref.part_keys(2049)) > K["kPartSlots"]
    # the tokens of the size cases: tags 0xA5 (the pattern byte) occur
    for n in (17, 16385, 40000):
        toks = ref.part_build_tokens(n)
        assert len(toks) == n and any(k[0] == ref.PATTERN for k in toks)
        for tag in (lambda k: k[0], ref.hash_tag):
            per = {}
            for k in set(toks):
                per.setdefault(tag(k), []).append(k)
            assert max(len(v) for v in per.values()) <= 1500
            assert max(ref.part_cluster(v) for v in per.values()) <= K["kPartProbes"]


def test_count_ranges():
    c = ref.big_counts(32768, 3)
    assert max(c) == 1 << 40 and min(c) == 1
    _, val = ref.ranks(list(ref.family("short", 4097)), ref.big_counts(4097, 3))
    assert (1 << 32) < max(val) and sum(c) < (1 << 62)
    for u in (1, 2047, 10000):
        sc = ref.scan_counts(u)
        assert (1 << 60) < sum(sc) < (1 << 61) + (1 << 60)
        assert all(sum(sc[i:i + K["kPackTile"]]) > (1 << 32) for i in range(0, u, K["kPackTile"]))


def test_insert_mix_has_repeats_of_every_family():
    toks = ref.insert_mix(5000)
    agg = ref.aggregate(toks)
    assert len(toks) == 5000 and 1000 < len(agg) < 5000 and max(agg.values()) > 1
    assert len(set(ref.part_keys(5000, b"w"))) == 5000 > K["kLdsSlots"] + K["kLdsProbes"]


# ---------------------------------------------------------------------------------------
# the refusals of the stage entry points (all before any device call)
# ---------------------------------------------------------------------------------------

BAD_KEY = b"a\0b" + bytes(29)
GOOD = ref.blob([pad(b"a"), pad(b"b"), pad(b"c")])


def refused(what, fn, *args):
    with pytest.raises(lc.LocustError, match=what):
        fn(*args)


def test_refusals_invalid_key():
    bad = GOOD + BAD_KEY
    refused("valid packed key", C.dict_insert, bad, None, 4, 4, 64, 8)
    refused("valid packed key", C.dict_part_build, bad, None, b"abca", 4, 4, 8)
    refused("valid packed key", C.dict_rank, bad, None, 4, 4)
    refused("valid packed key", C.dict_emit, bad, [1] * 4, [0, 1, 2, 3], [0] * 4, {"num_unique": 4}, 4)
    refused("valid packed key", C.dict_scatter, bad, [1] * 4, [0, 1, 2, 3], 4, 4)
    refused("valid packed key", C.dict_scan_pack, bad, [1] * 4, 4, 4)
    magic = pad(b"a" * 8)[:8] + K["kWordMagic"].to_bytes(8, "big") + bytes(16)
    refused("valid packed key", C.dict_insert, magic, None, 1, 1, 64, 8)


def test_refusals_insert_and_part_build_shapes():
    for slots in (0, 3, 48, 65):
        refused("power of two", C.dict_insert, GOOD, None, 3, 3, slots, 8)
    refused("one count per key", C.dict_insert, GOOD, [1, 2], 3, 3, 64, 8)
    refused("keys must be uploaded", C.dict_insert, GOOD, None, 4, 4, 64, 8)
    refused("within the guard", C.dict_insert, GOOD, None, 3 + K["kStageGuard"] + 1, 3, 64, 8)
    refused("workgroups", C.dict_insert, GOOD, None, 3, 3, 64, 8, 0)
    refused("one partition tag per key", C.dict_part_build, GOOD, None, b"ab", 3, 3, 8)
    refused("keys must be uploaded", C.dict_part_build, GOOD, None, b"abc", 5, 4, 8)
    refused("cap keys must be uploaded", C.dict_rank, GOOD, None, 3, 4)


def test_refusals_rank_permutation():
    for rank in ([0, 1, 1], [0, 1, 3], [1, 2, 3]):
        refused("permutation", C.dict_emit, GOOD, [1] * 3, rank, [0] * 3, {"num_unique": 3}, 3)
        refused("permutation", C.dict_scatter, GOOD, [1] * 3, rank, 3, 3)
    refused("one count, rank and val", C.dict_emit, GOOD, [1] * 3, [0, 1], [0] * 3, {"num_unique": 2}, 3)
    refused("one count and rank", C.dict_scatter, GOOD, [1] * 2, [0, 1, 2], 3, 3)


def test_refusals_scan_pack():
    refused("count sum too large", C.dict_scan_pack, GOOD, [1 << 61, 1 << 61, 0], 3, 3)
    refused("count sum too large", C.dict_scan_pack, GOOD, [1 << 62, 0, 0], 3, 3)
    refused("count sum too large", C.dict_scan_pack, GOOD, [(1 << 62) - 1, 1, 0], 2, 3)
    refused("must not exceed cap", C.dict_scan_pack, GOOD, [1] * 3, 4, 3)
    refused("cap keys must be uploaded", C.dict_scan_pack, GOOD, [1] * 3, 3, 4)


def test_refusals_part_plan():
    refused("one count per first word", C.part_plan, [1, 2, 3], [1, 1], 3, 3)
    refused("ucap entries must be uploaded", C.part_plan, [1, 2, 3], [1, 1, 1], 3, 4)
