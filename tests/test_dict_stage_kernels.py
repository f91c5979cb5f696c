"""The dictionary fallback kernels (dict.hip: dict_insert, dict_part_build, rank_sort,
rank_emit, rank_scatter, scan_pack) and the in-job partition plan (partplan.hip), each
launched alone on host-made input through the stage entry points of locust/dict_stage.hpp
and compared with the plain integer reference of the same step (tests/dict_ref.py).  Every
comparison is exact.

Whole jobs (test_gpu_engine.py, test_ordered_edges.py, test_stream.py,
test_large_ordered.py) reach these kernels but compare only the final entries with the CPU
engine, which leaves this much unseen:

* the plan: any ascending lo[] gives correct word counts; a plan cut at the wrong quantiles
  only shows as fallbacks (a 10x slower job).  Here the sampling stride i * U / S, the
  singleton weight, the quantile rule, U < 256, U = 0 and the clamp at ucap are pinned;
* overflow contracts: on kCtrDictOverflow or kCtrNotEmitted the host throws the dictionary
  away and redoes the job, so what the kernels left behind is never looked at -- kIdFull
  publication, num_unique past ucap, rank_sort / rank_emit / rank_scatter leaving their
  outputs untouched above kRankSortMax, scan_pack's emit_limit;
* val and total_count: the weighted rank accumulates in 64 bits and rank_emit takes
  total_count from the thread that holds rank u - 1; jobs check total_count only, with
  counts that fit 32 bits;
* probe paths: the HBM table's wrap-around at its last slot, the re-probe on a slot whose
  word 0 matches while words 1..3 differ, the LDS cache's spill after kLdsProbes, and keys
  that hash identically (key_hash drops the top bit of word 3);
* edges of dict_part_build: n not a multiple of 16, n around kPartWindow, a partition at
  its capacity, the zeroing of uval / urank.

Dense ids come from atomics, so dense arrays are compared as {key: count}, with an extra
check that they hold no duplicate.

dict_insert_kernel clamps *d_n to cap, which also bounds its grid (256 tokens per
workgroup, at most 1,024 workgroups): a workgroup streams more than one chunk only past
2^18 tokens.  The "one workgroup streams everything" cases therefore ask the launcher for
one workgroup (max_blocks = 1) with cap = n; cap = 256 with more keys is run too, and
inserts the first 256 tokens, as the clamp says."""
import random

import pytest

import locust_amd as lc

import dict_ref as ref

pytestmark = pytest.mark.gpu

C = lc._C
K = ref.K
pad, blob, unblob = ref.pad, ref.blob, ref.unblob
OVERFLOW = ref.DICT_OVERFLOW
ID_FULL = K["kIdFull"]


def shuffled(seq, seed):
    seq = list(seq)
    random.Random(seed).shuffle(seq)
    return seq


def dense_map(got):
    keys = unblob(got["keys"])
    assert len(set(keys)) == len(keys), "a key holds two dense ids"
    assert len(keys) == len(got["counts"])
    return dict(zip(keys, got["counts"]))


def pow2_at_least(x):
    p = 64
    while p < x:
        p *= 2
    return p


# ---------------------------------------------------------------------------------------
# dict_insert
# ---------------------------------------------------------------------------------------

def run_insert(keys, counts=None, d_n=None, cap=None, slots=None, ucap=None, max_blocks=1024):
    n = len(keys)
    d_n = n if d_n is None else d_n
    cap = n if cap is None else cap
    live = min(d_n, cap)
    want = ref.aggregate(keys[:live], None if counts is None else counts[:live])
    slots = pow2_at_least(2 * len(want)) if slots is None else slots
    ucap = len(want) + 3 if ucap is None else ucap
    got = C.dict_insert(blob(keys), counts, d_n, cap, slots, ucap, max_blocks)
    return got, want, slots


def check_insert(got, want, slots):
    """No overflow: everything the kernel leaves behind."""
    U = len(want)
    assert got["flags"] == 0
    assert got["num_unique"] == U
    assert dense_map(got) == want
    assert got["tail_intact"]
    dense = unblob(got["keys"])
    assert sorted(i for _, i, _ in got["table"]) == list(range(1, U + 1))
    for slot, i, key in got["table"]:
        assert key == dense[i - 1], slot
    assert {s for s, _, _ in got["table"]} == ref.occupied([ref.hbm_slot(k, slots) for k in want], slots)


@pytest.mark.parametrize("mode", ["grid", "one_workgroup", "cap256"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_insert_sizes(n, mode):
    keys = list(ref.insert_mix(n))
    got, want, slots = run_insert(keys, cap=256 if mode == "cap256" else n,
                                  max_blocks=1 if mode == "one_workgroup" else 1024)
    if mode == "cap256" and n > 256:
        assert want == ref.aggregate(keys[:256]) and sum(want.values()) == 256
    else:
        assert sum(want.values()) == n
    check_insert(got, want, slots)


@pytest.mark.parametrize("max_blocks", [1024, 1])
def test_insert_one_key_5000_times(max_blocks):
    got, want, slots = run_insert([pad(b"the")] * 5000, max_blocks=max_blocks)
    assert want == {pad(b"the"): 5000}
    check_insert(got, want, slots)


@pytest.mark.parametrize("max_blocks", [1, 1024])
def test_insert_5000_distinct_keys_spill_the_cache(max_blocks):
    """One workgroup, 5,000 distinct keys: its 1,024-slot cache fills and the rest goes
    straight to the HBM table, where the flushed cache meets it."""
    keys = shuffled(ref.part_keys(5000, b"w"), 11)
    got, want, slots = run_insert(keys * 2, max_blocks=max_blocks)
    assert len(want) == 5000 and set(want.values()) == {2}
    check_insert(got, want, slots)


@pytest.mark.parametrize("max_blocks", [1024, 1])
def test_insert_weighted_with_empty_records(max_blocks):
    keys = list(ref.insert_mix(5000))
    counts = ref.big_counts(5000, 21)
    dead = keys[4]  # every record of this key has count 0: it must not get an id
    for i in range(5000):
        if i % 7 == 3:
            keys[i] = ref.ZERO_KEY  # (with a count: still skipped)
        if i % 5 == 2 or keys[i] == dead:
            counts[i] = 0
    got, want, slots = run_insert(keys, counts, max_blocks=max_blocks)
    assert dead not in want and ref.ZERO_KEY not in want
    assert max(want.values()) > 1 << 40 and sum(want.values()) > 1 << 32
    check_insert(got, want, slots)


def test_insert_clamps_d_n_to_cap():
    keys = list(ref.insert_mix(1000))
    got, want, slots = run_insert(keys, d_n=1007, cap=1000)
    assert sum(want.values()) == 1000  # none of the seven pattern keys behind them
    check_insert(got, want, slots)
    got, want, slots = run_insert(keys, d_n=600, cap=1000)
    assert sum(want.values()) == 600
    check_insert(got, want, slots)


@pytest.mark.parametrize("max_blocks", [1024, 1])
@pytest.mark.parametrize("shape", ref.FAMILIES + ("equal_hash",))
def test_insert_tie_families(shape, max_blocks):
    """Keys equal in word 0 (and further): a slot whose word 0 matches while words 1..3
    differ is probed past.  equal_hash: pairs with one hash, so one home slot everywhere."""
    base = ref.equal_hash_pairs() if shape == "equal_hash" else ref.family(shape, 600)
    keys = shuffled(list(base) * 3, 5)
    counts = ref.big_counts(len(keys), 6)
    got, want, slots = run_insert(keys, counts, max_blocks=max_blocks)
    assert len(want) == len(base)
    check_insert(got, want, slots)


def test_insert_lds_cache_collisions():
    """kLdsProbes + 4 keys of one cache slot in one workgroup: four of them spill."""
    keys = shuffled(list(ref.lds_collide_keys()) * 3, 8)
    assert len(keys) <= K["kInsBlock"]
    got, want, slots = run_insert(keys, ref.big_counts(len(keys), 9))
    check_insert(got, want, slots)


@pytest.mark.parametrize("max_blocks", [1024, 1])
def test_insert_hbm_table_wraps_around(max_blocks):
    keys = shuffled(list(ref.wrap_keys()) * 20, 3)  # 280 tokens: two workgroups
    got, want, slots = run_insert(keys, slots=ref.WRAP_SLOTS, max_blocks=max_blocks)
    assert slots == 64 and len(want) == 14
    check_insert(got, want, slots)
    assert {0, 63} <= {s for s, _, _ in got["table"]}


def check_overflowed(got, want, ucap):
    assert got["flags"] == OVERFLOW
    assert got["tail_intact"]  # nothing past ucap
    dense = dense_map(got)
    assert len(dense) == min(got["num_unique"], ucap)
    for k, c in dense.items():
        assert want.get(k) == c, k  # keys of the input, with their exact counts


@pytest.mark.parametrize("max_blocks", [1024, 1])
def test_insert_dense_capacity(max_blocks):
    keys = shuffled(list(ref.part_keys(300, b"w")) * 4, 13)
    counts = ref.big_counts(len(keys), 14)
    got, want, slots = run_insert(keys, counts, ucap=300, max_blocks=max_blocks)
    check_insert(got, want, slots)  # ucap = U: no flag
    got, want, slots = run_insert(keys, counts, ucap=299, max_blocks=max_blocks)
    assert got["num_unique"] == 300
    check_overflowed(got, want, 299)
    # the key without a dense id is published as full; every other slot names its key
    ids = sorted(i for _, i, _ in got["table"])
    assert ids == list(range(1, 300)) + [ID_FULL]
    dense = unblob(got["keys"])
    for _, i, key in got["table"]:
        assert key in want and (i == ID_FULL or key == dense[i - 1])
    assert {s for s, _, _ in got["table"]} == ref.occupied([ref.hbm_slot(k, slots) for k in want], slots)


@pytest.mark.parametrize("max_blocks", [1024, 1])
def test_insert_table_full(max_blocks):
    keys = shuffled(list(ref.part_keys(65, b"w")) * 3, 15)
    got, want, _ = run_insert(keys, slots=64, ucap=70, max_blocks=max_blocks)
    assert len(want) == 65 and got["num_unique"] == 64
    check_overflowed(got, want, 70)
    assert len(got["table"]) == 64 and sorted(i for _, i, _ in got["table"]) == list(range(1, 65))
    # 64 keys in 64 slots: no flag
    got, want, slots = run_insert([k for k in keys if k != keys[0]], slots=64, ucap=70,
                                  max_blocks=max_blocks)
    check_insert(got, want, slots)


# ---------------------------------------------------------------------------------------
# dict_part_build
# ---------------------------------------------------------------------------------------

TAGS = {"first_byte": lambda k: k[0], "hash": ref.hash_tag}


def run_part_build(keys, counts, tag, d_n=None, cap=None, ucap=None):
    n = len(keys)
    d_n = n if d_n is None else d_n
    cap = n if cap is None else cap
    live = min(d_n, cap)
    want = ref.aggregate(keys[:live], None if counts is None else counts[:live])
    ucap = len(want) + 3 if ucap is None else ucap
    parts = bytes(tag(k) for k in keys)
    return C.dict_part_build(blob(keys), counts, parts, d_n, cap, ucap), want


def check_part_build(got, want, tag):
    assert got["flags"] == 0
    assert got["num_unique"] == len(want)
    assert dense_map(got) == want
    assert got["tail_intact"]
    assert got["uval"] == [0] * len(want) and got["urank"] == [0] * len(want)
    # every partition's keys lie contiguous: a tag never comes back after another one
    tags = [tag(k) for k in unblob(got["keys"])]
    runs = [t for i, t in enumerate(tags) if i == 0 or tags[i - 1] != t]
    assert len(runs) == len(set(runs))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("tagging", list(TAGS))
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 16383, 16384, 16385, 40000])
def test_part_build_sizes(n, tagging, weighted):
    keys = list(ref.part_build_tokens(n))
    counts = None
    if weighted:
        counts = ref.big_counts(n, 31)
        for i in range(5, n, 11):
            counts[i] = 0
        for i in range(3, n, 13):
            keys[i] = ref.ZERO_KEY
    got, want = run_part_build(keys, counts, TAGS[tagging])
    check_part_build(got, want, TAGS[tagging])


def test_part_build_clamps_d_n_to_cap():
    keys = list(ref.part_build_tokens(16385))[:1000]
    got, want = run_part_build(keys, None, TAGS["first_byte"], d_n=1007, cap=1000)
    assert sum(want.values()) == 1000
    check_part_build(got, want, TAGS["first_byte"])
    got, want = run_part_build(keys, None, TAGS["first_byte"], d_n=599, cap=1000)
    assert sum(want.values()) == 599
    check_part_build(got, want, TAGS["first_byte"])


def test_part_build_partition_at_capacity():
    """1,500 distinct keys in one partition: by the reference no cluster of its table
    passes kPartProbes (test_dict_ref.py), so it must not flag; 2,049 cannot fit 2,048
    slots; a dense capacity one short flags too."""
    tag = TAGS["first_byte"]
    keys = shuffled(list(ref.part_keys(1500)) * 2, 41)
    got, want = run_part_build(keys, ref.big_counts(len(keys), 42), tag)
    assert len(want) == 1500
    check_part_build(got, want, tag)
    got, want = run_part_build(keys, None, tag, ucap=1499)
    assert got["flags"] == OVERFLOW and got["num_unique"] == 1500 and got["tail_intact"]
    dense = dense_map(got)
    assert len(dense) == 1499 and all(want[k] == c for k, c in dense.items())
    got, want = run_part_build(shuffled(ref.part_keys(2049), 43), None, tag, ucap=2100)
    assert got["flags"] == OVERFLOW and got["tail_intact"]


# ---------------------------------------------------------------------------------------
# rank_sort
# ---------------------------------------------------------------------------------------

def check_rank(keys, counts, d_u=None, cap=None):
    cap = len(keys) if cap is None else cap
    d_u = cap if d_u is None else d_u
    u = min(d_u, cap)
    got = C.dict_rank(blob(keys), counts, d_u, cap)
    rank, val = ref.ranks(keys[:u], None if counts is None else counts[:u])
    assert got["tail_intact"]
    assert got["rank"] == rank + [0] * (cap - u)
    assert got["val"] == val + [0] * (cap - u)
    return val


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", ref.FAMILIES)
@pytest.mark.parametrize("u", [0, 1, 2, 255, 256, 257, 511, 513, 4097])
def test_rank_sort_sizes(u, shape, weighted):
    keys = shuffled(ref.family(shape, u), 51)
    val = check_rank(keys, ref.big_counts(u, 52) if weighted else None)
    if weighted and u >= 255:
        assert (1 << 32) < max(val) < (1 << 62)


def test_rank_sort_clamps_d_u_to_cap():
    keys = shuffled(ref.family("edges", 310), 53)
    check_rank(keys, ref.big_counts(310, 54), d_u=305, cap=300)
    check_rank(keys, ref.big_counts(310, 54), d_u=200, cap=300)


def test_rank_sort_at_its_limit():
    keys = shuffled(ref.family("short", K["kRankSortMax"]), 55)
    check_rank(keys, ref.big_counts(len(keys), 56))


def test_rank_sort_above_its_limit_writes_nothing():
    keys = shuffled(ref.family("short", K["kRankSortMax"] + 1), 57)
    got = C.dict_rank(blob(keys), ref.big_counts(len(keys), 58), len(keys), len(keys))
    assert got["tail_intact"]
    assert got["rank"] == [0] * len(keys) and got["val"] == [0] * len(keys)


# ---------------------------------------------------------------------------------------
# rank_emit / rank_scatter
# ---------------------------------------------------------------------------------------

CTR = {"num_records": 11, "map_tokens": 12, "overflow_lines": 13, "truncated": 14,
       "num_newlines": 15, "max_key_len": 16, "flags": 6, "total_count": 17}


def mixed_keys(u, seed):
    per = -(-u // len(ref.FAMILIES))
    return shuffled([k for f in ref.FAMILIES for k in ref.family(f, per)][:u], seed)


def check_emit(keys, counts, rank, val, num_unique, cap):
    ctr = dict(CTR, num_unique=num_unique)
    got = C.dict_emit(blob(keys), counts, rank, val, ctr, cap)
    recs, ctr_out = ref.emit(keys, counts, rank, val, ctr, cap)
    assert got["ctr_out"] == ctr_out
    assert got["tail_intact"]
    if recs is None:
        assert got["untouched"]
    else:
        assert list(zip(unblob(got["keys"]), got["counts"])) == recs
    return got


@pytest.mark.parametrize("u", [0, 1, 256, 257, 5000])
def test_emit_and_scatter_from_reference_ranks(u):
    cap = u + 3
    keys = mixed_keys(cap, 61)
    counts = ref.big_counts(cap, 62)
    rank, _ = ref.ranks(keys[:u])
    if u:
        counts[rank.index(u - 1)] |= 4  # the last key's count is above 1
    rank, val = ref.ranks(keys[:u], counts[:u])
    rank, val = rank + [7] * 3, val + [9] * 3
    got = check_emit(keys, counts, rank, val, u, cap)
    if u:
        last = rank.index(u - 1)
        assert counts[last] > 1 and got["ctr_out"]["total_count"] == sum(counts[:u])
        assert got["keys"] == blob(sorted(keys[:u]))
    else:
        assert got["ctr_out"]["total_count"] == 0
    sc = C.dict_scatter(blob(keys), counts, rank, u, cap)
    skeys, scounts = ref.scatter(keys, counts, rank, u, cap)
    assert sc["tail_intact"] and unblob(sc["keys"]) == skeys and sc["counts"] == scounts


def test_emit_chained_behind_rank_sort():
    u = 257
    keys = mixed_keys(u, 63)
    counts = ref.big_counts(u, 64)
    r = C.dict_rank(blob(keys), counts, u, u)
    got = check_emit(keys, counts, r["rank"], r["val"], u, u)
    assert got["keys"] == blob(sorted(keys))
    assert got["ctr_out"]["total_count"] == sum(counts)
    sc = C.dict_scatter(blob(keys), counts, r["rank"], u, u)
    assert sc["keys"] == blob(sorted(keys))


def test_emit_clamps_num_unique_to_cap():
    u = 300
    keys = mixed_keys(u, 65)
    counts = ref.big_counts(u, 66)
    rank, val = ref.ranks(keys, counts)
    got = check_emit(keys, counts, rank, val, u + 10, u)
    assert got["ctr_out"]["num_unique"] == u
    sc = C.dict_scatter(blob(keys), counts, rank, u + 10, u)
    assert sc["tail_intact"] and sc["keys"] == blob(sorted(keys))


def test_emit_and_scatter_above_the_rank_sort_limit():
    u = K["kRankSortMax"] + 1
    keys = list(ref.family("short", u))
    counts = [2] * u
    rank = list(range(u))
    got = check_emit(keys, counts, rank, [0] * u, u, u)
    assert got["ctr_out"]["flags"] == CTR["flags"] | ref.NOT_EMITTED and got["untouched"]
    assert got["ctr_out"]["total_count"] == ref.PATTERN_U64
    sc = C.dict_scatter(blob(keys), counts, rank, u, u)
    assert sc["tail_intact"]
    assert sc["keys"] == ref.PATTERN_KEY * u and sc["counts"] == [ref.PATTERN_U64] * u


# ---------------------------------------------------------------------------------------
# scan_pack
# ---------------------------------------------------------------------------------------

SCAN_SIZES = [0, 1, 2047, 2048, 2049, 4096, 10000]


@pytest.mark.parametrize("with_ctr_out", [True, False])
@pytest.mark.parametrize("u,short", [(u, 0) for u in SCAN_SIZES] + [(u, 1) for u in SCAN_SIZES if u])
def test_scan_pack(u, short, with_ctr_out):
    """short: emit_limit = u - 1 (flag, no record, no total_count); else emit_limit = u."""
    cap = u + 5
    skeys = sorted(mixed_keys(cap, 71))
    counts = ref.scan_counts(u) + [3] * 5
    limit = u - short
    got = C.dict_scan_pack(blob(skeys), counts, u, cap, limit, with_ctr_out, CTR)
    recs, total, ctr_out = ref.scan_pack(skeys, counts, u, limit, CTR)
    assert got["tail_intact"]
    if recs is None:
        assert got["untouched"]
    else:
        assert list(zip(unblob(got["keys"]), got["counts"])) == recs
    assert got["total_count"] == (ref.PATTERN_U64 if total is None else total)
    if with_ctr_out:
        assert got["ctr_out"] == ctr_out
    else:
        assert set(got["ctr_out"].values()) <= {ref.PATTERN_U32, ref.PATTERN_U64}
    if u and not short:
        assert total > 1 << 60


# ---------------------------------------------------------------------------------------
# part_plan
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ones", "twos", "zipf"])
@pytest.mark.parametrize("U", [0, 1, 2, 255, 256, 257, 8191, 8192, 8193, 20000])
def test_part_plan(U, kind):
    w0, counts = ref.plan_input(U, kind)
    assert C.part_plan(w0, counts, U, U) == ref.part_plan(w0, counts, U, U)
    if U >= 256:
        assert any(w >> 63 for w in w0) and ref.M64 in w0


@pytest.mark.parametrize("ucap", [200, 8192, 9000])
def test_part_plan_clamps_d_u_to_ucap(ucap):
    w0, counts = ref.plan_input(ucap + 9, "zipf")
    got = C.part_plan(w0, counts, ucap + 9, ucap)
    assert got == ref.part_plan(w0, counts, ucap + 9, ucap)
    assert got == ref.part_plan(w0[:ucap], counts[:ucap], ucap, ucap)


def test_part_plan_one_first_word_and_ties():
    word = ref.w0_of(pad(b"w" * 8))
    got = C.part_plan([word] * 300, [1, 2, 5] * 100, 300, 300)
    assert got == [0] + [word] * 255 + [ref.M64]
    # groups of equal first words with unequal weights: the tie order is the sort's own
    w0, counts = ref.plan_input(9000, "zipf")
    w0t = [w0[i // 4] for i in range(9000)]
    assert C.part_plan(w0t, counts, 9000, 9000) == ref.part_plan(w0t, counts, 9000, 9000)
