"""The shuffle's tail (csrc/kernels/merge.hip over the slot layout), each launch alone on
host-made slots through the stage entry points of locust/exch_stage.hpp and compared with the
plain integer reference (tests/exchange_ref.py): launch_merge_slots (merge_rank_kernel +
merge_emit_kernel, hdr_out), launch_merge_rank_slots (the merged array and the accumulator
triples) and launch_merge_emit_compact.  Every comparison is exact.

Whole jobs (test_dist.py) reach these kernels with consistent inputs at 1-8 ranks only; here
the slot lengths no healthy job produces (failed / redone slots with records, n beyond the
slot), the run-count edges (8 threads per record, 64 lanes of the run table), the walk-on
and both directions of the gallop, the accumulators, and the compact emit's refusals, offsets,
look-back, record forms and hand-off are pinned.

Not reachable with valid input, so left out:
* more than 64 slots, P > 64, me >= P: the kernels clamp or would index past their tables;
  the host refuses them before any launch, which is asserted;
* "every tile but the last holds only duplicates": a key has at most one copy per run, so
  1,024 consecutive merged slots hold at least 16 first copies.  The sparsest tiles there
  are -- 16 first copies among 1,008 zero-count duplicates -- are a case;
* records of count 0 (a record is a word that occurred)."""
import random
import struct

import pytest

import locust_amd as lc

import exchange_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

C = lc._C
pad = ref.pad32
OK, FAILED, REDO = ref.SLOT_OK, ref.SLOT_FAILED, ref.SLOT_REDO
PAT8 = int.from_bytes(b"\xa5" * 8, "little")
PAT_KEY = b"\xa5" * ref.KEY_BYTES
TILE = 1024  # merged slots per workgroup of the emit kernels


# ---------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------

def header(status, n, q=0):
    """80 header bytes; every field the merge does not read holds a value of its own."""
    return struct.pack("<iIQ5QQ2Q", status, 3, n, 1000 + q, 2000 + q, 3000 + q, 4000 + q,
                       5000 + q, 6000 + q, 7000 + q, 0x8000000000000000 + q)


def native(slots):
    return [(header(st, n, q), ref.blob(k for k, _ in recs), [c for _, c in recs])
            for q, (st, n, recs) in enumerate(slots)]


def full(runs):
    """Healthy slots of these runs."""
    return [(OK, len(run), run) for run in runs]


def check_acc(acc, runs):
    want = ref.acc_ref(runs)
    assert len(acc) == 3 * ref.ACC_SPREAD
    assert (sum(acc[0::3]), sum(acc[1::3]), sum(acc[2::3])) == want
    for f, t, w in zip(acc[0::3], acc[1::3], acc[2::3]):
        assert f <= want[0] and t <= want[1] and w <= want[2]  # (no wrapped negative)
        assert f > 0 or (t == 0 and w == 0)


def check_rank(slots, slot_records):
    runs = ref.slot_runs(slots, slot_records)
    got = C.exch_rank_slots(native(slots), slot_records)
    want = ref.merged_ref(runs)
    keys, counts = ref.unblob(got["keys"]), got["counts"]
    assert len(keys) == len(counts) == len(slots) * slot_records
    assert keys[:len(want)] == [k for k, _ in want]
    assert counts[:len(want)] == [c for _, c in want]
    # behind the merged records nothing was written
    assert all(k == PAT_KEY for k in keys[len(want):])
    assert all(c == PAT8 for c in counts[len(want):])
    check_acc(got["acc"], runs)
    return got


def check_merge(slots, slot_records):
    runs = ref.slot_runs(slots, slot_records)
    cs = native(slots)
    got = C.exch_merge_slots(cs, slot_records)
    recs, ctr = ref.merge_out_ref(runs)
    assert got["ctr"] == ctr and got["ctr_out"] == ctr
    assert ref.unblob(got["keys"]) == [k for k, _ in recs]
    assert got["counts"] == [c for _, c in recs]
    assert got["tail_intact"]
    assert got["headers"] == [h for h, _k, _c in cs]  # byte for byte
    return got


def check_both(slots, slot_records):
    check_merge(slots, slot_records)
    check_rank(slots, slot_records)


def word_keys(n, rng, lo=1, hi=12):
    out = set()
    while len(out) < n:
        out.add(pad(bytes(rng.choice(b"abcdefghij") for _ in range(rng.randint(lo, hi)))))
    return sorted(out)


COUNTS = [1, 1, 2, 77, (1 << 24) - 1, 1 << 24]  # (2^32: where the records are few)


def draw_run(universe, length, rng, counts=COUNTS):
    return [(k, rng.choice(counts)) for k in sorted(rng.sample(universe, length))]


# ---------------------------------------------------------------------------------------
# slot merge and rank kernel: shapes
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nslots,slot_records", [(1, 4), (2, 64), (7, 5), (8, 16), (9, 7),
                                                 (16, 33), (17, 8), (63, 4), (64, 6)])
def test_run_count_edges(nslots, slot_records):
    """Run lengths drawn from {0, 1, 2, slot_records - 1, slot_records}, every one of them
    at least once where there are runs enough; keys drawn from a small universe, so most
    occur in several runs."""
    rng = random.Random(nslots * 100 + slot_records)
    universe = word_keys(2 * slot_records, rng)
    lens = [0, 1, 2, slot_records - 1, slot_records]
    lengths = [lens[(q + nslots) % 5] if nslots >= 5 else rng.choice(lens[1:])
               for q in range(nslots)]
    rng.shuffle(lengths)
    runs = [draw_run(universe, n, rng) for n in lengths]
    check_both(full(runs), slot_records)


def split_total(total, nruns, rng):
    cuts = sorted(rng.sample(range(1, total), nruns - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


@pytest.mark.parametrize("total,nruns", [(1023, 2), (1024, 3), (1025, 8), (2047, 5), (2048, 2),
                                         (2049, 4), (4097, 7)])
def test_totals_around_the_emit_tile(total, nruns):
    rng = random.Random(total)
    lengths = split_total(total, nruns, rng)
    universe = word_keys(max(max(lengths), total * 2 // 3), rng, 2, 14)
    runs = [draw_run(universe, n, rng, [1, 2, 3, 1 << 24]) for n in lengths]
    assert sum(len(r) for r in runs) == total
    assert len(ref.merge_out_ref(runs)[0]) < total  # (keys are shared)
    check_both(full(runs), max(lengths))


def test_tiles_of_duplicates():
    """Every key in all 64 runs: each full tile of 1,024 merged slots holds 16 first copies
    and 1,008 zero-count duplicates (the fewest a tile can hold), the last tile one key."""
    rng = random.Random(5)
    keys = word_keys(17, rng)
    runs = [[(k, 1 + q + 64 * i) for i, k in enumerate(keys)] for q in range(64)]
    merged = ref.merged_ref(runs)
    assert len(merged) == 1088 and sum(1 for _k, c in merged[:TILE] if c) == 16
    check_both(full(runs), 17)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all_but_one", "all"])
def test_empty_runs(where):
    rng = random.Random(9)
    universe = word_keys(12, rng)
    runs = [draw_run(universe, 5, rng) for _ in range(9)]
    empty = {"first": [0], "middle": [3, 4, 8 - 3], "last": [8], "all_but_one": [0, 1, 2, 3, 4, 5, 6, 8],
             "all": range(9)}[where]
    for q in empty:
        runs[q] = []
    got = check_merge(full(runs), 8)
    check_rank(full(runs), 8)
    if where == "all":  # the counters are written, the output is not
        assert got["ctr"] == (0, 0, 0) and got["keys"] == b"" and got["tail_intact"]


# ---------------------------------------------------------------------------------------
# headers
# ---------------------------------------------------------------------------------------

def test_failed_and_redone_slots_count_as_empty():
    """Slots 1 and 3 announce records and hold real-looking ones (smaller than, equal to and
    between the healthy keys): none may be merged, counted or summed."""
    healthy = [(pad(b"m%02d" % i), 10 + i) for i in range(6)]
    ghost = [(pad(b"a0"), 5), (pad(b"m01"), 500), (pad(b"m015"), 7), (pad(b"zz"), 9),
             (pad(b"zza"), 1 << 24), (pad(b"zzb"), 1)]
    for bad in (FAILED, REDO):
        slots = [(OK, 6, healthy), (bad, 4, ghost), (OK, 3, healthy[1:4]), (bad, 1 << 40, ghost),
                 (OK, 0, ghost)]
        got = check_merge(slots, 6)
        assert got["ctr"] == (9, 6, sum(c for _k, c in healthy) + sum(c for _k, c in healthy[1:4]))
        check_rank(slots, 6)
    # every slot failed: nothing at all
    slots = [(FAILED, 4, ghost[:4]), (REDO, 2, ghost[:4])]
    assert check_merge(slots, 4)["ctr"] == (0, 0, 0)
    check_rank(slots, 4)


@pytest.mark.parametrize("n", [7, 1 << 32, (1 << 32) + 2, 1 << 40, 2**64 - 1])
def test_n_beyond_the_slot_clamps(n):
    """slot_records = 6: n = 7 and far more (also with low 32 bits 0 and 2) take 6 records."""
    rng = random.Random(n % 1000)
    universe = word_keys(10, rng)
    slots = [(OK, n, draw_run(universe, 6, rng)), (OK, 6, draw_run(universe, 6, rng)),
             (OK, n, draw_run(universe, 6, rng))]
    assert [len(r) for r in ref.slot_runs(slots, 6)] == [6, 6, 6]
    check_both(slots, 6)


def test_records_behind_n_do_not_appear():
    """n < slot_records with well-formed records behind n: keys smaller than everything (a
    sorted run would not hold them there, but the slot may, from an earlier job)."""
    run0 = [(pad(b"k%d" % i), i + 1) for i in range(3)]
    stale = [(pad(b"a%d" % i), 1 << 30) for i in range(5)]
    slots = [(OK, 3, run0 + stale), (OK, 0, stale), (OK, 1, [(pad(b"k1"), 7)] + stale[:4]),
             (OK, 7, [(pad(b"j%d" % i), 2) for i in range(7)] + stale[:1])]
    got = check_merge(slots, 8)
    assert got["ctr"] == (11, 10, 1 + 2 + 3 + 7 + 14)
    check_rank(slots, 8)


# ---------------------------------------------------------------------------------------
# duplicates
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["one_key_in_all", "every_key_in_every_run", "none_shared",
                                   "runs_0_7_8_63"])
def test_duplicates_over_64_runs(shape):
    rng = random.Random(shape)
    universe = word_keys(64 * 4 + 1, rng, 3, 10)
    shared, rest = universe[100], universe[:100] + universe[101:]
    runs = []
    for q in range(64):
        own = rest[4 * q:4 * q + 4] if shape != "every_key_in_every_run" else universe[:5]
        if shape == "one_key_in_all" or (shape == "runs_0_7_8_63" and q in (0, 7, 8, 63)):
            own = own + [shared]
        runs.append([(k, rng.choice(COUNTS)) for k in sorted(own)])
    tot = ref.merge_out_ref(runs)
    if shape == "none_shared":
        assert tot[1][0] == tot[1][1] == 256
    if shape == "runs_0_7_8_63":
        assert tot[1][0] - tot[1][1] == 3
        i = [k for k, _ in ref.merged_ref(runs)].index(shared)
        assert [c for _k, c in ref.merged_ref(runs)[i:i + 4]] == [dict(tot[0])[shared], 0, 0, 0]
    check_both(full(runs), 5)


# ---------------------------------------------------------------------------------------
# keys: later words, the walk-on, lengths and bytes
# ---------------------------------------------------------------------------------------

def later_word_keys(word, n):
    """n ascending keys equal in every word but `word` (1, 2 or 3)."""
    return [pad(b"p" * (8 * word) + b"%07d" % i) for i in range(n)]


@pytest.mark.parametrize("word", [1, 2, 3])
def test_keys_differing_in_one_later_word(word):
    keys = later_word_keys(word, 40)
    rng = random.Random(word)
    runs = [draw_run(keys, n, rng) for n in (40, 13, 1, 25, 40)]
    check_both(full(runs), 40)


def stretch_keys(n):
    """n ascending keys sharing word 0, neighbours differing only in word 1, 2 or 3."""
    tails = [b"%05d", b"qqqqqqqq%05d", b"qqqqqqqqrrrrrrrr%05d"]
    return sorted(pad(b"mmmmmmmm" + tails[i % 3] % i) for i in range(n))


@pytest.mark.parametrize("stretch", [1, 2, 65, 300])
def test_walk_on_over_stretches_sharing_the_first_word(stretch):
    """`stretch` consecutive records of a run share word 0; the other runs hold the same
    keys, keys between them (one byte longer), keys before, behind and next to word 0's
    value.  The lower bound on word 0 stops at the stretch's first record and walks on."""
    rng = random.Random(stretch)
    every = stretch_keys(300)
    between = [pad(k.rstrip(b"\0") + b"5") for k in every]
    around = [pad(b"a"), pad(b"mmmmmmm"), pad(b"mmmmmmml"), pad(b"mmmmmmmm"), pad(b"mmmmmmmn"),
              pad(b"z")]
    at = rng.randrange(300 - stretch + 1)
    body = every[at:at + stretch]
    runs = [[(k, 1 + i) for i, k in enumerate(sorted(body + [around[0], around[-1]]))],
            draw_run(sorted(set(every + between + around)), 60, rng),
            [(k, 5) for k in sorted(every + between)],
            [(every[0], 2), (every[-1], 3)],
            [(k, 7) for k in around],
            [(k, 11) for k in sorted(body + between[at:at + stretch])]]
    assert sum(1 for k, _ in runs[0] if k[:8] == b"mmmmmmmm") == stretch
    slot_records = max(len(r) for r in runs)
    check_both(full(runs), slot_records)
    check_both(full(runs[::-1]), slot_records)  # the stretch in the highest run


def test_key_lengths_and_bytes():
    """Keys of 1, 8, 16, 24 and 32 bytes exactly (a word boundary is the end of the key, the
    next word all NUL), their neighbours, and the bytes 0x80 and 0xff in every word."""
    keys = set()
    for n in (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32):
        for fill in (b"a", b"\x80", b"\xff", b"\x7f"):
            keys.add(pad(fill * n))
            keys.add(pad(b"a" * (n - 1) + fill))
    keys = sorted(keys)
    assert pad(b"\xff" * 32) == ref.ALL_ONES and ref.ALL_ONES in keys
    rng = random.Random(32)
    runs = [draw_run(keys, n, rng) for n in (len(keys), 20, 1, 33, len(keys) - 1)]
    runs.append([(pad(b"\xff" * 32), 9)])
    runs.append([(pad(b"\x01"), 9), (pad(b"\xff" * 32), 1)])
    check_both(full(runs), len(keys))


# ---------------------------------------------------------------------------------------
# gallop
# ---------------------------------------------------------------------------------------

def numbered(values, width=7):
    return [pad(b"k%0*d" % (width, v)) for v in values]


GALLOP = {
    # one record against 2,048: first, inside (present and absent) and last
    "one_low": ([-1], range(0, 4096, 2)),
    "one_mid_present": ([2048], range(0, 4096, 2)),
    "one_mid_absent": ([2049], range(0, 4096, 2)),
    "one_high": ([5000], range(0, 4096, 2)),
    # a dense run inside one gap of a sparse one, and the reverse
    "dense_in_gap": (range(3001, 3400), range(0, 40000, 1000)),
    "sparse_around_dense": (range(0, 40000, 1000), range(3001, 3400)),
    # every key smaller / larger than the other run's: the hint is at the wrong end
    "all_smaller": (range(0, 700), range(1000, 1300)),
    "all_larger": (range(1000, 1300), range(0, 700)),
    "ends_only": ([0, 99999], range(1, 3000)),
}


@pytest.mark.parametrize("case", list(GALLOP))
def test_gallop(case):
    a, b = GALLOP[case]
    mk = lambda vs: numbered([v + 1 for v in vs])  # noqa: E731  (-1 -> the smallest key)
    runs = [[(k, 3) for k in mk(a)], [(k, 5) for k in mk(b)]]
    slot_records = max(len(runs[0]), len(runs[1]))
    check_both(full(runs), slot_records)
    check_both(full(runs[::-1]), slot_records)
    # and with a third run between them that shares keys with both
    mid = sorted(set(mk(a)[::3]) | set(mk(b)[::5]))[:slot_records]
    check_both(full([runs[0], [(k, 1) for k in mid], runs[1]]), slot_records)


# ---------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, (1 << 24) - 1, 1 << 24, 1 << 32])
def test_counts_per_record(count):
    rng = random.Random(count)
    universe = word_keys(30, rng)
    runs = [draw_run(universe, n, rng, [count]) for n in (30, 12, 30, 1, 17)]
    check_both(full(runs), 30)


def test_count_total_at_the_limit_is_exact():
    """The emit's look-back value holds 40 bits of counts: a total of exactly 2^40 - 1, most
    of it in the last tile, then one more, which the host refuses."""
    keys = numbered(range(1500))
    runs = [[(k, 1) for k in keys[:1100]], [(k, 2) for k in keys[400:]]]
    spent = 1100 + 2 * 1100
    runs.append([(keys[-1], ref.MERGE_MAX_COUNT - spent)])
    assert ref.merge_out_ref(runs)[1] == (2201, 1500, ref.MERGE_MAX_COUNT)
    check_both(full(runs), 1100)
    runs[2] = [(keys[-1], ref.MERGE_MAX_COUNT - spent + 1)]
    with pytest.raises(lc.LocustError, match="count sum too large"):
        C.exch_merge_slots(native(full(runs)), 1100)
    check_rank(full(runs), 1100)  # (the accumulators are 64-bit sums)
    # records of a failed slot and behind n: not merged, yet part of the sum the host bounds
    # (a merge that read them must not overflow its scan either)
    runs[2] = [(keys[-1], ref.MERGE_MAX_COUNT - spent - 5)]
    slots = full(runs) + [(FAILED, 1, [(keys[0], 2)]), (OK, 0, [(keys[0], 3)])]
    assert check_merge(slots, 1100)["ctr"] == (2201, 1500, ref.MERGE_MAX_COUNT - 5)
    check_rank(slots, 1100)
    slots[-1] = (OK, 0, [(keys[0], 4)])
    with pytest.raises(lc.LocustError, match="count sum too large"):
        C.exch_merge_slots(native(slots), 1100)


def test_shapes_refused_on_the_host():
    one = (OK, 1, [(pad(b"a"), 1)])
    with pytest.raises(lc.LocustError, match="1..64 slots"):
        C.exch_merge_slots(native([one] * 65), 4)
    with pytest.raises(lc.LocustError, match="1..64 slots"):
        C.exch_rank_slots(native([one] * 65), 4)
    with pytest.raises(lc.LocustError, match="1..64 slots"):
        C.exch_emit_compact(native([one] * 65), 4, [(0, 0, 1)], None, 0, 1, 8, 0, 8, 1)
    big = (ref.MERGE_MAX_RECORDS + 1) // 64  # 64 slots of 65,536: one record too many
    for fn in (C.exch_merge_slots, C.exch_rank_slots):
        with pytest.raises(lc.LocustError, match="too many records"):
            fn(native([one] * 64), big)
    with pytest.raises(lc.LocustError, match="too many records"):
        C.exch_emit_compact(native([one] * 64), big, [(0, 0, 1)], None, 0, 1, 8, 0, 8, 1)
    with pytest.raises(lc.LocustError, match="bad shape"):
        C.exch_emit_compact(native([one]), 4, [(0, 0, 1)] * 65, None, 0, 1, 80, 0, 8, 1)
    with pytest.raises(lc.LocustError, match="bad shape"):
        C.exch_emit_compact(native([one]), 4, [], None, 0, 1, 80, 0, 8, 1)
    for P, me in [(1, 1), (3, 3), (64, 64), (2, 2**32 - 1)]:
        with pytest.raises(lc.LocustError, match="not one of the P ranks"):
            C.exch_emit_compact(native([one]), 4, [(0, 0, 1)] * P, None, 0, 1, 80, me, 8, 1)
    # a report smaller than the merged range would let the emit leave its region
    for fn in (C.exch_merge_slots, C.exch_rank_slots):  # also of a slot that does not count
        with pytest.raises(lc.LocustError, match="announces records the slot does not hold"):
            fn(native([one, (FAILED, 3, [(pad(b"a"), 1), (pad(b"b"), 1)])]), 4)
        with pytest.raises(lc.LocustError, match="slot overfilled"):
            fn(native([(OK, 1, [(pad(b"%d" % i), 1) for i in range(5)])]), 4)
    with pytest.raises(lc.LocustError, match="must cover the merged range"):
        C.exch_emit_compact(native([(OK, 2, [(pad(b"a"), 1), (pad(b"b"), 1)])]), 4, [(0, 0, 1)],
                            None, 0, 1, 8, 0, 8, 1)


# ---------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------

def fuzz_slots(rng):
    nslots = rng.choice([1, 2, 3, 7, 8, 9, 16, 17, 33, 64])
    slot_records = rng.randint(4, 64 if nslots <= 17 else 12)
    kind = rng.choice(["words", "later_word", "stretch", "bytes"])
    size = rng.randint(slot_records, 3 * slot_records)
    if kind == "words":
        universe = word_keys(size, rng, 1, 31)
    elif kind == "later_word":
        universe = later_word_keys(rng.choice([1, 2, 3]), size)
    elif kind == "stretch":
        universe = sorted({pad(rng.choice([b"a", b"mmmmmmmm", b"mmmmmmmmqqqqqqqq"])
                               + bytes(rng.choice(b"xyz") for _ in range(rng.randint(1, 14))))
                           for _ in range(3 * size)})
    else:
        universe = sorted({pad(bytes(rng.choice([1, 0x7f, 0x80, 0xff]) for _ in range(rng.randint(1, 32))))
                           for _ in range(3 * size)})
    counts = COUNTS + [1 << 32] if nslots * slot_records < 256 else COUNTS
    slots = []
    for _ in range(nslots):
        held = min(rng.choice([0, 1, 2, slot_records - 1, slot_records, rng.randint(0, slot_records)]),
                   len(universe))
        recs = draw_run(universe, held, rng, counts)
        roll = rng.random()
        if roll < 0.1:
            n = rng.choice([held, 1 << 40]) if held == slot_records else rng.randint(0, held)
            slots.append((rng.choice([FAILED, REDO]), n, recs))
        elif roll < 0.2 and held == slot_records:
            slots.append((OK, rng.choice([held + 1, 1 << 40, 2**64 - 1]), recs))
        elif roll < 0.3 and held:
            slots.append((OK, rng.randrange(held), recs))  # well-formed records behind n
        else:
            slots.append((OK, held, recs))
    return slots, slot_records


@pytest.mark.parametrize("seed", list(range(1, 41)))
def test_fuzz(seed):
    slots, slot_records = fuzz_slots(random.Random(seed))
    check_both(slots, slot_records)


# ---------------------------------------------------------------------------------------
# compact emit
# ---------------------------------------------------------------------------------------

NO_REGION = 2**64 - 1
SEQ = 0x1234567890


def check_emit(out, want, P, me, seq):
    dst, stamps = out["dst"], out["stamps"]
    assert out["done"] == 0  # handed back for the next job
    assert len(stamps) == P
    if want == ref.REFUSED:
        assert all(w == PAT8 for w in dst) and all(s == PAT8 for s in stamps)
        return
    first, words = want
    assert dst[first:first + len(words)] == words
    assert all(w == PAT8 for w in dst[:first])
    assert all(w == PAT8 for w in dst[first + len(words):])  # (the guard is part of dst)
    assert stamps[me] == seq
    assert all(s == PAT8 for q, s in enumerate(stamps) if q != me)


def run_emit(slots, slot_records, msg3, me, gather_records, region_records, region=0, regions=1,
             from_root=False, seq=SEQ):
    """One emit job checked against emit_ref.  from_root: the region goes through the root's
    header and the host's argument says "none"."""
    runs = ref.slot_runs(slots, slot_records)
    out = C.exch_emit_compact(native(slots), slot_records, msg3, region if from_root else None,
                              NO_REGION if from_root else region, regions, region_records, me,
                              gather_records, seq)
    assert len(out) == 1
    want = ref.emit_ref(runs, msg3, region, regions, region_records, me, gather_records)
    check_emit(out[0], want, len(msg3), me, seq)
    check_acc(out[0]["acc"], runs)
    return want


@pytest.fixture(scope="module")
def emit_slots():
    """Three runs, 61 records, 40 distinct keys of mixed record sizes."""
    rng = random.Random(40)
    universe = word_keys(40, rng, 1, 31)
    runs = [draw_run(universe, n, rng) for n in (30, 11, 20)]
    runs[2] = sorted(set(runs[2]) | {(k, 1) for k in universe
                                     if k not in {r[0] for run in runs for r in run}})
    assert ref.acc_ref(runs)[0] == 40
    return full(runs), max(len(r) for r in runs)


def lower_ranks(P, me, kind, gather):
    """(status, flags, n_out) of the P ranks: the ranks below me hold n_out below, equal to
    and above gather_records; the ranks above me whatever."""
    below = {"below": [0, 1, gather - 1], "equal": [gather], "above": [gather + 1, 1 << 40, gather]}[kind]
    return [(0, 0, below[q % len(below)]) if q < me else (0, 0, (7 * q) % (gather + 1))
            for q in range(P)]


@pytest.mark.parametrize("kind", ["below", "equal", "above"])
@pytest.mark.parametrize("P,me", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 3),
                                  (8, 7), (64, 0), (64, 31), (64, 63)])
def test_emit_offset_over_the_lower_ranks(emit_slots, P, me, kind):
    slots, slot_records = emit_slots
    gather = 40
    msg3 = lower_ranks(P, me, kind, gather)
    msg3[me] = (0, 0, 40)
    want = run_emit(slots, slot_records, msg3, me, gather, region_records=64 * gather + 40)
    r = sum(min(n, gather) for _s, _f, n in msg3[:me])
    assert want[0] == 5 * r and len(want[1]) == ref.acc_ref(ref.slot_runs(slots, slot_records))[2]
    if kind == "above" and me:
        assert r < sum(n for _s, _f, n in msg3[:me])  # (the clamp decides the offset)


@pytest.mark.parametrize("from_root", [False, True])
@pytest.mark.parametrize("regions,region", [(1, 0), (3, 0), (3, 1), (3, 2)])
def test_emit_region(emit_slots, regions, region, from_root):
    slots, slot_records = emit_slots
    msg3 = [(0, 0, 13), (0, 0, 40), (0, 0, 2)]
    want = run_emit(slots, slot_records, msg3, 1, 40, region_records=57, region=region,
                    regions=regions, from_root=from_root)
    assert want[0] == 5 * (57 * region + 13)


@pytest.mark.parametrize("from_root", [False, True])
def test_emit_refuses_a_region_that_does_not_exist(emit_slots, from_root):
    slots, slot_records = emit_slots
    for regions, region in [(1, 1), (3, 3), (3, NO_REGION), (3, 1 << 32)]:
        assert run_emit(slots, slot_records, [(0, 0, 40)], 0, 40, region_records=40, region=region,
                        regions=regions, from_root=from_root) == ref.REFUSED


@pytest.mark.parametrize("P,me,bad", [(1, 0, 0), (3, 1, 0), (3, 1, 1), (3, 1, 2), (64, 5, 63),
                                      (64, 63, 0), (8, 0, 7)])
def test_emit_refuses_any_status_and_any_flag(emit_slots, P, me, bad):
    """Rank `bad` (below me, me itself, above me) reports a status, then each flag alone."""
    slots, slot_records = emit_slots
    ok = [(0, 0, 3)] * P
    ok[me] = (0, 0, 40)
    flags = [ref.SEND_OVERFLOW, ref.RECV_TRUNCATED, ref.ABORT, ref.TOO_MANY_SAMPLES,
             ref.GATHER_OVERFLOW, 1 << 31]
    for status, flag in [(1, 0), (ref.MAP_REDO, 0), (-1, 0), (1 << 30, 0)] + [(0, f) for f in flags]:
        msg3 = list(ok)
        msg3[bad] = (status, flag, msg3[bad][2])
        assert run_emit(slots, slot_records, msg3, me, 40, region_records=3 * P + 40) == ref.REFUSED
    assert run_emit(slots, slot_records, ok, me, 40, region_records=3 * P + 40) != ref.REFUSED


def test_emit_own_range_against_gather_records(emit_slots):
    slots, slot_records = emit_slots
    msg3 = [(0, 0, 5), (0, 0, 40)]
    assert run_emit(slots, slot_records, msg3, 1, 40, region_records=100)[0] == 25  # equal: passes
    assert run_emit(slots, slot_records, msg3, 1, 39, region_records=100) == ref.REFUSED
    assert run_emit(slots, slot_records, [(0, 0, 5), (0, 0, 41)], 1, 40, region_records=100) == ref.REFUSED
    assert run_emit(slots, slot_records, [(0, 0, 5), (0, 0, 1 << 40)], 1, 40,
                    region_records=100) == ref.REFUSED


def test_emit_range_against_its_region(emit_slots):
    slots, slot_records = emit_slots
    msg3 = [(0, 0, 5), (0, 0, 100), (0, 0, 40)]  # r = 5 + 40 (clamped), n = 40
    for region in (0, 2):
        assert run_emit(slots, slot_records, msg3, 2, 40, region_records=85,
                        region=region, regions=3)[0] == 5 * (85 * region + 45)
    msg3 = [(0, 0, 5), (0, 0, 9), (0, 0, 40)]
    assert run_emit(slots, slot_records, msg3, 2, 40, region_records=54)[0] == 70  # r + n equal
    assert run_emit(slots, slot_records, msg3, 2, 40, region_records=53) == ref.REFUSED
    msg3[2] = (0, 0, 41)  # (a report above the distinct keys: room for one record more)
    assert run_emit(slots, slot_records, msg3, 2, 41, region_records=54) == ref.REFUSED
    assert run_emit(slots, slot_records, msg3, 2, 41, region_records=55)[0] == 70


# ---- record forms ----

FORM_LENGTHS = [1, 4, 5, 12, 13, 20, 21, 28, 29, 32]
FORM_COUNTS = [1, (1 << 24) - 1, 1 << 24, 1 << 40]


def test_emit_record_forms():
    """Every key length at a word boundary of either form x counts at the short/long edge,
    in one tile that mixes both forms; each also alone in its own job."""
    recs = sorted((pad(bytes([0x41 + 4 * i + j]) + b"\x80" * (n - 1)), c)
                  for i, n in enumerate(FORM_LENGTHS) for j, c in enumerate(FORM_COUNTS))
    assert len({k for k, _ in recs}) == 40
    sizes = {ref.compact_words_ref(k, c) for k, c in recs}
    assert sizes == {1, 2, 3, 4, 5}
    slots = full([recs[0::2], recs[1::2]])
    want = run_emit(slots, 20, [(0, 0, 40)], 0, 40, region_records=40)
    assert len(want[1]) == sum(ref.compact_words_ref(k, c) for k, c in recs)
    # decoded by the host, the records are the keys and counts again
    res = C.Result.from_compact(want[1], [(0, 40)])
    assert [(pad(k), c) for k, _v, c in res.entries()] == recs
    for k, c in recs[::3]:
        run_emit(full([[(k, c)]]), 4, [(0, 0, 1)], 0, 1, region_records=1)


@pytest.mark.parametrize("form", ["short", "long"])
def test_emit_tile_of_five_word_records(form):
    """1,024 first copies of five words each: the whole LDS staging area of a tile, and one
    tile more behind it."""
    keys = [pad(b"%04d" % i + b"\xfe" * 28) for i in range(1030)]
    count = 3 if form == "short" else 1 << 24
    runs = [[(k, count) for k in keys[0::2]], [(k, count) for k in keys[1::2]]]
    want = run_emit(full(runs), 515, [(0, 0, 1030)], 0, 1030, region_records=1030)
    assert len(want[1]) == 5 * 1030  # the records fill their 40-B room exactly
    want = run_emit(full([runs[0][:512], runs[1][:512]]), 515, [(0, 0, 1024)], 0, 1024,
                    region_records=1024)
    assert len(want[1]) == 5 * 1024


# ---- totals, look-back and the hand-off ----

@pytest.mark.parametrize("total", [0, 1, 1024, 1025, 4097])
def test_emit_totals_around_the_tile(total):
    rng = random.Random(total + 1)
    if total < 2:
        runs = [[], [(pad(b"only"), 5)][:total], []]
    else:
        lengths = split_total(total, 4, rng)
        universe = word_keys(max(max(lengths), total * 3 // 4), rng, 1, 20)
        runs = [draw_run(universe, n, rng) for n in lengths]
    slot_records = max(1, max(len(r) for r in runs))
    uniq = ref.acc_ref(runs)[0]
    msg3 = [(0, 0, 3), (0, 0, uniq), (0, 0, 1)]
    want = run_emit(full(runs), slot_records, msg3, 1, max(uniq, 3), region_records=uniq + 3)
    assert want[0] == 15
    if total == 0:
        assert want[1] == []  # the stamp is written (checked above), nothing else


def test_emit_small_total_in_a_large_grid():
    """8 slots of 2,048 records (16 tiles in the grid), 5 records merged: 15 workgroups find
    no tile of theirs and still count, so the last one stamps."""
    runs = [[] for _ in range(8)]
    runs[1] = [(pad(b"b"), 2), (pad(b"d"), 1 << 30)]
    runs[6] = [(pad(b"a"), 1), (pad(b"b"), 3), (pad(b"c" * 30), 9)]
    want = run_emit(full(runs), 2048, [(0, 0, 4)], 0, 4, region_records=4)
    assert len(want[1]) == 1 + 1 + 5 + 2  # a, b, thirty c's (short form), d (long form)
    assert run_emit(full([[] for _ in range(8)]), 2048, [(0, 0, 0)], 0, 0, region_records=1)[1] == []
    # headers that clamp, in the same grid
    big = [(k, 1) for k in numbered(range(2048))]
    slots = [(OK, 1 << 40, big), (REDO, 2048, big), (OK, 2048, big), (OK, 0, big)] + full(runs[4:])
    run_emit(slots, 2048, [(0, 0, 2052)], 0, 2052, region_records=2052)


@pytest.mark.parametrize("first_total,second_total", [(3000, 700), (700, 3000), (0, 1500), (1500, 0)])
def test_emit_two_jobs_on_the_same_scratch(first_total, second_total):
    """As enqueue_range_tail runs them: the second merge + emit reuses the look-back words,
    the tile counter, the done counter and the merged array as the first left them."""
    jobs = []
    for j, total in enumerate((first_total, second_total)):
        rng = random.Random(total + j)
        if total:
            lengths = split_total(total, 3, rng)
            universe = word_keys(max(max(lengths), total * 3 // 4), rng, 1 + j, 20)
            runs = [draw_run(universe, n, rng) for n in lengths]
        else:
            runs = [[], [], []]
        jobs.append(runs)
    slot_records = max(len(r) for runs in jobs for r in runs)
    msg3 = [[(0, 0, 2 + j), (0, 0, ref.acc_ref(runs)[0])] for j, runs in enumerate(jobs)]
    gather = max(m[1][2] for m in msg3)
    out = C.exch_emit_compact(native(full(jobs[0])), slot_records, msg3[0], None, 0, 1, gather + 3,
                              1, gather, SEQ, 2, native(full(jobs[1])), msg3[1])
    assert len(out) == 2
    for j in range(2):
        want = ref.emit_ref(jobs[j], msg3[j], 0, 1, gather + 3, 1, gather)
        assert want[0] == 5 * (2 + j)
        check_emit(out[j], want, 2, 1, SEQ + j)
        check_acc(out[j]["acc"], jobs[j])


def test_emit_second_job_behind_a_refused_one(emit_slots):
    """A refused emit leaves `done` at 0 and the scratch as the merge made it; the job behind
    it is exact."""
    slots, slot_records = emit_slots
    runs = ref.slot_runs(slots, slot_records)
    bad, good = [(0, ref.GATHER_OVERFLOW, 40)], [(0, 0, 40)]
    out = C.exch_emit_compact(native(slots), slot_records, bad, None, 0, 1, 40, 0, 40, SEQ, 2,
                              native(slots), good)
    check_emit(out[0], ref.REFUSED, 1, 0, SEQ)
    check_emit(out[1], ref.emit_ref(runs, good, 0, 1, 40, 0, 40), 1, 0, SEQ + 1)


@pytest.mark.parametrize("gather_delta", [0, -1])
def test_chain_rank_report_emit(gather_delta):
    """rank_slots -> exch_report on its accumulators -> the emit with that report as this
    rank's: the report's n_out, total and out_words are the reference's, and the emitted
    range is exactly out_words long (or, one record short of room, refused)."""
    rng = random.Random(77)
    universe = word_keys(900, rng, 1, 31)
    runs = [draw_run(universe, n, rng) for n in (700, 64, 0, 333, 512)]
    slots, slot_records = full(runs), 700
    firsts, tokens, words = ref.acc_ref(runs)
    gather = firsts + gather_delta
    acc = C.exch_rank_slots(native(slots), slot_records)["acc"]
    rep = C.exch_report([(st, n) for st, n, _r in slots], slot_records, 0, 700, acc, gather)
    assert (rep["n_out"], rep["total"], rep["out_words"]) == (firsts, tokens, words)
    assert rep["flags"] == (ref.GATHER_OVERFLOW if gather_delta else 0)
    msg3 = [(0, 0, 10), (rep["status"], rep["flags"], rep["n_out"]), (0, 0, 10)]
    want = run_emit(slots, slot_records, msg3, 1, max(gather, 10), region_records=firsts + 10)
    if gather_delta:
        assert want == ref.REFUSED
    else:
        assert want[0] == 50 and len(want[1]) == rep["out_words"]
