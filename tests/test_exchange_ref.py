"""The host's splitter choice (dist.cpp choose_splitters) against the exact reference of the
shuffle's rules (tests/exchange_ref.py), and the reference against hand-worked cases.  No GPU.

The device planner (exch_plan_kernel) works in integers; the host used to work in double
with weights count / s.  While s is a power of two the doubles are exact and the two rules
are one: the host skips samples while run + w <= total p / P; times s that is an inequality
over integers, and an integer x has x > y exactly when x > floor(y).  At s = 3, 10 and 63 the
double host disagreed with the exact rule (equal weights, distinct samples: the rounded
prefix sums miss the tie with the target and the neighbouring sample is picked), so the host
now uses the same integer arithmetic; those sample counts are kept as cases here."""
import random

import pytest

import locust_amd as lc

import exchange_ref as ref

C = lc._C


def host_splitters(lists, counts, S, parts):
    flat = ref.blob(k for lst in lists for k in lst)
    return ref.unblob(C.choose_splitters(flat, S, counts, parts))


def make_weights(kind, P, rng):
    if kind == "equal":
        return [rng.choice([1, 7, 1000])] * P
    if kind == "random_with_zeros":
        return [rng.choice([0, rng.randint(1, 10**6)]) for _ in range(P)]
    if kind == "one_heavy":
        w = [1] * P
        w[rng.randrange(P)] = 10**6
        return w
    assert kind == "tiny"
    return [rng.randint(0, 5) for _ in range(P)]


def make_samples(kind, P, S, weights, rng):
    lists = []
    for r in range(P):
        if weights[r] == 0:
            lst = [ref.ALL_ONES] * S  # an empty shard's samples
        elif kind == "distinct":
            lst = sorted(ref.pad(b"k%09d" % rng.randrange(10**9)) for _ in range(S))
        elif kind == "all_equal":
            lst = [ref.pad(b"same")] * S
        else:
            assert kind == "duplicates"
            lst = sorted(ref.pad(b"d%02d" % rng.randrange(4)) for _ in range(S))
        lists.append(lst)
    return lists


WEIGHTS = ["equal", "random_with_zeros", "one_heavy", "tiny"]
SAMPLES = ["distinct", "all_equal", "duplicates"]


# S = 1, 2, 8, 64: the powers of two at which the double host was already exact;
# S = 3, 10, 63: where it was not (see the module docstring)
@pytest.mark.parametrize("S", [1, 2, 8, 64, 3, 10, 63])
@pytest.mark.parametrize("P", [1, 2, 3, 8, 64])
def test_host_splitters_equal_reference(S, P):
    rng = random.Random(S * 1000 + P)
    for wk in WEIGHTS:
        for sk in SAMPLES:
            for _ in range(4):
                w = make_weights(wk, P, rng)
                lists = make_samples(sk, P, S, w, rng)
                assert host_splitters(lists, w, S, P) == ref.splitters(lists, w, P), (wk, sk, w)


@pytest.mark.parametrize("S,P,count", [(3, 3, 7), (10, 2, 7), (63, 2, 1000), (63, 3, 1000)])
def test_host_splitters_ties_at_odd_sample_counts(S, P, count):
    """Equal weights and distinct samples: the inclusive weight of sample (S p - 1) equals
    total p / P exactly, so the splitter is the NEXT sample.  count / S summed in double
    overshoots that tie (0.1 + 0.1 + 0.1 > 0.3) and stopped one sample early."""
    lists = [[ref.pad(b"r%dk%03d" % (r, i)) for i in range(S)] for r in range(P)]
    order = sorted(k for lst in lists for k in lst)
    want = [order[S * p] for p in range(1, P)]  # S p samples weigh exactly total p / P
    assert ref.splitters(lists, [count] * P, P) == want
    assert host_splitters(lists, [count] * P, S, P) == want


def test_host_splitters_parts_differ_from_ranks():
    """The splitter count is `parts`, whatever the number of ranks that sampled."""
    rng = random.Random(5)
    for ranks, parts in [(1, 4), (4, 1), (3, 8), (8, 3)]:
        w = [rng.randint(1, 50) for _ in range(ranks)]
        lists = make_samples("distinct", ranks, 8, w, rng)
        assert host_splitters(lists, w, 8, parts) == ref.splitters(lists, w, parts)


def test_host_splitters_large_counts_stay_exact():
    """Counts near 2^40 with 64 samples of 64 ranks: the products pass 2^53, where a double
    would start to round."""
    rng = random.Random(6)
    w = [(1 << 40) + rng.randrange(1000) for _ in range(64)]
    lists = make_samples("distinct", 64, 64, w, rng)
    assert host_splitters(lists, w, 64, 64) == ref.splitters(lists, w, 64)


# ---- the reference itself, on cases small enough to work out by hand ----

def K(s):
    return ref.pad(s)


def test_reference_constants_match_the_headers():
    assert (ref.SEND_OVERFLOW, ref.RECV_TRUNCATED, ref.ABORT, ref.TOO_MANY_SAMPLES,
            ref.GATHER_OVERFLOW) == (C.EXCH_SEND_OVERFLOW, C.EXCH_RECV_TRUNCATED, C.EXCH_ABORT,
                                     C.EXCH_TOO_MANY_SAMPLES, C.EXCH_GATHER_OVERFLOW)
    assert (ref.SLOT_OK, ref.SLOT_FAILED, ref.SLOT_REDO) == (C.SLOT_OK, C.SLOT_FAILED, C.SLOT_REDO)
    assert (ref.MAX_PLAN_SAMPLES, ref.MAX_RANKS, ref.MAP_REDO) == (
        C.EXCH_MAX_PLAN_SAMPLES, C.EXCH_MAX_RANKS, C.EXCH_MAP_REDO)
    assert ref.pad(b"ab")[:8] == C.pack_key(b"ab")[0].to_bytes(8, "big")
    assert ref.ALL_ONES == b"".join(w.to_bytes(8, "big") for w in [2**64 - 1] * 4)


def test_reference_samples_by_hand():
    """n = 5, S = 2: indices 1*5//4 = 1 and 3*5//4 = 3.  n = 2, S = 4: 1*2//8 = 0, 3*2//8 = 0,
    5*2//8 = 1, 7*2//8 = 1.  n = 0: the all-ones key."""
    keys = [K(b"a"), K(b"b"), K(b"c"), K(b"d"), K(b"e")]
    assert ref.samples(keys, 2) == [K(b"b"), K(b"d")]
    assert ref.samples(keys[:2], 4) == [K(b"a"), K(b"a"), K(b"b"), K(b"b")]
    assert ref.samples(keys, 1) == [K(b"c")]
    assert ref.samples([], 3) == [ref.ALL_ONES] * 3


def test_reference_splitters_two_ranks_by_hand():
    """Rank 0: samples a, c, weight 10 each.  Rank 1: samples b, d, weight 2 each.
    Order a(10) b(2) c(10) d(2): inclusive 10, 12, 22, 24; total 24.
    P = 2: target 12 -> first inclusive weight above 12 is c (22).
    P = 3: targets 8 and 16 -> a (10 > 8) and c (22 > 16).
    P = 4: targets 6, 12, 18 -> a, c, c."""
    lists = [[K(b"a"), K(b"c")], [K(b"b"), K(b"d")]]
    w = [10, 2]
    assert ref.splitters(lists, w, 2) == [K(b"c")]
    assert ref.splitters(lists, w, 3) == [K(b"a"), K(b"c")]
    assert ref.splitters(lists, w, 4) == [K(b"a"), K(b"c"), K(b"c")]
    assert ref.splitters(lists, w, 1) == []


def test_reference_splitters_three_ranks_with_an_empty_one_by_hand():
    """Ranks 0 and 2 hold 3 records each, rank 1 none (all-ones samples, weight 0), S = 1.
    Order m(3, rank 0) m(3, rank 2) ones(0): inclusive 3, 6, 6; total 6.
    P = 3: targets 2 and 4 -> m (3 > 2) and m (6 > 4).  With every weight 0 the total is 0,
    no inclusive weight exceeds the target 0 and every splitter is the all-ones key."""
    lists = [[K(b"m")], [ref.ALL_ONES], [K(b"m")]]
    assert ref.splitters(lists, [3, 0, 3], 3) == [K(b"m"), K(b"m")]
    assert ref.splitters(lists, [0, 0, 0], 3) == [ref.ALL_ONES, ref.ALL_ONES]


def test_reference_offsets_and_slots_by_hand():
    """Keys b d f h with splitters d (equal to a key: it opens the upper bucket) and g:
    offsets 0, 1, 3, 4.  slot_records = 1: bucket 1 (d, f) overflows -> redo, n = 2, one
    record kept; the flag is set; the other slots are whole."""
    keys = [K(b"b"), K(b"d"), K(b"f"), K(b"h")]
    assert ref.offsets(keys, [K(b"d"), K(b"g")]) == [0, 1, 3, 4]
    assert ref.offsets(keys, [K(b"a"), ref.ALL_ONES]) == [0, 0, 4, 4]
    assert ref.offsets([], [K(b"a")]) == [0, 0, 0]
    # P = 3 ranks with S = 1: samples d, g, z with equal weights 1 -> order d g z, inclusive
    # 1 2 3, total 3, targets 1 and 2 -> splitters g (2 > 1) and z (3 > 2): offsets 0 3 4 4
    got = ref.plan_pack(3, 1, [0, 0, 0], [1, 1, 1], [[K(b"d")], [K(b"g")], [K(b"z")]], keys,
                        [5, 6, 7, 8], 2)
    assert got["off"] == [0, 3, 4, 4] and got["max_bucket"] == 3
    assert got["flags"] == ref.SEND_OVERFLOW
    s0, s1, s2 = got["slots"]
    assert (s0["status"], s0["n"], s0["keys"], s0["counts"]) == (ref.SLOT_REDO, 3, keys[:2], [5, 6])
    assert (s1["status"], s1["n"], s1["keys"], s1["counts"]) == (ref.SLOT_OK, 1, keys[3:], [8])
    assert (s2["status"], s2["n"], s2["keys"]) == (ref.SLOT_OK, 0, [])
    # a failed rank: every header failed, no records, the offsets as planned
    got = ref.plan_pack(3, 1, [0, 9, 0], [1, 1, 1], [[K(b"d")], [K(b"g")], [K(b"z")]], keys,
                        [5, 6, 7, 8], 8)
    assert got["flags"] == ref.ABORT and got["off"] == [0, 3, 4, 4]
    assert [s["status"] for s in got["slots"]] == [ref.SLOT_FAILED] * 3
    assert [s["n"] for s in got["slots"]] == [3, 1, 0] and not any(s["keys"] for s in got["slots"])


def test_reference_report_by_hand():
    acc = [0] * 192
    acc[0:3] = [2, 10, 4]
    acc[189:192] = [1, 5, 3]
    ok = [(ref.SLOT_OK, 4), (ref.SLOT_OK, 0)]
    r = ref.report(ok, 4, 0, 7, acc, 3)
    assert r == {"status": 0, "flags": 0, "max_bucket": 7, "n_out": 3, "total": 15, "out_words": 7}
    assert ref.report(ok, 4, 0, 7, acc, 2)["flags"] == ref.GATHER_OVERFLOW
    assert ref.report([(ref.SLOT_OK, 5)], 4, 0, 7, acc, 3)["flags"] == ref.RECV_TRUNCATED
    assert ref.report([(ref.SLOT_REDO, 1)], 4, 0, 7, acc, 3)["flags"] == ref.RECV_TRUNCATED
    dead = ref.report(ok, 4, ref.ABORT, 7, acc, 0)
    assert (dead["flags"], dead["n_out"], dead["total"], dead["out_words"]) == (ref.ABORT, 0, 0, 0)


# ---- the tail's reference: slot runs, merge, accumulators, compact records, emit ----

A, B, Cc, D = K(b"a"), K(b"b"), K(b"c"), K(b"d")
RUNS = [[(A, 1), (Cc, 2)], [(A, 10), (B, 20), (Cc, 30)], [(Cc, 100), (D, 5)]]


def test_tail_constants_match_the_headers():
    assert (ref.MERGE_MAX_RECORDS, ref.MERGE_MAX_COUNT) == (C.MERGE_MAX_RECORDS, C.MERGE_MAX_COUNT)
    assert ref.MAX_RANKS == C.MAX_SLOT_RANKS
    assert ref.pad32(b"x" * 32) == b"x" * 32 and ref.pad32(b"x") == ref.pad(b"x")


def test_reference_slot_runs_by_hand():
    """slot_records = 3.  Only an ok slot counts, by min(n, 3): a failed and a redone slot
    with records are empty, n = 2 hides the third record, n = 4 and n = 2^40 clamp to 3."""
    recs = [(A, 1), (B, 2), (Cc, 3)]
    slots = [(ref.SLOT_OK, 2, recs), (ref.SLOT_FAILED, 2, recs), (ref.SLOT_REDO, 1, recs),
             (ref.SLOT_OK, 4, recs), (ref.SLOT_OK, 1 << 40, recs), (ref.SLOT_OK, 0, recs),
             (ref.SLOT_OK, 3, recs)]
    assert ref.slot_runs(slots, 3) == [recs[:2], [], [], recs, recs, [], recs]


def test_reference_merge_by_hand():
    """a: runs 0, 1 (1 + 10); b: run 1; c: runs 0, 1, 2 (2 + 30 + 100); d: run 2."""
    assert ref.merged_ref(RUNS) == [(A, 11), (A, 0), (B, 20), (Cc, 132), (Cc, 0), (Cc, 0), (D, 5)]
    assert ref.merge_out_ref(RUNS) == ([(A, 11), (B, 20), (Cc, 132), (D, 5)], (7, 4, 168))
    assert ref.acc_ref(RUNS) == (4, 168, 4)  # four one-byte keys: one word each
    # empty runs anywhere change nothing; no run at all gives nothing
    assert ref.merged_ref([[], RUNS[0], [], RUNS[1], RUNS[2], []]) == ref.merged_ref(RUNS)
    assert ref.merge_out_ref([[], []]) == ([], (0, 0, 0)) and ref.acc_ref([[]]) == (0, 0, 0)
    # no key shared: the runs interleave, every count its own
    two = [[(A, 1), (Cc, 3)], [(B, 2), (D, 1 << 32)]]
    assert ref.merged_ref(two) == [(A, 1), (B, 2), (Cc, 3), (D, 1 << 32)]
    assert ref.acc_ref(two) == (4, 6 + (1 << 32), 1 + 1 + 1 + 2)  # d takes the long form


def test_reference_compact_records_by_hand():
    """Short: [key bytes 0-3][count : 24][0][kb : 6][0].  'ab' x 3: 0x6162_0000, 3 << 8,
    2 << 1.  'abcdef' x 5: bytes 4-5 'ef' open a second word.  Long, 'abcde' x 2^24:
    2^24 << 8 | 5 << 1 | 1, then the packed key word."""
    assert ref.compact_record_ref(b"ab", 3) == [0x6162000000000304]
    assert ref.compact_record_ref(b"abcdef", 5) == [0x616263640000050C, 0x6566000000000000]
    assert ref.compact_record_ref(b"abcde", 1 << 24) == [0x10000000B, 0x6162636465000000]
    assert ref.compact_record_ref(K(b"ab"), 3) == [0x6162000000000304]  # padded or not
    words = {(1, 1): 1, (4, 1): 1, (5, 1): 2, (12, 1): 2, (13, 1): 3, (20, 1): 3, (21, 1): 4,
             (28, 1): 4, (29, 1): 5, (32, 1): 5, (4, (1 << 24) - 1): 1,
             (1, 1 << 24): 2, (8, 1 << 24): 2, (9, 1 << 24): 3, (16, 1 << 40): 3,
             (17, 1 << 40): 4, (24, 1 << 24): 4, (25, 1 << 24): 5, (32, 1 << 40): 5}
    for (kb, count), want in words.items():
        key = ref.pad32(b"k" * kb)
        assert ref.compact_words_ref(key, count) == want, (kb, count)
        assert len(ref.compact_record_ref(key, count)) == want, (kb, count)


def test_reference_emit_by_hand():
    """Three ranks with ranges of 3, 4 and 9 keys, gather_records = 4, regions of 10 records.
    Rank 1 in region 1: r = 3, 3 + 4 <= 10, first word 5 (10 + 3) = 65.  Rank 2: its own
    9 > 4 is refused; with gather_records = 9, r = 7 and 7 + 9 > 10 is refused, 7 + 3 fits."""
    m = [(0, 0, 3), (0, 0, 4), (0, 0, 9)]
    words = [(0x61 << 56) | (11 << 8) | 2, (0x62 << 56) | (20 << 8) | 2,
             (0x63 << 56) | (132 << 8) | 2, (0x64 << 56) | (5 << 8) | 2]
    assert ref.emit_ref(RUNS, m, 1, 2, 10, 1, 4) == (65, words)
    assert ref.emit_ref(RUNS, m, 0, 2, 10, 0, 4) == (0, words)
    assert ref.emit_ref(RUNS, m, 0, 1, 10, 2, 4) == ref.REFUSED
    assert ref.emit_ref(RUNS, m, 0, 1, 10, 2, 9) == ref.REFUSED
    assert ref.emit_ref(RUNS, m[:2] + [(0, 0, 3)], 0, 1, 10, 2, 9) == (35, words)
    assert ref.emit_ref(RUNS, m[:2] + [(0, 0, 4)], 0, 1, 10, 2, 9) == ref.REFUSED
    # a lower rank's n_out above gather_records counts as gather_records
    assert ref.emit_ref(RUNS, [(0, 0, 50), (0, 0, 4)], 0, 1, 10, 1, 4) == (20, words)
    # the region must exist; any status, any flag, of any rank refuses
    assert ref.emit_ref(RUNS, m, 2, 2, 10, 1, 4) == ref.REFUSED
    assert ref.emit_ref(RUNS, [(0, 0, 3), (0, 0, 4), (1, 0, 9)], 1, 2, 10, 1, 4) == ref.REFUSED
    assert ref.emit_ref(RUNS, [(0, 16, 3), (0, 0, 4), (0, 0, 9)], 1, 2, 10, 1, 4) == ref.REFUSED
    # nothing merged: accepted, no words
    assert ref.emit_ref([[], []], [(0, 0, 0)], 0, 1, 10, 0, 4) == (0, [])


@pytest.mark.parametrize("count", [1, (1 << 24) - 1, 1 << 24, (1 << 40) - 1])
def test_reference_compact_records_decode(count):
    """Every key length through the host decoder (Result.from_compact)."""
    keys = [bytes([0x41 + n % 26]) + bytes((0x80 + 7 * i) % 256 or 0xff for i in range(n - 1))
            for n in range(1, 33)]
    keys.sort()
    assert sorted(len(k) for k in keys) == list(range(1, 33)) and all(b"\0" not in k for k in keys)
    words = []
    for k in keys:
        rec = ref.compact_record_ref(ref.pad32(k), count)
        assert len(rec) == ref.compact_words_ref(ref.pad32(k), count)
        words += rec
    r = C.Result.from_compact(words, [(0, len(keys))])
    assert [(k, c) for k, _v, c in r.entries()] == [(k, count) for k in keys]


def test_slot_gather_takes_the_standard_path_beyond_the_merge_bounds():
    """The gather strategy's root merge is enqueued behind the all-gather, before any header
    is known; its look-back value holds 22 bits of records and 40 bits of counts.  The job
    enters it only for a shape that fits and falls back when the headers announce more
    tokens than it can count."""
    fits = C.slot_merge_fits
    assert fits(1, 2048, 0) and fits(8, 2048, 12345) and fits(64, 65535, 0)
    assert fits(64, 65536, 0) is False  # 2^22 records
    assert fits(3, (1 << 22) // 3, 0) and not fits(3, (1 << 22) // 3 + 1, 0)
    assert fits(1, (1 << 22) - 1, 0) and not fits(1, 1 << 22, 0)
    assert not fits(65, 1, 0)
    assert not fits(1 << 32, 1 << 32, 0)  # (the product does not wrap)
    assert fits(8, 2048, (1 << 40) - 1) and not fits(8, 2048, 1 << 40)
    assert not fits(8, 2048, 2**64 - 1)
