"""The device shuffle's kernels (exchange.hip, shuffle.hip), each launched alone on host-made
input through the stage entry points of locust/exch_stage.hpp and compared with the plain
integer reference of the same step (tests/exchange_ref.py).  Every comparison is exact.

Whole jobs (test_dist.py) only show that the final word counts are right, which any
consistent splitters give; here the splitters themselves, the 64-ary lower bound at its
off-by-one positions, the paths no job enters (unsorted samples, too many samples, P = 64,
empty ranks), the slot layout, both samplers, the header and the report are pinned.

Left out: P = 65.  exch_pack_kernel copies ctl->off[0..P] into a table of 65 entries and
reads s_off[d + 1] for d < P, so at P = 65 it would leave that table; the host refuses the
shape before any launch (ShardEngine and the stage entry points alike), which is asserted."""
import random

import pytest

import locust_amd as lc

import exchange_ref as ref

pytestmark = pytest.mark.gpu

C = lc._C
pad = ref.pad


# ---------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------

def run_plan(P, S, status, n_local, lists, keys, counts, slot_records, pack_cap=0):
    assert len(lists) == P and all(len(lst) == S for lst in lists)
    return C.exch_plan_pack(P, S, status, n_local, ref.blob(k for lst in lists for k in lst),
                            ref.blob(keys), counts, slot_records, pack_cap)


def check_slots(got_slots, want_slots, slot_records, failed):
    assert len(got_slots) == len(want_slots)
    for d, (g, w) in enumerate(zip(got_slots, want_slots)):
        head = (g["status"], g["record_flags"], g["n"], g["slot_cap"])
        assert head == (w["status"], w["record_flags"], w["n"], w["slot_cap"]), d
        assert g["rest"] == [0] * 7, d  # the header's other fields are written as zeros
        held = len(w["keys"])
        # records past `held` are untouched; the last held one is written (a record never
        # equals the fill pattern: its key is NUL padded)
        assert g["dirty_records"] == held, (d, g["dirty_records"], held)
        if failed:
            continue  # (no record written at all: dirty_records == 0 above)
        assert g["tail_intact"], d
        assert held == min(w["n"], slot_records)
        assert ref.unblob(g["keys"]) == w["keys"], d
        assert g["counts"] == w["counts"], d


def check_plan(got, want, slot_records):
    assert got["off"] == want["off"]
    assert got["flags"] == want["flags"]
    assert got["max_bucket"] == want["max_bucket"]
    failed = bool(want["flags"] & (ref.ABORT | ref.TOO_MANY_SAMPLES))
    check_slots(got["slots"], want["slots"], slot_records, failed)


def chunks(seq, size):
    return [seq[i:i + size] for i in range(0, len(seq), size)]


# ---------------------------------------------------------------------------------------
# lower bound: the plan kernel's 64-ary search and bucket_offsets_kernel's binary search
# ---------------------------------------------------------------------------------------

KEYSETS = {
    # key i of each set; the sets ascend with i
    "first_word": lambda v: b"k%07d" % v,                  # differ in bytes 1..7
    "second_word": lambda v: b"q" * 8 + b"%08d" % v,       # differ only in bytes 8..15
    "fourth_word": lambda v: b"p" * 24 + b"%07d" % v,      # differ only in bytes 24..30
}
LB_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 100003]

_lb_cache = {}


def lb_case(keyset, n):
    """Local keys (value 2 i for i < n) and the sorted table of splitter values."""
    if (keyset, n) in _lb_cache:
        return _lb_cache[keyset, n]
    mk = KEYSETS[keyset]
    keys = [pad(mk(2 * i)) for i in range(n)]
    assert keys == sorted(keys)
    pos = set()
    if n:
        pos.update({0, n - 1})
        step = -(-n // 64)  # round 1 probes lane * step
        first = [lane * step for lane in range(64) if lane * step < n]
        pos.update(first)
        # round 2, for a splitter behind probe j: lo = j step + 1, hi = min((j + 1) step, n).
        # Every interval j up to n = 4097 (that is every key or every other one); at 100,003
        # the first, a middle and the last interval, to keep the case to a few launches.
        for j in range(len(first)) if n <= 5000 else (0, len(first) // 2, len(first) - 1):
            lo, hi = first[j] + 1, min(first[j] + step, n)
            if lo < hi:
                step2 = -(-(hi - lo) // 64)
                pos.update(q for q in range(lo, hi, step2))
    table = {mk(0)[:1], mk(0)[:1] + b"zzz", ref.ALL_ONES}  # below every key, above every key
    table = {t if len(t) == ref.KEY_BYTES else pad(t) for t in table}
    for q in sorted(pos):
        table.add(pad(mk(2 * q)))      # equal to key q: key q opens the upper bucket
        table.add(pad(mk(2 * q + 1)))  # just above key q (between q and q + 1, or past the end)
    if n == 0:
        table.update({pad(mk(0)), pad(mk(1))})
    table = sorted(table)
    _lb_cache.clear()  # (one case at a time: the big ones are megabytes)
    _lb_cache[keyset, n] = (keys, table)
    return keys, table


def test_lower_bound_table_covers_the_edge_positions():
    keys, table = lb_case("first_word", 129)
    # below the first key, equal to key 0, between keys 0 and 1, equal to / above the last
    assert table[0] < keys[0] and keys[0] in table and pad(b"k%07d" % 1) in table
    assert keys[-1] in table and pad(b"k%07d" % 257) in table and table[-1] == ref.ALL_ONES
    # every round-1 probe of n = 129 (step 3) as a key and just above it
    assert all(pad(b"k%07d" % (6 * lane)) in table and pad(b"k%07d" % (6 * lane + 1)) in table
               for lane in range(43))


@pytest.mark.parametrize("n", LB_SIZES)
@pytest.mark.parametrize("keyset", list(KEYSETS))
def test_plan_lower_bound(keyset, n):
    """P = 64, S = 1, every n_local = 1: the inclusive weights are 1..64 and the targets
    1..63, so the 63 sorted samples behind the first ARE the 63 splitters -- one launch
    searches 63 chosen values."""
    keys, table = lb_case(keyset, n)
    blob = ref.blob(keys)
    counts = list(range(1, n + 1))
    lowest = table[0]
    for group in chunks(table, 63):
        group = group + [ref.ALL_ONES] * (63 - len(group))
        lists = [[lowest]] + [[s] for s in group]
        want = ref.plan_pack(64, 1, [0] * 64, [1] * 64, lists, keys, counts, 8)
        # the reference's splitters are the chosen values, and a key equal to one lands in
        # the upper bucket
        assert ref.splitters(lists, [1] * 64, 64) == group
        for p, s in enumerate(group):
            if s in keys[:4] or (keys and s == keys[-1]):
                assert keys[want["off"][p + 1]] == s
        got = C.exch_plan_pack(64, 1, [0] * 64, [1] * 64, ref.blob(k for lst in lists for k in lst),
                               blob, counts, 8, 0)
        check_plan(got, want, 8)


@pytest.mark.parametrize("n", LB_SIZES)
@pytest.mark.parametrize("keyset", list(KEYSETS))
def test_bucket_offsets(keyset, n):
    """bucket_offsets_kernel over the same table; at P = 64 the launch has 65 threads of
    work: a second workgroup."""
    keys, table = lb_case(keyset, n)
    blob = ref.blob(keys)
    assert C.exch_offsets(blob, b"", 1) == [0, n]
    for P in (2, 63, 64):
        groups = chunks(table, P - 1)
        if P == 2:  # one splitter per launch: the ends and a spread of the middle
            picks = sorted({0, 1, 2, len(table) // 3, len(table) // 2, len(table) - 3,
                            len(table) - 2, len(table) - 1} & set(range(len(table))))
            groups = [[table[i]] for i in picks]
        for group in groups:
            group = group + [ref.ALL_ONES] * (P - 1 - len(group))
            assert C.exch_offsets(blob, ref.blob(group), P) == ref.offsets(keys, group), (P, group[0])


# ---------------------------------------------------------------------------------------
# splitter choice
# ---------------------------------------------------------------------------------------

def word_key(rng):
    return pad(bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(1, 12))))


@pytest.fixture(scope="module")
def local_records():
    rng = random.Random(11)
    keys = sorted({word_key(rng) for _ in range(3500)})
    return keys, [rng.randint(1, 1 << 40) for _ in keys]


PS = [(1, 64), (2, 64), (3, 64), (16, 64), (17, 60), (18, 56), (64, 16), (64, 1), (5, 7)]
WEIGHTS = ["equal", "random", "one_huge", "half_empty", "all_empty"]
SAMPLES = ["distinct", "one_key", "half_repeated", "same_lists", "one_list_unsorted"]


def choice_case(P, S, weights, samples, rng):
    if weights == "equal":
        n_local = [1234] * P
    elif weights == "random":
        n_local = [rng.randint(1, 10**6) for _ in range(P)]
    elif weights == "one_huge":
        n_local = [1] * P
        n_local[rng.randrange(P)] = 4 * 10**9
    elif weights == "half_empty":
        n_local = [0 if r % 2 else rng.randint(1, 10**6) for r in range(P)]
    else:
        n_local = [0] * P

    def distinct():
        out = set()
        while len(out) < S:
            out.add(word_key(rng))
        return sorted(out)

    if samples == "distinct":
        lists = [distinct() for _ in range(P)]
    elif samples == "one_key":
        lists = [[pad(b"same")] * S for _ in range(P)]
    elif samples == "half_repeated":  # n_local < S: a key is sampled several times
        lists = []
        for _ in range(P):
            lst = distinct()
            lst[:S // 2] = [lst[0]] * (S // 2)
            lists.append(sorted(lst))
    elif samples == "same_lists":  # every tie crosses the ranks
        lists = [distinct()] * P
    else:  # one list out of order: the all-pairs rank walk
        lists = [distinct() for _ in range(P)]
        lists[rng.randrange(P)].reverse()
    # an empty shard sends the all-ones key S times
    lists = [[ref.ALL_ONES] * S if n_local[r] == 0 else lists[r] for r in range(P)]
    return n_local, lists


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("P,S", PS)
def test_plan_splitter_choice(local_records, P, S, weights, samples):
    keys, counts = local_records
    rng = random.Random(f"{P}/{S}/{weights}/{samples}")
    n_local, lists = choice_case(P, S, weights, samples, rng)
    want = ref.plan_pack(P, S, [0] * P, n_local, lists, keys, counts, 64)
    check_plan(run_plan(P, S, [0] * P, n_local, lists, keys, counts, 64), want, 64)


def test_plan_unsorted_list_with_ties(local_records):
    """The all-pairs walk with equal keys inside and across the lists."""
    keys, counts = local_records
    rng = random.Random(3)
    lists = [[pad(b"k%d" % rng.randrange(6)) for _ in range(16)] for _ in range(5)]
    assert any(lst != sorted(lst) for lst in lists)
    n_local = [5, 0, 1000, 3, 77]
    want = ref.plan_pack(5, 16, [0] * 5, n_local, lists, keys, counts, 4000)
    check_plan(run_plan(5, 16, [0] * 5, n_local, lists, keys, counts, 4000), want, 4000)


# ---------------------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,S", [(32, 64), (64, 17)])
def test_plan_too_many_samples(local_records, P, S):
    keys, counts = local_records
    rng = random.Random(P)
    n_local, lists = choice_case(P, S, "random", "distinct", rng)
    n = len(keys)
    for slot_records in (16, n):
        got = run_plan(P, S, [0] * P, n_local, lists, keys, counts, slot_records)
        assert got["flags"] & ref.TOO_MANY_SAMPLES
        # every splitter is the all-ones key: bucket 0 holds every record
        assert got["off"] == [0] + [n] * P and got["max_bucket"] == n
        assert bool(got["flags"] & ref.SEND_OVERFLOW) == (n > slot_records)
        for s in got["slots"]:
            assert s["status"] == ref.SLOT_FAILED and s["dirty_records"] == 0
        check_plan(got, ref.plan_pack(P, S, [0] * P, n_local, lists, keys, counts, slot_records),
                   slot_records)


def test_more_than_64_ranks_is_refused_on_the_host():
    with pytest.raises(lc.LocustError, match="bad shape"):
        run_plan(65, 1, [0] * 65, [1] * 65, [[pad(b"a")]] * 65, [], [], 4)
    with pytest.raises(lc.LocustError, match="bad shape"):
        C.exch_pack([0] * 67, 0, b"", [], 4)


# (at P = 64 the ranks are 0..63: a rank of 64 or more does not exist, so the last rank and
# one in the middle stand for "a high rank")
@pytest.mark.parametrize("P,bad", [(3, 0), (3, 2), (64, 0), (64, 63), (64, 37)])
def test_plan_abort(local_records, P, bad):
    keys, counts = local_records
    rng = random.Random(P * 100 + bad)
    n_local, lists = choice_case(P, 16, "random", "distinct", rng)
    status = [0] * P
    status[bad] = ref.MAP_REDO if bad else 7
    got = run_plan(P, 16, status, n_local, lists, keys, counts, len(keys))
    assert got["flags"] == ref.ABORT
    for s in got["slots"]:
        assert s["status"] == ref.SLOT_FAILED and s["dirty_records"] == 0
    check_plan(got, ref.plan_pack(P, 16, status, n_local, lists, keys, counts, len(keys)), len(keys))


def test_plan_send_overflow_threshold(local_records):
    keys, counts = local_records
    rng = random.Random(8)
    n_local, lists = choice_case(3, 64, "equal", "distinct", rng)
    big = ref.plan_pack(3, 64, [0] * 3, n_local, lists, keys, counts, len(keys))["max_bucket"]
    assert 1 < big < len(keys)
    for slot_records in (big - 1, big, big + 1):
        got = run_plan(3, 64, [0] * 3, n_local, lists, keys, counts, slot_records)
        assert got["flags"] == (ref.SEND_OVERFLOW if slot_records < big else 0)
        for d, s in enumerate(got["slots"]):
            size = got["off"][d + 1] - got["off"][d]
            assert s["n"] == size  # the whole bucket, also when it is truncated
            assert s["status"] == (ref.SLOT_REDO if size > slot_records else ref.SLOT_OK)
            assert len(s["counts"]) == min(size, slot_records) and s["tail_intact"]
        assert max(s["n"] for s in got["slots"]) == big
        check_plan(got, ref.plan_pack(3, 64, [0] * 3, n_local, lists, keys, counts, slot_records),
                   slot_records)


# ---------------------------------------------------------------------------------------
# pack layout
# ---------------------------------------------------------------------------------------

def run_pack(off, flags, keys, counts, slot_records, pack_cap=0):
    got = C.exch_pack(off, flags, ref.blob(keys), counts, slot_records, pack_cap)
    assert got["off"] == off and got["flags"] == flags
    failed = bool(flags & (ref.ABORT | ref.TOO_MANY_SAMPLES))
    check_slots(got["slots"], ref.pack(off, flags, keys, counts, slot_records), slot_records, failed)
    return got


@pytest.mark.parametrize("slot_records", [600, 150, 1])
def test_pack_empty_buckets(slot_records):
    """Empty buckets in front, three in a row in the middle, and at the end."""
    keys = [pad(b"k%07d" % i) for i in range(1000)]
    counts = [7 * i + 1 for i in range(1000)]  # distinct: a misplaced record shows
    off = [0, 0, 0, 100, 300, 300, 300, 300, 900, 1000, 1000, 1000]
    got = run_pack(off, 0, keys, counts, slot_records)
    assert [s["n"] for s in got["slots"]] == [0, 0, 100, 200, 0, 0, 0, 600, 100, 0, 0]


def test_pack_no_records():
    got = run_pack([0] * 5, 0, [], [], 8)
    assert all(s["status"] == ref.SLOT_OK and s["n"] == 0 for s in got["slots"])
    run_pack([0, 0], 0, [], [], 8)


@pytest.mark.parametrize("flags", [ref.ABORT, ref.TOO_MANY_SAMPLES, ref.ABORT | ref.SEND_OVERFLOW])
def test_pack_failed_plan_writes_headers_only(flags):
    keys = [pad(b"k%07d" % i) for i in range(500)]
    run_pack([0, 200, 200, 500], flags, keys, list(range(1, 501)), 100)


def test_pack_grid_stride_trips():
    """300,000 records into 64 slots with the grid bounded by cap = 70,000: 274 workgroups
    of 256 threads, so the grid-stride loop takes five trips."""
    n = 300000
    rng = random.Random(4)
    keys = [pad(b"k%07d" % i) for i in range(n)]
    counts = [3 * i + 1 for i in range(n)]
    cuts = [rng.randrange(n + 1) for _ in range(60)] + [n] * 4  # (the last buckets are empty)
    off = [0] + sorted(cuts)
    assert len(off) == 65 and off[-1] == n
    run_pack(off, 0, keys, counts, 5000, pack_cap=70000)


# ---------------------------------------------------------------------------------------
# samplers: sample_keys_kernel and the one fused into exch_header_kernel
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many_keys():
    return [pad(b"k%07d" % i) for i in range(100003)]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 128])
def test_samplers(many_keys, S):
    for n in sorted({0, 1, 2, S - 1, S, S + 1, 100003}):
        keys = many_keys[:n]
        blob = ref.blob(keys)
        want = ref.samples(keys, S)
        assert ref.unblob(C.exch_sample(blob, S)) == want, n
        h = C.exch_header({"num_unique": n}, {}, False, blob, S)
        assert ref.unblob(h["samples"]) == want, n
        assert h["tail_intact"] and h["n_local"] == n


# ---------------------------------------------------------------------------------------
# header fields
# ---------------------------------------------------------------------------------------

CTR = {"flags": 0, "num_unique": 1101, "num_records": 2202, "map_tokens": 3303,
       "overflow_lines": 44, "truncated": 55, "max_key_len": 66}
TMPL = {"status": 0, "record_flags": 3, "n_local": 999999, "lines": 777, "tokens": 888888,
        "overflow_lines": 1, "truncated": 2, "max_key_len": 3, "out_region": 5}
HDR_KEYS = [pad(b"k%07d" % i) for i in range(10)]


def header(ctr=None, tmpl=None, combined=False, S=4):
    return C.exch_header({**CTR, **(ctr or {})}, {**TMPL, **(tmpl or {})}, combined,
                         ref.blob(HDR_KEYS), S)


@pytest.mark.parametrize("combined", [False, True])
def test_header_fields(combined):
    h = header(combined=combined)
    assert h["status"] == 0 and h["n_local"] == 1101
    assert h["tokens"] == (3303 if combined else 2202)
    assert (h["overflow_lines"], h["truncated"], h["max_key_len"]) == (44, 55, 66)
    # the template's own fields pass through
    assert (h["record_flags"], h["lines"], h["out_region"]) == (3, 777, 5)
    assert ref.unblob(h["samples"]) == ref.samples(HDR_KEYS, 4) and h["tail_intact"]


def test_header_dict_overflow_is_a_map_redo():
    over = C.ctr_dict_overflow_flag()
    h = header(ctr={"flags": over | 2})
    assert h["status"] == ref.MAP_REDO and h["n_local"] == 0 and h["tokens"] == 2202
    # other counter flags alone are no redo
    h = header(ctr={"flags": 0xFFFFFFFF & ~over})
    assert h["status"] == 0 and h["n_local"] == 1101


@pytest.mark.parametrize("flags", [0, 1])
def test_header_keeps_a_failed_template_status(flags):
    assert flags in (0, C.ctr_dict_overflow_flag())
    for status in (1, 9, -4):
        h = header(ctr={"flags": flags}, tmpl={"status": status})
        assert h["status"] == status and h["n_local"] == 0


def test_header_without_samples_writes_the_header_only():
    h = header(S=0)
    assert h["samples"] == b"" and h["tail_intact"] and h["n_local"] == 1101


# ---------------------------------------------------------------------------------------
# pack_records / unpack_records
# ---------------------------------------------------------------------------------------

PART_LO = [p << 55 for p in range(256)] + [2**64 - 1]  # not the first-byte map


@pytest.mark.parametrize("with_counts", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_pack_unpack_round_trip(n, with_counts):
    rng = random.Random(n)
    raw = [bytes(rng.randint(1, 255) for _ in range(rng.randint(1, 31))) for _ in range(n)]
    keys = [pad(k) for k in raw]
    counts = [rng.randint(1, 1 << 50) for _ in range(n)] if with_counts else None
    want_counts = counts if with_counts else [1] * n
    got = C.exch_roundtrip(ref.blob(keys), counts, PART_LO)
    assert got["packed_keys"] == ref.blob(keys) and got["packed_counts"] == want_counts
    assert got["keys"] == ref.blob(keys) and got["counts"] == want_counts
    # PART_LO cuts at every 2^55: partition = first word >> 55, capped (as part_of_key says)
    want_parts = bytes(min(255, int.from_bytes(k[:8], "big") >> 55) for k in keys)
    for i in range(0, n, max(1, n // 300)):
        assert want_parts[i] == C.part_of_key(PART_LO, raw[i])
    assert want_parts != bytes(k[0] for k in raw)
    assert got["parts"] == want_parts
    if n == 257:  # the default map: the first key byte
        assert C.exch_roundtrip(ref.blob(keys), counts, [])["parts"] == bytes(k[0] for k in raw)


# ---------------------------------------------------------------------------------------
# report
# ---------------------------------------------------------------------------------------

SLOT = 4
ACC = [v for lane in range(64) for v in (lane + 1, (1 << 40) + 3 * lane, (1 << 34) + 7 * lane)]
N_OUT = sum(ACC[0::3])


def run_report(headers, flags, gather_records, acc=ACC, max_bucket=12345):
    got = C.exch_report(headers, SLOT, flags, max_bucket, acc, gather_records)
    assert got["acc"] == [0] * 192  # re-zeroed for the next job
    assert got["pad"] == [0, 0, 0]
    want = ref.report(headers, SLOT, flags, max_bucket, acc, gather_records)
    assert {k: got[k] for k in want} == want
    return got


@pytest.mark.parametrize("P", [1, 2, 64])
def test_report(P):
    ok = [(ref.SLOT_OK, q % (SLOT + 1)) for q in range(P)]
    got = run_report(ok, 0, N_OUT)
    assert got["flags"] == 0 and got["n_out"] == N_OUT == 2080
    assert got["total"] == sum(ACC[1::3]) and got["out_words"] == sum(ACC[2::3])
    # a failed / redone slot in the last place only
    for st in (ref.SLOT_FAILED, ref.SLOT_REDO):
        assert run_report(ok[:-1] + [(st, 0)], 0, N_OUT)["flags"] == ref.RECV_TRUNCATED
    # an ok slot that held one record more than the slot takes
    for q in {0, P // 2, P - 1}:
        hs = list(ok)
        hs[q] = (ref.SLOT_OK, SLOT + 1)
        assert run_report(hs, 0, N_OUT)["flags"] == ref.RECV_TRUNCATED
        hs[q] = (ref.SLOT_OK, SLOT)
        assert run_report(hs, 0, N_OUT)["flags"] == 0
    # the range against the gather buffer
    assert run_report(ok, 0, N_OUT - 1)["flags"] == ref.GATHER_OVERFLOW
    assert run_report(ok, ref.SEND_OVERFLOW, N_OUT)["flags"] == ref.SEND_OVERFLOW
    # a dead plan reports no range
    for dead in (ref.ABORT, ref.TOO_MANY_SAMPLES, ref.ABORT | ref.SEND_OVERFLOW):
        got = run_report(ok, dead, 0)
        assert (got["flags"], got["n_out"], got["total"], got["out_words"]) == (dead, 0, 0, 0)


def test_report_sums_are_64_bit():
    acc = [(1 << 57) + lane if i == 1 else 0 for lane in range(64) for i in range(3)]
    got = run_report([(ref.SLOT_OK, 0)], 0, 0, acc=acc)
    assert got["total"] == (1 << 63) + 2016 and got["n_out"] == 0
