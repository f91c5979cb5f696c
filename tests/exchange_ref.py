"""Plain reference of the device shuffle's control steps (csrc/include/locust/exch.hpp):
samples, weighted-quantile splitters, bucket offsets, plan flags and the packed slots.

Written from the documented rules, in exact integer arithmetic (Python ints, no floats):

* sample k of S over n sorted keys is ``keys[(2k+1) n // (2S)]``; an empty shard samples the
  all-ones key S times;
* all P x S samples are ordered by (key, rank, index); a sample of rank r weighs
  ``n_local[r]``; ``total`` is the sum over the samples; splitter p (p = 1..P-1) is the key
  of the first sample in that order whose inclusive weight exceeds ``total * p // P``, the
  all-ones key if there is none;
* ``off[p]`` is the lower bound of splitter p-1 in this rank's sorted keys (a key equal to a
  splitter goes to the upper bucket), ``off[0] = 0``, ``off[P] = n``;
* flags: too-many-samples when P x S > 1024 or P > 64 (every splitter is then the all-ones
  key, so bucket 0 holds everything), abort when any rank's status is non-zero,
  send-overflow when a bucket exceeds ``slot_records``;
* slot d: status failed under abort / too-many-samples, redo when its bucket exceeds
  ``slot_records``, else ok; ``n`` is the whole bucket; the records are its first
  ``min(n, slot_records)`` in order (none under abort / too-many-samples).

A key is its 32-byte packed form: the key's bytes (no NUL, at most 31) padded with NULs,
which is the big-endian image of the four packed u64 words, so ``bytes`` comparison is the
packed comparison.

The shuffle's tail (csrc/kernels/merge.hip), from the rules in kernels.hpp, slot.hpp and the
format comment of kv.hpp:

* a slot is (status, n, records); its run is empty unless the status is ok, else its first
  ``min(n, slot_records)`` records.  A run is a list of (key, count), ascending and distinct;
* the merged array holds every record of every run in stable (key, run index) order; the
  first copy of a key carries the key's count summed over all runs, every later copy 0;
* the output is the first copies in that order; the counters are the number of records, of
  distinct keys and the count total (every count is at least 1);
* the accumulators sum to (distinct keys, count total, words of the compact records);
* a compact record of (key, count), kb = the key's length: count < 2^24 -> one word [key
  bytes 0-3 : 32][count : 24][0][kb : 6][0] (high to low) and ceil((kb - 4) / 8) words of the
  key bytes from 4 on; otherwise one word [count : 56][0][kb : 6][1] and ceil(kb / 8) words of
  the key; key bytes big-endian, NUL padded;
* the compact emit of rank ``me`` refuses (writes nothing) when any rank's report has a
  status or a flag, when its own n_out exceeds gather_records, when the region is not below
  ``regions``, or when r + n_out[me] exceeds region_records, r being the lower ranks' n_out,
  each clamped to gather_records; else its records start at word
  5 (region x region_records + r).
"""
from bisect import bisect_left

KEY_BYTES = 32
ALL_ONES = b"\xff" * KEY_BYTES

# exch.hpp / slot.hpp (kept as literals: the reference does not read them from the module
# under test; test_exchange_ref.py checks that they agree)
SEND_OVERFLOW, RECV_TRUNCATED, ABORT, TOO_MANY_SAMPLES, GATHER_OVERFLOW = 1, 2, 4, 8, 16
MAP_REDO = 3
SLOT_OK, SLOT_FAILED, SLOT_REDO = 0, 1, 2
MAX_PLAN_SAMPLES, MAX_RANKS = 1024, 64
RECORD_FLAGS = 3  # sorted | distinct


def pad(key: bytes) -> bytes:
    """The packed form of a key of at most 31 bytes without NUL."""
    assert len(key) < KEY_BYTES and b"\0" not in key, key
    return key.ljust(KEY_BYTES, b"\0")


def blob(keys) -> bytes:
    return b"".join(keys)


def unblob(b: bytes):
    assert len(b) % KEY_BYTES == 0
    return [b[i:i + KEY_BYTES] for i in range(0, len(b), KEY_BYTES)]


def samples(keys, S):
    """S evenly spaced keys of a sorted list."""
    n = len(keys)
    if n == 0:
        return [ALL_ONES] * S
    return [keys[(2 * k + 1) * n // (2 * S)] for k in range(S)]


def splitters(sample_lists, n_local, parts):
    """The parts - 1 splitters from every rank's sample list and record count."""
    order = sorted((key, r, i) for r, lst in enumerate(sample_lists) for i, key in enumerate(lst))
    total = sum(n_local[r] for _, r, _ in order)
    out = []
    for p in range(1, parts):
        target = total * p // parts
        run, chosen = 0, ALL_ONES
        for key, r, _ in order:
            run += n_local[r]
            if run > target:
                chosen = key
                break
        out.append(chosen)
    return out


def offsets(keys, split):
    """P + 1 bucket offsets of P - 1 splitters in a sorted key list."""
    return [0] + [bisect_left(keys, s) for s in split] + [len(keys)]


def plan_pack(P, S, status, n_local, sample_lists, keys, counts, slot_records):
    """What launch_exch_plan + launch_exch_pack must produce: the ExchCtl fields and, per
    slot, the header fields and the records."""
    too_many = P * S > MAX_PLAN_SAMPLES or P > MAX_RANKS
    split = [ALL_ONES] * (P - 1) if too_many else splitters(sample_lists, n_local, P)
    off = offsets(keys, split)
    buckets = [off[p + 1] - off[p] for p in range(P)]
    flags = 0
    if too_many:
        flags |= TOO_MANY_SAMPLES
    if any(status):
        flags |= ABORT
    if any(b > slot_records for b in buckets):
        flags |= SEND_OVERFLOW
    return {"off": off, "flags": flags, "max_bucket": max(buckets),
            "slots": pack(off, flags, keys, counts, slot_records)}


def pack(off, flags, keys, counts, slot_records):
    """The slots launch_exch_pack writes behind given offsets and plan flags."""
    failed = bool(flags & (ABORT | TOO_MANY_SAMPLES))
    slots = []
    for d in range(len(off) - 1):
        n = off[d + 1] - off[d]
        held = 0 if failed else min(n, slot_records)
        slots.append({
            "status": SLOT_FAILED if failed else SLOT_REDO if n > slot_records else SLOT_OK,
            "record_flags": RECORD_FLAGS,
            "n": n,
            "slot_cap": slot_records,
            "keys": list(keys[off[d]:off[d] + held]),
            "counts": list(counts[off[d]:off[d] + held]),
        })
    return slots


def report(headers, slot_records, ctl_flags, max_bucket, acc, gather_records):
    """ExchMsg3 of launch_exch_report: headers are (status, n) of the received slots, acc the
    64 (firsts, tokens, words) accumulator triples."""
    dead = bool(ctl_flags & (ABORT | TOO_MANY_SAMPLES))
    n_out = 0 if dead else sum(acc[0::3])
    flags = ctl_flags
    if any(st != SLOT_OK or n > slot_records for st, n in headers):
        flags |= RECV_TRUNCATED
    if n_out > gather_records:
        flags |= GATHER_OVERFLOW
    return {"status": 0, "flags": flags, "max_bucket": max_bucket, "n_out": n_out,
            "total": 0 if dead else sum(acc[1::3]),
            "out_words": 0 if dead else sum(acc[2::3])}


# ---- the shuffle's tail: slot merge, accumulators, compact emit ----

OUT_WORDS = 5              # 8-B words of a 40-B output record
COMPACT_SHORT_MAX = (1 << 24) - 1
MERGE_MAX_RECORDS, MERGE_MAX_COUNT = (1 << 22) - 1, (1 << 40) - 1
ACC_SPREAD = 64
REFUSED = "refused"


def pad32(key: bytes) -> bytes:
    """As pad(), for keys of up to 32 bytes (a key of 32 fills all four words)."""
    assert 1 <= len(key) <= KEY_BYTES and b"\0" not in key, key
    return key.ljust(KEY_BYTES, b"\0")


def slot_runs(slots, slot_records):
    """The effective runs of (status, n, records) slots."""
    runs = []
    for status, n, records in slots:
        held = min(n, slot_records) if status == SLOT_OK else 0
        assert held <= len(records), "the slot does not hold what its header announces"
        runs.append(list(records[:held]))
    return runs


def _totals(runs):
    tot = {}
    for run in runs:
        assert [k for k, _ in run] == sorted({k for k, _ in run}), "a run ascends, distinct"
        for k, c in run:
            tot[k] = tot.get(k, 0) + c
    return tot


def merged_ref(runs):
    """The merged array: (key, count) in stable (key, run) order, the sum on the first copy."""
    tot = _totals(runs)
    order = sorted((k, q) for q, run in enumerate(runs) for k, _ in run)
    out, seen = [], set()
    for k, _q in order:
        out.append((k, 0 if k in seen else tot[k]))
        seen.add(k)
    return out


def merge_out_ref(runs):
    """(output records, (num_records, num_unique, total_count))."""
    tot = _totals(runs)
    recs = sorted(tot.items())
    return recs, (sum(len(r) for r in runs), len(recs), sum(tot.values()))


def compact_words_ref(key: bytes, count: int) -> int:
    kb = len(key.rstrip(b"\0"))
    if count <= COMPACT_SHORT_MAX:
        return 1 + (-(-(kb - 4) // 8) if kb > 4 else 0)
    return 1 + -(-kb // 8)


def compact_record_ref(key: bytes, count: int):
    """kv.hpp's compact record, written independently: short form (count < 2^24) packs key
    bytes 0-3 into the header word, then key bytes 4.. in 8-byte words; long form keeps a
    56-bit count and the packed key words."""
    kb = len(key.rstrip(b"\0"))
    if count < (1 << 24):
        head = (int.from_bytes(key[:4].ljust(4, b"\0"), "big") << 32) | (count << 8) | (kb << 1)
        rest = key[4:kb]
        extra = [int.from_bytes(rest[i:i + 8].ljust(8, b"\0"), "big") for i in range(0, len(rest), 8)]
        return [head] + extra
    full = key.ljust(KEY_BYTES, b"\0")
    w = [int.from_bytes(full[8 * j:8 * j + 8], "big") for j in range(4)]
    return [(count << 8) | (kb << 1) | 1] + w[:(kb + 7) // 8]


def acc_ref(runs):
    """(firsts, tokens, words): what the 64 accumulator triples sum to."""
    recs, (_n, uniq, total) = merge_out_ref(runs)
    return uniq, total, sum(compact_words_ref(k, c) for k, c in recs)


def emit_ref(runs, msg3_all, region, regions, region_records, me, gather_records):
    """REFUSED, or (first word, the words) of rank me's compact emit.  msg3_all: (status,
    flags, n_out) of every rank; region: the one in force (the host's or the root's)."""
    n = msg3_all[me][2]
    r = sum(min(n_out, gather_records) for _st, _fl, n_out in msg3_all[:me])
    if (any(st != 0 or fl != 0 for st, fl, _n in msg3_all) or n > gather_records
            or region >= regions or r + n > region_records):
        return REFUSED
    words = []
    for k, c in merge_out_ref(runs)[0]:
        words += compact_record_ref(k, c)
    return OUT_WORDS * (region * region_records + r), words
