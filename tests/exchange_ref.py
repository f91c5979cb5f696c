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
