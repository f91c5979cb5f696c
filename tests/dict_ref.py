"""Plain-integer reference of the dictionary fallback kernels (csrc/kernels/dict.hip:
dict_insert, dict_part_build, rank_sort, rank_emit, rank_scatter, scan_pack) and of the
in-job partition plan (csrc/kernels/partplan.hip), one function per launch, as their
comments in kernels.hpp state them; a port of the key hash (device/hash.hpp) with the slot
rules of the three hash tables; and the inputs of tests/test_dict_stage_kernels.py, built
here so that tests/test_dict_ref.py can check their properties without a GPU.

A key is its 32 packed bytes (NUL padded): bytes compare like the four big-endian words
do.  Kernel constants come from the module's one binding (``dict_constants``), not from
copies."""
import bisect
import functools
import random

import locust_amd as lc

import ordered_keys as ok

K = lc._C.dict_constants()
KEY_BYTES = 32
M64 = (1 << 64) - 1
PARTS = K["kDictParts"]
DICT_OVERFLOW = K["kCtrDictOverflow"]
NOT_EMITTED = K["kCtrNotEmitted"]
RANK_MAX = K["kRankSortMax"]
PATTERN = K["kStagePattern"]
PATTERN_U32 = int.from_bytes(bytes([PATTERN]) * 4, "little")
PATTERN_U64 = int.from_bytes(bytes([PATTERN]) * 8, "little")
PATTERN_KEY = bytes([PATTERN]) * KEY_BYTES
ZERO_KEY = bytes(KEY_BYTES)
CTR_FIELDS = ("num_records", "map_tokens", "num_unique", "overflow_lines", "truncated",
              "num_newlines", "max_key_len", "flags", "total_count")


def pad(key: bytes) -> bytes:
    assert len(key) <= KEY_BYTES and b"\0" not in key, key
    return key.ljust(KEY_BYTES, b"\0")


def blob(keys) -> bytes:
    return b"".join(keys)


def unblob(b: bytes):
    assert len(b) % KEY_BYTES == 0
    return [b[i:i + KEY_BYTES] for i in range(0, len(b), KEY_BYTES)]


def words(key: bytes):
    return tuple(int.from_bytes(key[j:j + 8], "big") for j in range(0, KEY_BYTES, 8))


def w0_of(key: bytes) -> int:
    return int.from_bytes(key[:8], "big")


def valid_key(key: bytes) -> bool:
    """Bytes, then NUL padding only."""
    return len(key) == KEY_BYTES and b"\0" not in key.rstrip(b"\0")


# ---------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------

def aggregate(keys, counts=None):
    """{key: count} of dict_insert / dict_part_build: empty records (word 0 == 0) and
    records of count 0 are skipped."""
    out = {}
    for i, k in enumerate(keys):
        c = 1 if counts is None else counts[i]
        if w0_of(k) == 0 or c == 0:
            continue
        out[k] = out.get(k, 0) + c
    return out


def ranks(keys, counts=None):
    """Per key: the number of smaller keys, and the sum of their counts (0 without
    counts).  The order is that of the 32 padded bytes, unsigned."""
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    skeys = [keys[i] for i in order]
    pre = [0]
    for i in order:
        pre.append(pre[-1] + (counts[i] if counts is not None else 0))
    rank, val = [], []
    for k in keys:
        r = bisect.bisect_left(skeys, k)
        rank.append(r)
        val.append(pre[r])
    return rank, val


def ctr_out_of(ctr, u, flags, total):
    out = {f: ctr.get(f, 0) for f in CTR_FIELDS}
    out["num_unique"] = u
    out["flags"] = flags
    out["total_count"] = PATTERN_U64 if total is None else total
    return out


def emit(keys, counts, rank, val, ctr, cap):
    """rank_emit: (records or None when nothing is emitted, ctr_out).  ctr_out is written
    field by field: num_unique clamped to cap, kCtrNotEmitted above kRankSortMax;
    total_count = val + count of the key of rank u - 1, 0 for u == 0, unwritten (pattern)
    when nothing is emitted."""
    u = min(ctr.get("num_unique", 0), cap)
    if u > RANK_MAX:
        return None, ctr_out_of(ctr, u, ctr.get("flags", 0) | NOT_EMITTED, None)
    recs = [None] * u
    total = 0
    for i in range(u):
        recs[rank[i]] = (keys[i], counts[i])
        if rank[i] == u - 1:
            total = val[i] + counts[i]
    return recs, ctr_out_of(ctr, u, ctr.get("flags", 0), total)


def scatter(keys, counts, rank, d_u, cap):
    """rank_scatter: the sorted keys and counts (cap entries; the pattern where unwritten)."""
    skeys, scounts = [PATTERN_KEY] * cap, [PATTERN_U64] * cap
    u = min(d_u, cap)
    if u <= RANK_MAX:
        for i in range(u):
            skeys[rank[i]], scounts[rank[i]] = keys[i], counts[i]
    return skeys, scounts


def scan_pack(skeys, counts, num_unique, emit_limit, ctr=None):
    """scan_pack: (records or None, ctr.total_count or None when unwritten, ctr_out)."""
    ctr = dict(ctr or {})
    u = num_unique
    if u > emit_limit:
        return None, None, ctr_out_of(ctr, u, ctr.get("flags", 0) | NOT_EMITTED, None)
    recs = [(skeys[i], counts[i]) for i in range(u)]
    total = sum(counts[:u])
    # no tile runs for u == 0: only the first thread's ctr_out->total_count = 0
    return recs, (total if u else None), ctr_out_of(ctr, u, ctr.get("flags", 0), total)


def part_plan(w0, counts, d_u, ucap, tie_rng=None):
    """The 257 range starts.  tie_rng: shuffles the samples before the (stable) sort, so
    samples of equal first word come in another order."""
    U = min(d_u, ucap)
    S = min(U, K["kPlanSamples"])
    lo = [0] * (PARTS + 1)
    lo[PARTS] = M64
    samples = []
    for i in range(S):
        e = i * U // S
        samples.append((w0[e], K["kSingletonWeight"] if counts[e] == 1 else 1))
    if tie_rng is not None:
        tie_rng.shuffle(samples)
    samples.sort(key=lambda s: s[0])
    W = sum(w for _, w in samples)
    if W == 0:
        for q in range(1, PARTS):
            lo[q] = q << 56
        return lo
    pre = 0
    for k, w in samples:
        for q in range(pre * PARTS // W + 1, (pre + w) * PARTS // W + 1):
            if q < PARTS:
                lo[q] = k
        pre += w
    return lo


# ---------------------------------------------------------------------------------------
# the key hash (device/hash.hpp) and the tables' slots
# ---------------------------------------------------------------------------------------

def mix64(x: int) -> int:
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x


def key_hash(key: bytes) -> int:
    k = words(key)
    return mix64(k[0] ^ mix64(k[1] ^ (k[2] * 0x9e3779b97f4a7c15 & M64) ^ (k[3] << 1 & M64)))


def hbm_slot(key: bytes, slots: int) -> int:
    return key_hash(key) & 0xFFFFFFFF & (slots - 1)


def lds_slot(key: bytes) -> int:
    return (key_hash(key) >> 40) & 0xFFFFFFFF & (K["kLdsSlots"] - 1)


def part_slot(key: bytes) -> int:
    return (key_hash(key) >> 8) & 0xFFFFFFFF & (K["kPartSlots"] - 1)


def hash_tag(key: bytes) -> int:
    return key_hash(key) >> 56


def occupied(homes, slots: int):
    """The slots a linear-probing table of `slots` slots ends up occupying after one insert
    per home slot: the same set in whatever order they arrive."""
    occ = set()
    homes = list(homes)
    assert len(homes) <= slots
    for h in homes:
        while h in occ:
            h = (h + 1) % slots
        occ.add(h)
    return occ


def longest_cluster(occ, slots: int) -> int:
    """The longest run of occupied slots, around the table's end."""
    if len(occ) >= slots:
        return slots
    best = run = 0
    start = next(s for s in range(slots) if s not in occ)  # begin behind a free slot
    for d in range(1, slots + 1):
        run = run + 1 if (start + d) % slots in occ else 0
        best = max(best, run)
    return best


def numbered(prefix: bytes, digits: int = 7):
    """prefix0000000, prefix0000001, ... (padded): a family to draw from."""
    i = 0
    while True:
        yield pad(prefix + b"%0*d" % (digits, i))
        i += 1


def search(family, want, pred):
    """The first `want` keys of the family (an iterator of padded keys) for which pred holds."""
    out = []
    for k in family:
        if pred(k):
            out.append(k)
            if len(out) == want:
                return out
    raise AssertionError("family exhausted")


# ---------------------------------------------------------------------------------------
# inputs of the GPU tests (test_dict_ref.py checks their properties)
# ---------------------------------------------------------------------------------------

FAMILIES = ok.SHAPES


@functools.lru_cache(maxsize=None)
def family(shape: str, m: int, lead: bytes = b"w"):
    keys = [pad(k) for k in ok.family(shape, m, lead)]
    return tuple(keys)


def big_counts(n: int, seed: int, top: int = 1 << 40):
    """Counts in [1, top], the first few at the ends of the range: sums pass 2^32."""
    rng = random.Random(seed)
    c = [rng.randrange(1, top + 1) for _ in range(n)]
    for i, v in enumerate((top, 1, top - 1, 2)[:n]):
        c[i] = v
    return c


def scan_counts(u: int):
    """u counts of about 2^61 / u each: every tile's sum passes 2^32, the total is near 2^61."""
    base = (1 << 61) // max(u, 1)
    return [base - (i * 7919 % 1000) for i in range(u)]


@functools.lru_cache(maxsize=None)
def insert_mix(n: int):
    """n tokens: every family, each key several times, in a fixed shuffled order."""
    d = max(1, n // 3)
    per = -(-d // len(FAMILIES))
    pool = [k for f in FAMILIES for k in family(f, per)][:d]
    rng = random.Random(1000 + n)
    toks = [pool[rng.randrange(len(pool))] for _ in range(n)]
    return tuple(toks)


@functools.lru_cache(maxsize=None)
def equal_hash_pairs(m: int = 40):
    """2 m keys, in pairs that differ only in bit 7 of byte 24 (the top bit of word 3,
    which key_hash shifts out): the two of a pair hash identically."""
    out = []
    for i in range(m):
        stem = b"h" * 20 + b"%04d" % i
        out.append(pad(stem + b"\x41" + b"tl"))
        out.append(pad(stem + b"\xc1" + b"tl"))
    return tuple(out)


WRAP_SLOTS = 64


@functools.lru_cache(maxsize=None)
def wrap_keys(want: int = 14):
    """Keys whose home slot in a 64-slot HBM table is one of its last four: most of them
    land behind the table's end, in slots 0.."""
    return tuple(search(numbered(b"wr"), want, lambda k: hbm_slot(k, WRAP_SLOTS) >= WRAP_SLOTS - 4))


@functools.lru_cache(maxsize=None)
def lds_collide_keys():
    """kLdsProbes + 4 keys of one LDS cache slot: the last four find the probe window
    taken and spill to the HBM table."""
    first = pad(b"lc0000000")
    slot = lds_slot(first)
    return tuple(search(numbered(b"lc"), K["kLdsProbes"] + 4, lambda k: lds_slot(k) == slot))


@functools.lru_cache(maxsize=None)
def part_keys(m: int, lead: bytes = b"p"):
    """m distinct keys of one first byte (one partition of the first-byte tagging)."""
    per = -(-m // len(FAMILIES))
    return tuple([k for f in FAMILIES for k in family(f, per, lead)][:m])


def part_cluster(keys) -> int:
    return longest_cluster(occupied([part_slot(k) for k in keys], K["kPartSlots"]), K["kPartSlots"])


@functools.lru_cache(maxsize=None)
def part_build_tokens(n: int):
    """n tokens over a few hundred keys of several first bytes -- 0xA5, the stage pattern
    byte, among them: pattern bytes behind the tags would count for that partition."""
    leads = [b"a", b"b", b"w", bytes([PATTERN]), b"\xfe"]
    d = max(1, min(n // 2, 600))
    per = -(-d // len(leads))
    pool = [k for ld in leads for k in part_keys(per, ld)][:d]
    rng = random.Random(2000 + n)
    return tuple(pool[rng.randrange(len(pool))] for _ in range(n))


def plan_input(U: int, kind: str, seed: int = 7):
    """(w0, counts) of U distinct first words in no key order.  kind: ones | twos | zipf."""
    rng = random.Random(seed * 100003 + U)
    w0 = set()
    while len(w0) < U:
        # letters mostly, some with the top bit set
        b = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz\x80\xc3\xff") for _ in range(rng.randrange(1, 9)))
        w0.add(int.from_bytes(b.ljust(8, b"\0"), "big"))
    w0 = list(w0)
    rng.shuffle(w0)
    if U >= 3:
        w0[U // 2] = M64  # a first word of all ones: the kernel pads its sort with it
    if kind == "ones":
        counts = [1] * U
    elif kind == "twos":
        counts = [2] * U
    else:
        counts = [max(1, int(U / (1 + rng.randrange(U)))) if rng.random() < 0.5 else 1
                  for _ in range(U)]
    return w0, counts
