"""Key families and texts shared by the ordered dictionary build's edge tests
(test_ordered_edges.py).  Every comparison is exact against ``oracle.wordcount``.

A key is four 8-byte words on the device (csrc/include/locust/kv.hpp); the ordered kernel
(csrc/kernels/dict.hip ``ordered_partition``) sorts a partition's distinct keys by word 0
first and breaks ties on words 1..3 in separate code: the all-pairs ranks up to 256 keys,
the bitonic network's ``ord_greater`` up to 1,024, the LDS radix over words 3..1 above, and
``key_lt`` in the HBM-table fallback.  The families put ``m`` distinct keys into ONE
partition of the first-byte map (``lead``) and decide their order in a chosen word."""
import functools
import random

from locust_amd.utils import oracle

SHAPES = ("short", "tie8", "tie16", "tie24", "edges")
JOBS = 3  # jobs per case on one engine

# edges: stems end just before, exactly at and just after every word edge; the tails make
# keys that are prefixes of one another and put bytes either side of 0x80 into the word
# that decides (a signed compare orders 0x80 and 0xff before 0x7f)
EDGE_STEMS = (7, 8, 9, 15, 16, 17, 23, 24, 25, 27)
EDGE_TAILS = (b"", b"0", b"\x7f", b"\x80", b"\xff", b"\x80\x7f", b"\xff\xff")


def family(shape: str, m: int, lead: bytes = b"w", digits: int = 5) -> list[bytes]:
    """``m`` distinct keys that all start with ``lead``, hold no delimiter byte and are at
    most 29 bytes long (``digits=7``: tie24 at 31 bytes, for ``max_key_len=31``)."""
    num = b"%%0%dd" % digits
    if shape == "short":  # distinct first words: the control
        return [lead + num % i for i in range(m)]
    if shape in ("tie8", "tie16", "tie24"):  # equal up to word 1, 2 or 3
        return [lead * int(shape[3:]) + num % i for i in range(m)]
    if shape == "edges":
        out = []
        for i in range(m):
            stem_len = EDGE_STEMS[i % 10]
            stem = (lead + b"%04d" % (i // 70)).ljust(stem_len, b"q")[:stem_len]
            out.append((stem + EDGE_TAILS[(i // 10) % 7])[:29])
        return out
    raise ValueError(shape)


def _lines(toks: list[bytes], seed: int, per_line: int = 10) -> bytes:
    """The tokens shuffled with a fixed seed, 10 per line (the emit cap is 20)."""
    random.Random(seed).shuffle(toks)
    return b"".join(b" ".join(toks[i:i + per_line]) + b"\n" for i in range(0, len(toks), per_line))


def background(mid: bool = True) -> list[bytes]:
    """Keys of other partitions on both sides of 'w': the look-back prefix (and so ``val``)
    of the partition under test is non-trivial, and so is what follows it."""
    toks = [b"a%03d" % (i % 150) for i in range(400)]
    if mid:
        toks += [b"m" * 9 + b"%02d" % (i % 40) for i in range(100)]
    toks += [b"x%03d" % (i % 90) for i in range(300)] + [b"zz"] * 50
    return toks


def family_text(keys: list[bytes], seed: int) -> bytes:
    """Key i occurs 1 + i % 3 times, among the background keys."""
    toks = []
    for i, k in enumerate(keys):
        toks += [k] * (1 + i % 3)
    return _lines(toks + background(), seed)


def crowded(shape: str, n: int, distinct: int, lead: bytes = b"w"):
    """(keys, tokens): exactly ``n`` tokens of ``distinct`` keys in partition ``lead``.
    hot: short keys, one of them carries every token past one each; twolevel: 8 first words,
    each shared by distinct / 8 keys that differ in word 1 (a quantile cut on the first word
    always has that many keys on it); any family: the extra tokens go round the keys."""
    if shape == "hot":
        keys = family("short", distinct, lead)
        mult = [1] * distinct
        mult[distinct // 2] += n - distinct
    elif shape == "twolevel":
        keys = [lead + b"%07d" % (g * 1111111 % 10000000) + b"%04d" % i
                for g in range(8) for i in range(distinct // 8)]
        mult = [1] * len(keys)
        mult[0] += n - len(keys)
    else:
        keys = family(shape, distinct, lead)
        mult = [1] * distinct
        for i in range(n - distinct):
            mult[i % distinct] += 1
    toks = [k for k, c in zip(keys, mult) for _ in range(c)]
    assert len(toks) == n and len(set(keys)) == len(keys)
    return keys, toks


def crowded_text(toks: list[bytes], seed: int) -> bytes:
    return _lines(list(toks) + background(mid=False), seed)


def fixed_length_keys(length: int, m: int, lead: bytes = b"w") -> list[bytes]:
    """``m`` distinct keys of exactly ``length`` >= 7 bytes: ``lead`` repeated, 5 digits."""
    return [lead * (length - 5) + b"%05d" % i for i in range(m)]


def only_text(keys: list[bytes], seed: int) -> bytes:
    """A text of nothing but the keys, key i 1 + i % 3 times: texts of equally many keys
    have their tokens at the same positions (same seed, same shuffle)."""
    toks = []
    for i, k in enumerate(keys):
        toks += [k] * (1 + i % 3)
    return _lines(toks, seed)


def want(text: bytes, max_key: int = 29):
    """(entries, num_tokens, num_unique) of the oracle."""
    ent, ntok, _over = oracle.wordcount(text, max_key=max_key)
    return ent, ntok, len(ent)


def got(res):
    return res.entries(), res.num_tokens, res.num_unique


def num_lines(text: bytes) -> int:
    return text.count(b"\n") + 1


def tokens_of(text: bytes, lead: bytes = b"w") -> int:
    """Tokens of the text that fall into partition ``lead`` of the first-byte map."""
    return sum(1 for t in text.split() if t[:1] == lead)


# ---- the wrong orders the families must tell from the right one ----

def order_by_prefix(keys: list[bytes], nbytes: int) -> list[bytes]:
    """A sort that compares only the first ``nbytes`` bytes (ties on words past them are
    left as they came: in descending order here)."""
    return sorted(sorted(keys, reverse=True), key=lambda k: k[:nbytes])


def order_signed(keys: list[bytes]) -> list[bytes]:
    """A sort that compares bytes as signed chars."""
    return sorted(keys, key=lambda k: [b - 256 if b >= 128 else b for b in k])


def order_word_prefix_equal(keys: list[bytes]) -> list[bytes]:
    """A sort whose compare walks the 8-byte words and stops, calling the keys equal, when
    one of them has run out of words: a key that ends exactly on a word edge then equals
    every longer key it starts (its zero-padded neighbours), and they stay as they came --
    in descending order here."""
    def cmp(a: bytes, b: bytes) -> int:
        for j in range(0, 32, 8):
            x, y = a[j:j + 8], b[j:j + 8]
            if not x or not y:
                return 0
            x, y = x.ljust(8, b"\0"), y.ljust(8, b"\0")
            if x != y:
                return -1 if x < y else 1
        return 0
    return sorted(sorted(keys, reverse=True), key=functools.cmp_to_key(cmp))
