"""Word-edge and threshold tests for the ordered dictionary build (csrc/kernels/dict.hip
``ordered_partition`` and its token sources).

The key families of tests/ordered_keys.py put a chosen number ``m`` of distinct keys into
one partition of the first-byte map and decide their order in key word 1, 2 or 3, at a key's
last byte before / on / after a word edge, and in bytes either side of 0x80.  The cases sit
on both sides of every size at which the kernel changes its path:

  distinct keys m     256 | 257 (all-pairs ranks | bitonic network), 1,024 | 1,025 (bitonic |
                      LDS radix), 2,048 | 2,049 (LDS table | HBM-table fallback, ``key_lt``)
  partition tokens    384 | 385 (small table | ``grow_table``), 16,384 | 16,385 (the token
                      window), and for the in-job plan (``TileSource::build_split``)
                      4,096 | 4,097 (register | list path), 16,128 | 16,129 (its list)

Every comparison is exact against the pure-Python oracle: ``entries()`` as (key, val,
count) in order, ``num_tokens`` and ``num_unique``; engines are built with ``check=True``
and every case runs 3 jobs on one engine."""
import pytest

import locust_amd as lc
from tests import ordered_keys as ok
from tests.ordered_keys import JOBS, SHAPES


def gpu_test(fn):
    """Needs an MI355X; a few seconds each."""
    return pytest.mark.gpu(pytest.mark.timeout(120)(fn))


SORT_SIZES = (1, 2, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1280)
NEAR_FULL = (1500, 1900, 2047, 2048)
SOURCE_SIZES = (256, 257, 1024, 1025, 2049)
SOURCE_SHAPES = ("tie8", "tie24", "edges")
SPLIT_TOKENS = (4095, 4096, 4097, 16128, 16129)


def check(res, exp, label):
    """Exact: num_tokens, num_unique and every (key, val, count) in order."""
    ent, ntok, nuniq = exp
    got_ent, got_tok, got_uniq = ok.got(res)
    assert (got_tok, got_uniq) == (ntok, nuniq), label
    if got_ent != ent:
        at = next((i for i, (a, b) in enumerate(zip(got_ent, ent)) if a != b), min(len(got_ent), len(ent)))
        pytest.fail(f"{label}: entry {at} of {len(ent)} is {got_ent[at:at + 1]}, "
                    f"expected {ent[at:at + 1]} (got {len(got_ent)} entries)")


def gpu_engine(texts, **cfg):
    """One engine that holds the largest of ``texts``."""
    return lc._C.GpuEngine(lc.make_config("gpu", reduce_path="lds", check=True, **cfg),
                           max(len(t) for t in texts), max(ok.num_lines(t) for t in texts))


def run_jobs(eng, text, label, max_key=29):
    """JOBS jobs of ``text``, each exact; returns the fallbacks they took."""
    exp = ok.want(text, max_key)
    before = eng.stats()["fallbacks"]
    for j in range(JOBS):
        check(eng.run(text), exp, f"{label} job {j}")
    return eng.stats()["fallbacks"] - before


# ---------------------------------------------------------------------------------------
# CPU: the inputs can catch the bugs they are meant for, and the CPU engine agrees
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [257, 1025])
def test_families_discriminate(m):
    """Each wrong order differs from the right one on the family made for it."""
    for shape, nbytes in (("tie8", 8), ("tie16", 16), ("tie24", 24)):
        keys = ok.family(shape, m)
        assert ok.order_by_prefix(keys, nbytes) != sorted(keys), shape
        assert ok.order_by_prefix(keys, nbytes + 8) == sorted(keys), shape  # and only that word
    keys = ok.family("edges", m)
    assert ok.order_signed(keys) != sorted(keys)
    assert ok.order_word_prefix_equal(keys) != sorted(keys)
    # the control: first words decide
    assert ok.order_by_prefix(ok.family("short", m), 8) == sorted(ok.family("short", m))


def test_families_are_what_they_claim():
    delims = set(lc.utils.oracle.DEFAULT_DELIMS) | {0, 10, 13}
    for shape in SHAPES:
        for m in SORT_SIZES + NEAR_FULL + (2049,):
            keys = ok.family(shape, m)
            assert len(set(keys)) == m, (shape, m)
            assert all(k[:1] == b"w" and 0 < len(k) <= 29 and not delims & set(k) for k in keys)
    assert {len(k) for k in ok.family("tie24", 256)} == {29}
    assert {len(k) for k in ok.family("tie24", 256, digits=7)} == {31}
    lens = {len(k) for k in ok.family("edges", 70)}
    assert {7, 8, 9, 15, 16, 17, 23, 24, 25, 27, 29} <= lens
    text = ok.family_text(ok.family("tie24", 2049), 2049)
    ent, ntok, _ = ok.want(text)
    assert len(text) < (1 << 18) and ntok < 17200
    assert [k for k, _v, _c in ent if k[:1] == b"w"] == sorted(ok.family("tie24", 2049))
    assert ent[0][0][:1] == b"a" and ent[-1][0] == b"zz"  # partitions on both sides


@pytest.mark.parametrize("shape,distinct", [("short", 6000), ("tie8", 1000), ("tie8", 3000),
                                            ("hot", 1500), ("twolevel", 1600)])
def test_crowded_texts_are_what_they_claim(shape, distinct):
    """Exactly n tokens in partition 'w', under 256 KB and 17,200 tokens, and every 1 KiB
    tile holds at least 65 of them (past the map's plan trigger of 48)."""
    for n in SPLIT_TOKENS:
        if distinct > n:
            continue
        keys, toks = ok.crowded(shape, n, distinct)
        text = ok.crowded_text(toks, n)
        assert ok.tokens_of(text) == n and len(text) < (1 << 18)
        assert ok.want(text)[1] == n + 750 < 17200
        tiles = [ok.tokens_of(b" " + text[i:i + 1024]) for i in range(0, len(text) - 1024, 1024)]
        assert min(tiles) >= 65, (shape, n, min(tiles))


@pytest.mark.parametrize("m", [257, 1025])
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_engine_matches_oracle(shape, m):
    text = ok.family_text(ok.family(shape, m), m)
    check(lc.wordcount_text(text, backend="cpu"), ok.want(text), f"{shape} m={m}")


# ---------------------------------------------------------------------------------------
# GPU group A: one workgroup per partition -- partition 'w' holds exactly m distinct keys
# ---------------------------------------------------------------------------------------

@pytest.fixture
def one_workgroup(monkeypatch):
    """The untuned first-byte map without the in-job plan (read when an engine is built)."""
    monkeypatch.setenv("LOCUST_PART_TUNE", "0")
    monkeypatch.setenv("LOCUST_PART_DEFAULT", "byte")
    monkeypatch.setenv("LOCUST_VPLAN", "0")


@gpu_test
@pytest.mark.parametrize("shape", SHAPES)
def test_three_sorts_no_fallback(one_workgroup, shape):
    """m on both sides of 256 and 1,024, all on one engine back to back (the self-cleaning
    scratch sees jobs of very different shape).  At most 1,280 of 2,048 slots are taken
    (62 %), so the 512-probe limit cannot trip: no job falls back."""
    texts = {m: ok.family_text(ok.family(shape, m), m) for m in SORT_SIZES}
    eng = gpu_engine(texts.values())
    for m, text in texts.items():
        assert run_jobs(eng, text, f"{shape} m={m}") == 0, (shape, m, eng.stats())


@gpu_test
@pytest.mark.parametrize("shape", SHAPES)
def test_near_full_table(one_workgroup, shape):
    """1,500 .. 2,048 keys in the 2,048-slot table: exact, whether or not a long probe run
    reports the table full (that depends on the hash; the counts are printed)."""
    texts = {m: ok.family_text(ok.family(shape, m), m) for m in NEAR_FULL}
    eng = gpu_engine(texts.values())
    for m, text in texts.items():
        fb = run_jobs(eng, text, f"{shape} m={m}")
        print(f"near-full {shape} m={m}: {fb} fallbacks in {JOBS} jobs")


@gpu_test
@pytest.mark.parametrize("shape", SHAPES)
def test_table_overflow_falls_back_and_recovers(one_workgroup, shape):
    """2,049 keys cannot fit 2,048 slots: every job redoes its Process stage on the HBM
    table (rank_sort_kernel / key_lt break the ties there) and is still exact; a small job
    on the same engine afterwards takes no fallback."""
    big = ok.family_text(ok.family(shape, 2049), 2049)
    small = ok.family_text(ok.family(shape, 64), 64)
    eng = gpu_engine([big, small])
    assert run_jobs(eng, big, f"{shape} m=2049") == JOBS, eng.stats()
    assert run_jobs(eng, small, f"{shape} m=64 after the overflow") == 0, eng.stats()


@gpu_test
@pytest.mark.parametrize("max_key_len", [29, 31])
def test_staging_capacity(one_workgroup, max_key_len):
    """256 keys of 29 (31) bytes: the small path stages 256 compact records of 5 words,
    its staging area's last word included."""
    keys = ok.family("tie24", 256, digits=5 if max_key_len == 29 else 7)
    assert {len(k) for k in keys} == {max_key_len}
    text = ok.family_text(keys, 256)
    eng = gpu_engine([text], max_key_len=max_key_len)
    assert run_jobs(eng, text, f"tie24 x256, {max_key_len} bytes", max_key=max_key_len) == 0


@gpu_test
@pytest.mark.parametrize("n,distinct,falls_back", [(384, 384, False), (385, 385, False),
                                                  (4096, 100, False), (4097, 100, False),
                                                  (16384, 100, False), (16385, 100, True)])
def test_token_thresholds(one_workgroup, n, distinct, falls_back):
    """Exactly n tokens in the partition: 384 | 385 is where the 512-slot table grows to
    2,048 (kSmallTableTokens); 4,096 | 4,097 a second batch of gathers (kGatherBatch x
    kPartBlock); 16,385 tokens pass the token window (kPartWindow)."""
    _keys, toks = ok.crowded("tie8", n, distinct)
    text = ok.crowded_text(toks, n)
    assert ok.tokens_of(text) == n
    eng = gpu_engine([text])
    assert run_jobs(eng, text, f"tie8 {n} tokens of {distinct}") == (JOBS if falls_back else 0), eng.stats()


@gpu_test
def test_stale_words(one_workgroup):
    """A job of 29-byte keys only, then jobs of as many tokens at the same positions whose
    keys end at 7 .. 24 bytes: the map writes only the words a key has, so the token arrays
    still hold the long keys' words 1..3 there -- none of them may reach a result."""
    m = 700
    texts = [ok.only_text(ok.family("tie24", m), 5)]
    texts += [ok.only_text(ok.fixed_length_keys(n, m), 5) for n in (7, 8, 15, 16, 23, 24)]
    assert len({ok.want(t)[1] for t in texts}) == 1  # the same token count
    eng = gpu_engine(texts)
    for n, text in zip((7, 8, 15, 16, 23, 24), texts[1:]):
        assert run_jobs(eng, texts[0], "29-byte keys") == 0
        assert run_jobs(eng, text, f"{n}-byte keys after 29-byte keys") == 0


@gpu_test
@pytest.mark.parametrize("shape", ["tie24", "edges"])
def test_index_and_top_jobs_same_inputs(one_workgroup, shape):
    """The inverted index and the top-K job take the ordered kernel's other outputs (the
    40-byte records and the sorted key arrays instead of the compact host records): the
    same three sorts, the same keys."""
    texts = [ok.family_text(ok.family(shape, m), m) for m in (256, 257, 1025)]
    eng = lc.Engine(lc.make_config("gpu", check=True), max(map(len, texts)),
                    max(map(ok.num_lines, texts)))
    for text in texts:
        ent, ntok, nuniq = ok.want(text)
        want_e, want_p = lc.utils.oracle.index(text)
        assert want_e == ent
        for _ in range(JOBS):
            r = eng.run_index(text)
            assert (r.num_tokens, r.num_unique) == (ntok, nuniq)
            assert r.entries() == ent and r.postings() == want_p
            t = eng.run_top(text, 10)
            assert t.entries() == lc.utils.oracle.top(ent, 10)


# ---------------------------------------------------------------------------------------
# GPU group B: the in-job plan splits partition 'w' over sibling workgroups
# ---------------------------------------------------------------------------------------

@pytest.fixture(params=["always", "trigger"])
def planned(monkeypatch, request):
    """The untuned first-byte map with the in-job plan: forced in every job, or left to the
    map's trigger (every tile of these texts holds >= 65 'w' tokens, kPlanTrigger = 48)."""
    monkeypatch.setenv("LOCUST_PART_TUNE", "0")
    monkeypatch.setenv("LOCUST_PART_DEFAULT", "byte")
    if request.param == "always":
        monkeypatch.setenv("LOCUST_PLAN_TRIGGER", "0")
    return request.param


def crowded_texts(shape, distinct, tokens=SPLIT_TOKENS):
    return {n: ok.crowded_text(ok.crowded(shape, n, distinct)[1], n) for n in tokens}


@gpu_test
def test_split_short_keys(planned, monkeypatch):
    """6,000 distinct short keys: the siblings' quantile cuts keep every table small at
    16,128 tokens; at 16,129 the plan's token list is cut short by its sample area and the
    job falls back.  The same text without the plan falls back: the split happened."""
    texts = crowded_texts("short", 6000, (16128, 16129))
    eng = gpu_engine(texts.values())
    assert run_jobs(eng, texts[16128], "short x6000, 16128 tokens") == 0, eng.stats()
    assert run_jobs(eng, texts[16129], "short x6000, 16129 tokens") == JOBS, eng.stats()
    monkeypatch.setenv("LOCUST_VPLAN", "0")
    eng = gpu_engine(texts.values())
    assert run_jobs(eng, texts[16128], "short x6000 unplanned") == JOBS, eng.stats()


@gpu_test
def test_split_tied_first_word_one_sibling(planned):
    """1,000 keys that share their first word: every cut is that word, the last sibling
    takes all of them (they fit one table) and the others stay empty."""
    texts = crowded_texts("tie8", 1000)
    eng = gpu_engine(texts.values())
    for n, text in texts.items():
        fb = run_jobs(eng, text, f"tie8 x1000, {n} tokens")
        print(f"plan tie8 x1000 n={n} ({planned}): {fb} fallbacks in {JOBS} jobs")
        # 16,129: the list is cut short in every sibling (n > kPartWindow - 256)
        assert fb == (0 if n <= 16128 else JOBS), (n, eng.stats())


@gpu_test
def test_split_tied_first_word_unsplittable(planned):
    """3,000 keys that share their first word cannot be split on it: every job falls back."""
    texts = crowded_texts("tie8", 3000)
    eng = gpu_engine(texts.values())
    for n, text in texts.items():
        assert run_jobs(eng, text, f"tie8 x3000, {n} tokens") == JOBS, (n, eng.stats())


@gpu_test
@pytest.mark.parametrize("split_min", [None, "16"])
@pytest.mark.parametrize("shape,distinct", [("hot", 1500), ("twolevel", 1600)])
def test_split_hot_and_repeated_cuts(planned, monkeypatch, shape, distinct, split_min):
    """A hot key (63 % .. 91 % of the tokens: most sample values repeat, sibling ranges are
    left empty) and 8 first words of 200 keys each (every cut value has 200 keys on it):
    every key lands in exactly one sibling -- a key lost or doubled shows in num_unique and
    the counts.  LOCUST_SPLIT_MIN=16: many thin siblings."""
    if split_min:
        monkeypatch.setenv("LOCUST_SPLIT_MIN", split_min)
    texts = crowded_texts(shape, distinct)
    eng = gpu_engine(texts.values())
    for n, text in texts.items():
        fb = run_jobs(eng, text, f"{shape} x{distinct}, {n} tokens")
        print(f"plan {shape} n={n} ({planned}, split_min={split_min}): {fb} fallbacks in {JOBS} jobs")


# ---------------------------------------------------------------------------------------
# GPU group C: the other token sources feed the same sorts
# ---------------------------------------------------------------------------------------

def source_texts(shape):
    return {m: ok.family_text(ok.family(shape, m), m) for m in SOURCE_SIZES}


@gpu_test
@pytest.mark.parametrize("devplan", [False, True], ids=["byte_map", "device_plan"])
@pytest.mark.parametrize("shape", SOURCE_SHAPES)
def test_large_pass(monkeypatch, shape, devplan):
    """The two-kernel build (dict_partials_kernel + PartialsSource): an engine for 1 MiB
    without the small-pass route.  byte_map: the untuned first-byte map and no device plan,
    so that partition 'w' merges exactly m distinct keys from its slices' partials (2,049
    never fit; up to 1,025 take at most half the table).  device_plan: every pass cuts its
    own partitions from its text (partplan.hip) -- exactness only."""
    monkeypatch.setenv("LOCUST_SMALL_PASS_KB", "0")
    monkeypatch.setenv("LOCUST_PART_TUNE", "0")
    if not devplan:
        monkeypatch.setenv("LOCUST_DEVPLAN", "0")
        monkeypatch.setenv("LOCUST_PART_DEFAULT", "byte")
    eng = lc._C.GpuEngine(lc.make_config("gpu", reduce_path="lds", check=True), 1 << 20, 1 << 16)
    assert eng.capacity > (1 << 18)  # past kPartBuildMaxTokens: the large build
    texts = source_texts(shape)
    for m, text in texts.items():
        fb = run_jobs(eng, text, f"large pass {shape} m={m}")
        if not devplan:
            assert fb == (JOBS if m == 2049 else 0), (m, eng.stats())
    passes = eng.stats()["planned_passes"]
    print(f"large pass {shape} devplan={devplan}: {passes} planned passes, "
          f"{eng.stats()['fallbacks']} fallbacks in {JOBS * len(texts)} jobs")
    assert (passes > 0) == devplan, eng.stats()


@gpu_test
@pytest.mark.parametrize("lead", [b"w", b"\xe9"], ids=["w", "xe9"])
@pytest.mark.parametrize("shape", SOURCE_SHAPES)
def test_default_configuration(shape, lead):
    """No switches: the starting map, the in-job plan and the retuning between jobs.  Lead
    byte 0xe9: the first word's top bit is set as well (the partition cuts compare it)."""
    texts = {m: ok.family_text(ok.family(shape, m, lead), m) for m in SOURCE_SIZES}
    eng = gpu_engine(texts.values())
    for m, text in texts.items():
        run_jobs(eng, text, f"default {shape} m={m}")


@gpu_test
@pytest.mark.parametrize("combine", [False, True], ids=["runs", "combined"])
@pytest.mark.parametrize("shape", SOURCE_SHAPES)
def test_gather_merge(monkeypatch, shape, combine):
    """Three ranks, gather strategy.  Without the map-side combine the root merges the
    ranks' sorted runs in the ordered kernel (RunsSource, launch_dict_merge_runs) -- on the
    untuned first-byte map, so partition 'w' again holds exactly m keys; with it the runs
    hold distinct keys and the root merges them by binary search (the default route)."""
    monkeypatch.setenv("LOCUST_PART_TUNE", "0")
    monkeypatch.setenv("LOCUST_PART_DEFAULT", "byte")
    for m, text in source_texts(shape).items():
        exp = ok.want(text)
        for j in range(JOBS):
            r = lc.run_multi(text, 3, strategy="gather", comm="loopback", check=True, combine=combine)
            check(r, exp, f"gather {shape} m={m} job {j}")


@gpu_test
@pytest.mark.parametrize("shape", SHAPES)
def test_radix_engine_same_inputs(shape):
    """The radix-sort engine is held to the same inputs as the dictionary."""
    text = ok.family_text(ok.family(shape, 1025), 1025)
    eng = lc._C.GpuEngine(lc.make_config("gpu", sort="radix", check=True), len(text),
                          ok.num_lines(text))
    exp = ok.want(text)
    for j in range(JOBS):
        check(eng.run(text), exp, f"radix {shape} job {j}")

