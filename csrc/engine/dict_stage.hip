// Stage-level entry points of the dictionary fallback kernels and the partition plan
// (locust/dict_stage.hpp): one launch_* of dict.hip / partplan.hip per call, on plain device
// buffers of its own.
// Every size a kernel indexes by is checked here first, so no launch can leave its buffers.
#include "locust/dict_stage.hpp"

#include <algorithm>
#include <cstring>

#include "locust/device/dict_consts.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"
#include "stage_buf.hpp"

namespace locust {
namespace {

using stage::DevBuf;
using stage::DevKeys;
using stage::sync;
constexpr u64 kGuard = kDictStageGuard;

template <class T>
bool all_pattern(const T* p, u64 count) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
  for (u64 i = 0; i < count * sizeof(T); ++i)
    if (b[i] != kDictStagePattern) return false;
  return true;
}
template <class T>
bool all_zero(const T* p, u64 count) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
  for (u64 i = 0; i < count * sizeof(T); ++i)
    if (b[i] != 0) return false;
  return true;
}

void check_keys(const std::vector<PackedKey>& keys) {
  LOCUST_CHECK_ARG(keys.size() < (1ull << 31), "dict stage: too many keys");
  for (const PackedKey& k : keys)
    LOCUST_CHECK_ARG(dict_stage_valid_key(k.w), "dict stage: not a valid packed key");
}

// The tokens of insert / part_build: the keys and their counts, then a guard of pattern
// entries (valid keys of 32 non-NUL bytes: a kernel that read past its bound would count
// them, not spin on them).
struct DevTokens {
  DevKeys keys;
  DevBuf<u64> counts;
  DevBuf<u32> d_n;
  DevTokens(const std::vector<PackedKey>& k, const std::vector<u64>* c, u32 n_dev)
      : keys(k.size() + kGuard), counts(k.size() + kGuard), d_n(1) {
    keys.fill(kDictStagePattern);
    counts.fill(kDictStagePattern);
    keys.upload(k.data(), k.size());
    if (c) counts.upload(c->data(), c->size());
    d_n.upload(&n_dev, 1);
  }
};

void check_tokens(const std::vector<PackedKey>& keys, const std::vector<u64>* counts, u32 d_n,
                  u64 cap) {
  check_keys(keys);
  LOCUST_CHECK_ARG(!counts || counts->size() == keys.size(), "dict stage: one count per key");
  LOCUST_CHECK_ARG(std::min<u64>(d_n, cap) <= keys.size(),
                   "dict stage: min(d_n, cap) keys must be uploaded");
  LOCUST_CHECK_ARG((u64)d_n <= keys.size() + kGuard,
                   "dict stage: d_n must stay within the guard behind the keys");
}

// The dense arrays of a DictWorkspace: ucap entries and the guard.
struct DevDense {
  u32 ucap;
  DevKeys ukeys;
  DevBuf<u64> ucount, uval;
  DevBuf<u32> urank;
  DevBuf<MapCounters> ctr;
  explicit DevDense(u32 cap)
      : ucap(cap), ukeys(cap + kGuard), ucount(cap + kGuard), uval(cap + kGuard),
        urank(cap + kGuard), ctr(1) {
    ukeys.fill(kDictStagePattern);
    ucount.fill(kDictStagePattern);
    uval.fill(kDictStagePattern);
    urank.fill(kDictStagePattern);
    ctr.fill(0);
  }
  DictWorkspace workspace(DictSlot* table, u32 mask) {
    DictWorkspace dw{};
    dw.table = table;
    dw.mask = mask;
    dw.ukeys = ukeys.soa();
    dw.ucount = ucount.p;
    dw.uval = uval.p;
    dw.ucap = ucap;
    dw.urank = urank.p;
    return dw;
  }
  // The dense view after the launch.  zeroed_counts: ucount[0, ucap) started as zeros
  // (insert), else as pattern like everything else (part_build, which also fills uval /
  // urank of its entries).
  DictStageDense read(bool zeroed_counts) {
    DictStageDense r;
    MapCounters c;
    ctr.download(&c, 1);
    r.num_unique = c.num_unique;
    r.flags = c.flags;
    const u64 all = (u64)ucap + kGuard;
    const u64 held = std::min<u64>(c.num_unique, ucap);
    std::vector<PackedKey> k = ukeys.download_all();
    std::vector<u64> cnt = ucount.download_all(), val = uval.download_all();
    std::vector<u32> rk = urank.download_all();
    bool ok = all_pattern(k.data() + held, all - held);
    if (zeroed_counts) {
      ok = ok && all_zero(cnt.data() + held, ucap - held) && all_pattern(cnt.data() + ucap, kGuard);
      ok = ok && all_pattern(val.data(), all) && all_pattern(rk.data(), all);
    } else {
      ok = ok && all_pattern(cnt.data() + held, all - held);
      ok = ok && all_pattern(val.data() + held, all - held) && all_pattern(rk.data() + held, all - held);
      r.uval.assign(val.begin(), val.begin() + held);
      r.urank.assign(rk.begin(), rk.begin() + held);
    }
    r.tail_intact = ok;
    r.keys.assign(k.begin(), k.begin() + held);
    r.counts.assign(cnt.begin(), cnt.begin() + held);
    return r;
  }
};

MapCounters to_ctr(const DictStageCounters& c) {
  MapCounters m{};
  m.num_records = c.num_records;
  m.map_tokens = c.map_tokens;
  m.num_unique = c.num_unique;
  m.overflow_lines = c.overflow_lines;
  m.truncated = c.truncated;
  m.num_newlines = c.num_newlines;
  m.max_key_len = c.max_key_len;
  m.total_count = c.total_count;
  m.flags = c.flags;
  return m;
}
DictStageCounters from_ctr(const MapCounters& m) {
  DictStageCounters c;
  c.num_records = m.num_records;
  c.map_tokens = m.map_tokens;
  c.num_unique = m.num_unique;
  c.overflow_lines = m.overflow_lines;
  c.truncated = m.truncated;
  c.num_newlines = m.num_newlines;
  c.max_key_len = m.max_key_len;
  c.total_count = m.total_count;
  c.flags = m.flags;
  return c;
}

// rank[0, u) must be a permutation of [0, u): the emit and the scatter index their output
// by it.
void check_permutation(const std::vector<u32>& rank, u64 u) {
  std::vector<char> seen(u, 0);
  for (u64 i = 0; i < u; ++i) {
    LOCUST_CHECK_ARG(rank[i] < u && !seen[rank[i]], "dict stage: rank must be a permutation of [0, u)");
    seen[rank[i]] = 1;
  }
}

static_assert(sizeof(OutRecord) == sizeof(KeyCount), "output records read back as KeyCount");

}  // namespace

bool dict_stage_valid_key(const u64* w) {
  bool ended = false;
  for (int i = 0; i < kKeyBytes; ++i) {
    const unsigned c = (unsigned)(w[i >> 3] >> (56 - 8 * (i & 7))) & 0xffu;
    if (c == 0)
      ended = true;
    else if (ended)
      return false;
  }
  return true;
}

std::vector<std::pair<std::string, u64>> dict_stage_constants() {
  return {{"kLdsSlots", (u64)kLdsSlots},
          {"kLdsProbes", (u64)kLdsProbes},
          {"kInsBlock", (u64)kInsBlock},
          {"kPartSlots", (u64)kPartSlots},
          {"kPartProbes", (u64)kPartProbes},
          {"kPartWindow", (u64)kPartWindow},
          {"kPlanSamples", (u64)kPlanSamples},
          {"kSingletonWeight", (u64)kSingletonWeight},
          {"kRankI", (u64)kRankI},
          {"kPackTile", (u64)kPackTile},
          {"kRankSortMax", (u64)kRankSortMax},
          {"kDictParts", (u64)kDictParts},
          {"kWordMagic", kWordMagic},
          {"kIdFull", (u64)kIdFull},
          {"kCtrDictOverflow", (u64)kCtrDictOverflow},
          {"kCtrNotEmitted", (u64)kCtrNotEmitted},
          {"kStagePattern", (u64)kDictStagePattern},
          {"kStageGuard", (u64)kDictStageGuard}};
}

DictStageDense dict_stage_insert(const std::vector<PackedKey>& keys,
                                 const std::vector<u64>* counts, u32 d_n, u64 cap,
                                 u64 table_slots, u32 ucap, u32 max_blocks) {
  check_tokens(keys, counts, d_n, cap);
  LOCUST_CHECK_ARG(table_slots >= 1 && (table_slots & (table_slots - 1)) == 0 &&
                       table_slots <= (1ull << 31),
                   "dict stage: table_slots must be a power of two");
  LOCUST_CHECK_ARG(max_blocks >= 1 && max_blocks <= 1024, "dict insert: 1..1024 workgroups");
  DevTokens tok(keys, counts, d_n);
  DevBuf<DictSlot> table(table_slots);
  table.fill(0);
  DevDense dense(ucap);
  dense.ucount.fill(0, ucap);  // only ever updated by atomics: zeroed per run
  const DictWorkspace dw = dense.workspace(table.p, (u32)(table_slots - 1));
  launch_dict_insert(tok.keys.soa(), counts ? tok.counts.p : nullptr, tok.d_n.p, cap, dw,
                     dense.ctr.p, nullptr, max_blocks);
  sync();
  DictStageDense r = dense.read(true);
  const std::vector<DictSlot> slots = table.download_all();
  for (u64 s = 0; s < table_slots; ++s) {
    const DictSlot& sl = slots[s];
    if (sl.w[0] == 0 && sl.id == 0) continue;
    DictStageSlot e;
    e.slot = (u32)s;
    e.id = sl.id;
    e.key.w[0] = sl.w[0];
    for (int j = 1; j < kKeyWords; ++j) e.key.w[j] = sl.w[j] ^ kWordMagic;
    r.table.push_back(e);
  }
  return r;
}

DictStageDense dict_stage_part_build(const std::vector<PackedKey>& keys,
                                     const std::vector<u64>* counts, const std::vector<u8>& parts,
                                     u32 d_n, u64 cap, u32 ucap) {
  check_tokens(keys, counts, d_n, cap);
  LOCUST_CHECK_ARG(parts.size() == keys.size(), "dict stage: one partition tag per key");
  DevTokens tok(keys, counts, d_n);
  // readable to align_up(n, 16), and a block more; pattern bytes behind the tags
  DevBuf<u8> d_parts(align_up(keys.size() + kGuard, 16) + 16);
  d_parts.fill(kDictStagePattern);
  d_parts.upload(parts.data(), parts.size());
  DevDense dense(ucap);
  const DictWorkspace dw = dense.workspace(nullptr, 0);
  launch_dict_part_build(tok.keys.soa(), counts ? tok.counts.p : nullptr, d_parts.p, tok.d_n.p,
                         cap, dw, dense.ctr.p, nullptr);
  sync();
  return dense.read(false);
}

DictStageRank dict_stage_rank(const std::vector<PackedKey>& keys, const std::vector<u64>* counts,
                              u32 d_u, u64 cap) {
  check_keys(keys);
  LOCUST_CHECK_ARG(!counts || counts->size() == keys.size(), "dict stage: one count per key");
  LOCUST_CHECK_ARG(cap <= keys.size(), "dict stage: cap keys must be uploaded");
  DevKeys d_keys(keys.size());
  d_keys.upload(keys.data(), keys.size());
  DevBuf<u64> d_counts(keys.size());
  if (counts) d_counts.upload(counts->data(), counts->size());
  DevBuf<u32> d_du(1);
  d_du.upload(&d_u, 1);
  DevBuf<u32> d_rank(cap + kGuard);
  DevBuf<u64> d_val(cap + kGuard);
  d_rank.fill(kDictStagePattern);
  d_val.fill(kDictStagePattern);
  d_rank.fill(0, cap);  // the kernel accumulates into both
  d_val.fill(0, cap);
  launch_rank_sort(d_keys.soa(), counts ? d_counts.p : nullptr, d_du.p, cap, d_rank.p,
                   counts ? d_val.p : nullptr, nullptr);
  sync();
  DictStageRank r;
  r.rank = d_rank.download_all();
  r.val = d_val.download_all();
  r.tail_intact = all_pattern(r.rank.data() + cap, kGuard) && all_pattern(r.val.data() + cap, kGuard);
  r.rank.resize(cap);
  r.val.resize(cap);
  return r;
}

DictStageEmit dict_stage_emit(const std::vector<PackedKey>& keys, const std::vector<u64>& counts,
                              const std::vector<u32>& rank, const std::vector<u64>& val,
                              const DictStageCounters& ctr, u64 cap) {
  check_keys(keys);
  LOCUST_CHECK_ARG(counts.size() == keys.size() && rank.size() == keys.size() &&
                       val.size() == keys.size(),
                   "dict stage: one count, rank and val per key");
  LOCUST_CHECK_ARG(cap <= keys.size(), "dict stage: cap keys must be uploaded");
  const u64 u = std::min<u64>(ctr.num_unique, cap);
  if (u <= (u64)kRankSortMax) check_permutation(rank, u);
  DevKeys d_keys(keys.size());
  d_keys.upload(keys.data(), keys.size());
  DevBuf<u64> d_counts(keys.size()), d_val(keys.size());
  d_counts.upload(counts.data(), counts.size());
  d_val.upload(val.data(), val.size());
  DevBuf<u32> d_rank(keys.size());
  d_rank.upload(rank.data(), rank.size());
  const MapCounters c = to_ctr(ctr);
  DevBuf<MapCounters> d_ctr(1), d_ctr_out(1);
  d_ctr.upload(&c, 1);
  d_ctr_out.fill(kDictStagePattern);
  DevBuf<OutRecord> d_out(cap + kGuard);
  d_out.fill(kDictStagePattern);
  launch_rank_emit(d_keys.soa(), d_counts.p, d_rank.p, d_val.p, cap, d_ctr.p, d_out.p,
                   d_ctr_out.p, nullptr);
  sync();
  DictStageEmit r;
  MapCounters co;
  d_ctr_out.download(&co, 1);
  r.ctr_out = from_ctr(co);
  std::vector<KeyCount> all(cap + kGuard);
  d_out.download(reinterpret_cast<OutRecord*>(all.data()), all.size());
  r.untouched = all_pattern(all.data(), all.size());
  r.tail_intact = all_pattern(all.data() + u, all.size() - u);
  all.resize(u);
  r.records = std::move(all);
  return r;
}

DictStageScatter dict_stage_scatter(const std::vector<PackedKey>& keys,
                                    const std::vector<u64>& counts, const std::vector<u32>& rank,
                                    u32 d_u, u64 cap) {
  check_keys(keys);
  LOCUST_CHECK_ARG(counts.size() == keys.size() && rank.size() == keys.size(),
                   "dict stage: one count and rank per key");
  LOCUST_CHECK_ARG(cap <= keys.size(), "dict stage: cap keys must be uploaded");
  const u64 u = std::min<u64>(d_u, cap);
  if (u <= (u64)kRankSortMax) check_permutation(rank, u);
  DevKeys d_keys(keys.size());
  d_keys.upload(keys.data(), keys.size());
  DevBuf<u64> d_counts(keys.size());
  d_counts.upload(counts.data(), counts.size());
  DevBuf<u32> d_rank(keys.size());
  d_rank.upload(rank.data(), rank.size());
  DevBuf<u32> d_du(1);
  d_du.upload(&d_u, 1);
  DevKeys d_sorted(cap + kGuard);
  d_sorted.fill(kDictStagePattern);
  DevBuf<u64> d_sc(cap + kGuard);
  d_sc.fill(kDictStagePattern);
  launch_rank_scatter(d_keys.soa(), d_counts.p, d_rank.p, d_du.p, cap, d_sorted.soa(), d_sc.p,
                      nullptr);
  sync();
  DictStageScatter r;
  r.sorted = d_sorted.download_all();
  r.counts = d_sc.download_all();
  r.tail_intact = all_pattern(r.sorted.data() + cap, kGuard) && all_pattern(r.counts.data() + cap, kGuard);
  r.sorted.resize(cap);
  r.counts.resize(cap);
  return r;
}

DictStageScanPack dict_stage_scan_pack(const std::vector<PackedKey>& sorted,
                                       const std::vector<u64>& counts,
                                       const DictStageCounters& ctr, u64 cap, u32 emit_limit,
                                       bool with_ctr_out) {
  check_keys(sorted);
  LOCUST_CHECK_ARG(counts.size() == sorted.size(), "dict stage: one count per key");
  LOCUST_CHECK_ARG(cap <= sorted.size(), "dict stage: cap keys must be uploaded");
  LOCUST_CHECK_ARG(ctr.num_unique <= cap, "dict stage: num_unique must not exceed cap");
  u64 sum = 0;
  for (u64 c : counts) {
    LOCUST_CHECK_ARG(c < (1ull << 62) && sum + c < (1ull << 62),
                     "dict stage: count sum too large for the look-back word");
    sum += c;
  }
  const u64 u = ctr.num_unique;
  DevKeys d_keys(sorted.size());
  d_keys.upload(sorted.data(), sorted.size());
  DevBuf<u64> d_counts(sorted.size());
  d_counts.upload(counts.data(), counts.size());
  MapCounters c = to_ctr(ctr);
  std::memset(&c.total_count, kDictStagePattern, sizeof c.total_count);
  DevBuf<MapCounters> d_ctr(1), d_ctr_out(1);
  d_ctr.upload(&c, 1);
  d_ctr_out.fill(kDictStagePattern);
  DevBuf<u64> d_status(div_up(cap ? cap : 1, kPackTile) + 1);
  d_status.fill(0);
  DevBuf<u32> d_tile(1);
  d_tile.fill(0);
  DevBuf<OutRecord> d_out(cap + kGuard);
  d_out.fill(kDictStagePattern);
  launch_scan_pack(d_keys.soa(), d_counts.p, cap, d_ctr.p, d_out.p,
                   LookbackScratch{d_status.p, d_tile.p}, nullptr,
                   with_ctr_out ? d_ctr_out.p : nullptr, emit_limit);
  sync();
  DictStageScanPack r;
  MapCounters co;
  d_ctr.download(&co, 1);
  r.total_count = co.total_count;
  d_ctr_out.download(&co, 1);
  r.ctr_out = from_ctr(co);
  std::vector<KeyCount> all(cap + kGuard);
  d_out.download(reinterpret_cast<OutRecord*>(all.data()), all.size());
  r.untouched = all_pattern(all.data(), all.size());
  r.tail_intact = all_pattern(all.data() + u, all.size() - u);
  all.resize(u);
  r.records = std::move(all);
  return r;
}

std::vector<u64> dict_stage_part_plan(const std::vector<u64>& w0, const std::vector<u64>& counts,
                                      u32 d_u, u32 ucap) {
  LOCUST_CHECK_ARG(w0.size() < (1ull << 31) && counts.size() == w0.size(),
                   "dict stage: one count per first word");
  LOCUST_CHECK_ARG((u64)ucap <= w0.size(), "dict stage: ucap entries must be uploaded");
  DevBuf<u64> d_w0(w0.size()), d_cnt(w0.size());
  d_w0.upload(w0.data(), w0.size());
  d_cnt.upload(counts.data(), counts.size());
  DevBuf<u32> d_du(1);
  d_du.upload(&d_u, 1);
  DevBuf<PartMapTables> d_out(1);
  d_out.fill(kDictStagePattern);
  launch_part_plan(d_w0.p, d_cnt.p, d_du.p, ucap, d_out.p, nullptr);
  sync();
  PartMapTables t;
  d_out.download(&t, 1);
  return std::vector<u64>(t.lo, t.lo + kDictParts + 1);
}

}  // namespace locust
