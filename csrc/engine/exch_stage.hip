// Stage-level entry points of the device-resident shuffle (locust/exch_stage.hpp): one
// launch_* of exchange.hip / shuffle.hip / merge.hip per call, on plain device buffers of
// its own.
// Every size a kernel indexes by is checked here first, so no launch can leave its buffers.
#include "locust/exch_stage.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <utility>

#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"
#include "stage_buf.hpp"

namespace locust {
namespace {

using stage::DevBuf;
using stage::DevKeys;
using stage::kStageMaxBytes;
using stage::sync;

bool all_pattern(const char* p, u64 bytes) {
  for (u64 i = 0; i < bytes; ++i)
    if ((unsigned char)p[i] != kExchStagePattern) return false;
  return true;
}

// launch_exch_pack behind the ExchCtl in d_ctl, then the send buffer taken apart.
void pack_and_read(const ExchCtl* d_ctl, u32 P, const std::vector<KeyCount>& records,
                   u32 slot_records, u64 pack_cap, ExchStagePlan* out) {
  const u64 sb = exch_slot_bytes(slot_records);
  LOCUST_CHECK_ARG((u64)P * sb <= kStageMaxBytes, "exchange stage: send buffer too large");
  const u32 n = (u32)records.size();
  DevBuf<KeyCount> d_recs(n);
  d_recs.upload(records.data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  DevBuf<char> d_send((u64)P * sb);
  d_send.fill(kExchStagePattern);
  launch_exch_pack(d_recs.p, d_n.p, pack_cap ? pack_cap : n, d_ctl, P, slot_records, d_send.p,
                   nullptr);
  sync();
  std::vector<char> send((u64)P * sb);
  d_send.download(send.data(), send.size());
  out->slots.resize(P);
  for (u32 d = 0; d < P; ++d) {
    ExchStageSlot& sl = out->slots[d];
    const char* base = send.data() + (u64)d * sb;
    std::memcpy(&sl.header, base, sizeof(SlotHeader));
    const char* area = base + sizeof(SlotHeader);
    const u64 held = std::min<u64>(sl.header.n, slot_records);
    sl.records.resize(held);
    if (held) std::memcpy(sl.records.data(), area, held * sizeof(KeyCount));
    sl.tail_intact = all_pattern(area + held * sizeof(KeyCount), (slot_records - held) * sizeof(KeyCount));
    sl.dirty_records = 0;
    for (u64 r = slot_records; r > 0; --r)
      if (!all_pattern(area + (r - 1) * sizeof(KeyCount), sizeof(KeyCount))) {
        sl.dirty_records = r;
        break;
      }
  }
}

}  // namespace

ExchStagePlan exch_stage_plan_pack(u32 P, u32 S, const std::vector<i32>& status,
                                   const std::vector<u64>& n_local,
                                   const std::vector<PackedKey>& samples,
                                   const std::vector<KeyCount>& records, u32 slot_records,
                                   u64 pack_cap) {
  // (the same shape check as ShardEngine's exchange: the kernels' tables hold 64 ranks)
  LOCUST_CHECK_ARG(P >= 1 && P <= kExchMaxRanks, "exchange: bad shape");
  LOCUST_CHECK_ARG(S >= 1 && S <= 4096, "exchange stage: 1..4096 samples per rank");
  LOCUST_CHECK_ARG(status.size() == P && n_local.size() == P && samples.size() == (u64)P * S,
                   "exchange stage: need P statuses, P counts and P x S samples");
  LOCUST_CHECK_ARG(records.size() < (1ull << 32), "exchange stage: too many records");
  const u64 mb = exch_msg1_bytes(S);
  std::vector<char> msgs((u64)P * mb);
  for (u32 r = 0; r < P; ++r) {
    ExchMsg1 h{};
    h.status = status[r];
    h.n_local = n_local[r];
    std::memcpy(msgs.data() + (u64)r * mb, &h, sizeof h);
    std::memcpy(msgs.data() + (u64)r * mb + sizeof h, samples.data() + (u64)r * S,
                (u64)S * sizeof(PackedKey));
  }
  const u32 n = (u32)records.size();
  DevBuf<char> d_msgs(msgs.size());
  d_msgs.upload(msgs.data(), msgs.size());
  DevKeys d_keys(n);
  d_keys.upload(records.data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  DevBuf<ExchCtl> d_ctl(1);
  d_ctl.fill(kExchStagePattern);
  launch_exch_plan(d_msgs.p, P, S, d_keys.soa(), d_n.p, slot_records, d_ctl.p, nullptr);
  sync();
  ExchStagePlan out;
  d_ctl.download(&out.ctl, 1);
  // the pack kernel indexes the records by these offsets: they must describe them
  for (u32 p = 0; p < P; ++p)
    if (out.ctl.off[p] > out.ctl.off[p + 1] || out.ctl.off[p + 1] > n)
      throw Error("exchange stage: the plan's offsets leave the records");
  if (out.ctl.off[0] != 0 || out.ctl.off[P] != n)
    throw Error("exchange stage: the plan's offsets do not cover the records");
  pack_and_read(d_ctl.p, P, records, slot_records, pack_cap, &out);
  return out;
}

ExchStagePlan exch_stage_pack(const ExchCtl& ctl, u32 P, const std::vector<KeyCount>& records,
                              u32 slot_records, u64 pack_cap) {
  LOCUST_CHECK_ARG(P >= 1 && P <= kExchMaxRanks, "exchange: bad shape");
  LOCUST_CHECK_ARG(records.size() < (1ull << 32), "exchange stage: too many records");
  LOCUST_CHECK_ARG(ctl.off[0] == 0 && ctl.off[P] == records.size(),
                   "exchange stage: offsets must cover the records");
  for (u32 p = 0; p < P; ++p)
    LOCUST_CHECK_ARG(ctl.off[p] <= ctl.off[p + 1], "exchange stage: offsets must ascend");
  DevBuf<ExchCtl> d_ctl(1);
  d_ctl.upload(&ctl, 1);
  ExchStagePlan out;
  out.ctl = ctl;
  pack_and_read(d_ctl.p, P, records, slot_records, pack_cap, &out);
  return out;
}

std::vector<PackedKey> exch_stage_sample(const std::vector<PackedKey>& sorted, u32 S) {
  LOCUST_CHECK_ARG(S >= 1 && S <= (1u << 20), "exchange stage: 1..2^20 samples");
  LOCUST_CHECK_ARG(sorted.size() < (1ull << 32), "exchange stage: too many keys");
  const u32 n = (u32)sorted.size();
  DevKeys d_keys(n);
  d_keys.upload(sorted.data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  DevBuf<PackedKey> d_out(S);
  d_out.fill(kExchStagePattern);
  launch_sample_keys(d_keys.soa(), d_n.p, S, d_out.p, nullptr);
  sync();
  std::vector<PackedKey> out(S);
  d_out.download(out.data(), S);
  return out;
}

u32 exch_stage_dict_overflow_flag() { return kCtrDictOverflow; }

ExchStageHeader exch_stage_header(const ExchStageCounters& c, const ExchMsg1& tmpl,
                                  bool combined, const std::vector<PackedKey>& sorted, u32 S,
                                  u32 guard) {
  LOCUST_CHECK_ARG(S <= (1u << 20) && guard <= 1024, "exchange stage: too many samples");
  LOCUST_CHECK_ARG(sorted.size() < (1ull << 32), "exchange stage: too many keys");
  MapCounters ctr{};
  ctr.flags = c.flags;
  ctr.num_unique = c.num_unique;
  ctr.num_records = c.num_records;
  ctr.map_tokens = c.map_tokens;
  ctr.overflow_lines = c.overflow_lines;
  ctr.truncated = c.truncated;
  ctr.max_key_len = c.max_key_len;
  const u32 n = (u32)sorted.size();
  DevBuf<MapCounters> d_ctr(1);
  d_ctr.upload(&ctr, 1);
  DevKeys d_keys(n);
  d_keys.upload(sorted.data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  const u64 bytes = exch_msg1_bytes(S + guard);
  DevBuf<char> d_out(bytes);
  d_out.fill(kExchStagePattern);
  launch_exch_header(d_ctr.p, tmpl, combined, reinterpret_cast<ExchMsg1*>(d_out.p), nullptr,
                     d_keys.soa(), d_n.p, S);
  sync();
  std::vector<char> raw(bytes);
  d_out.download(raw.data(), bytes);
  ExchStageHeader out;
  std::memcpy(&out.msg, raw.data(), sizeof(ExchMsg1));
  out.samples.resize(S);
  if (S) std::memcpy(out.samples.data(), raw.data() + sizeof(ExchMsg1), (u64)S * sizeof(PackedKey));
  out.tail_intact = all_pattern(raw.data() + exch_msg1_bytes(S), (u64)guard * sizeof(PackedKey));
  return out;
}

std::vector<u64> exch_stage_offsets(const std::vector<PackedKey>& sorted,
                                    const std::vector<PackedKey>& splitters, u32 P) {
  LOCUST_CHECK_ARG(P >= 1 && P <= (1u << 16) && splitters.size() == (u64)P - 1,
                   "exchange stage: P buckets need P - 1 splitters");
  LOCUST_CHECK_ARG(sorted.size() < (1ull << 32), "exchange stage: too many keys");
  const u32 n = (u32)sorted.size();
  DevKeys d_keys(n);
  d_keys.upload(sorted.data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  DevBuf<PackedKey> d_sp(P - 1);
  d_sp.upload(splitters.data(), P - 1);
  DevBuf<u64> d_off((u64)P + 1);
  d_off.fill(kExchStagePattern);
  launch_bucket_offsets(d_keys.soa(), d_n.p, d_sp.p, P, d_off.p, nullptr);
  sync();
  std::vector<u64> out((u64)P + 1);
  d_off.download(out.data(), out.size());
  return out;
}

ExchStageRoundTrip exch_stage_roundtrip(const std::vector<PackedKey>& keys,
                                        const std::vector<u64>* counts,
                                        const std::vector<u64>& lo) {
  LOCUST_CHECK_ARG(keys.size() < (1ull << 32), "exchange stage: too many keys");
  LOCUST_CHECK_ARG(!counts || counts->size() == keys.size(), "exchange stage: one count per key");
  LOCUST_CHECK_ARG(lo.empty() || lo.size() == (size_t)kDictParts + 1,
                   "lo needs kDictParts + 1 entries");
  const u32 n = (u32)keys.size();
  DevKeys d_keys(n), d_back(n);
  d_keys.upload(keys.data(), n);
  DevBuf<u64> d_counts(n), d_counts_back(n);
  if (counts) d_counts.upload(counts->data(), n);
  DevBuf<u32> d_n(1);
  d_n.upload(&n, 1);
  DevBuf<KeyCount> d_recs(n);
  d_recs.fill(kExchStagePattern);
  DevBuf<u8> d_parts(n);
  DevBuf<u64> d_lo(kDictParts + 1);
  PartMap pm;
  if (!lo.empty()) {
    d_lo.upload(lo.data(), lo.size());
    pm.lo = d_lo.p;
  }
  for (int j = 0; j < kKeyWords; ++j)
    LOCUST_HIP_CHECK(hipMemset(d_back.word(j), kExchStagePattern, (u64)std::max(n, 1u) * sizeof(u64)));
  d_counts_back.fill(kExchStagePattern);
  d_parts.fill(kExchStagePattern);
  launch_pack_records(d_keys.soa(), counts ? d_counts.p : nullptr, d_n.p, n, d_recs.p, nullptr);
  launch_unpack_records(d_recs.p, n, d_back.soa(), d_counts_back.p, d_parts.p, nullptr, pm);
  sync();
  ExchStageRoundTrip out;
  out.packed.resize(n);
  out.keys.resize(n);
  out.counts.resize(n);
  out.parts.resize(n);
  d_recs.download(out.packed.data(), n);
  d_back.download(out.keys.data(), n);
  d_counts_back.download(out.counts.data(), n);
  d_parts.download(out.parts.data(), n);
  return out;
}

ExchStageReport exch_stage_report(const std::vector<SlotHeader>& headers, u32 slot_records,
                                  const ExchCtl& ctl, const std::vector<u64>& acc,
                                  u32 gather_records) {
  const u32 P = (u32)headers.size();
  LOCUST_CHECK_ARG(headers.size() >= 1 && headers.size() <= kExchMaxRanks, "exchange: bad shape");
  LOCUST_CHECK_ARG(acc.size() == 3u * kMergeAccSpread, "exchange stage: 64 accumulator triples");
  const u64 sb = exch_slot_bytes(slot_records);
  LOCUST_CHECK_ARG((u64)P * sb <= kStageMaxBytes, "exchange stage: receive buffer too large");
  std::vector<char> recv((u64)P * sb, (char)kExchStagePattern);
  for (u32 q = 0; q < P; ++q) std::memcpy(recv.data() + (u64)q * sb, &headers[q], sizeof(SlotHeader));
  DevBuf<char> d_recv(recv.size());
  d_recv.upload(recv.data(), recv.size());
  DevBuf<ExchCtl> d_ctl(1);
  d_ctl.upload(&ctl, 1);
  DevBuf<u64> d_acc(acc.size());
  d_acc.upload(acc.data(), acc.size());
  DevBuf<ExchMsg3> d_msg(1);
  d_msg.fill(kExchStagePattern);
  launch_exch_report(d_recv.p, P, slot_records, d_ctl.p, d_acc.p, gather_records, d_msg.p,
                     nullptr);
  sync();
  ExchStageReport out;
  d_msg.download(&out.msg, 1);
  out.acc.resize(acc.size());
  d_acc.download(out.acc.data(), out.acc.size());
  return out;
}

// ---- the shuffle tail (merge.hip) ----
namespace {

static_assert(sizeof(OutRecord) == sizeof(KeyCount), "output records read back as KeyCount");

// Host image of the slot buffer: pattern bytes, then each slot's header and records.
std::vector<KeyCount> slot_image(const std::vector<ExchStageMergeSlot>& slots, u32 slot_records) {
  LOCUST_CHECK_ARG(slots.size() >= 1 && slots.size() <= (size_t)kMaxMergeRunsHost,
                   "merge stage: 1..64 slots");
  LOCUST_CHECK_ARG(slot_records >= 1 && (u64)slots.size() * slot_records <= kMergeMaxRecords,
                   "merge stage: too many records to merge");
  const u64 stride = (u64)kSlotHeaderRecords + slot_records;
  std::vector<KeyCount> img(slots.size() * stride);
  std::memset(img.data(), kExchStagePattern, img.size() * sizeof(KeyCount));
  for (size_t q = 0; q < slots.size(); ++q) {
    LOCUST_CHECK_ARG(slots[q].records.size() <= slot_records, "merge stage: slot overfilled");
    // whatever its status: no reading of the header may take pattern bytes for records
    LOCUST_CHECK_ARG(std::min<u64>(slots[q].header.n, slot_records) <= slots[q].records.size(),
                     "merge stage: a header announces records the slot does not hold");
    std::memcpy(&img[q * stride], &slots[q].header, sizeof(SlotHeader));
    if (!slots[q].records.empty())
      std::memcpy(&img[q * stride + kSlotHeaderRecords], slots[q].records.data(),
                  slots[q].records.size() * sizeof(KeyCount));
  }
  return img;
}

// What the kernels will take as run q: the records of the image, pattern ones included.
std::pair<const KeyCount*, u64> effective_run(const std::vector<KeyCount>& img, size_t q,
                                              u32 slot_records) {
  const u64 stride = (u64)kSlotHeaderRecords + slot_records;
  SlotHeader h;
  std::memcpy(&h, &img[q * stride], sizeof h);
  const u64 len = h.status == kSlotOk ? std::min<u64>(h.n, slot_records) : 0;
  return {&img[q * stride + kSlotHeaderRecords], len};
}

u64 distinct_keys(const std::vector<KeyCount>& img, size_t nslots, u32 slot_records) {
  std::vector<PackedKey> keys;
  for (size_t q = 0; q < nslots; ++q) {
    const auto run = effective_run(img, q, slot_records);
    for (u64 i = 0; i < run.second; ++i) {
      PackedKey k;
      std::memcpy(k.w, run.first[i].w, sizeof k.w);
      keys.push_back(k);
    }
  }
  std::sort(keys.begin(), keys.end(), key_less);
  return (u64)(std::unique(keys.begin(), keys.end(),
                           [](const PackedKey& a, const PackedKey& b) {
                             return key_compare(a.w, b.w) == 0;
                           }) - keys.begin());
}

struct MergeScratch {  // merged array + look-back words + tile counter, pattern-filled
  DevBuf<KeyCount> merged;
  DevBuf<u64> status;
  DevBuf<u32> tile;
  explicit MergeScratch(u64 cap) : merged(cap), status(merge_scratch_words(cap)), tile(1) {
    merged.fill(kExchStagePattern);
    status.fill(kExchStagePattern);
    tile.fill(kExchStagePattern);
  }
  LookbackScratch lb() { return LookbackScratch{status.p, tile.p}; }
};

ExchStageCtr stage_ctr(const MapCounters& c) {
  ExchStageCtr o;
  o.num_records = c.num_records;
  o.num_unique = c.num_unique;
  o.total_count = c.total_count;
  return o;
}

}  // namespace

ExchStageMerge exch_stage_merge_slots(const std::vector<ExchStageMergeSlot>& slots,
                                      u32 slot_records) {
  const std::vector<KeyCount> img = slot_image(slots, slot_records);
  const u32 nslots = (u32)slots.size();
  const u64 cap = (u64)nslots * slot_records;
  // The count sum is "checked by the caller" (the emit's look-back value holds 40 bits of
  // it).  Summed over every record given, also those no run holds: whatever subset a merge
  // reads, its scan cannot carry into the record count it places the output by.
  u64 sum = 0;
  for (const ExchStageMergeSlot& sl : slots)
    for (const KeyCount& r : sl.records) {
      LOCUST_CHECK_ARG(r.count <= kMergeMaxCount && sum + r.count <= kMergeMaxCount,
                       "merge stage: count sum too large to merge");
      sum += r.count;
    }
  constexpr u64 kGuard = 128;  // output records behind the last one the merge may write
  DevBuf<KeyCount> d_slots(img.size());
  d_slots.upload(img.data(), img.size());
  MergeScratch scratch(cap);
  // (the emit sums whatever counts lie in `merged`: zeros, so that a slot the rank kernel
  // left unwritten is skipped like a duplicate and shows as a missing record)
  scratch.merged.fill(0);
  DevBuf<MapCounters> d_ctr(1), d_ctr_out(1);
  d_ctr.fill(kExchStagePattern);
  d_ctr_out.fill(kExchStagePattern);
  DevBuf<OutRecord> d_out(cap + kGuard);
  d_out.fill(kExchStagePattern);
  DevBuf<SlotHeader> d_hdr(nslots);
  d_hdr.fill(kExchStagePattern);
  launch_merge_slots(d_slots.p, nslots, slot_records, scratch.merged.p, d_ctr.p, d_out.p,
                     d_ctr_out.p, scratch.lb(), d_hdr.p, nullptr);
  sync();
  ExchStageMerge r;
  MapCounters c;
  d_ctr.download(&c, 1);
  r.ctr = stage_ctr(c);
  d_ctr_out.download(&c, 1);
  r.ctr_out = stage_ctr(c);
  r.headers.resize(nslots);
  d_hdr.download(r.headers.data(), nslots);
  std::vector<KeyCount> all(cap + kGuard);
  d_out.download(reinterpret_cast<OutRecord*>(all.data()), all.size());
  const u64 held = std::min<u64>(r.ctr.num_unique, cap);
  r.tail_intact = all_pattern(reinterpret_cast<const char*>(all.data() + held),
                              (all.size() - held) * sizeof(KeyCount));
  all.resize(held);
  r.out = std::move(all);
  return r;
}

ExchStageRank exch_stage_rank_slots(const std::vector<ExchStageMergeSlot>& slots,
                                    u32 slot_records) {
  const std::vector<KeyCount> img = slot_image(slots, slot_records);
  const u32 nslots = (u32)slots.size();
  const u64 cap = (u64)nslots * slot_records;
  DevBuf<KeyCount> d_slots(img.size());
  d_slots.upload(img.data(), img.size());
  MergeScratch scratch(cap);
  DevBuf<u64> d_acc(3 * kMergeAccSpread);
  d_acc.fill(0);
  launch_merge_rank_slots(d_slots.p, nslots, slot_records, scratch.merged.p, d_acc.p, scratch.lb(),
                          nullptr);
  sync();
  ExchStageRank r;
  r.merged.resize(cap);
  scratch.merged.download(r.merged.data(), cap);
  r.acc.resize(3 * kMergeAccSpread);
  d_acc.download(r.acc.data(), r.acc.size());
  return r;
}

std::vector<ExchStageEmit> exch_stage_emit_compact(const std::vector<ExchStageEmitJob>& jobs,
                                                   u32 slot_records, bool use_root_region,
                                                   u64 root_region, u64 region, u32 regions,
                                                   u64 region_records, u32 me,
                                                   u32 gather_records, u64 seq) {
  LOCUST_CHECK_ARG(jobs.size() >= 1 && jobs.size() <= 4, "merge stage: 1..4 jobs");
  const u32 P = (u32)jobs[0].msg3.size();
  LOCUST_CHECK_ARG(P >= 1 && P <= kExchMaxRanks, "exchange: bad shape");
  LOCUST_CHECK_ARG(me < P, "merge stage: this rank is not one of the P ranks");
  LOCUST_CHECK_ARG(regions <= 1024 && region_records <= kMergeMaxRecords,
                   "merge stage: output too large");
  std::vector<std::vector<KeyCount>> imgs;
  u64 cap = 0;
  for (const ExchStageEmitJob& j : jobs) {
    LOCUST_CHECK_ARG(j.msg3.size() == P, "merge stage: every job needs P reports");
    imgs.push_back(slot_image(j.slots, slot_records));
    cap = std::max<u64>(cap, (u64)j.slots.size() * slot_records);
    // an accepted emit writes the first copies behind the lower ranks' records and trusts
    // its own report for their number: it must cover them, or the range leaves its region
    LOCUST_CHECK_ARG(distinct_keys(imgs.back(), j.slots.size(), slot_records) <= j.msg3[me].n_out,
                     "merge stage: the report must cover the merged range");
  }
  // the guard: a region more and five words per merged slot -- an emit into region
  // `regions`, or of every slot, neither of which may happen, would still land in dst
  const u64 guard = (region_records + cap) * kOutWords + kExchStageEmitGuard;
  const u64 dst_words = (u64)regions * region_records * kOutWords + guard;
  const size_t J = jobs.size();
  std::vector<std::unique_ptr<DevBuf<KeyCount>>> d_slots;
  std::vector<std::unique_ptr<DevBuf<ExchMsg3>>> d_msg3;
  std::vector<std::unique_ptr<DevBuf<u64>>> d_dst, d_stamps, d_acc_snap;
  DevBuf<u32> d_done(1), d_done_snap(J);
  d_done.fill(0);
  d_done_snap.fill(kExchStagePattern);
  for (size_t j = 0; j < J; ++j) {
    d_slots.emplace_back(new DevBuf<KeyCount>(imgs[j].size()));
    d_slots.back()->upload(imgs[j].data(), imgs[j].size());
    d_msg3.emplace_back(new DevBuf<ExchMsg3>(P));
    d_msg3.back()->upload(jobs[j].msg3.data(), P);
    d_dst.emplace_back(new DevBuf<u64>(dst_words));
    d_dst.back()->fill(kExchStagePattern);
    d_stamps.emplace_back(new DevBuf<u64>(P));
    d_stamps.back()->fill(kExchStagePattern);
    d_acc_snap.emplace_back(new DevBuf<u64>(3 * kMergeAccSpread));
  }
  ExchMsg1 root{};
  root.out_region = root_region;
  DevBuf<ExchMsg1> d_root(1);
  d_root.upload(&root, 1);
  MergeScratch scratch(cap);
  DevBuf<u64> d_acc(3 * kMergeAccSpread);
  for (size_t j = 0; j < J; ++j) {
    const u32 nslots = (u32)jobs[j].slots.size();
    LOCUST_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, 3 * kMergeAccSpread * sizeof(u64), nullptr));
    launch_merge_rank_slots(d_slots[j]->p, nslots, slot_records, scratch.merged.p, d_acc.p,
                            scratch.lb(), nullptr);
    launch_merge_emit_compact(d_slots[j]->p, nslots, slot_records, scratch.merged.p, d_msg3[j]->p,
                              use_root_region ? d_root.p : nullptr, region, regions,
                              region_records, P, me, gather_records, d_dst[j]->p, d_stamps[j]->p,
                              seq + j, d_done.p, scratch.lb(), nullptr);
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_done_snap.p + j, d_done.p, sizeof(u32),
                                    hipMemcpyDeviceToDevice, nullptr));
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_acc_snap[j]->p, d_acc.p, 3 * kMergeAccSpread * sizeof(u64),
                                    hipMemcpyDeviceToDevice, nullptr));
  }
  sync();
  std::vector<u32> done(J);
  d_done_snap.download(done.data(), J);
  std::vector<ExchStageEmit> out(J);
  for (size_t j = 0; j < J; ++j) {
    out[j].dst.resize(dst_words);
    d_dst[j]->download(out[j].dst.data(), dst_words);
    out[j].stamps.resize(P);
    d_stamps[j]->download(out[j].stamps.data(), P);
    out[j].done = done[j];
    out[j].acc.resize(3 * kMergeAccSpread);
    d_acc_snap[j]->download(out[j].acc.data(), out[j].acc.size());
  }
  return out;
}

}  // namespace locust
