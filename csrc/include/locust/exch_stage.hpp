// Stage-level entry points of the device-resident shuffle (locust/exch.hpp): each runs ONE
// launch_* of exchange.hip / shuffle.hip / merge.hip alone on host-made input -- plain
// device buffers, upload, launch, synchronise, download everything the kernel wrote -- so a test can compare
// a single kernel with a reference of the same step (tests/test_exchange_kernels.py), like
// GpuWordCount::sort_keys / reduce_sorted / merge_runs do for theirs.  They do not go
// through ShardEngine.  No HIP dependency in this header.
#pragma once

#include <vector>

#include "locust/common.hpp"
#include "locust/exch.hpp"
#include "locust/kv.hpp"
#include "locust/slot.hpp"

namespace locust {

// Byte the stage entry points fill an output buffer with before the launch: what a kernel
// did not write still holds it afterwards.
constexpr unsigned char kExchStagePattern = 0xA5;

// One all-to-all slot of the send buffer after launch_exch_pack.
struct ExchStageSlot {
  SlotHeader header;              // as written by the kernel (pattern bytes if it was not)
  std::vector<KeyCount> records;  // the first min(header.n, slot_records) records of the slot
  u64 dirty_records = 0;          // 1 + the last record of the record area that no longer
                                  // holds the pattern (0: the whole area is untouched)
  bool tail_intact = false;       // the area behind min(header.n, slot_records) records is
};
struct ExchStagePlan {
  ExchCtl ctl;                    // written by launch_exch_plan (or given, exch_stage_pack)
  std::vector<ExchStageSlot> slots;
};

// launch_exch_plan + launch_exch_pack.  The P messages are free-standing: status[r],
// n_local[r] and samples[r * S .. r * S + S) of rank r; `records` are this rank's sorted
// (key, count) records; pack_cap is launch_exch_pack's grid bound (0: the record count).
ExchStagePlan exch_stage_plan_pack(u32 P, u32 S, const std::vector<i32>& status,
                                   const std::vector<u64>& n_local,
                                   const std::vector<PackedKey>& samples,
                                   const std::vector<KeyCount>& records, u32 slot_records,
                                   u64 pack_cap = 0);
// launch_exch_pack alone behind a given ExchCtl (off[0..P], flags).
ExchStagePlan exch_stage_pack(const ExchCtl& ctl, u32 P, const std::vector<KeyCount>& records,
                              u32 slot_records, u64 pack_cap = 0);

// launch_sample_keys(sorted, n, S) -> S keys.
std::vector<PackedKey> exch_stage_sample(const std::vector<PackedKey>& sorted, u32 S);

// The MapCounters fields launch_exch_header reads.  (kernels.hpp, which names the flag
// bits, needs the HIP headers: exch_stage_dict_overflow_flag() is its kCtrDictOverflow.)
u32 exch_stage_dict_overflow_flag();
struct ExchStageCounters {
  u32 flags = 0, num_unique = 0, num_records = 0, map_tokens = 0, overflow_lines = 0,
      truncated = 0, max_key_len = 0;
};
struct ExchStageHeader {
  ExchMsg1 msg;                    // as written
  std::vector<PackedKey> samples;  // the S samples behind it
  bool tail_intact = false;        // `guard` PackedKeys behind the samples still hold the pattern
};
ExchStageHeader exch_stage_header(const ExchStageCounters& ctr, const ExchMsg1& tmpl,
                                  bool combined, const std::vector<PackedKey>& sorted, u32 S,
                                  u32 guard = 4);

// launch_bucket_offsets(sorted, n, splitters, P) -> P + 1 offsets (splitters: P - 1 keys).
std::vector<u64> exch_stage_offsets(const std::vector<PackedKey>& sorted,
                                    const std::vector<PackedKey>& splitters, u32 P);

// launch_pack_records, then launch_unpack_records of what it wrote with the partition map
// `lo` (kDictParts + 1 range starts; empty: the default first-byte map).  `counts` may be
// null (every record then counts 1).
struct ExchStageRoundTrip {
  std::vector<KeyCount> packed;  // after launch_pack_records
  std::vector<PackedKey> keys;   // after launch_unpack_records
  std::vector<u64> counts;
  std::vector<u8> parts;
};
ExchStageRoundTrip exch_stage_roundtrip(const std::vector<PackedKey>& keys,
                                        const std::vector<u64>* counts,
                                        const std::vector<u64>& lo);

// launch_exch_report over P received slot headers, an ExchCtl and the kMergeAccSpread
// (firsts, tokens, words) accumulator triples (acc: 3 * kMergeAccSpread values).
struct ExchStageReport {
  ExchMsg3 msg;
  std::vector<u64> acc;  // the accumulators after the launch
};
ExchStageReport exch_stage_report(const std::vector<SlotHeader>& headers, u32 slot_records,
                                  const ExchCtl& ctl, const std::vector<u64>& acc,
                                  u32 gather_records);

// ---- the shuffle tail (merge.hip) over the slot layout ----
// One input slot: its header as given and the records that follow it.  The slot's record
// area holds `records` (at most slot_records, at least the min(header.n, slot_records) the
// header announces, whatever its status) and pattern bytes behind them, so whatever a
// kernel reads past them is visibly junk.
struct ExchStageMergeSlot {
  SlotHeader header;
  std::vector<KeyCount> records;
};
struct ExchStageCtr {  // the MapCounters fields the merge's emit writes
  u32 num_records = 0, num_unique = 0;
  u64 total_count = 0;
};

// launch_merge_slots with a device hdr_out.  `out`: the first min(num_unique, nslots *
// slot_records) output records (40-B OutRecords: key words + count).  Refused before any
// launch: more than kMaxSlotRanks slots, nslots * slot_records > kMergeMaxRecords, a count
// sum above kMergeMaxCount (over every record given, also those of failed slots and behind
// n: whatever a merge reads, its 40-bit count scan cannot overflow).
struct ExchStageMerge {
  std::vector<KeyCount> out;
  ExchStageCtr ctr, ctr_out;        // device counters / their host copy (ctr_out)
  std::vector<SlotHeader> headers;  // hdr_out
  bool tail_intact = false;         // the output behind `out` (and a guard) is untouched
};
ExchStageMerge exch_stage_merge_slots(const std::vector<ExchStageMergeSlot>& slots,
                                      u32 slot_records);

// launch_merge_rank_slots with zeroed accumulators: the whole `merged` array (nslots *
// slot_records records, pattern where unwritten) and the 3 * kMergeAccSpread accumulators.
struct ExchStageRank {
  std::vector<KeyCount> merged;
  std::vector<u64> acc;
};
ExchStageRank exch_stage_rank_slots(const std::vector<ExchStageMergeSlot>& slots,
                                    u32 slot_records);

// launch_merge_rank_slots + launch_merge_emit_compact, once per job, the jobs back to back
// on one stream and on the same scratch (look-back words, tile counter, done counter,
// merged array: pattern-filled once, except `done`, which starts at 0) with no host-side
// reset between them, job j stamping seq + j.  P = msg3.size().  Each job has a
// pattern-filled dst of regions * region_records * kOutWords words + a guard (a region
// more, kOutWords words per merged slot and kExchStageEmitGuard words) and P pattern-filled
// stamps of its own.  The accumulators are zeroed before each job (in a job that is
// launch_exch_report's part).  root_region (when use_root_region) goes into an ExchMsg1
// handed to the kernel as root_msg in place of `region`.
// Refused before any launch, besides the slot checks above (not the count sum): P = 0 or
// P > kExchMaxRanks, me >= P, and a report msg3[me].n_out below the distinct keys of the
// job's effective runs (the kernel trusts it for the room its records take).
struct ExchStageEmitJob {
  std::vector<ExchStageMergeSlot> slots;
  std::vector<ExchMsg3> msg3;
};
struct ExchStageEmit {
  std::vector<u64> dst;     // with the guard
  std::vector<u64> stamps;  // P
  u32 done = 0;             // the done counter behind this job
  std::vector<u64> acc;     // the job's accumulators
};
constexpr u32 kExchStageEmitGuard = 64;
std::vector<ExchStageEmit> exch_stage_emit_compact(const std::vector<ExchStageEmitJob>& jobs,
                                                   u32 slot_records, bool use_root_region,
                                                   u64 root_region, u64 region, u32 regions,
                                                   u64 region_records, u32 me,
                                                   u32 gather_records, u64 seq);

}  // namespace locust
