// Stage-level entry points of the dictionary fallback kernels (dict.hip: dict_insert,
// dict_part_build, rank_sort, rank_emit, rank_scatter, scan_pack) and of the in-job
// partition plan (partplan.hip): each runs ONE launch_* alone on host-made input -- plain
// device buffers of its own, every output filled with a pattern byte, upload, launch on the
// null stream, synchronise, download everything the kernel may have written plus a guard
// area behind it -- so a test can compare a single kernel with a reference of the same step
// (tests/test_dict_stage_kernels.py).  None of them goes through DevicePipeline.  No HIP
// dependency in this header.
//
// What each leaves to the caller:
//   insert      the table, ucount, num_unique and flags start zeroed, as the kernel's
//               contract asks; the caller chooses d_n apart from the keys it uploads (the
//               kernel clamps it to cap), the table size and ucap, and reads an overflow
//               from `flags` itself.  The dense ids come from atomics: their order is not
//               defined, only the set of (key, count) pairs is.
//   part_build  the caller tags every key (parts); a tagging that gives one key two tags
//               makes two dense entries of it, which is the kernel's contract, not an error.
//   rank        rank / val start zeroed (the kernel accumulates); keys need not be distinct
//               (equal keys get equal ranks).
//   emit        rank / val are the caller's: the entry point only refuses ranks that would
//               leave the output (not a permutation); a wrong val shows in total_count.
//   scatter     as emit.
//   scan_pack   `sorted` is taken as given (the kernel does not compare keys); look-back
//               words and the tile counter start zeroed.
//   part_plan   w0 / counts in any order; the result is the 257 range starts, not checked.
// Every size a kernel indexes by is checked before the launch (LOCUST_CHECK_ARG), so no
// launch can leave its buffers: see the refusals listed at each entry point.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "locust/common.hpp"
#include "locust/kv.hpp"

namespace locust {

// Byte the stage entry points fill an output buffer with before the launch: what a kernel
// did not write still holds it afterwards.
constexpr unsigned char kDictStagePattern = 0xA5;
// Entries behind every output array (and behind the uploaded tokens) that no launch may
// touch; they are downloaded and compared with the pattern.
constexpr u32 kDictStageGuard = 64;

// A valid packed key: its bytes, then NUL padding only -- no non-zero byte (so no non-zero
// word) after a zero byte.  Word 0 may be 0: the empty record the kernels skip.  Only a
// valid key can never hold a word equal to kWordMagic, which a claimer's spin relies on.
bool dict_stage_valid_key(const u64* w);

// Kernel constants by name (dict_consts.hpp, kernels.hpp), for the bindings.
std::vector<std::pair<std::string, u64>> dict_stage_constants();

// The MapCounters fields, for the entry points that take or return whole counters.
struct DictStageCounters {
  u32 num_records = 0, map_tokens = 0, num_unique = 0, overflow_lines = 0, truncated = 0,
      num_newlines = 0, max_key_len = 0, flags = 0;
  u64 total_count = 0;
};

struct DictStageSlot {  // an occupied slot of the HBM table
  u32 slot = 0, id = 0;  // id as stored: dense id + 1, or kIdFull
  PackedKey key;         // words 1..3 with kWordMagic taken off again
};
struct DictStageDense {
  u32 num_unique = 0, flags = 0;
  std::vector<PackedKey> keys;  // dense entries [0, min(num_unique, ucap))
  std::vector<u64> counts;
  std::vector<u64> uval;        // part_build only: of the same entries
  std::vector<u32> urank;
  // everything behind those entries is untouched: ukeys (and part_build's ucount, uval,
  // urank) hold the pattern up to ucap + kDictStageGuard; insert's ucount is still zero up
  // to ucap and pattern in the guard
  bool tail_intact = false;
  std::vector<DictStageSlot> table;  // insert only, in slot order
};

// launch_dict_insert.  cap bounds the grid and clamps *d_n; max_blocks as the launcher's.
// Refused: an invalid key, counts of another length than keys, table_slots not a power of
// two (or 0), min(d_n, cap) keys not uploaded, d_n past the guard behind the uploaded keys.
DictStageDense dict_stage_insert(const std::vector<PackedKey>& keys,
                                 const std::vector<u64>* counts, u32 d_n, u64 cap,
                                 u64 table_slots, u32 ucap, u32 max_blocks = 1024);

// launch_dict_part_build.  parts: one tag per key; the device copy is readable to
// align_up(n, 16) + 16 with pattern bytes behind the tags.  Refused: an invalid key, counts
// or parts of another length than keys, min(d_n, cap) keys not uploaded, d_n past the guard.
DictStageDense dict_stage_part_build(const std::vector<PackedKey>& keys,
                                     const std::vector<u64>* counts, const std::vector<u8>& parts,
                                     u32 d_n, u64 cap, u32 ucap);

// launch_rank_sort on zeroed rank / val: both whole arrays (cap entries; val stays zero
// without counts).  Refused: an invalid key, cap keys not uploaded.
struct DictStageRank {
  std::vector<u32> rank;
  std::vector<u64> val;
  bool tail_intact = false;  // the guard behind both arrays
};
DictStageRank dict_stage_rank(const std::vector<PackedKey>& keys, const std::vector<u64>* counts,
                              u32 d_u, u64 cap);

// launch_rank_emit with a device ctr_out (pattern-filled before).  Refused: an invalid key,
// arrays of other lengths than keys, cap keys not uploaded, and -- when u = min(num_unique,
// cap) <= kRankSortMax -- rank[0, u) that is not a permutation of [0, u).
struct DictStageEmit {
  std::vector<KeyCount> records;  // [0, min(num_unique, cap)) of the output
  DictStageCounters ctr_out;
  bool tail_intact = false;  // the output behind the records, guard included
  bool untouched = false;    // the whole output still holds the pattern
};
DictStageEmit dict_stage_emit(const std::vector<PackedKey>& keys, const std::vector<u64>& counts,
                              const std::vector<u32>& rank, const std::vector<u64>& val,
                              const DictStageCounters& ctr, u64 cap);

// launch_rank_scatter: the whole sorted arrays (cap entries, pattern where unwritten).
// Refusals as dict_stage_emit's, with u = min(d_u, cap).
struct DictStageScatter {
  std::vector<PackedKey> sorted;
  std::vector<u64> counts;
  bool tail_intact = false;  // the guard behind both
};
DictStageScatter dict_stage_scatter(const std::vector<PackedKey>& keys,
                                    const std::vector<u64>& counts, const std::vector<u32>& rank,
                                    u32 d_u, u64 cap);

// launch_scan_pack on zeroed look-back words and tile counter.  ctr.num_unique is the
// record count; ctr.total_count is replaced by pattern bytes before the launch, so
// `total_count` shows whether the kernel wrote it.  Refused: an invalid key, counts of
// another length, a count sum of 2^62 or more (the look-back word carries 62 value bits),
// num_unique > cap, cap keys not uploaded.
struct DictStageScanPack {
  std::vector<KeyCount> records;  // [0, num_unique)
  u64 total_count = 0;            // ctr->total_count after the launch
  DictStageCounters ctr_out;      // pattern fields when with_ctr_out is false
  bool tail_intact = false;
  bool untouched = false;
};
DictStageScanPack dict_stage_scan_pack(const std::vector<PackedKey>& sorted,
                                       const std::vector<u64>& counts,
                                       const DictStageCounters& ctr, u64 cap, u32 emit_limit,
                                       bool with_ctr_out);

// launch_part_plan: the kDictParts + 1 range starts.  Refused: counts of another length than
// w0, ucap entries not uploaded.
std::vector<u64> dict_stage_part_plan(const std::vector<u64>& w0, const std::vector<u64>& counts,
                                      u32 d_u, u32 ucap);

}  // namespace locust
