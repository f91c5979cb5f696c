// Host-side launchers for the HIP/CDNA4 kernels.  Every launcher only enqueues work on
// the given stream (no allocation, no synchronisation), so whole pipelines can be
// captured into a hipGraph.  Element counts that are produced on the device (token
// count, unique count) are passed as device pointers and kernels early-exit past them;
// host-side `cap` arguments only bound the grid.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "locust/common.hpp"
#include "locust/config.hpp"
#include "locust/dstring.hpp"
#include "locust/engine.hpp"
#include "locust/exch.hpp"
#include "locust/kv.hpp"
#include "locust/partmap.hpp"
#include "locust/slot.hpp"

namespace locust {

// Packed keys, structure-of-arrays: w[j][i] is word j of key i.
struct KeysSoA {
  u64* w[kKeyWords];
};
struct ConstKeysSoA {
  const u64* w[kKeyWords];
  ConstKeysSoA() = default;
  ConstKeysSoA(const KeysSoA& k) {  // NOLINT: implicit by design
    for (int j = 0; j < kKeyWords; ++j) w[j] = k.w[j];
  }
};

// Device-side counters written by the pipeline stages.
struct alignas(8) MapCounters {
  u32 num_records;      // records to sort: emitted tokens (kv_num_map) or received records
  // tokens a combining map emitted (num_records counts its records); shares one 64-bit
  // word with num_records, so a combining tile updates both with a single atomic
  u32 map_tokens;
  u32 num_unique;       // kv_num_reduce
  u32 overflow_lines;   // lines that had more than emits_per_line tokens (WARN lines)
  u32 truncated;        // tokens longer than max_key_len (truncated)
  u32 num_newlines;     // line index size
  u32 max_key_len;      // longest token seen (before truncation)
  u64 total_count;      // sum of record counts (== num_records when every count is 1)
  u32 flags;            // kCtr* status bits
  u32 pad;
};
static_assert(offsetof(MapCounters, map_tokens) == 4, "num_records + map_tokens: one u64");
constexpr u32 kCtrDictOverflow = 1u;  // dictionary table full: rerun on the radix path
constexpr u32 kCtrSortOverflow = 2u;  // a psort partition held more than kPsortMax tokens
constexpr u32 kCtrNotEmitted = 0x80000000u;  // rank_emit skipped (too many distinct keys)

// Look-back scratch: a zeroed region of 64-bit status words plus a tile counter.
struct LookbackScratch {
  u64* status;
  u32* tile_counter;
};

// ---------------- map.hip ----------------
constexpr int kMapBlock = 256;
// Tile bytes = 4 waves x steps x 64 B.  Small inputs: 1 KiB tiles (run as 16 waves x one
// 64-B step, launch_map_fast: more workgroups in flight; 768-B tiles measured neutral,
// profiles/r6/map/tile768_ab.txt), large inputs 16 steps (4 KiB tiles: fewer overlaps).
constexpr int kMapSegStepsSmall = 4;
constexpr int kMapSegStepsLarge = 16;
constexpr int kMapTileBytesMin = (kMapBlock / 64) * kMapSegStepsSmall * 64;
constexpr u64 kMapLargeInput = 8ull << 20;  // switch to large tiles above 8 MiB
constexpr int kLineIdxBlock = 256;
constexpr int kLineIdxItems = 16;                             // bytes per thread
constexpr int kLineIdxTile = kLineIdxBlock * kLineIdxItems;

// Newline positions (stable order) -> nl_pos[0..num_newlines).  `text` has `bytes` bytes.
void launch_line_index(const char* text, u64 bytes, u64* nl_pos, MapCounters* ctr,
                       LookbackScratch lb, hipStream_t s);

// Reference-layout map: one thread per line runs device strtok_r in place over `text`
// (which must have a writable NUL byte at text[bytes]) and writes up to E tokens into
// slots [line*E + k]; line_counts[line] = number of emitted tokens.
void launch_map_compat(char* text, u64 bytes, const u64* nl_pos, u32 num_lines,
                       const char* d_delims, int emits_per_line, int max_key_len,
                       KeysSoA slots, u32* line_counts, MapCounters* ctr, hipStream_t s);

// Stable compaction of the fixed slots into a dense key array (Process step 1).
void launch_compact_slots(const u32* line_counts, u32 num_lines, int emits_per_line,
                          ConstKeysSoA slots, KeysSoA out, MapCounters* ctr,
                          LookbackScratch lb, hipStream_t s);

// ---------------- partition map: see locust/partmap.hpp ----------------
struct PartMap {                 // device view of a PartMapTables image
  const u64* lo = nullptr;       // [kDictParts + 1] range starts; null: first key byte
};
__device__ __forceinline__ u32 part_of(const PartMap& pm, u64 w0) {
  return pm.lo ? part_of_w0(pm.lo, w0) : (u32)(w0 >> 56);
}

// Byte-parallel tokenizer: tokens compacted in text order straight into `out`.
// trace (diagnostics, optional): per tile < 4096, s_memrealtime stamps at trace[t*8+0..5].
// part_off (optional): the tokens of each tile (map_tile_bytes(bytes): 1 KiB below
// kMapLargeInput, else 4 KiB) are written grouped by PartMap partition and
// part_off[t * kPartTable + p] is the absolute index of tile t's first partition-p token
// ([.. + kPartTable - 1] = the tile's end), so a partition's tokens are found without
// scanning every token's tag.
// counts (optional, 4 KiB tiles with part_off): per-tile combining -- in every tile, the
// first one-word key (<= 7 bytes) of each partition and all its repeats become ONE record
// at the head of the partition's run, with counts[i] = its multiplicity (1 for the other
// records); num_records then counts records, not tokens.  Zipfian text loses most of its
// hot-key volume before it is ever written.
constexpr int kPartTable = 257;
constexpr int kMapTileBytesLarge = (kMapBlock / 64) * kMapSegStepsLarge * 64;
inline u64 map_tile_bytes(u64 bytes) {
  return bytes < kMapLargeInput ? (u64)kMapTileBytesMin : (u64)kMapTileBytesLarge;
}
// part_occ (optional, small 1 KiB tiles with part_off): per tile, kPartOccWords words of a
// 256-bit mask of its non-empty partitions (OrderedExtra::part_occ).
constexpr int kPartOccWords = kDictParts / 32;
void launch_map_fast(const char* text, u64 bytes, const DelimMask& dm, int emits_per_line,
                     int max_key_len, KeysSoA out, u8* parts, u64 out_cap, MapCounters* ctr,
                     LookbackScratch lb, hipStream_t s, u64* trace = nullptr,
                     u32* part_off = nullptr, PartMap pm = PartMap{}, bool large_tiles = false,
                     u64* counts = nullptr, u32* part_occ = nullptr, u32* plan_flag = nullptr,
                     int ngram = 1);
// The same map with one record per word n-gram of a line (ngram in [2, kMaxNgram]; what
// launch_map_fast dispatches to, ngram.hip): the words joined by single 0x20 bytes, never
// across a line end or a NUL, the key the first max_key_len bytes of the joined words.
// Output contract and arguments as launch_map_fast.
void launch_map_ngram(int ngram, const char* text, u64 bytes, const DelimMask& dm,
                      int emits_per_line, int max_key_len, KeysSoA out, u8* parts, u64 out_cap,
                      MapCounters* ctr, hipStream_t s, u64* trace, u32* part_off, PartMap pm,
                      bool large_tiles, u64* counts, u32* part_occ, u32* plan_flag);

// ---------------- radix_sort.hip ----------------
constexpr int kSortBlock = 256;
constexpr int kSortItems = 16;
constexpr int kSortTile = kSortBlock * kSortItems;  // 4096 keys per tile
constexpr int kNumPositions = kKeyBytes;            // one 8-bit digit per key byte

constexpr int kSmallSortMax = 8192;                  // single-workgroup LDS sort up to here
constexpr u64 kUnknownCount = ~0ull;                 // "n only known on the device"

struct SortPassInfo {
  u32 active;      // digit position not constant -> needs a pass
  u32 src;         // reserved
};
struct SortPlan {
  u32 n;
  u32 pad[3];
  SortPassInfo pass[kNumPositions];           // indexed by key byte position
  u32 digit_offset[kNumPositions][256];       // exclusive scan of the digit histogram
};

struct RadixWorkspace {
  u32* hist_part;      // [radix_hist_blocks(cap)][kNumPositions * 256] partial histograms
  SortPlan* plan;      // device plan
  u64* keys[2];        // ping-pong key words
  u32* vals[2];        // ping-pong permutation
  u32* tile_counters;  // [kNumPositions], followed immediately by `status`
  u32* status;         // per-pass look-back status [tiles][256]: [31:30] flag, [29:0] count
  u64 cap;             // max keys
};

u64 radix_status_words(u64 cap);  // u32 status words needed for one pass
u32 radix_hist_blocks(u64 cap);   // histogram blocks (partials) for `cap` keys
u64 radix_zero_bytes(u64 cap);    // bytes of tile_counters + status zeroed per sort

// Sorts the *d_n packed keys (SoA) into `sorted` (+ optional counts permuted alongside,
// + optional permutation).  host_n: the count if the host knows it (then n <= 8192 runs
// the single-workgroup LDS sort, larger n reads the plan back and launches only live
// passes with exact grids), or kUnknownCount (graph mode: every kernel is launched and
// the ones not needed early-exit on the device-side count / plan).
// skip_upto: in graph mode, every kernel also exits when *d_n <= skip_upto (another sort
// handles that range; 0 = none).
void radix_sort(ConstKeysSoA keys, const u32* d_n, u64 host_n, RadixWorkspace& ws,
                const u64* counts_in, KeysSoA sorted, u64* counts_out, u32* perm_out,
                SortPlan* h_plan, hipStream_t s, u32 skip_upto = 0);

// ---------------- psort.hip ----------------
// Partitioned LDS radix sort of the tokens of a small-input fast map (part_off = its
// per-tile partition table over `ntiles` tiles, launch_map_fast): workgroup p sorts the
// tokens of PartMap partition p in LDS and writes them at their global sorted position.
// The map's counters must still be in `ctr` (num_records); a partition with more than
// kPsortMax tokens sets kCtrSortOverflow (then `sorted` is incomplete).  part_w
// (optional, host-mapped): per-partition work (tokens + kPartDistinctWeight x distinct
// first words), for the partition map's retuning.
constexpr int kPsortMax = 5120;
// trace (diagnostics, optional): per partition p, stamps at trace[p*16 + k] (see psort.hip).
void launch_psort(ConstKeysSoA tokens, const u32* part_off, u32 ntiles, u64 cap, KeysSoA sorted,
                  MapCounters* ctr, u32* part_w, hipStream_t s, u64* trace = nullptr);

// ---------------- reduce.hip ----------------
constexpr int kReduceBlock = 256;
constexpr int kReduceItems = 8;
constexpr int kReduceTile = kReduceBlock * kReduceItems;

// Exclusive scan of u64 record counts in sorted order (weighted reduce: combined or
// shuffled records carry counts > 1).  Writes ctr->total_count.
void launch_scan_counts(const u64* counts, u64 cap, u64* prefix, MapCounters* ctr,
                        LookbackScratch lb, hipStream_t s);

// Reduce steps 1+2: segment-head marking (key[i] != key[i-1]) fused with the stable
// compaction of heads.  head_val[j] = start of run j in token units: i itself when
// `prefix` is null (every count 1: the reference's kernFindUniqBool value), else prefix[i].
// Writes ctr->num_unique (and ctr->total_count when prefix is null).
void launch_mark_compact_heads(ConstKeysSoA sorted, const u64* prefix, u64 cap, ReducePath path,
                               KeysSoA head_keys, u64* head_val, MapCounters* ctr,
                               LookbackScratch lb, hipStream_t s);
// Reduce step 3 (kernGetCount): count[j] = val[j+1] - val[j]; last = total - val[last].
void launch_adjacent_diff(const u64* head_val, u64 cap, ReducePath path, u64* head_count,
                          const MapCounters* ctr, hipStream_t s);
// val[j] += *offset (global start index of this rank's key range).
void launch_add_offset(u64* head_val, u64 cap, const u64* d_offset, const MapCounters* ctr,
                       hipStream_t s);

// Output records for the host: {packed key, count}, 40 B (KeyCount's layout).  The
// reference's val (start of the key's run in the sorted token order) is the exclusive
// prefix of the counts and is rebuilt on the host (EntryVals, engine.hpp) instead of
// crossing PCIe with every record (round 2 wrote 48-B {key, val, count} records).
struct OutRecord {
  u64 w[kKeyWords];
  u64 count;
};
static_assert(sizeof(OutRecord) == 40, "OutRecord 40 B");
constexpr u32 kOutWords = sizeof(OutRecord) / 8;  // 5 u64 words per record
// Unweighted reduce steps 1-3 + output records in one kernel (LDS-staged tiles): `out`
// (room for out_cap records; host-mapped allowed) receives {key, count} in key order,
// ctr->num_unique / total_count are set and ctr_out (optional, host-mapped) gets a
// snapshot.  `lb` needs div_up(cap, kReduceTile) + 1 zeroed status words and a zeroed
// tile counter.
void launch_reduce_fused(ConstKeysSoA sorted, u64 cap, MapCounters* ctr, OutRecord* out,
                         u64 out_cap, MapCounters* ctr_out, LookbackScratch lb, hipStream_t s);
// Process + Reduce of the reference algorithm in ONE kernel (psort.hip): the partitioned
// LDS sort above, then inside each partition's workgroup the head mark (key[i] !=
// key[i-1]; runs never cross partitions, which are key ranges), counts as distances to the
// next head, the record index from a look-back over the
// partitions' head counts -- and the records straight into `out` (host-mapped allowed).
// The sorted token array is never written.  Self-cleaning like the ordered dictionary
// kernel: `status` (kDictParts look-back words) and `done_counter` must be zero before and
// are left zero; the last workgroup to finish re-zeroes the map's look-back words
// (map_lb, map_words) and counters, writes the ctr_out snapshot and, if given, publishes
// host_done_value to host_done (the lean job's completion word).  A partition past
// kPsortMax tokens sets kCtrSortOverflow: no records, nothing re-zeroed, the host redoes
// the pass with the device-wide sort.
struct PsortReduceArgs {
  OutRecord* out = nullptr;
  u64 out_cap = 0;
  MapCounters* ctr_out = nullptr;
  u64* status = nullptr;
  u32* done_counter = nullptr;
  LookbackScratch map_lb{};
  u32 map_words = 0;
  u32* host_done = nullptr;
  u32 host_done_value = 0;
};
void launch_psort_reduce(ConstKeysSoA tokens, const u32* part_off, u32 ntiles, u64 cap,
                         MapCounters* ctr, u32* part_w, const PsortReduceArgs& ra, hipStream_t s,
                         u64* trace = nullptr);
// ctr_out (optional, host-mapped): a snapshot of the final counters.
void launch_pack_output(ConstKeysSoA head_keys, const u64* head_val, const u64* head_count,
                        u64 cap, const MapCounters* ctr, OutRecord* out, hipStream_t s,
                        MapCounters* ctr_out = nullptr);

// ---------------- dict.hip ----------------
constexpr int kRankSortMax = 32768;  // all-pairs rank sort up to here, radix above

struct DictSlot {  // one hash-table slot (40 B): key words 1..3 stored XOR a magic value
  u64 w[kKeyWords];
  u32 id;          // dense id + 1 (0 = not yet published)
  u32 pad;
};
struct DictWorkspace {
  DictSlot* table;  // power-of-two slots, zeroed per run
  u32 mask;         // slots - 1 (this run)
  KeysSoA ukeys;    // dense distinct keys (ids from ctr->num_unique)
  u64* ucount;      // per-id occurrence counts, zeroed per run
  u64* uval;        // per-id weighted rank (= output val), zeroed per run
  u32 ucap;         // capacity of ukeys/ucount/uval: a key that would get id >= ucap sets
                    // kCtrDictOverflow (num_unique may then exceed ucap; consumers clamp)
  u32* urank;       // per-id rank (rank sort output), zeroed per run
};
// Partitioned build (small inputs): every token carries its partition (parts[i], the first
// byte of its key, written by the map kernel or by unpack_records); workgroup p aggregates
// partition p in LDS and appends its distinct keys to ukeys/ucount (and zeroes uval/urank).
// No table and no reset needed.  parts must be readable up to align_up(n, 16).
constexpr u64 kPartBuildMaxTokens = 1ull << 18;  // beyond: the HBM-table insert scales better
void launch_dict_part_build(ConstKeysSoA tokens, const u64* counts, const u8* parts,
                            const u32* d_n, u64 cap, const DictWorkspace& dw, MapCounters* ctr,
                            hipStream_t s);
// Ordered build (partitions = PartMap ranges, default the first key byte): aggregation,
// per-partition LDS sort,
// look-back offsets and the final (key, count) records in ONE kernel.  `out` needs
// room for every distinct key; `lb` needs kDictParts + 1 zeroed status words and a zeroed
// tile counter.  Sets ctr->num_unique / total_count (and ctr_out, if given, like the
// emit kernels); a partition past kPartSlots distinct keys sets kCtrDictOverflow.
// `trace` (diagnostics, optional): per partition p, s_memtime stamps at trace[p*16 + k]:
// 0 start, 1 built, 2 published, 8 histogram, 7 bucketed, 9 ranked, 3 sorted, 4 prefix
// known, 5 written; the key count at [p*16+6].
// Optional extra outputs of the ordered build (the distributed map): the sorted distinct
// keys as KeyCount records and/or SoA keys + counts, and the gather slot's header (`tmpl`
// completed on the device by the last partition).  `out` may then be null.
struct OrderedExtra {
  KeyCount* recs = nullptr;
  KeysSoA sorted{};
  u64* counts = nullptr;
  SlotHeader* hdr = nullptr;
  SlotHeader tmpl{};
  // Self-cleaning job: unless a partition overflowed, the last workgroup to finish
  // re-zeroes the accumulated counters of `ctr` (num_unique / total_count keep this run's
  // values), this kernel's look-back scratch and the map's (`map_lb`, map_words status
  // words), so the next job needs no memset in front.
  bool self_clean = false;
  LookbackScratch map_lb{};
  u32 map_words = 0;
  u32* done_counter = nullptr;  // zeroed counter of finished workgroups (self_clean)
  // With self_clean (optional, host-mapped): the last workgroup publishes host_done_value
  // here once every workgroup's writes are visible system-wide -- the lean job's completion
  // word without a kernel of its own behind this one.
  u32* host_done = nullptr;
  u32 host_done_value = 0;
  // Tokens from the small-input fast map with its per-tile partition table (launch_map_fast
  // part_off): partitions read their token ranges from it instead of scanning the tags.
  const u32* part_off = nullptr;
  u32 part_tiles = 0;
  // With part_off and part_occ (the map's per-tile occupancy masks): plan the workgroups
  // inside the job from THIS job's map statistics.  Every workgroup ORs the occupancy
  // masks (which partitions are non-empty: exact), estimates the partitions' token counts
  // from the same evenly spaced rows of the per-tile table, deals the kDictParts
  // workgroups out over the non-empty partitions in proportion to them, and a partition
  // with K > 1 workgroups is cut into K key ranges at quantiles of a sample of its own
  // tokens (every sibling draws the same sample): virtual partitions in key order, one
  // look-back over all of them.  A first-letter partition map on English text leaves ~200
  // of 256 workgroups idle and puts 's'/'t' on the critical path without it.  (Inputs of
  // at most kPartBlock tiles; larger ones keep one workgroup per partition.)
  const u32* part_occ = nullptr;
  // With part_occ (optional, zeroed device word): the map sets it when a tile holds
  // kPlanTrigger tokens of one partition; the ordered kernel plans only then (otherwise
  // one workgroup per map partition, without the plan's loads), and the self-clean
  // re-zeroes it.  Null: plan every pass.
  u32* plan_flag = nullptr;
  u32 split_min = 0;            // planned workgroups: tokens per extra sibling (0: default)
  // The partition map the tokens' partitions were computed with (default: first byte).
  PartMap pm{};
  // Optional (host-mapped): part_w[p] = partition p's work (tokens + kPartDistinctWeight x
  // distinct keys), written every run; the host retunes `pm` when it is unbalanced.
  u32* part_w = nullptr;
  // Records `out` holds: a job with more distinct keys writes none (the host sees
  // num_unique > out_cap and takes another path).
  u64 out_cap = ~0ull;
  // Compact host output (kv.hpp compact records) instead of the 40-B
  // records at `out`: virtual partition v writes its entries, in key order, from word
  // 5 * (entries before v) of `cout` -- where its 40-B records would have started, so the
  // look-back is unchanged and the capacity is out_cap records' worth of words -- and
  // ctab[v] = entries | words << 16 | first entry << 32 (host-mapped, every v of the launch;
  // ~0: not written).
  u64* cout = nullptr;
  u64* ctab = nullptr;
};
void launch_dict_ordered(ConstKeysSoA tokens, const u64* counts, const u8* parts,
                         const u32* d_n, u64 cap, MapCounters* ctr, OutRecord* out,
                         MapCounters* ctr_out, LookbackScratch lb, hipStream_t s,
                         u64* trace = nullptr, const OrderedExtra& ex = OrderedExtra{});
// Writes `value` to the host-mapped `word` once everything earlier on `s` has completed
// (signal.hip; the lean job path polls it instead of synchronising the stream).
void launch_signal_host(u32* word, u32 value, hipStream_t s);
// bytes (a multiple of 16, 16-B aligned) from device memory into a host-mapped buffer
// through its device pointer, by a kernel (signal.hip)
void launch_copy_to_mapped(void* dst_mapped_dev, const void* src, u64 bytes, hipStream_t s);

// Large ordered build (passes past kPartBuildMaxTokens whose map wrote a partition table,
// dict.hip): launch_dict_partials splits tiles [tile_begin, tile_end) into `nslices`
// slices; workgroup (p, k) aggregates partition p's records of slice k and writes the
// distinct keys + counts to partial slot p * nslots + slot_base + k (`partials`:
// kDictParts * nslots * kPartSlotsHost records, `partial_n`: one length per slot, all ones
// if its table overflowed).  Upload pieces each get their own slot, filled right after the
// piece's map (the aggregation overlaps the remaining H2D).  launch_dict_ordered_partials
// merges each partition's nslots slots and finishes like launch_dict_ordered (overflow:
// kCtrDictOverflow).
constexpr int kOrdWorkers = 4;         // slices of a one-launch large pass
constexpr int kMaxPartialSlots = 32;   // slots per partition (pieces of a piecewise pass)
constexpr int kPartSlotsHost = 2048;  // distinct keys per LDS table (dict.hip kPartSlots)
// trace (diagnostics, optional): kDictParts * kOrdWorkers * 8 stamps (see dict.hip).
// counts: per-record multiplicities of a combining map (null: every record is 1).
void launch_dict_partials(ConstKeysSoA tokens, const u64* counts, const u32* part_off,
                          u32 tile_begin, u32 tile_end, u32 nslices, u32 slot_base, u32 nslots,
                          u64 cap, KeyCount* partials, u32* partial_n, hipStream_t s,
                          u64* trace = nullptr);
void launch_dict_ordered_partials(const KeyCount* partials, const u32* partial_n, u32 nslots,
                                  MapCounters* ctr, OutRecord* out, MapCounters* ctr_out,
                                  LookbackScratch lb, hipStream_t s, u64* trace = nullptr,
                                  const OrderedExtra& ex = OrderedExtra{});
// Same, over runs of KeyCount records each sorted by key (the gather strategy's per-rank
// combined outputs); duplicates across runs are summed.  Run 0 is `own`, runs 1.. lie
// back to back in `recv`; `meta` (device) = [nruns <= 64, len_0, len_1, ...].
constexpr int kMaxMergeRunsHost = kMaxSlotRanks;
void launch_dict_merge_runs(const KeyCount* own, const KeyCount* recv, const u32* meta,
                            MapCounters* ctr, OutRecord* out, MapCounters* ctr_out,
                            LookbackScratch lb, hipStream_t s, PartMap pm = PartMap{});
// ---------------- partplan.hip ----------------
// A partition map cut at equal weights of a sample's distinct keys (first words
// ukeys_w0[0 .. min(*d_u, ucap)), in any order, with their sample counts; a key seen once
// weighs more: it stands for the rare keys not sampled yet): writes out->lo (device).
void launch_part_plan(const u64* ukeys_w0, const u64* ucount, const u32* d_u, u32 ucap,
                      PartMapTables* out, hipStream_t s);
// ---------------- merge.hip ----------------
// Merge of sorted runs (same run layout and meta as launch_dict_merge_runs) by lock-step
// binary search + one look-back scan: `merged` (room for every record, bounded by `cap`)
// is scratch; out / ctr / ctr_out as for launch_dict_ordered.  `lb` needs
// merge_scratch_words(cap) status words and a tile counter; the merge resets them itself
// (no memset needed).  Requires fewer than 2^22 records and a total count below 2^40
// (checked by the caller).
u64 merge_scratch_words(u64 cap);
void launch_merge_sorted_runs(const KeyCount* own, const KeyCount* recv, const u32* meta,
                              u64 cap, KeyCount* merged, MapCounters* ctr, OutRecord* out,
                              MapCounters* ctr_out, LookbackScratch lb, hipStream_t s);
// Same over the all-gathered slots: `nslots` slots of kSlotHeaderRecords + slot_records
// records each, run q = slot q's records, its length min(header.n, slot_records) (0 when
// the header's status is not kSlotOk).  `merged` needs nslots * slot_records records.
// hdr_out (optional, host-mapped): every slot's header, copied by the merge.
void launch_merge_slots(const KeyCount* slots, u32 nslots, u32 slot_records, KeyCount* merged,
                        MapCounters* ctr, OutRecord* out, MapCounters* ctr_out,
                        LookbackScratch lb, SlotHeader* hdr_out, hipStream_t s);
// (kMergeMaxRecords, kMergeMaxCount: locust/slot.hpp)

// Hash every token (with its count; null = 1) into the table; distinct keys land in
// ukeys[0 .. ctr->num_unique) with summed counts in ucount.  At most max_blocks workgroups
// (each streams its share of the tokens through one LDS cache; past 2^18 tokens a workgroup
// takes more than one chunk -- a stage test asks for fewer to stream a small input).
void launch_dict_insert(ConstKeysSoA tokens, const u64* counts, const u32* d_n, u64 cap,
                        const DictWorkspace& dw, MapCounters* ctr, hipStream_t s,
                        u32 max_blocks = 1024);
// rank[i] = number of keys smaller than key i (distinct keys; rank zeroed by the caller);
// with counts/val also val[i] = total count of the smaller keys (zeroed by the caller).
// Early-exits (device-side) when *d_u > kRankSortMax.
void launch_rank_sort(ConstKeysSoA keys, const u64* counts, const u32* d_u, u64 cap, u32* rank,
                      u64* val, hipStream_t s);
// out[rank[i]] = {key i, count i} (val feeds total_count only); optional host-mapped
// counter snapshot.
void launch_rank_emit(ConstKeysSoA keys, const u64* counts, const u32* rank, const u64* val,
                      u64 cap, const MapCounters* ctr, OutRecord* out, MapCounters* ctr_out,
                      hipStream_t s);
void launch_rank_scatter(ConstKeysSoA keys, const u64* counts, const u32* rank, const u32* d_u,
                         u64 cap, KeysSoA sorted, u64* sorted_counts, hipStream_t s);
// Scan of the sorted counts (-> ctr->total_count) and the OutRecords.
void launch_scan_pack(ConstKeysSoA sorted, const u64* counts, u64 cap, MapCounters* ctr,
                      OutRecord* out, LookbackScratch lb, hipStream_t s,
                      MapCounters* ctr_out = nullptr, u32 emit_limit = 0xFFFFFFFFu);

// ---------------- shuffle.hip ----------------
// SoA keys (+ counts, null = 1) -> AoS KeyCount records (the all-to-all payload).
void launch_pack_records(ConstKeysSoA keys, const u64* counts, const u32* d_n, u64 cap,
                         KeyCount* out, hipStream_t s);

// AoS KeyCount -> SoA keys + counts (+ parts, optional: partition tag per record for the
// partitioned dictionary builds).
void launch_unpack_records(const KeyCount* in, u64 n, KeysSoA keys, u64* counts, u8* parts,
                           hipStream_t s, PartMap pm = PartMap{});
// S evenly spaced keys of a sorted array of *d_n keys: sample[k] = keys[floor((k+0.5)*n/S)].
void launch_sample_keys(ConstKeysSoA sorted, const u32* d_n, u32 num_samples, PackedKey* out,
                        hipStream_t s);
// This rank's ExchMsg1 from the device counters (asynchronous-map exchange, exchange.hip):
// tmpl's status (host-side failure) or kExchMapRedo on a partition overflow; n_local,
// tokens (map_tokens of a combining map, else num_records) and the map statistics.  With
// num_samples, the same launch writes the samples of `sorted` (as launch_sample_keys) as
// PackedKeys right behind the header.
void launch_exch_header(const MapCounters* ctr, const ExchMsg1& tmpl, bool combined,
                        ExchMsg1* out, hipStream_t s, ConstKeysSoA sorted = ConstKeysSoA{},
                        const u32* d_n = nullptr, u32 num_samples = 0);
// offsets[p] = lower_bound(sorted, splitter[p-1]) for p in 1..P-1, offsets[0] = 0,
// offsets[P] = n.
void launch_bucket_offsets(ConstKeysSoA sorted, const u32* d_n, const PackedKey* splitters,
                           u32 num_buckets, u64* offsets, hipStream_t s);

// ---------------- exchange.hip (device-resident shuffle, locust/exch.hpp) ----------------
// Merge of nslots all-to-all slots (as launch_merge_slots) writing at most out_limit
// output records (counters still count all of them).
// The shuffle tail in two launches around the C3 all-gather:
// launch_merge_rank_slots merges the received slots into `merged` and sums the distinct
// keys / tokens / compact words into `acc`, kMergeAccSpread (firsts, tokens, words) u64
// triples (zeroed beforehand:
// launch_exch_report sums and re-zeroes them); launch_merge_emit_compact then writes this
// rank's range as compact
// records (kv.hpp) straight into the shared host output -- region `region` (or the root's,
// root_msg), word kOutWords x (region x region_records + the lower ranks' records) of
// `dst` -- and stamps `seq` when the whole range is out (locust/shm.hpp).  Nothing is
// written when a report flags a problem.  `lb`: merge_scratch_words status words + a tile
// counter, reset by launch_merge_rank_slots (a second emit of the same merge needs them
// zeroed again).
constexpr int kMergeAccSpread = 64;
void launch_merge_rank_slots(const KeyCount* slots, u32 nslots, u32 slot_records,
                             KeyCount* merged, u64* acc, LookbackScratch lb, hipStream_t s);
void launch_merge_emit_compact(const KeyCount* slots, u32 nslots, u32 slot_records,
                               const KeyCount* merged, const ExchMsg3* msg3_all,
                               const ExchMsg1* root_msg, u64 region, u32 regions,
                               u64 region_records, u32 P, u32 me, u32 gather_records, u64* dst,
                               u64* stamps, u64 seq, u32* done, LookbackScratch lb,
                               hipStream_t s);
void launch_exch_plan(const char* msg1_all, u32 P, u32 S, ConstKeysSoA keys, const u32* d_n,
                      u32 slot_records, ExchCtl* ctl, hipStream_t s,
                      u64* trace = nullptr);
void launch_exch_pack(const KeyCount* recs, const u32* d_n, u64 cap, const ExchCtl* ctl, u32 P,
                      u32 slot_records, char* send, hipStream_t s);
// (acc: launch_merge_rank_slots' accumulators, summed and re-zeroed here)
void launch_exch_report(const char* recv, u32 P, u32 slot_records, const ExchCtl* ctl,
                        u64* acc, u32 gather_records, ExchMsg3* msg3, hipStream_t s);
// ---------------- topk.hip ----------------
// Top-K by count over `n` output records in key order (engine.hpp "top-K words by count"):
// the min(k, n) records with the largest count, ordered by (count descending, index
// ascending), each with its exact u64 val (exclusive prefix of the counts in key order).
// k <= kTopKMax (engine.hpp; the winners' final sort is one workgroup's LDS).
//
// A sequence of kernels on `s`; data moves between workgroups only across the kernel
// boundaries -- no polled words, no look-back, nothing a workgroup waits for:
//   extract     counts -> dense array, per-tile count sums, the largest count
//   digit x 8   radix select of the k-th largest count, most significant byte first: the
//               histogram of byte b over the counts that match the digits chosen so far
//               (LDS histogram per workgroup, one global atomic per non-empty bin).  Every
//               workgroup re-derives the chosen digits from the earlier passes' finished
//               histograms, so the threshold and the remaining quota live in device memory
//               only.  Passes above the largest count's top byte exit at once.
//   tile count  per tile: records above the threshold T, records equal to it
//   scan        one workgroup: exclusive scans of the tile arrays (val bases, slot bases)
//   scatter     (count, index, val) of every record with count > T and of the first
//               `quota` records (key order) with count == T into their candidate slots
//   final       one workgroup sorts the <= kTopKMax candidates in LDS, gathers the keys and
//               writes the TopRecords and their number
struct TopRecord {
  u64 w[kKeyWords];
  u64 count;
  u64 val;
};
static_assert(sizeof(TopRecord) == sizeof(TopEntry), "TopRecord == TopEntry (48 B)");
constexpr int kTopKBlock = 256;
constexpr int kTopKItems = kTopKTile / kTopKBlock;
static_assert(kTopKTile % kTopKBlock == 0 && kTopKItems == 8, "2048-record tiles");
static_assert((kTopKMax & (kTopKMax - 1)) == 0 && kTopKMax >= 1024 && kTopKMax <= 4096,
              "the final sort holds kTopKMax candidates in 48 KiB of LDS");
struct TopKWorkspace {
  u64* counts = nullptr;      // [cap] dense counts
  u64* tile_val = nullptr;    // [tiles] count sums, scanned in place: the tiles' val bases
  u64* tile_ge = nullptr;     // [tiles] (#gt << 32 | #eq), scanned in place: slot bases
  u64* sel = nullptr;         // [1 + 8 * 128]: the largest count, then 8 x 256 u32 bins
  u64* cand_count = nullptr;  // [kTopKMax] candidates: count, record index, val
  u32* cand_idx = nullptr;
  u64* cand_val = nullptr;
  u64 cap = 0;                // records the arrays hold
};
constexpr u64 kTopKSelWords = 1 + 8 * 256 / 2;
u64 topk_workspace_bytes(u64 cap);
// Carves `base` (topk_workspace_bytes(cap) bytes, 256-B aligned) into the arrays.
void topk_workspace_carve(char* base, u64 cap, TopKWorkspace* ws);
// Enqueues the selection over recs[0 .. n) (n <= ws.cap, n < 2^32, 1 <= k <= kTopKMax):
// `out` (host-mapped allowed, room for min(k, n) records) and *out_n.  Zeroes every word
// the kernels accumulate into (ws.sel) itself, on every call.
void launch_top_select(const OutRecord* recs, u64 n, u32 k, const TopKWorkspace& ws,
                       TopRecord* out, u32* out_n, hipStream_t s);

// ---------------- index.hip ----------------
// Inverted index behind a word job (engine.hpp "inverted index"): over the `n` key-ordered
// output records of the job and the text its map read, the line number of every emitted
// token in (key, line) order -- word i's postings are [val_i, val_i + count_i).
//
// A sequence of kernels on `s`; this file adds no wait between workgroups (the line index
// and the radix sort it reuses keep their own look-back):
//   offsets     val[0 .. n] = exclusive scan of the counts (tile sums, one-workgroup scan
//               of the tile array, per-tile scan) and the total
//   line index  launch_line_index over the text
//   map         one wave per line re-tokenises it with the word job's rules, packs each
//               emitted token's key (bit-identical to the map's), binary-searches its rank r
//               among the records and writes the pair word r << 32 | line.  The slots come
//               from one atomic per wave and group of up to 64 consecutive lines, whose
//               emitted tokens the wave counts first; a key not found counts as a miss
//   order       radix_sort() of the pair words as one-word keys
//   emit        postings[j] = first_line + low32(sorted[j]); pairs outside their word's
//               [val, val + count) count as misplaced
struct IndexCounters {  // zeroed per job
  u64 total;      // sum of the records' counts
  u32 written;    // pair words the map wrote
  u32 miss;       // emitted tokens whose key is not among the records
  u32 sort_n;     // pairs handed to the sort: `written` if it is the expected number, else 0
  u32 misplaced;  // sorted pairs outside their word's range
};
constexpr int kIndexBlock = 256;
constexpr int kIndexItems = 8;
constexpr int kIndexTile = kIndexBlock * kIndexItems;  // records per workgroup of the offsets
struct IndexWorkspace {
  char* zero = nullptr;  // [MapCounters | IndexCounters | line-index look-back], zeroed per job
  u64 zero_bytes = 0;
  MapCounters* lctr = nullptr;  // the line index's counters (num_newlines)
  IndexCounters* ctr = nullptr;
  LookbackScratch lb{};
  u64* pairs = nullptr;     // [pair_cap] rank << 32 | line, in arbitrary order
  u64* zeros = nullptr;     // [pair_cap] zero: key words 1..3 of the sort
  u64* sorted = nullptr;    // [pair_cap] the pair words ascending
  u64* spare = nullptr;     // [pair_cap] where the sort puts its copies of the zero words
  u32* postings = nullptr;  // [pair_cap]
  u64* val = nullptr;       // [rec_cap + 1]
  u64* tile_val = nullptr;  // [tiles]
  u64* nl_pos = nullptr;    // [line_cap + 1]
  RadixWorkspace rx{};      // the sort's own buffers (pair_cap keys)
  u64 pair_cap = 0, rec_cap = 0, line_cap = 0, text_cap = 0;
};
u64 index_zero_bytes(u64 text_cap);
u64 index_workspace_bytes(u64 pair_cap, u64 rec_cap, u64 line_cap, u64 text_cap);
// Carves `base` (index_workspace_bytes(...) bytes, 256-B aligned).  The caller zeroes
// ws->zeros once.
void index_workspace_carve(char* base, u64 pair_cap, u64 rec_cap, u64 line_cap, u64 text_cap,
                           IndexWorkspace* ws);
struct IndexJob {
  const OutRecord* recs = nullptr;  // the word job's records, key order, device memory
  u64 n = 0;                        // ... their number (num_unique)
  u64 tokens = 0;                   // the word job's num_tokens: the pairs to expect
  const char* text = nullptr;       // the text the map read (16-B aligned; host-mapped allowed)
  u64 bytes = 0;
  u64 num_lines = 0;                // its lines (sizes the grid; <= ws.line_cap)
  u64 first_line = 0;               // global number of line 0
  DelimMask dm{};
  int emits_per_line = 0, max_key_len = 0;
};
// Enqueues the stage; ws.postings[0 .. tokens) and ws.ctr are complete when `s` has
// drained.  With more than kSmallSortMax tokens the sort reads its plan back through
// h_plan (pinned) and synchronises `s` once, as radix_sort does.
void launch_index(const IndexJob& job, IndexWorkspace& ws, SortPlan* h_plan, hipStream_t s);

// ---------------- append.hip ----------------
// The merge of two indexes in device memory (engine.hpp "appending to the index"): A, the
// resident one, and B, what launch_index just left for a block whose first line follows A's
// last, so B's postings are global already.  C, in buffers of its own, is the index a single
// pass over A's text followed by B's would have left.
//
// A sequence of kernels on `s`; data crosses between workgroups only at kernel boundaries, no
// output array is written with atomics and every output word has exactly one writer:
//   locate    one thread per record: a B record's lower bound among A's records (and whether
//             its key is absent there: fresh), an A record's lower bound among B's
//   scan      sB = exclusive scan of fresh (tile sums, one-workgroup scan of the tile array,
//             per-tile scan); nC = nA + sB[nB]
//   records   pos(A[i]) = i + sB[lbB[i]], pos(B[j]) = lbA[j] + sB[j].  The A thread writes the
//             coalesced record (countA + countB when B holds the key), a B thread only a fresh
//             key; both leave their record's position for the postings kernel
//   offsets   valC = exclusive scan of C's counts (the same three kernels), valC[nC] = TA + TB
//   postings  tiles of kAppendTile source elements, A's tiles then B's.  A tile finds the
//             words its elements belong to by two binary searches in the source val, stages
//             their source offsets and destination shifts in LDS, and every element then finds
//             its word there: a list of any length is moved by as many workgroups as it has
//             tiles, and each element moves exactly once
//   lines     nl_posC = nl_posA ++ (nl_posB + bytesA), num_newlines = nlA + nlB
// The text is two device-to-device copies and 16 zero bytes behind them.
struct AppendCounters {  // one 64-byte readback, zeroed per append
  u64 moved;      // postings moved
  u32 records;    // records written to C
  u32 fresh;      // words of B that A did not hold
  u32 misplaced;  // a destination outside [valC[p], valC[p+1]), a record position >= nC, a
                  // key order violation seen by the records kernel
  u32 pad[11];
};
static_assert(sizeof(AppendCounters) == 64, "AppendCounters: one 64-byte readback");
constexpr int kAppendBlock = 256;
constexpr int kAppendItems = 4;
constexpr int kAppendTile = kAppendBlock * kAppendItems;  // postings per workgroup
// One side of a merge, or its destination (device memory).
struct AppendIndex {
  OutRecord* recs = nullptr;    // [n] key order
  u64* val = nullptr;           // [n + 1]
  u32* postings = nullptr;      // [tokens]
  char* text = nullptr;
  u64* nl_pos = nullptr;        // [num_newlines]
  MapCounters* lctr = nullptr;  // num_newlines
  u64 n = 0, tokens = 0, bytes = 0;
  u64 lines = 0;  // the text's lines: bounds num_newlines (a destination: its capacity)
};
struct AppendScratch {
  AppendCounters* ctr = nullptr;
  u32* a_pos = nullptr;     // [nA] lbB, then pos(A[i])
  u32* b_pos = nullptr;     // [nB] lbA, then pos(B[j])
  u64* fresh = nullptr;     // [nB] 1: B's key is absent from A (the scans read u64 words)
  u64* sb = nullptr;        // [nB + 1]
  u64* tile_val = nullptr;  // [div_up(nA + nB, kIndexTile) + 1]
  u64 rec_cap_a = 0, rec_cap_b = 0;
};
u64 append_scratch_bytes(u64 rec_cap_a, u64 rec_cap_b);
void append_scratch_carve(char* base, u64 rec_cap_a, u64 rec_cap_b, AppendScratch* ws);
// Enqueues the merge of a and b into c (c's arrays hold a.n + b.n records, a.tokens + b.tokens
// postings, a.bytes + b.bytes + 16 text bytes and a.lines + b.lines line starts); ws.ctr is
// complete when `s` has drained.
void launch_append(const AppendIndex& a, const AppendIndex& b, const AppendIndex& c,
                   AppendScratch& ws, hipStream_t s);

// ---------------- drop.hip ----------------
// Dropping the oldest lines of an index in device memory (engine.hpp "dropping the oldest
// lines"): the mirror image of the merge.  A is the resident index over the lines
// [F, F + N), d <= N the number of lines to drop and cut_line = F + d.  Every list is
// non-decreasing in the line number, so what a word loses is a prefix of its list.  C, in
// buffers of its own, is the index a single pass over A's text without its first d lines,
// numbered from cut_line, would have left.  Nothing is renumbered and nothing is sorted.
//
// A sequence of kernels on `s`; data crosses between workgroups only at kernel boundaries, no
// output array is written with atomics and every output word has exactly one writer:
//   cut       one thread per record: k_w = the lower bound of cut_line in the word's list (the
//             postings < cut_line; duplicates of cut_line are kept), survive_w = k_w < count_w
//   scan      pos = exclusive scan of survive (device/tile_scan.hpp's three kernels);
//             nC = pos[nA] stays on the device
//   records   a survivor writes its record once, count = count_w - k_w, at pos[w], and leaves
//             its source word there for the postings kernel; keys are checked to ascend
//   offsets   valC = exclusive scan of C's counts (the same three kernels), valC[nC] = TC
//   postings  tiles of kAppendTile DESTINATION elements: a tile finds the words of C its
//             elements belong to by two binary searches in valC, stages their offsets and
//             their shifts to the source in LDS, and every element then finds its word there.
//             The grid is the host's bound (A's tokens); a tile past TC leaves at once
//   lines     B = the byte behind the newline of line d - 1 (all bytes when the last,
//             unterminated line goes too); nl_posC[k] = nl_posA[d + k] - B,
//             num_newlines -= min(d, num_newlines)
//   text      the suffix from B, read on the device, with 16 zero bytes behind it
//   stats     one wave per dropped line walks it as index.hip does and counts the lines over
//             the emit cap and, among each line's emitted tokens, those longer than max_key_len
struct DropCounters {  // one 64-byte readback, zeroed per drop
  u64 moved;           // postings moved
  u64 dropped;         // postings below cut_line
  u64 cut_byte;        // B: the text bytes removed
  u32 records;         // records written to C
  u32 vanished;        // words whose list emptied
  u32 misplaced;       // a destination outside [valC[p], valC[p+1]), a position >= nC, a key
                       // order violation, a non-ascending val
  u32 nc;              // survivors: C's records (the scan's total)
  u32 overflow_lines;  // dropped lines with more than emits_per_line tokens
  u32 truncated;       // emitted tokens of the dropped lines longer than max_key_len
  u32 pad[4];
};
static_assert(sizeof(DropCounters) == 64, "DropCounters: one 64-byte readback");
constexpr int kDropStatWaves = 4;  // waves (lines in flight) per workgroup of the stats walk
struct DropScratch {
  DropCounters* ctr = nullptr;
  u32* k = nullptr;         // [nA] postings of word w below cut_line
  u64* keep = nullptr;      // [nA] 1: the word survives (the scans read u64 words)
  u64* pos = nullptr;       // [nA + 1] exclusive scan of keep
  u32* src_of = nullptr;    // [nA] the source word of C's record p
  u64* tile_val = nullptr;  // [div_up(nA, kIndexTile) + 1]
  u64 rec_cap = 0;
};
u64 drop_scratch_bytes(u64 rec_cap);
void drop_scratch_carve(char* base, u64 rec_cap, DropScratch* ws);
// The word job's token rules, for the statistics of the dropped lines.
struct DropRules {
  DelimMask dm{};
  int emits_per_line = 0, max_key_len = 0;
};
// Enqueues the drop of a's first d lines (1 <= d <= a.lines; cut_line = a's first line + d)
// into c, whose arrays hold a.n records, a.tokens postings, a.bytes + 16 text bytes and
// a.lines - d line starts (c's n, tokens, bytes and lines are its capacities).  a's line index
// must exist (a text without tokens: launch_line_index first).  ws.ctr is complete when `s`
// has drained; C's sizes are nc, moved and a.bytes - cut_byte.
void launch_drop(const AppendIndex& a, const AppendIndex& c, u32 cut_line, u64 d,
                 const DropRules& rules, DropScratch& ws, hipStream_t s);

// ---------------- search.hip ----------------
// All/any/phrase/near word queries over the inverted index launch_index left on the device
// (engine.hpp "index search"): the key-ordered records, the CSR offsets `val` and the sorted
// postings; a phrase or a `near` query is verified against the text the index was built
// from, which is resident too.  A batch holds Q <= kSearchMaxQueries queries of
// <= kSearchMaxTerms terms.
//
// A sequence of kernels on `s`; data moves between workgroups only across the kernel
// boundaries (the radix sort it reuses keeps its own look-back), no polled word:
//   match    (only in a batch that has a pattern term, b.pat != null; engine.hpp "pattern
//            terms") a grid walks the records in tiles of kSearchBlock, one record per thread,
//            the key in registers, and loops over the batch's pattern slots (grid y: a share
//            of the queries).  A pattern is wave-uniform: its words and its metacharacter map
//            come by scalar loads.  One ballot per wave and pattern; a wave with a match adds,
//            by one lane, its matching words and their summed counts to the slot's `words`
//            and `len` and leaves one matching rank.  (pattern slots) x (dictionary words)
//            matcher calls (device/glob.hpp)
//   lookup   one thread per (query, term): find_rank of the packed key, the term's val and
//            length; per query the distinct terms, the driver (the shortest list, `all`), the
//            dead flag (`all` with an absent term) and the bound on its hits = the elements
//            it walks: the driver's length (`all`) or the distinct terms' lengths (`any`).
//            A phrase or a `near` query is looked up as `all`: its bound covers its
//            candidates and its hits.
//            A prefix term (engine.hpp "prefix terms"; q_meta bit 16 + t, the key's non-zero
//            bytes are the prefix) finds its words' rank range [lo, hi) with
//            dev::find_prefix_range: the lower bound of p padded with 0x00, the upper bound
//            of p padded with 0xff.  Its list is postings[val[lo] .. val[hi]), its length
//            val[hi] - val[lo].  Terms are distinct when their ranges differ; the score mask
//            (q_info bits 24..31) leaves out a term whose range lies inside another's, and
//            `any` walks only the score mask's terms (a list inside another adds no line).
//            x_len = the length of a list of two or more words that repeats no earlier
//            term's of its query: it has to be merged; the lengths add up in ctr->merge (one
//            atomic per wave that has any)
//            Exclusion terms (engine.hpp "exclusion terms"; q_meta bit 24 + t: term t is
//            one, and the host packs them behind the positive terms) are resolved like any
//            term into t_val, t_len, x_len and the merge total, and left out of the driver
//            choice, the bound, the dead flag, the distinct-term mask and the score mask,
//            which all see the positive terms as if they were the whole query.  The present
//            ones go to the hit kernel as q_info bits 8..15: bit i is set when an exclusion
//            term's words are those of term i, the query's first term with them (itself, an
//            earlier exclusion term or a positive term), so every exclusion list is read once
//            and a merged list through the slot that owns it
//            A pattern slot takes its length and its words from the match stage, not from a
//            range search: one word, t_val = val[rank] and the list stays in place; two or
//            more and no dup, it is wide and adds its length to x_len and ctr->merge exactly as
//            a wide prefix slot does.  It is dup when an earlier pattern term of its query has
//            equal pattern words and metacharacter map (the host lower-cases a folding
//            batch's patterns); it takes no part in the range rules: never the same as a plain
//            or prefix term, never inside one, none inside it.  An `any` query's bound is
//            summed in u64; one past 32 bits counts in ctr->anyover
//   scan     one workgroup: q_start[0 .. Q] = exclusive scan of the bounds, the total B
//   (the host reads B, the merge total X and the term counts in one readback, and sizes the
//   hit workspace for max(B, X))
//   expand   (only when X > 0: the batch has a prefix term that covers two or more words;
//            every other batch runs the launches, copies and synchronisations it ran before
//            prefix terms existed)
//            scan     x_start[0 .. Q * 8] = exclusive scan of x_len over the slots
//            gather   the flattened [0, X) in tiles of kSearchTile, grid-stride: a binary
//                     search in x_start finds the element's slot, the key is
//                     slot << 32 | (line - first_line), written to the hit workspace's
//                     `pairs` (idle until the hit stage); its first thread sets merge_n = X.
//                     It skips the elements of pattern slots
//            scatter  (pattern batches) the match stage's walk and match once more, over the
//                     wide pattern slots only.  Per wave and pattern: a wave prefix sum of the
//                     matching words' counts, one atomic on the slot's cursor reserves the
//                     room, then the whole wave copies each matching word's postings in turn,
//                     coalesced (never one thread per word: `the` has thousands), as keys
//                     slot << 32 | (line - first_line) at x_start[slot] + the reserved offset,
//                     never outside the slot's part of [0, X).  The order of the words does
//                     not matter: the sort decides
//            order    radix_sort() of the keys as one-word keys: (slot, line)
//            strip    merged[e] = first_line + low32(sorted[e]); a key outside its slot's
//                     x_start range counts in `unmerged` (the host throws), and so does a
//                     pattern slot whose cursor does not end at its x_len; the merged
//                     slots' t_val become kSearchMerged | x_start[slot]
//            The hit, phrase-candidate and score stages read such a term's list from
//            merged + x_start[slot], t_len elements, as they read any list
//   hits     a grid walks the flattened (query, list element) space in tiles of kSearchTile.
//            An element counts when it is the first of its line in its list; `all`: when a
//            binary search finds the line in every other distinct term's list; `any`: when
//            none of the earlier distinct terms' lists holds it.  A hit is the pair word
//            query << 32 | (line - first_line); its slot comes from one atomic per wave and
//            step, the per-query hit counts from one atomic per wave, step and query.  An
//            element of a phrase of two or more terms that passes the `all` test is a
//            candidate: the same pair word goes to `cands`, its slot from one atomic per wave
//            and step on the candidate counter, and q_hits is left alone.  The same holds
//            for a `near` query that needs verification (kSearchNear) and has two or more
//            distinct terms; its candidates have a counter of their own (ncands) and fill
//            `cands` from its last word downwards, so neither verify kernel sees the
//            other's (cands + ncands <= B <= cap: the two ends never meet).
//            Before the hit / candidate split, an element of a query with exclusion lists is
//            dropped when a binary search finds its line in one of them (term_list: merged
//            lists too): excluded lines reach neither `cands` nor `pairs` nor q_hits.  A
//            batch without exclusion terms only tests the empty mask
//   phrase   (only when the batch has a phrase of two or more terms) one wave per candidate,
//            up to 64 consecutive candidates per wave and round.  The wave re-tokenises the
//            candidate's line with the word job's rules (device/linetok.hpp, as index.hip's
//            map), compares every emitted token's key with the query's packed term keys
//            (bit j of a token's mask: it equals term j; for a prefix term: it starts with
//            the term's bytes, (w_i & key_word_mask(k_i)) == k_i for the four key words, the
//            masks computed in registers) and runs the shift-and automaton
//            state = ((state << 1) | 1) & mask over the tokens in order; bit m - 1 set
//            is a hit (m: the positive terms, nterms - the exclusion terms; only their keys
//            are compared).  After a round lane i holds candidate i's verdict and the hits are
//            written as the hit kernel writes them: one atomic per wave and round for the
//            slots, one per distinct query for q_hits; one more counts the verified candidates
//   near     (only when the batch has a `near` query that needs verification: two or more
//            terms and W < emits_per_line) the phrase kernel's skeleton and token masks over
//            the `near` candidates.  In place of the automaton the wave keeps, per term, 1 +
//            the ordinal of the last token that matched it (0: none yet): lane j < 8 holds
//            term min(j, m - 1)'s (m as the phrase kernel's) in one register, updated by a select.  It walks only
//            the step's tokens whose mask is non-zero, in order; behind each, the minimum
//            over lanes 0 .. 7 (three DPP row shifts) is non-zero when every term has been
//            seen, and the line matches if ord + 1 - min < W (a minimal covering window
//            ends at a matching token).  The state carries across the 64-byte steps;
//            ordinals and W are full u32.  Commits as the phrase kernel does; `nverified`
//            counts the decided candidates
//            A batch that has a pattern term runs the two kernels' siblings instead
//            (search_globphrase_kernel, search_globnear_kernel: the same bodies, compiled with
//            the matcher): a token matches a pattern term when glob_match says so of its cut
//            key, with the batch's fold; plain and prefix terms of such a batch match as ever.
//            Every other batch runs the kernels it ran before, at their resources.  A batch
//            that has a fuzzy term runs fuzzy.hip's match, scatter, phrase and near kernels:
//            the same bodies once more, with the fuzzy matcher beside the pattern matcher; one
//            that has a regex term regex.hip's
//   seal    one thread: the sort's length, capped by the workspace
//   (the host reads the number of hits H: the sort takes its regime from it)
//   order    radix_sort() of the pair words as one-word keys
//   offsets  one workgroup: offsets[0 .. Q] = exclusive scan of the per-query hit counts
//   emit     lines[j] = first_line + low32(sorted[j]); a pair outside the offsets range of
//            the query it names counts as misplaced
// A ranked batch (engine.hpp "ranked search"; launch_search_rank in place of
// launch_search_order) goes on from the seal with the unsorted pairs:
//   offsets  the same scan of the per-query hit counts (the matches, and the segments of the
//            sorted keys), and once more over min(hits, K): out_off[0 .. Q], where each
//            query's returned lines go.  All in u64: K = 2^32 - 1 overflows nothing
//   score    one thread per pair: per term of the score mask tf = upper bound - lower bound
//            of the line in the term's list (never outside it), weight =
//            32 - clz(N / t_len) with N = val[n]; the pair becomes the rank key
//            query << 54 | (kRankScoreMax - score) << 32 | rel_line in `cands`, which the
//            phrase kernel has left.  A score of 0 or above 32 * emits_per_line (a batch that
//            has a pattern term: times 8, its lists may overlap) counts in `unscored`
//   order    radix_sort() of the rank keys as one-word keys: (query, score descending, line
//            ascending); the keys are distinct
//   top      one thread per sorted key at j: pos = j - offsets[q], the misplaced check as
//            emit's, and when pos < K lines[out_off[q] + pos] = first_line + rel_line and
//            scores[out_off[q] + pos] = score.  No atomics: every position is determined
struct SearchCounters {  // zeroed per batch
  u64 bound;      // B: the elements the hit kernel walks = the upper bound on the hits
  u32 written;    // hits the hit kernel found
  u32 sort_n;     // pairs handed to the sort: `written` if the workspace holds them, else 0
  u32 misplaced;  // sorted pairs outside their query's range
  u32 cands;      // phrase candidates the hit kernel wrote
  u32 verified;   // phrase candidates the phrase kernel has decided
  u32 unscored;   // ranked: hits whose score is 0 or above 32 * emits_per_line
  u64 merge;      // X: the list elements of the prefix terms to merge (the lookup's sum)
  u32 merge_n;    // keys handed to the merge's sort: X if the workspace holds them, else 0
  u32 unmerged;   // sorted merge keys outside their slot's x_start range
  u32 ncands;     // `near` candidates the hit kernel wrote (from the end of `cands` down)
  u32 nverified;  // `near` candidates the near kernel has decided
  u32 anyover;    // `any` (and `expr`: looked up as `any`, planned by expr.hip) queries whose bound (the sum of their lists' lengths; pattern terms'
                  // lists may overlap) does not fit 32 bits: the host throws
  u32 ebound;     // E: the elements expr_hit_kernel walks ("expr.hip"), saturated at 2^32 - 1
                  // (the host refuses a batch that walks 2^32 elements or more anyway)
};
static_assert(sizeof(SearchCounters) <= 64, "the counters share one 64-byte block");
constexpr int kSearchBlock = 256;
constexpr int kSearchItems = 4;
constexpr int kSearchTile = kSearchBlock * kSearchItems;  // elements per workgroup and step
constexpr int kSearchMaxBlocks = 2048;                     // the hit kernel's grid cap
constexpr u32 kSearchAny = 1u << 8;                        // q_meta: nterms | mode bit
constexpr u32 kSearchPhrase = 1u << 9;                     // (neither bit: `all`)
constexpr u32 kSearchNear = 1u << 10;  // a `near` query to verify (W < emits_per_line, two or
                                       // more terms); every other `near` query goes as `all`
constexpr u32 kSearchExpr = 1u << 11;  // an `expr` query (kernels.hpp "expr.hip"): looked up as
                                       // `any` (kSearchAny is set too), walked by expr.hip
constexpr int kSearchPrefixShift = 16;  // q_meta bit 16 + t: term t is a prefix term
constexpr int kSearchExcludeShift = 24;  // q_meta bit 24 + t: term t is an exclusion term (the
                                         // last terms of the query: positive terms stand first)
constexpr u64 kSearchMerged = 1ull << 63;  // t_val: the list lies in `merged`, not in postings
constexpr u32 kSearchSlots = kSearchMaxQueries * kSearchMaxTerms;  // (query, term) slots
// The pattern arrays (engine.hpp "pattern terms"): one allocation of u32 words, made by an
// engine's first batch that has a pattern term.  The first two parts are uploaded per pattern
// batch, the other four zeroed per pattern batch:
//   flags  [kSearchMaxQueries] bit t: term t is evaluated as a pattern term, its pattern's
//          bytes in the slot's `keys` words; kSearchFold: ASCII letters match either case
//   meta   [kSearchSlots] the pattern's metacharacter map (device/glob.hpp)
//   words  [kSearchSlots] the index keys the pattern matches (the match kernel's count)
//   len    [kSearchSlots] the sum of their counts: the list's length (< 2^32: the words are
//          distinct, and the index holds fewer postings than that)
//   rank   [kSearchSlots] the rank of one matching word (the word, when there is just one)
//   cursor [kSearchSlots] the scatter kernel's fill of the slot's part of [0, X)
// A fuzzy term (engine.hpp "fuzzy terms") is a pattern slot too: its flag bit t is set, so the
// lookup, gather and strip stages treat it as they treat any pattern slot, and besides
//   flags  bit kSearchFuzzyShift + t: the slot's `keys` words hold the word w, no pattern
//   meta   kFuzzyMeta | d (device/fuzzy.hpp): the budget, and a bit no metacharacter map has,
//          so a fuzzy slot never compares equal to a pattern slot in the lookup's identity rule
// A batch with such a bit sets SearchBatch::fuzzy and runs fuzzy.hip's kernels.
// A regex term (engine.hpp "regex terms") is a pattern slot as well, and besides
//   flags  bit kSearchRegexShift + t: the slot stands for a compiled program
//   meta   the program's index in the batch's program table (SearchBatch::regex)
//   keys   kRegexKeyTag (device/regex.hpp), the index, 0, 0: equal for the identical sources of
//          a batch, which share one program, and equal to no pattern's or fuzzy term's bytes --
//          the tag's top byte is NUL -- in the lookup's identity rule
// A batch with such a bit sets SearchBatch::regex and runs regex.hip's kernels.
constexpr u32 kSearchFold = 1u << 8;
constexpr int kSearchFuzzyShift = 16;
constexpr int kSearchRegexShift = 24;
constexpr u64 kSearchPatMeta = kSearchMaxQueries;
constexpr u64 kSearchPatWords = kSearchPatMeta + kSearchSlots;
constexpr u64 kSearchPatLen = kSearchPatWords + kSearchSlots;
constexpr u64 kSearchPatRank = kSearchPatLen + kSearchSlots;
constexpr u64 kSearchPatCursor = kSearchPatRank + kSearchSlots;
constexpr u64 kSearchPatEnd = kSearchPatCursor + kSearchSlots;
inline u64 search_pattern_bytes() { return kSearchPatEnd * sizeof(u32); }
inline u64 search_pattern_upload_bytes() { return kSearchPatWords * sizeof(u32); }
// The index a batch is answered from (all device memory, launch_index's output).
struct SearchIndex {
  const OutRecord* recs = nullptr;  // [n] key order
  const u64* val = nullptr;         // [n + 1] CSR offsets
  const u32* postings = nullptr;    // [val[n]] global line numbers
  u32 n = 0;
  u32 first_line = 0;
  // what the phrase and near kernels read: the text the index was built from (the engine's own
  // device copy), its line starts as launch_index left them, and the job's token rules
  const char* text = nullptr;
  u64 bytes = 0;
  const u64* nl_pos = nullptr;         // [num_newlines] IndexWorkspace::nl_pos
  const MapCounters* lctr = nullptr;   // num_newlines
  DelimMask dm{};
  int emits_per_line = 0, max_key_len = 0;
};
// The per-batch arrays: fixed size (kSearchMaxQueries), made by the first search job.
struct SearchBatch {
  char* upload = nullptr;  // [q_meta | keys | within]: one H2D per batch
  u32* q_meta = nullptr;   // [kSearchMaxQueries] nterms | mode bit | prefix bits | exclusion bits
  u64* keys = nullptr;     // [Q * kSearchMaxTerms][kKeyWords] packed as kv.hpp packs
                           // (behind them, only in a batch that verifies a `near` query, the
                           // Q windows: search_within)
  char* zero = nullptr;    // [SearchCounters | q_hits], zeroed per batch
  u64 zero_bytes = 0;
  SearchCounters* ctr = nullptr;
  u32* q_hits = nullptr;   // [Q] hits per query
  u64* t_val = nullptr;    // [Q * kSearchMaxTerms] the term's CSR offset; behind the expand
                           // stage kSearchMerged | its offset in `merged` for a merged list
  u32* t_len = nullptr;    // [Q * kSearchMaxTerms] its list's length = the count of its word
                           // (prefix term: of its words); 0: absent
  u32* q_info = nullptr;   // [Q] driver | dead << 3 | exclusion lists << 8 | distinct-term
                           // mask << 16 | score mask << 24 (the terms whose key range lies
                           // inside no other's); both masks: positive terms only
  u32* x_len = nullptr;    // [Q * kSearchMaxTerms] the slot's merged length: t_len of a prefix
                           // term that covers two or more words and repeats no earlier term
                           // of its query, else 0
  u64* x_start = nullptr;  // [kSearchSlots + 1] expand: exclusive scan of x_len
  u32* merged = nullptr;   // [merged_cap] expand: the merged lists, slot after slot (an
  u64 merged_cap = 0;      // allocation of its own, grown on demand: the engine sets both)
  u32* pat = nullptr;      // the pattern arrays (above) of a batch that has a pattern term; null
                           // in every other batch (the engine sets it per batch), and then no
                           // pattern stage runs
  bool fuzzy = false;      // the batch has a fuzzy term (pat is set, too): the dictionary scan,
                           // the verify and the show kernels are fuzzy.hip's (the engine sets it
                           // per batch)
  const u32* regex = nullptr;  // the batch has a regex term (pat is set, too): its program table,
                           // [programs][kRegexWords] (device/regex.hpp), and the dictionary
                           // scan, the verify and the show kernels are regex.hip's (the engine
                           // sets it per batch; null in every other batch)
  u32* expr = nullptr;     // the expression arrays ("expr.hip") of a batch that has an `expr` query;
                           // null in every other batch (the engine sets it per batch), and then
                           // nothing of expr.hip runs
  u32* q_bound = nullptr;  // [Q]
  u64* q_start = nullptr;  // [Q + 1]
  u64* offsets = nullptr;  // [Q + 1]
  u64* out_off = nullptr;  // [Q + 1] ranked: scan of min(hits, K).  The same words as q_start,
                           // which nothing reads behind the hit kernel
};
// The hit arrays, sized by the batch's bound B (grown on demand).
struct SearchHits {
  u64* pairs = nullptr;   // [cap] query << 32 | line, in arbitrary order
  u64* cands = nullptr;   // [cap] phrase candidates: the same pair words, not yet verified;
                          // `near` candidates from cands[cap - 1] downwards
  u64* zeros = nullptr;   // [cap] zero: key words 1..3 of the sort
  u64* sorted = nullptr;  // [cap]
  u64* spare = nullptr;   // [cap]
  u32* lines = nullptr;   // [cap]
  RadixWorkspace rx{};
  u64 cap = 0;
};
// Ranked: the returned lines' scores [cap], parallel to h.lines, in the words of h.pairs (the
// score kernel has turned every pair into its rank key by then).
inline u32* search_rank_scores(const SearchHits& h) { return reinterpret_cast<u32*>(h.pairs); }
// bytes of SearchBatch::upload a batch of Q fills (within: with one window per query)
u64 search_upload_bytes(u32 queries, bool within = false);
// The windows of a batch of `queries` that verifies a `near` query: [queries] u32 behind keys.
inline u32* search_within(u64* keys, u32 queries) {
  return reinterpret_cast<u32*>(keys + (u64)queries * kSearchMaxTerms * kKeyWords);
}
u64 search_batch_bytes();
void search_batch_carve(char* base, SearchBatch* b);
u64 search_hits_bytes(u64 cap);
// Carves `base` (search_hits_bytes(cap) bytes, 256-B aligned).  The caller zeroes h->zeros once.
void search_hits_carve(char* base, u64 cap, SearchHits* h);
// lookup + scan: b.ctr->bound, b.ctr->merge, b.t_len and b.q_start are complete when `s` has
// drained.  A batch with b.expr runs launch_expr_plan between the two.
void launch_search_lookup(const SearchIndex& ix, const SearchBatch& b, u32 queries, hipStream_t s);
// expand (only when the lookup reported merge = X > 0): scan + gather + order + strip.
// b.merged[0 .. X) holds the merged lists and b.t_val names them when `s` has drained; the
// gather's keys and the sort use h (X <= h.cap, X <= b.merged_cap), which the hit stage may
// overwrite behind it.  b.ctr->unmerged counts sorted keys outside their slot's range.  More
// than kSmallSortMax elements read the sort's plan back and synchronise `s` once, as
// launch_search_order does.
void launch_search_expand(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          SearchHits& h, SortPlan* h_plan, hipStream_t s);
// hits (+ phrase, when `verify`: the batch has a phrase of two or more terms; + near, when
// `near`: the batch has a kSearchNear query and its windows) + seal over the `bound`
// elements the lookup reported (bound <= h.cap).
void launch_search_hits(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                        bool verify, bool near, const SearchHits& h, hipStream_t s);
// order + offsets + emit of the `hits` pairs the hit kernel wrote (b.ctr->sort_n == hits):
// b.offsets[0 .. Q], h.lines[0 .. hits) and b.ctr->misplaced.  More than kSmallSortMax hits
// read the sort's plan back through h_plan and synchronise `s` once, as radix_sort does.
void launch_search_order(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 hits,
                         SearchHits& h, SortPlan* h_plan, hipStream_t s);
// The ranked way from the same point (b.ctr->sort_n == hits): offsets + score + order + top.
// b.offsets[0 .. Q] (the matches), b.out_off[0 .. Q], h.lines and search_rank_scores(h)
// [0 .. out_off[Q]), b.ctr->misplaced and b.ctr->unscored.  1 <= k; ix.emits_per_line <=
// kRankMaxEmits.  Synchronises as launch_search_order does.
void launch_search_rank(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 hits,
                        u32 k, SearchHits& h, SortPlan* h_plan, hipStream_t s);

// ---------------- corpus.hip ----------------
// The restrict stage of a search batch (engine.hpp "corpus", "file sets"): of the H unsorted pair
// words the hit and verify kernels left, those whose line lies in a segment of their query's
// file set.  The arrays are one allocation, made by an engine's first batch with a file set and
// grown on demand:
//   ctr      CorpusCounters, zeroed per restricted batch
//   table    [seg_cap] the resident segments' first lines (global, u32, ascending; [0] is the
//            index's first_line): the device mirror of the engine's table, uploaded only when
//            the table has changed since the last batch that needed it
//   q_set    [kSearchMaxQueries] the query's row of `bitmaps`, or kCorpusNoSet: uploaded per batch
//   bitmaps  [sets][ceil(S / 32)] bit o of a row: the resident segment of ordinal o is in the
//            set (ids that are not resident have no bit): one row per distinct set of the
//            batch, uploaded per batch
// The stage adds no workspace per hit: the kept pairs go to SearchHits::cands, idle between the
// verify kernels and the score kernel.
// A deliberate choice: inside a tile the kept pairs' positions come from a workgroup scan, but a
// tile's base is one atomic add on `kept`, not a second pass over a tile array
// (device/tile_scan.hpp).  The pairs are "in arbitrary order" by contract -- the hit kernels
// reserve their slots with atomics too -- and the sort behind the stage fixes the answer, so a
// deterministic layout would buy nothing and cost two more launches.  The layout of the kept
// pairs therefore differs from run to run; the answer does not.
struct CorpusCounters {
  u32 kept;   // pairs the restrict kernel kept
  u32 stray;  // pairs that name no query of the batch, or a line in front of the table
  // the by-file stage's (its own block, CorpusByFile::ctr)
  u32 sort_n;     // keys handed to the sort of a ranked batch: the returned lines
  u32 runs;       // (query, file) runs among the keys: the CSR's entries
  u32 unlocated;  // returned lines outside the table or outside every query's range
};
constexpr int kCorpusBlock = 256;
constexpr int kCorpusItems = 4;
constexpr int kCorpusTile = kCorpusBlock * kCorpusItems;  // pairs per workgroup and step
constexpr int kCorpusMaxBlocks = 2048;
constexpr u32 kCorpusNoSet = 0xffffffffu;
constexpr int kCorpusLdsSegs = 2048;  // the resolve kernel stages a table of up to this many
                                      // segments in LDS (8 KiB); a longer one is read from
                                      // global memory
struct CorpusSets {
  CorpusCounters* ctr = nullptr;
  u32* table = nullptr;
  u32* ids = nullptr;      // [seg_cap] the segments' ids, uploaded with the table
  u32* q_set = nullptr;
  u32* bitmaps = nullptr;
  u64 seg_cap = 0, set_cap = 0;
};
u64 corpus_sets_bytes(u64 seg_cap, u64 set_cap);
// Carves `base` (corpus_sets_bytes bytes, 256-B aligned); c == nullptr: only *bytes.
void corpus_sets_carve(char* base, u64 seg_cap, u64 set_cap, CorpusSets* c, u64* bytes = nullptr);
// restrict + seal over the `hits` pairs in h.pairs (b.ctr->written == hits): b.q_hits rebuilt,
// b.ctr->written and sort_n the kept pairs, c.ctr complete when `s` has drained.  The kept
// pairs are h.pairs afterwards: the launcher swaps h.pairs and h.cands.
void launch_corpus_restrict(const SearchIndex& ix, const SearchBatch& b, const CorpusSets& c,
                            u32 segments, u32 sets, u32 queries, u64 hits, SearchHits& h,
                            hipStream_t s);
// The by-file stage (engine.hpp "answers by file") behind emit / top, over the E returned lines
// h.lines[0 .. E) and their per-query offsets [Q + 1]:
//   resolve  one returned line per thread: its query by binary search in the offsets, its
//            segment by the restrict stage's binary search -- in a copy of the table staged in
//            LDS while S <= kCorpusLdsSegs, in global memory above that -- then line_file (the
//            id), line_local (line - first_line + base; only the first segment has a base) and
//            the key query << 32 | segment ordinal
//   order    (ranked only: unranked keys ascend already) radix_sort() of the keys
//   heads    a key that differs from the one before it heads a run.  Three kernels, data crossing
//            at the kernel boundaries only: the heads of every tile of kCorpusTile keys counted,
//            one workgroup scans the tile array (the total: `runs`), then every head takes its
//            place from a workgroup scan inside its tile, finds its run's end by binary search
//            (as tally.hip's run heads do) and writes one (id, count) and its key.  No atomics
//            on any output
//   offsets  one thread per query: file_off[q] = the lower bound of q << 32 among the run keys
// The arrays are one allocation, grown by the batch's returned lines (40 B each).
struct CorpusByFile {
  CorpusCounters* ctr = nullptr;  // zeroed per by-file batch
  u64* keys = nullptr;        // [cap]
  u64* sorted = nullptr;      // [cap] ranked: the sorted keys
  u64* run_keys = nullptr;    // [cap] a run's key, in CSR order
  u64* tile_val = nullptr;    // [ceil(cap / kCorpusTile) + 1]
  u64* file_off = nullptr;    // [kSearchMaxQueries + 1]
  u32* line_file = nullptr;   // [cap] parallel to h.lines
  u32* line_local = nullptr;  // [cap]
  u32* file_ids = nullptr;    // [cap] the CSR: ids ascending per query
  u32* file_counts = nullptr; // [cap]
  u64 cap = 0;
};
void corpus_by_file_carve(char* base, u64 cap, CorpusByFile* f, u64* bytes = nullptr);
// offsets: the returned lines' per-query offsets on the device ([queries + 1], offsets[queries]
// == lines).  base0: the first segment's base.  f.ctr->runs, f.file_off and the outputs are
// complete when `s` has drained; a ranked batch of more than kSmallSortMax lines synchronises
// `s` once, as radix_sort does.
void launch_corpus_by_file(const CorpusSets& c, u32 segments, u64 base0, const u64* offsets,
                           u32 queries, u64 lines, bool ranked, SearchHits& h, CorpusByFile& f,
                           SortPlan* h_plan, hipStream_t s);

// ---------------- expr.hip ----------------
// `expr` queries (engine.hpp "boolean expressions"): a batch that has one carries, in an
// allocation of its own made by the engine's first such batch, these u32 words.  The first two
// parts are uploaded per batch (kSearchMaxQueries + Q * 8 words), the rest written by the plan:
//   alias  [kSearchMaxQueries] the host's identification of the query's pattern slots: bits
//          24 + t: term t is a pattern slot; bits 3 t .. 3 t + 2 of such a slot: the query's
//          first term with an equal pattern (itself, mostly).  0 for a query of another mode
//   truth  [kSearchSlots] query q's truth table in words q * 8 .. q * 8 + 7
//   plan   [kSearchMaxQueries] S | P << 8: the walked set and the present terms
//   src    [kSearchMaxQueries] bits 3 t .. 3 t + 2: the query's first term with term t's list
//   bound  [kSearchMaxQueries] the elements the query walks: the lengths of S's lists
//   start  [kSearchMaxQueries + 1] u64: the exclusive scan of bound; start[Q] = the batch's E
//          (also, saturated, in SearchCounters::ebound: the lookup's readback brings it)
// The lookup treats an `expr` query (q_meta: kSearchExpr | kSearchAny) as `any` over all its
// terms, which gives t_val, t_len, x_len and the score mask.  Then, for such a batch only:
//   plan     expr_plan_kernel, one workgroup, one thread per query, between the lookup and the
//            scan of the bounds, so before the expand stage rewrites t_val.  src: a pattern slot takes the
//            host's identification; any other present term the first earlier non-pattern term
//            with equal t_val and t_len (the same CSR range: the same words).  A wide term that
//            repeats an earlier term's words is not merged, so its own t_val names an unsorted
//            concatenation: every later reader goes through src.  S: the greedy choice of
//            engine.hpp "the walked set" -- "some m inside U has truth[m] set" is eight masked
//            word tests on the table in registers.  bound = the summed lengths of S's lists
//            (past 32 bits: ctr->anyover, as `any`); q_bound[q] = 0, so search_hit_kernel never
//            sees the query.  A query of another mode gets bound 0 here.  The same pass scans
//            the bounds into start[0 .. Q] (a block scan per 256 queries, the carry in a
//            register) and leaves E in ctr->ebound: one launch, no copy of its own
//   (the host reads E with the lookup's readback; B + E sizes the hit workspace and joins the
//   batch's 2^32 check)
//   hits     expr_hit_kernel, in front of search_hit_kernel: the element space [0, E) in tiles of
//            kSearchTile, grid-stride.  An element finds its query by a binary search in start,
//            then its term of S and its position in that term's list.  It counts when it is the
//            first of its line in the list and no earlier list of S holds the line; its mask
//            comes from list_has over the other present terms (each distinct list searched
//            once), and the table bit decides.  Hits go through commit_hits into the same
//            pairs and q_hits: seal, order, emit, rank and show run unchanged.  No polled word,
//            no LDS, no scratch
constexpr u64 kExprAlias = 0;
constexpr u64 kExprTruth = kExprAlias + kSearchMaxQueries;
constexpr u64 kExprPlan = kExprTruth + kSearchSlots;
constexpr u64 kExprSrc = kExprPlan + kSearchMaxQueries;
constexpr u64 kExprBound = kExprSrc + kSearchMaxQueries;
constexpr u64 kExprStart = kExprBound + kSearchMaxQueries;  // (u64 words: an even offset)
constexpr u64 kExprEnd = kExprStart + 2 * ((u64)kSearchMaxQueries + 1);
static_assert(kExprStart % 2 == 0, "start holds u64 words");
inline u64 search_expr_bytes() { return kExprEnd * sizeof(u32); }
inline u64 search_expr_upload_bytes(u32 queries) {
  return (kExprTruth + (u64)queries * kSearchMaxTerms) * sizeof(u32);
}
LOCUST_HD inline const u64* search_expr_start(const u32* expr) {
  return reinterpret_cast<const u64*>(expr + kExprStart);
}
// plan and scan in one launch (called by launch_search_lookup for a batch with b.expr).
void launch_expr_plan(const SearchBatch& b, u32 queries, hipStream_t s);
// hits over the `ebound` elements the plan reported (b.expr's start[Q]); before
// launch_search_hits, whose seal closes the batch's hits.  ebound + the plain bound <= h.cap.
void launch_expr_hits(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 ebound,
                      const SearchHits& h, hipStream_t s);

// ---------------- show.hip ----------------
// The show stage of a search batch (engine.hpp "show"): for each of the E returned lines, in
// result order (h.lines; the per-query segments in b.offsets, ranked: b.out_off), the line's
// first N bytes and the spans of its emitted tokens that match a positive term of the entry's
// query.  Everything it reads is resident: the text, nl_pos, the batch's keys and pattern
// arrays, the returned lines.
//   measure  one wave per entry, up to 64 consecutive entries per wave and round (lane i finds
//            entry i's query by a binary search in the offsets; the query's keys go to the
//            wave's LDS, reloaded only when the query changes).  The verify kernels' walk, 64
//            bytes per step with the 32-byte look-ahead row: the step's matching emitted tokens
//            are counted by ballot and popcount.  Per entry n_spans and t_len = min(line
//            length, N); the lines longer than N count in ShowCounters::cut
//   scan     one workgroup: exclusive u64 scans of both arrays into span_off and text_off
//            [E + 1]; the totals also to ShowCounters::spans and ::text
//   (the host reads the counters: it sizes, or refuses, the payload)
//   write    the same walk: a step's spans go to span_off[i] + (spans so far) + lanes_below;
//            a token that runs past its step stays open, wave-uniformly, and its length is
//            written when a later step (or the line's end) closes it; the step's 64 bytes go to
//            text_off[i] + the step's offset while below t_len.  Every word is written once, at
//            a determined place: no atomics, no compaction.  An entry whose spans do not number
//            what measure counted adds to ShowCounters::mismatch (the host throws)
// A batch that has a pattern term runs the siblings compiled with the matcher
// (show_globmeasure_kernel, show_globwrite_kernel); one with a fuzzy term fuzzy.hip's, one
// with a regex term regex.hip's.
struct ShowCounters {  // zeroed per show batch
  u64 text;       // T: the payload's text bytes
  u64 spans;      // S: its span triples
  u32 cut;        // entries whose line is longer than N
  u32 mismatch;   // write: entries whose spans do not number what measure counted
  u32 pad[2];
};
static_assert(sizeof(ShowCounters) == 32, "one readback");
// The stage's arrays: the per-entry part (sized by E) and the payload (sized by T and S), two
// allocations of the engine's, grown on demand.
struct ShowBuffers {
  ShowCounters* ctr = nullptr;
  u32* n_spans = nullptr;   // [E]
  u32* t_len = nullptr;     // [E]
  u64* span_off = nullptr;  // [E + 1]
  u64* text_off = nullptr;  // [E + 1]
  u64 cap_entries = 0;
  char* text = nullptr;     // [cap_text]
  u32* spans = nullptr;     // [cap_spans][3]: start, len, mask
  u64 cap_text = 0, cap_spans = 0;
};
u64 show_entry_bytes(u64 entries);
void show_entry_carve(char* base, u64 entries, ShowBuffers* sb);
// measure + scan over the `entries` lines at `lines` (offsets: [queries + 1], their per-query
// segments).  sb.ctr is complete when `s` has drained.
void launch_show_measure(const SearchIndex& ix, const SearchBatch& b, u32 queries,
                         const u32* lines, const u64* offsets, u64 entries, u32 show,
                         const ShowBuffers& sb, hipStream_t s);
// write: sb.text[0 .. T) and sb.spans[0 .. 3 S) (T <= sb.cap_text, S <= sb.cap_spans).
void launch_show_write(const SearchIndex& ix, const SearchBatch& b, u32 queries, const u32* lines,
                       const u64* offsets, u64 entries, const ShowBuffers& sb, hipStream_t s);

// ---------------- tally.hip ----------------
// The tally stage of a search batch (engine.hpp "tally: the words of the returned lines"): for
// every query the K most frequent index words of its returned lines.  It reads what the show
// stage reads -- the text, nl_pos, the returned lines (h.lines) and their per-query segments
// (b.offsets, ranked: b.out_off) -- and the key-ordered records; it is independent of how the
// lines were found, so one set of kernels serves every batch (no matcher siblings).
// A sequence of kernels on `s`; data moves between workgroups only across the kernel boundaries
// (the radix sort it reuses keeps its own look-back), no polled word:
//   measure  one wave per entry, up to 64 consecutive entries per wave and round: index.hip's
//            counting walk (step_starts ballots, the emit cap).  Per entry n_tok
//   scan     one workgroup: tok_off[0 .. E] = exclusive u64 scan of n_tok, the total T to
//            TallyCounters::tokens
//   (the host reads the counters: it sizes, or refuses, the workspace and fixes the key split)
//   map      the same walk with the look-ahead row: every emitted token's key is packed
//            (pack_row_key) and ranked (find_rank); token `ord` of entry i, which belongs to
//            query q (lane i's binary search in the offsets), writes the pair word
//            q << 32 | rank at tok_off[i] + ord.  Every word is written once at a determined
//            place, below the entry's end and the capacity: no atomics on the output.  A key not
//            among the records counts in `miss`, an entry whose tokens do not number what
//            measure counted in `mismatch` (the host throws for either)
//   seal     one thread: sort_n = T when the map agreed with the measure pass and the index,
//            else 0 -- the sort never runs over words nobody wrote
//   order    radix_sort() of the pair words as one-word keys: (query, rank)
//   runs     one thread per sorted word.  A run head (j == 0 or s[j] != s[j - 1]) finds its
//            run's end by an upper-bound binary search of its own word in the sorted array (a
//            run of `the` is thousands long: never walked) and writes the rank key
//            q << 54 | (cmask - count) << r | rank; its slot comes from one atomic per wave
//            (ballot + popcount) on TallyCounters::runs, in arbitrary order: the next sort
//            decides.  One more atomic per wave and distinct query counts the query's words
//            (q_words), which the host reads with U = runs: they size what comes back
//   (the host reads U and q_words: the second sort takes its regime from U, as the search's
//   order stage takes its from the hits)
//   order    radix_sort() of the U rank keys: (query, count descending, rank ascending); the
//            keys are distinct, so the order is total
//   offsets  one workgroup: run_off[q] = the lower bound of q << 54 among the sorted keys
//            (run_off[Q] = U), words[q] their difference, out_off = the exclusive scan of
//            min(K, words), tokens[q] = tok_off[offsets[q + 1]] - tok_off[offsets[q]]
//   top      one thread per sorted key at j: pos = j - run_off[q]; when pos < K the record
//            {recs[rank].w[0 .. 3], count} goes to out[out_off[q] + pos].  A key whose query or
//            rank is out of range, whose count is 0 or which lies outside its query's run_off
//            range counts as misplaced (the host throws).  No atomics on the output
struct TallyCounters {  // zeroed per tally batch
  u64 tokens;     // T: the emitted tokens of the returned lines = the pair words
  u32 miss;       // map: emitted tokens whose key is not among the records
  u32 mismatch;   // map: entries whose tokens do not number what measure counted
  u32 sort_n;     // pair words handed to the first sort: T if the map agreed, else 0
  u32 runs;       // U: the distinct (query, word) runs = the rank keys
  u32 misplaced;  // runs or sorted rank keys that name no query, no word, no count or lie
                  // outside their query's range
  u32 pad[9];
};
static_assert(sizeof(TallyCounters) == 64, "one readback");
// (the rank key's split: TallyKeySplit, tally_key_split -- engine.hpp, a pure host function)
// The stage's arrays: the per-entry and per-query part (sized by E) and the pair part (sized by
// T and the records that come back), two allocations of the engine's, made by its first tally
// batch and grown on demand.
struct TallyBuffers {
  char* zero = nullptr;      // [TallyCounters | q_words], zeroed per tally batch
  u64 zero_bytes = 0;
  TallyCounters* ctr = nullptr;
  u32* q_words = nullptr;    // [kSearchMaxQueries] the runs kernel's count of each query's words
  u32* n_tok = nullptr;      // [E]
  u64* tok_off = nullptr;    // [E + 1]
  u64* run_off = nullptr;    // [kSearchMaxQueries + 1]
  u64* words = nullptr;      // [kSearchMaxQueries] tally_words
  u64* tokens = nullptr;     // [kSearchMaxQueries] tally_tokens
  u64* out_off = nullptr;    // [kSearchMaxQueries + 1]
  u64 cap_entries = 0;
  u64* pairs = nullptr;      // [cap_pairs] the pair words; behind the first sort: the rank keys
  u64* zeros = nullptr;      // [cap_pairs] zero: key words 1..3 of the sorts
  u64* sorted = nullptr;     // [cap_pairs] the sorted pair words; behind the runs: the rank keys
  u64* spare = nullptr;      // [cap_pairs]
  OutRecord* out = nullptr;  // [cap_out] the winners' records
  RadixWorkspace rx{};
  u64 cap_pairs = 0, cap_out = 0;
};
u64 tally_entry_bytes(u64 entries);
void tally_entry_carve(char* base, u64 entries, TallyBuffers* tb);
u64 tally_pair_bytes(u64 pairs, u64 out);
// Carves `base` (tally_pair_bytes(...) bytes, 256-B aligned).  The caller zeroes tb->zeros once.
void tally_pair_carve(char* base, u64 pairs, u64 out, TallyBuffers* tb);
// measure + scan over the `entries` lines at `lines`.  tb.ctr->tokens is complete when `s` has
// drained.
void launch_tally_measure(const SearchIndex& ix, const u32* lines, u64 entries,
                          const TallyBuffers& tb, hipStream_t s);
// map + seal + order + runs over the `tokens` pair words the measure pass reported (tokens <=
// tb.cap_pairs; offsets: [queries + 1], the entries' per-query segments).  tb.ctr and tb.q_words
// are complete when `s` has drained.  More than kSmallSortMax pair words read the sort's plan
// back through h_plan and synchronise `s` once, as radix_sort does.
void launch_tally_map(const SearchIndex& ix, u32 queries, const u32* lines, const u64* offsets,
                      u64 entries, u64 tokens, const TallyKeySplit& ks, TallyBuffers& tb,
                      SortPlan* h_plan, hipStream_t s);
// order + offsets + top over the `runs` rank keys the runs kernel wrote (runs <= tb.cap_pairs):
// tb.words, tb.tokens, tb.out_off, tb.out[0 .. out_off[queries]) and tb.ctr->misplaced.
// Synchronises as launch_tally_map does.
void launch_tally_top(const SearchIndex& ix, u32 queries, const u64* offsets, u64 runs, u32 k,
                      const TallyKeySplit& ks, TallyBuffers& tb, SortPlan* h_plan, hipStream_t s);

// ---------------- fuzzy.hip ----------------
// The kernels of a batch that has a fuzzy term (engine.hpp "fuzzy terms"; SearchBatch::fuzzy):
// the bodies search.hip and show.hip instantiate (device/dictscan.hpp, device/verify.hpp,
// device/showwalk.hpp), compiled once more with the fuzzy matcher (device/fuzzy.hpp) beside the
// pattern matcher -- such a batch may hold pattern terms and the fold as well:
//   match    fuzzy_match_kernel: the dictionary scan; a fuzzy slot's words are the keys within
//            its budget of its word
//   scatter  fuzzy_scatter_kernel: the same walk and match over the wide slots
//   phrase   fuzzy_phrase_kernel, near: fuzzy_near_kernel: a token matches a fuzzy term when
//            its cut key is within the budget of the word, under the batch's fold
//   show     fuzzy_showmeasure_kernel, fuzzy_showwrite_kernel: the same token rule
// launch_search_lookup, launch_search_expand, launch_search_hits, launch_show_measure and
// launch_show_write call these in place of their own kernels for such a batch, with the grids
// and arguments of the siblings they replace; every other batch launches none of them.
void launch_fuzzy_match(const SearchIndex& ix, const SearchBatch& b, u32 queries, hipStream_t s);
void launch_fuzzy_scatter(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          const SearchHits& h, hipStream_t s);
void launch_fuzzy_phrase(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                         const SearchHits& h, hipStream_t s);
void launch_fuzzy_near(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                       const SearchHits& h, hipStream_t s);

// ---------------- regex.hip ----------------
// The kernels of a batch that has a regex term (engine.hpp "regex terms"; SearchBatch::regex):
// the same bodies a third time, with the regex matcher (device/regex.hpp) beside the pattern and
// the fuzzy matcher -- such a batch may hold pattern and fuzzy terms and the fold as well.  Every
// kernel takes the batch's program table; a regex slot's meta word indexes it:
//   match    regex_match_kernel: the dictionary scan, one key per lane; a regex slot's words are
//            the keys its program accepts
//   scatter  regex_scatter_kernel: the same walk and match over the wide slots
//   phrase   regex_phrase_kernel, near: regex_near_kernel: one token per lane; a token matches a
//            regex term when the program accepts its cut key
//   show     regex_showmeasure_kernel, regex_showwrite_kernel: the same token rule
// The programs are read from global memory: first, last, follow[] and the position count by
// scalar loads (the program is wave-uniform), B[] through the vector cache, each lane by its own
// byte.  Nothing is staged in LDS: a program is 1168 bytes that every wave of a launch reads
// over and over, so it stays in the caches, while a staged copy would cost the scan a workgroup
// barrier pair per (tile, slot) and the walks up to eight tables per wave.
// A regex batch's launch functions call these in place of their own kernels (before the fuzzy
// siblings), with the grids and arguments of the siblings they replace; every other batch
// launches none of them.
void launch_regex_match(const SearchIndex& ix, const SearchBatch& b, u32 queries, hipStream_t s);
void launch_regex_scatter(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          const SearchHits& h, hipStream_t s);
void launch_regex_phrase(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                         const SearchHits& h, hipStream_t s);
void launch_regex_near(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                       const SearchHits& h, hipStream_t s);

// ---- device self-test of the string library (tests only; StringTestOut in engine.hpp) ----
void launch_string_selftest(const char* blob, const u32* off, u32 n, const char* delims,
                            const int* ints, StringTestOut* out, hipStream_t s);

// ---------------- code-object warm-up ----------------
// The runtime loads a file's code object at the first launch of one of its kernels (lazy
// loading); a one-shot job would pay that inside its first kernels.  warm_kernel_modules()
// loads every kernel file of this library up front (engine construction) -- and only them:
// HIP_ENABLE_DEFERRED_LOADING=0 would also load the RCCL library's device code (a
// 573 MB fat binary), +1.3 GB of host memory and ~150 ms per process.
void warm_module_append();  // (as index: the code object only, no buffers)
void warm_module_corpus();  // (as search: the code object only, no buffers)
void warm_module_dict();
void warm_module_drop();  // (as append)
void warm_module_exchange();
void warm_module_expr();  // (as search: the code object only, no buffers)
void warm_module_fuzzy();  // (as search: the code object only, no buffers)
void warm_module_regex();  // (as fuzzy)
void warm_module_index();  // (as topk below: the code object only, no buffers)
void warm_module_map();
void warm_module_merge();
void warm_module_ngram();
void warm_module_partplan();
void warm_module_psort();
void warm_module_radix_sort();
void warm_module_reduce();
void warm_module_search();  // (as index: the code object only, no buffers)
void warm_module_show();  // (as search: the code object only, no buffers)
void warm_module_shuffle();
void warm_module_signal();
void warm_module_tally();  // (as show: the code object only, no buffers)
void warm_module_tokenize();
// The selection's code object is loaded with the others (every kernel file is: a first top
// job does no one-time loading either, tests/test_cold_path.py); its workspace and pinned
// buffer are made by an engine's first top job only.
void warm_module_topk();
inline void warm_kernel_modules() {
  warm_module_append();
  warm_module_corpus();
  warm_module_dict();
  warm_module_drop();
  warm_module_exchange();
  warm_module_expr();
  warm_module_fuzzy();
  warm_module_regex();
  warm_module_index();
  warm_module_map();
  warm_module_merge();
  warm_module_ngram();
  warm_module_partplan();
  warm_module_psort();
  warm_module_radix_sort();
  warm_module_reduce();
  warm_module_search();
  warm_module_show();
  warm_module_shuffle();
  warm_module_signal();
  warm_module_tally();
  warm_module_tokenize();
  warm_module_topk();
}

}  // namespace locust
