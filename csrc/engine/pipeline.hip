// Out-of-line members of DevicePipeline (csrc/engine/pipeline.hpp): the engine's host-side
// job logic -- construction and sizing, uploads, the map / Process / Reduce enqueue paths,
// partition-map retuning, graph capture, streaming and the result hand-over -- compiled once
// here instead of in every translation unit that includes the header.
#include "pipeline.hpp"

#include <map>

#include "locust/device/fuzzy.hpp"
#include "locust/device/regex.hpp"

namespace locust {
namespace detail {

u64 DevicePipeline::piece_target() {
  static const u64 b = [] {
    const char* e = std::getenv("LOCUST_PIECE_MB");
    const long mb = e ? std::atol(e) : 10;
    return (u64)std::max<long>(mb, 4) << 20;
  }();
  return b;
}

u64 DevicePipeline::pinned_bytes() const {
  u64 b = 0;
  if (h_text) b += cap_bytes + 64;
  for (const auto& o : out_pool) b += o->cap * sizeof(OutRecord) + kDictParts * sizeof(u64);
  for (int k = 0; k < 2; ++k)
    if (h_stage[k]) b += cap_bytes + 64;
  for (int i = 0; i < kRingPieces; ++i)
    if (h_ring[i]) b += ring_piece + 64;
  b += h_keys_cap * kKeyWords * sizeof(u64);
  b += h_chunk_cap * sizeof(MapCounters);
  if (h_top) b += (kTopKMax + 1) * sizeof(TopRecord);
  if (h_ictr) b += h_post_cap * sizeof(u32) + sizeof(IndexCounters);
  if (h_supload)
    b += search_upload_bytes(kSearchMaxQueries, true) + h_slines_cap * sizeof(u32) +
         ((u64)kSearchMaxQueries * (kSearchMaxTerms * 4 + 8 + 4) + 72);
  b += 2 * sizeof(MapCounters) + sizeof(SortPlan) + 2 * sizeof(PartMapTables) +
       kMaxSamples * sizeof(PackedKey) + (kMaxRanks + 8) * sizeof(u64) + 64 +
       kDictParts * sizeof(u32);
  return b;
}

void DevicePipeline::issue_piece_copies(const char* src) {
  ensure_piece_events(pieces.size());
  for (size_t k = 0; k < pieces.size(); ++k) {
    const u64 off = pieces[k].first, len = pieces[k].second;
    hipStream_t cs = piece_stream(k);
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_text + off, src + off, len, hipMemcpyHostToDevice, cs));
    LOCUST_HIP_CHECK(hipEventRecord(ev_piece[k], cs));
  }
  pieces_issued = true;
}

void DevicePipeline::ensure_plan() {
  if (d_plan) return;
  const u64 slots = 2 * kPlanCap;  // load factor <= 0.5
  const u64 ctr_b = align_up(sizeof(MapCounters), 256), tab_b = align_up(slots * sizeof(DictSlot), 256);
  plan_zero_bytes = ctr_b + tab_b + kPlanCap * 8;
  const u64 total = plan_zero_bytes + 256 + (4 + 4 + 1) * kPlanCap * 8 + kPlanCap * 4 + 4096;
  LOCUST_HIP_CHECK(hipMalloc(&d_plan, total));
  char* c = d_plan;
  d_plan_ctr = reinterpret_cast<MapCounters*>(c);
  plan_dict.table = reinterpret_cast<DictSlot*>(c + ctr_b);
  plan_dict.ucount = reinterpret_cast<u64*>(c + ctr_b + tab_b);
  c = d_plan + align_up(plan_zero_bytes, 256);
  for (int j = 0; j < kKeyWords; ++j, c += kPlanCap * 8) plan_dict.ukeys.w[j] = reinterpret_cast<u64*>(c);
  for (int j = 0; j < kKeyWords; ++j, c += kPlanCap * 8) plan_keys.w[j] = reinterpret_cast<u64*>(c);
  plan_dict.uval = reinterpret_cast<u64*>(c);
  c += kPlanCap * 8;
  plan_dict.urank = reinterpret_cast<u32*>(c);
  plan_dict.mask = (u32)(slots - 1);
  plan_dict.ucap = (u32)kPlanCap;
}

void DevicePipeline::enqueue_devplan(const char* host, u64 len0, const DelimMask& dm,
                       const char* dev_text) {
  u64 n = std::min<u64>(len0, kPlanSampleBytes);
  if (n < len0) {
    const void* nl = memrchr(host, '\n', (size_t)n);
    if (nl) n = (u64)(static_cast<const char*>(nl) - host) + 1;
  }
  launch_map_fast(dev_text ? dev_text : d_text, n, dm, cfg.emits_per_line, cfg.max_key_len,
                  plan_keys, nullptr, kPlanCap, d_plan_ctr, lb_map, stream, nullptr, nullptr,
                  PartMap{}, false, nullptr, nullptr, nullptr, cfg.ngram);
  launch_dict_insert(plan_keys, nullptr, &d_plan_ctr->num_records, kPlanCap, plan_dict,
                     d_plan_ctr, stream);
  launch_part_plan(plan_dict.ukeys.w[0], plan_dict.ucount, &d_plan_ctr->num_unique,
                   plan_dict.ucap, d_pmap, stream);
}

void DevicePipeline::warm_modules_once(int device) {
  static std::mutex mu;
  static u64 warmed = 0;  // bit per device
  std::lock_guard<std::mutex> lk(mu);
  const u64 bit = 1ull << (device & 63);
  if (warmed & bit) return;
  warm_kernel_modules();
  // the first roctx range of a process initialises the library (~0.12 ms, measured inside
  // a fresh engine's first job): pay it here
  { TraceRange warm("locust:warm"); }
  warmed |= bit;
}

// The arena's layout for a planned pass: the same sequence of buffers the constructor
// takes, so plan_device_pass prices an engine exactly before it exists.
DevicePipeline::ArenaShape DevicePipeline::shape_arena(const JobConfig& cfg, const DevicePassPlan& p,
                                                       u64 small_pass_bytes) {
  ArenaShape sh;
  const bool compat = cfg.map_path == MapPath::kCompat;
  const u64 cap_bytes = p.chunk_bytes, pass_bytes = p.pass_bytes, cap_lines = p.cap_lines;
  const u64 cap = p.cap, ucap = p.ucap, rcap = p.rcap;
  const bool streaming = p.streaming;
  // the reference algorithm's head buffers (boundary mark, prefix, adjacent difference):
  // a dictionary engine whose sort buffers hold its distinct keys only never reduces
  // that way until ensure_radix_full makes them
  const u64 hcap = rcap < cap ? 1 : rcap;
  sh.slot_cap = compat ? cap_lines * (u64)cfg.emits_per_line : 1;
  sh.t_line = div_up(pass_bytes, kLineIdxTile) + 1;
  sh.t_compact = div_up(cap_lines, 256) + 1;
  sh.t_map = div_up(pass_bytes, kMapTileBytesMin) + 1;
  sh.t_heads = div_up(cap, kReduceTile) + 1;
  sh.t_scan = div_up(cap, kReduceTile) + 1;
  sh.rx_zero_words = radix_zero_bytes(rcap) / 4;
  // Hash table: >= 2x the distinct keys it can see (load factor <= 0.5), capped at
  // 2^25 slots (16M distinct keys per call; beyond that the radix path takes over).
  sh.dict_slots = 1024;
  while (sh.dict_slots < 2 * ucap) sh.dict_slots <<= 1;
  // [table | ucount | uval | rank]
  sh.dict_zero_bytes = align_up(sh.dict_slots * sizeof(DictSlot), 256) +
                       2 * align_up(ucap * 8, 256) + ucap * 4;
  sh.rx_part_words = (u64)radix_hist_blocks(rcap) * kNumPositions * 256;
  sh.sync_bytes = 256 + 8 * (sh.t_line + sh.t_compact + sh.t_map + sh.t_heads + sh.t_scan +
                             kDictParts + 1);

  SizingPlan sz;
  sz.add<char>(cap_bytes + 64);
  sz.add<u64>(compat ? cap_lines + 1 : 1);  // the line index: compat map only
  sz.add<char>(64);
  for (int j = 0; j < kKeyWords; ++j) {
    sz.add<u64>(sh.slot_cap);
    sz.add<u64>(cap);   // tokens
    sz.add<u64>(rcap);  // sorted
    sz.add<u64>(hcap);  // heads
  }
  sz.add<u32>(compat ? cap_lines : 1);
  sz.add<u64>(cap);   // d_counts (per token)
  sz.add<u64>(rcap);  // d_sorted_counts
  for (int k = 0; k < 3; ++k) sz.add<u64>(hcap);  // d_prefix, d_head_val, d_head_count
  sz.add<u32>(rcap);
  sz.add<u8>(align_up(cap, 16) + 16);
  // A pass of at most small_pass_bytes (1 KiB tiles <= kPartBlock: the in-job plan's
  // range) takes the one-kernel ordered build whatever its worst-case token count: natural
  // text has a third of the tokens the capacity allows, and the large build's device plan
  // cost ~0.2 ms of a 0.3 ms untuned job at 3-5x Hamlet (docs/PERFORMANCE.md round 5).
  sh.small_pass = cap > kPartBuildMaxTokens && cap_bytes <= small_pass_bytes && !streaming &&
                  cfg.map_path == MapPath::kFast && cfg.sort_path == SortPath::kDict;
  if ((cap <= kPartBuildMaxTokens || sh.small_pass) && cap_bytes < kMapLargeInput) {
    sh.part_off_tiles = div_up(cap_bytes, kMapTileBytesMin);
  } else if (!streaming && cfg.map_path == MapPath::kFast && cfg.sort_path == SortPath::kDict) {
    // large single passes (the two-kernel ordered build): 1 KiB tiles below
    // kMapLargeInput, 4 KiB tiles (whole inputs or upload pieces) above
    sh.part_off_tiles =
        std::max<u64>(div_up(std::min<u64>(cap_bytes, kMapLargeInput), kMapTileBytesMin),
                      div_up(cap_bytes, kMapTileBytesLarge) + kMaxPieces);
    sh.large_ordered = cap > kPartBuildMaxTokens;
  }
  if (sh.part_off_tiles) sz.add<u32>(sh.part_off_tiles * kPartTable);
  if (sh.part_off_tiles) sz.add<u32>(sh.part_off_tiles * kPartOccWords);
  sh.partial_slots_cap = sh.large_ordered
                             ? (u32)std::clamp<u64>(div_up(cap_bytes, kPieceBytes) + 3,
                                                    kOrdWorkers, kMaxPartialSlots)
                             : 0u;
  const u64 partial_slots = (u64)kDictParts * sh.partial_slots_cap;
  if (partial_slots) {
    sz.add<KeyCount>(partial_slots * kPartSlotsHost);
    sz.add<u32>(partial_slots);
  }
  sz.add<OutRecord>(rcap);
  sz.add<KeyCount>(std::max<u64>(cap, kSlotRecordsMin) + kSlotHeaderRecords);  // d_records
  sz.add<PackedKey>(kMaxSamples);
  sz.add<PackedKey>(kMaxRanks);
  sz.add<u64>(kMaxRanks + 1);
  sz.add<u64>(1);
  sz.add<char>(sh.sync_bytes);
  sz.add<u32>(sh.rx_zero_words);
  sz.add<u32>(sh.rx_part_words);
  sz.add<SortPlan>(1);
  for (int b = 0; b < 2; ++b) {
    sz.add<u64>(rcap);
    sz.add<u32>(rcap);
  }
  for (int j = 0; j < kKeyWords; ++j) sz.add<u64>(ucap);
  sz.add<char>(sh.dict_zero_bytes);
  sh.arena_bytes = align_up(sz.bytes + 4096, kDevPageBytes);
  return sh;
}

// The every-token sort / reduce buffers a dictionary engine leaves out of its arena
// (rcap == ucap): sorted and head keys, sorted counts, prefix, head val / count, the
// permutation, the output records and the radix scratch, at cap.
static u64 radix_full_bytes(u64 cap) {
  SizingPlan sz;
  for (int j = 0; j < kKeyWords; ++j) {
    sz.add<u64>(cap);
    sz.add<u64>(cap);
  }
  for (int k = 0; k < 4; ++k) sz.add<u64>(cap);
  sz.add<u32>(cap);
  sz.add<OutRecord>(cap);
  sz.add<u32>(radix_zero_bytes(cap) / 4);
  sz.add<u32>((u64)radix_hist_blocks(cap) * kNumPositions * 256);
  for (int b = 0; b < 2; ++b) {
    sz.add<u64>(cap);
    sz.add<u32>(cap);
  }
  return align_up(sz.bytes + 4096, DevicePipeline::kDevPageBytes);
}

void DevicePipeline::ensure_radix_full() {
  if (rcap >= cap) return;
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  LOCUST_HIP_CHECK(hipStreamIsCapturing(stream, &cst));
  LOCUST_CHECK_ARG(cst == hipStreamCaptureStatusNone,
                   "internal: the every-token sort buffers must exist before a capture");
  const u64 bytes = radix_full_bytes(cap);
  LOCUST_LOG_INFO("dictionary engine enters the every-token sort: +%.1f MiB of device memory",
                  bytes / 1048576.0);
  sync();  // nothing in flight may still use the buffers being replaced
  for (auto& g : dict_graphs) LOCUST_HIP_CHECK(hipGraphExecDestroy(g.exec));
  dict_graphs.clear();
  for (auto& g : graph_cache) LOCUST_HIP_CHECK(hipGraphExecDestroy(g.exec));
  graph_cache.clear();
  size_t got = 0;
  radix_base = static_cast<char*>(dev_block_alloc(bytes, &got));
  radix_block = got;
  Arena a;
  a.base = radix_base;
  a.size = bytes;
  for (int j = 0; j < kKeyWords; ++j) {
    sorted.w[j] = a.take<u64>(cap);
    heads.w[j] = a.take<u64>(cap);
  }
  d_sorted_counts = a.take<u64>(cap);
  d_prefix = a.take<u64>(cap);
  d_head_val = a.take<u64>(cap);
  d_head_count = a.take<u64>(cap);
  d_perm = a.take<u32>(cap);
  d_out = a.take<OutRecord>(cap);
  const u64 zw = radix_zero_bytes(cap) / 4;
  rx.cap = cap;
  rx.tile_counters = a.take<u32>(zw);
  rx.status = rx.tile_counters + kNumPositions;
  rx.hist_part = a.take<u32>((u64)radix_hist_blocks(cap) * kNumPositions * 256);
  for (int b = 0; b < 2; ++b) {
    rx.keys[b] = a.take<u64>(cap);
    rx.vals[b] = a.take<u32>(cap);
  }
  LOCUST_HIP_CHECK(hipMemsetAsync(rx.tile_counters, 0, zw * 4, stream));
  rcap = cap;
  ++layout_gen;
}

u64 DevicePipeline::device_bytes() const {
  u64 b = arena.size + (radix_base ? radix_full_bytes(cap) : 0);
  if (d_text_alt) b += cap_bytes + 64;
  if (d_plan) b += plan_zero_bytes;  // (+ the plan's key arrays: small)
  b += topk_bytes;                   // (0 until the first top job)
  b += index_bytes;                  // (0 until the first index job)
  b += sbatch_bytes + shits_bytes;   // (0 until the first search job)
  b += sbatch.merged_cap * sizeof(u32);  // (0 until a batch merges a prefix term's lists)
  b += store_bytes();                    // (0 until the first append)
  return b;
}

DevicePipeline::DevicePipeline(const JobConfig& c, u64 max_bytes, u64 max_lines, u64 cap_records)
    : cfg(c) {
  LOCUST_CHECK_ARG(cfg.emits_per_line > 0, "emits_per_line must be > 0");
  LOCUST_CHECK_ARG(cfg.max_key_len > 0 && cfg.max_key_len <= kKeyBytes - 1,
                   "max_key_len must be in [1, 31]");
  check_ngram(cfg);
  LOCUST_CHECK_ARG(cfg.ngram == 1 || cfg.map_path == MapPath::kFast,
                   "ngram > 1 needs the fast map (map_path fast): the compat map emits words only");
  // construction phases, logged at LOCUST_LOG=debug (the cold CLI breakdown's engine_ms)
  u64 tc[6] = {now_ns(), 0, 0, 0, 0, 0};
  LOCUST_HIP_CHECK(hipSetDevice(cfg.device));
  {  // the device pass, planned against the HBM this engine may use (engine.hpp)
    size_t fr = 0, tot = 0;
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    hbm_free = fr;
    hbm_total = tot;
    const DevicePassPlan plan = plan_device_pass(cfg, max_bytes, max_lines, cap_records, fr);
    cap_bytes = plan.chunk_bytes;
    cap_lines = plan.cap_lines;
    cap = plan.cap;
    ucap = plan.ucap;
    rcap = plan.rcap;
    map_window = plan.map_window;
    pass_bytes = plan.pass_bytes;
    streaming = plan.streaming;
    if (plan.streaming && !(cfg.chunk_bytes && max_bytes > cfg.chunk_bytes))
      LOCUST_LOG_INFO("device pass: %llu B input planned as a stream of %llu B chunks (%s)",
                      (unsigned long long)max_bytes, (unsigned long long)cap_bytes,
                      plan.why.c_str());
  }
  warm_modules_once(cfg.device);
  tc[1] = now_ns();
  LOCUST_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  for (auto& e : ev) LOCUST_HIP_CHECK(hipEventCreate(&e));
  tc[2] = now_ns();

  const bool compat = cfg.map_path == MapPath::kCompat;
  const u64 hcap = rcap < cap ? 1 : rcap;  // (shape_arena)
  DevicePassPlan plan;
  plan.streaming = streaming;
  plan.chunk_bytes = cap_bytes;
  plan.pass_bytes = pass_bytes;
  plan.map_window = map_window;
  plan.cap_lines = cap_lines;
  plan.cap = cap;
  plan.ucap = ucap;
  plan.rcap = rcap;
  const ArenaShape sh = shape_arena(cfg, plan, small_pass_bytes);
  const u64 slot_cap = sh.slot_cap;
  const u64 t_line = sh.t_line, t_compact = sh.t_compact, t_map = sh.t_map;
  const u64 t_heads = sh.t_heads, t_scan = sh.t_scan;
  const u64 rx_zero_words = sh.rx_zero_words, rx_part_words = sh.rx_part_words;
  dict_slots = sh.dict_slots;
  dict_zero_bytes = sh.dict_zero_bytes;
  sync_bytes = sh.sync_bytes;
  small_pass = sh.small_pass;
  part_off_tiles = sh.part_off_tiles;
  large_ordered = sh.large_ordered;
  partial_slots_cap = sh.partial_slots_cap;
  const u64 partial_slots = (u64)kDictParts * partial_slots_cap;
  arena.size = sh.arena_bytes;
  {
    size_t got = 0;  // the process-wide block cache (locust/devcache.hpp)
    arena.base = static_cast<char*>(dev_block_alloc(arena.size, &got));
    arena_block = got;
  }

  d_text = arena.take<char>(cap_bytes + 64);
  d_nl = arena.take<u64>(compat ? cap_lines + 1 : 1);
  d_delims = arena.take<char>(64);
  for (int j = 0; j < kKeyWords; ++j) {
    slots.w[j] = arena.take<u64>(slot_cap);
    tokens.w[j] = arena.take<u64>(cap);
    sorted.w[j] = arena.take<u64>(rcap);
    heads.w[j] = arena.take<u64>(hcap);
  }
  d_line_counts = arena.take<u32>(compat ? cap_lines : 1);
  d_counts = arena.take<u64>(cap);
  d_sorted_counts = arena.take<u64>(rcap);
  d_prefix = arena.take<u64>(hcap);
  d_head_val = arena.take<u64>(hcap);
  d_head_count = arena.take<u64>(hcap);
  d_perm = arena.take<u32>(rcap);
  d_parts = arena.take<u8>(align_up(cap, 16) + 16);
  if (part_off_tiles) d_part_off = arena.take<u32>(part_off_tiles * kPartTable);
  if (part_off_tiles) d_part_occ = arena.take<u32>(part_off_tiles * kPartOccWords);
  if (partial_slots) {
    d_partials = arena.take<KeyCount>(partial_slots * kPartSlotsHost);
    d_partial_n = arena.take<u32>(partial_slots);
  }
  d_out = arena.take<OutRecord>(rcap);
  // room for a gather slot header in front: d_records - kSlotHeaderRecords is the slot
  d_records = arena.take<KeyCount>(slot_records_cap() + kSlotHeaderRecords) + kSlotHeaderRecords;
  d_samples = arena.take<PackedKey>(kMaxSamples);
  d_splitters = arena.take<PackedKey>(kMaxRanks);
  d_offsets = arena.take<u64>(kMaxRanks + 1);
  d_offset = arena.take<u64>(1);

  // sync block: [MapCounters | tile counters | status regions]
  d_sync = arena.take<char>(sync_bytes);
  d_ctr = reinterpret_cast<MapCounters*>(d_sync);
  u32* counters = reinterpret_cast<u32*>(d_sync + 128);
  u64* st = reinterpret_cast<u64*>(d_sync + 256);
  lb_line = {st, counters + 0};
  st += t_line;
  lb_compact = {st, counters + 1};
  st += t_compact;
  lb_map = {st, counters + 2};
  st += t_map;
  lb_heads = {st, counters + 3};
  st += t_heads;
  lb_scan = {st, counters + 4};
  st += t_scan;
  lb_dict = {st, counters + 5};
  // counters[6] is the ordered kernels' done counter (lb_dict.tile_counter + 1);
  d_plan_flag = counters + 7;  // OrderedExtra::plan_flag

  rx.cap = rcap;
  rx.tile_counters = arena.take<u32>(rx_zero_words);
  rx.status = rx.tile_counters + kNumPositions;
  rx.hist_part = arena.take<u32>(rx_part_words);
  rx.plan = arena.take<SortPlan>(1);
  for (int b = 0; b < 2; ++b) {
    rx.keys[b] = arena.take<u64>(rcap);
    rx.vals[b] = arena.take<u32>(rcap);
  }
  for (int j = 0; j < kKeyWords; ++j) dict.ukeys.w[j] = arena.take<u64>(ucap);
  {
    char* z = arena.take<char>(dict_zero_bytes);
    dict.table = reinterpret_cast<DictSlot*>(z);
    dict.ucount = reinterpret_cast<u64*>(z + align_up(dict_slots * sizeof(DictSlot), 256));
    dict.uval = reinterpret_cast<u64*>(reinterpret_cast<char*>(dict.ucount) + align_up(ucap * 8, 256));
    d_rank = reinterpret_cast<u32*>(reinterpret_cast<char*>(dict.uval) + align_up(ucap * 8, 256));
    dict.mask = (u32)(dict_slots - 1);
    dict.ucap = (u32)ucap;
    dict.urank = d_rank;
  }

  char delim_buf[64] = {0};
  LOCUST_CHECK_ARG(cfg.delimiters.size() < sizeof(delim_buf), "too many delimiters");
  std::memcpy(delim_buf, cfg.delimiters.data(), cfg.delimiters.size());
  // on this pipeline's own stream: a legacy-stream copy would conflict with another
  // thread's graph capture (loopback ranks share the process)
  LOCUST_HIP_CHECK(
      hipMemcpyAsync(d_delims, delim_buf, sizeof(delim_buf), hipMemcpyHostToDevice, stream));
  // the counters and look-back words start zeroed, as a self-cleaning job leaves them: the
  // first job skips its reset memset (a fill kernel, and ~13 us of a first enqueue)
  LOCUST_HIP_CHECK(hipMemsetAsync(d_sync, 0, sync_bytes, stream));
  LOCUST_HIP_CHECK(hipStreamSynchronize(stream));
  sync_clean = true;

  tc[3] = now_ns();
  // A streaming engine reads files through its two staging halves; its one-pass buffer
  // is pinned only when a caller stages text there (input_buffer(), a one-pass job).
  if (!streaming && !cfg.records_only) ensure_h_text();
  LOCUST_HIP_CHECK(hipHostMalloc(&h_ctr, sizeof(MapCounters), hipHostMallocDefault));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_plan, sizeof(SortPlan), hipHostMallocDefault));
  // Output records and the counter snapshot are host-mapped: the emit kernel writes them
  // over PCIe directly (zero-copy), so a dictionary run needs no D2H copy at all.  The
  // kernels that write it directly emit at most kMappedOutMax records (larger results
  // take the radix path, whose download grows the buffer), so a streaming engine with a
  // 16M-key dictionary does not pin 800 MB per output buffer.
  out_pool.push_back(std::make_shared<HostOut>(std::min<u64>(ucap, kMappedOutMax)));
  use_out(0);
  // and a second one: a job's result holds its buffer while the next job runs, so jobs
  // alternate between two -- allocated here, not inside the second job (pinning a
  // 12 MiB mapped buffer took ~1 ms of a cold CLI-style job).  A streaming engine's jobs
  // take hundreds of ms: its second buffer is pinned when a second job needs it (host
  // memory of `--gpus N` file ranks, one streaming engine each).
  if (!streaming && !cfg.records_only) out_pool.push_back(std::make_shared<HostOut>(h_out_cap));
  // and a third for small engines: the partition map's retune reads the first job's
  // output on the worker thread, so a caller holding each job's result (the CLI, a
  // Python loop) found both buffers taken at its third job and waited ~0.2 ms for the
  // worker (measured); pinning it here costs well under a millisecond of construction
  if (!streaming && !cfg.records_only && h_out_cap * sizeof(OutRecord) <= (8ull << 20))
    out_pool.push_back(std::make_shared<HostOut>(h_out_cap));
  use_out(0);
  LOCUST_HIP_CHECK(hipHostMalloc(&h_ctr_mapped, sizeof(MapCounters),
                                 hipHostMallocMapped | hipHostMallocCoherent));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_done, 64, hipHostMallocMapped | hipHostMallocCoherent));
  *h_done = 0;
  LOCUST_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_done), h_done, 0));
  LOCUST_HIP_CHECK(
      hipHostGetDevicePointer(reinterpret_cast<void**>(&d_ctr_mapped), h_ctr_mapped, 0));
  LOCUST_HIP_CHECK(hipMalloc(&d_pmap, sizeof(PartMapTables)));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_pmap, sizeof(PartMapTables), hipHostMallocDefault));
  part_map_default(h_pmap);
  LOCUST_HIP_CHECK(hipMemcpyAsync(d_pmap, h_pmap, sizeof(PartMapTables), hipMemcpyHostToDevice,
                                  stream));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_pw, kDictParts * sizeof(u32),
                                 hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(h_pw, 0, kDictParts * sizeof(u32));
  LOCUST_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_pw), h_pw, 0));
  LOCUST_HIP_CHECK(hipStreamSynchronize(stream));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_small, kMaxSamples * sizeof(PackedKey), hipHostMallocDefault));
  LOCUST_HIP_CHECK(hipHostMalloc(&h_u64, (kMaxRanks + 8) * sizeof(u64), hipHostMallocDefault));
  std::memset(h_ctr, 0, sizeof(MapCounters));
  tc[4] = now_ns();
  if (large_ordered && cfg.map_path == MapPath::kFast && !cfg.records_only) {
    // what a piecewise pass needs, made here and not inside the first job: the copy
    // streams and piece events, and the plan's scratch
    ensure_piece_events(partial_slots_cap);
    if (devplan_env) ensure_plan();
    warm_copy_streams();
  }
  // the retune worker of a small engine is made here, not inside its first job (a
  // streaming engine's jobs take hundreds of ms: it makes it when first needed)
  if (!streaming) {
    retune_worker.start();
    // a first kernel launch on this engine's stream (its hardware queue's first dispatch,
    // kernel-argument space): here, not inside the first job -- a fresh engine's first job
    // spent ~35 us more than later ones enqueuing its launches (measured, bench cold_start)
    launch_signal_host(d_done, 0, stream);
    LOCUST_HIP_CHECK(hipStreamSynchronize(stream));
  }
  tc[5] = now_ns();
  LOCUST_LOG_DEBUG("engine (%llu B text, %llu tokens, %llu records%s): modules %.2f ms, stream "
                   "%.2f ms, device arena %.2f ms (%.1f MiB of %.1f GiB free), pinned host "
                   "buffers %.2f ms, copy streams %.2f ms",
                   (unsigned long long)cap_bytes, (unsigned long long)cap,
                   (unsigned long long)rcap, streaming ? ", streaming" : "",
                   (tc[1] - tc[0]) * 1e-6, (tc[2] - tc[1]) * 1e-6, (tc[3] - tc[2]) * 1e-6,
                   arena.size / 1048576.0, hbm_free / 1073741824.0, (tc[4] - tc[3]) * 1e-6,
                   (tc[5] - tc[4]) * 1e-6);
}

void DevicePipeline::warm_copy_streams() {
  if (!h_text || !cstream || !cstream2) return;
  const u64 n = std::min<u64>(cap_bytes, kPieceBytes);
  for (hipStream_t s : {cstream, cstream2, stream}) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_text, h_text, n, hipMemcpyHostToDevice, s));
    LOCUST_HIP_CHECK(hipMemsetAsync(d_text + 1, 0, 16, s));
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_u64, d_text, 8, hipMemcpyDeviceToHost, s));
    LOCUST_HIP_CHECK(hipStreamSynchronize(s));
  }
}

DevicePipeline::~DevicePipeline() {
  retune_worker.stop();  // its task may hold an output buffer
  if (stream) (void)hipStreamSynchronize(stream);
  for (auto& g : dict_graphs) (void)hipGraphExecDestroy(g.exec);
  for (auto& g : graph_cache) (void)hipGraphExecDestroy(g.exec);
  if (d_ord_trace) (void)hipFree(d_ord_trace);
  if (d_partials_trace) (void)hipFree(d_partials_trace);
  if (d_map_trace) (void)hipFree(d_map_trace);
  if (cstream) (void)hipStreamSynchronize(cstream);
  if (cstream2) (void)hipStreamSynchronize(cstream2);

  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  for (int b = 0; b < 2; ++b) {
    if (ev_copied[b]) (void)hipEventDestroy(ev_copied[b]);
    if (ev_consumed[b]) (void)hipEventDestroy(ev_consumed[b]);
    pinned_free(h_stage[b]);
  }
  for (int i = 0; i < kRingPieces; ++i) {
    pinned_free(h_ring[i]);
    if (ev_ring[i]) (void)hipEventDestroy(ev_ring[i]);
  }
  for (auto e : ev_piece) (void)hipEventDestroy(e);
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (cstream) (void)hipStreamDestroy(cstream);
  if (cstream2) (void)hipStreamDestroy(cstream2);

  if (d_text_alt) dev_block_free(d_text_alt, d_text_alt_block);
  if (radix_base) dev_block_free(radix_base, radix_block);
  if (d_dctr) (void)hipFree(d_dctr);
  if (h_chunk_ctr) (void)hipHostFree(h_chunk_ctr);
  if (stream) (void)hipStreamDestroy(stream);
  if (arena.base) dev_block_free(arena.base, arena_block);  // every stream synchronised above
  pinned_free(h_text);
  pinned_free(h_keys);
  for (void* p : {(void*)h_ctr, (void*)h_plan, (void*)h_small, (void*)h_u64,
                  (void*)h_ctr_mapped, (void*)h_pmap, (void*)h_pw, (void*)h_done})
    if (p) (void)hipHostFree(p);
  if (d_pmap) (void)hipFree(d_pmap);
  if (d_plan) (void)hipFree(d_plan);
  if (d_topk) (void)hipFree(d_topk);
  pinned_free(h_top);
  for (auto& e : ev_top)
    if (e) (void)hipEventDestroy(e);
  if (d_index) (void)hipFree(d_index);
  pinned_free(h_post);
  pinned_free(h_ictr);
  for (auto& e : ev_index)
    if (e) (void)hipEventDestroy(e);
  for (auto& h : store)
    if (h.base) (void)hipFree(h.base);
  if (d_append) (void)hipFree(d_append);
  pinned_free(h_actr);
  for (auto& e : ev_append)
    if (e) (void)hipEventDestroy(e);
  if (d_drop) (void)hipFree(d_drop);
  pinned_free(h_dctr);
  for (auto& e : ev_drop)
    if (e) (void)hipEventDestroy(e);
  if (d_sbatch) (void)hipFree(d_sbatch);
  if (d_shits) (void)hipFree(d_shits);
  if (d_smerged) (void)hipFree(d_smerged);
  if (d_spat) (void)hipFree(d_spat);
  pinned_free(h_spat);
  if (d_srx) (void)hipFree(d_srx);
  pinned_free(h_srx);
  if (d_sexpr) (void)hipFree(d_sexpr);
  if (d_corpus) (void)hipFree(d_corpus);
  if (d_byfile) (void)hipFree(d_byfile);
  pinned_free(h_byfile);
  pinned_free(h_corpus);
  pinned_free(h_sexpr);
  pinned_free(h_supload);
  pinned_free(h_sres);
  pinned_free(h_slines);
  for (auto& e : ev_search)
    if (e) (void)hipEventDestroy(e);
  if (d_show_entries) (void)hipFree(d_show_entries);
  if (d_show_text) (void)hipFree(d_show_text);
  if (d_show_spans) (void)hipFree(d_show_spans);
  pinned_free(h_show);
  if (d_tally_entries) (void)hipFree(d_tally_entries);
  if (d_tally_pairs) (void)hipFree(d_tally_pairs);
  pinned_free(h_tally);
  for (auto& e : ev_tally)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ev_show)
    if (e) (void)hipEventDestroy(e);
}

void DevicePipeline::use_out(size_t i) {
  out_idx = i;
  h_out = out_pool[i]->h;
  d_out_mapped = out_pool[i]->d;
  h_out_cap = out_pool[i]->cap;
  h_ctab = out_pool[i]->ctab_h;
  d_ctab_mapped = out_pool[i]->ctab_d;
}

void DevicePipeline::select_out() {
  if (!out_pool.empty() && out_pool[out_idx].use_count() == 1) return;
  for (size_t i = 0; i < out_pool.size(); ++i)
    if (out_pool[i].use_count() == 1) return use_out(i);
  if (retune_pending) {
    // a background retune reads a buffer a result no longer needs: wait until it has let
    // go of it (one pass over the output) rather than pin a new buffer (~2 ms for a large
    // engine's)
    while (!retune_task.released.load(std::memory_order_acquire)) std::this_thread::yield();
    poll_retune();
    for (size_t i = 0; i < out_pool.size(); ++i)
      if (out_pool[i].use_count() == 1) return use_out(i);
  }
  const u64 t0 = now_ns();
  out_pool.push_back(std::make_shared<HostOut>(h_out_cap));
  use_out(out_pool.size() - 1);
  LOCUST_LOG_DEBUG("output buffer #%zu: %llu records, %.2f ms", out_pool.size(),
                   (unsigned long long)h_out_cap, (now_ns() - t0) * 1e-6);
}

void DevicePipeline::grow_host_out(u64 n) {
  select_out();
  if (n <= h_out_cap) return;
  sync();  // the device may still write the buffer being replaced
  out_pool[out_idx] = std::make_shared<HostOut>(n);
  use_out(out_idx);
}

void DevicePipeline::grow_host_keys(u64 n) {
  if (n <= h_keys_cap) return;
  pinned_free(h_keys);
  h_keys_cap = std::max<u64>(n, 1);
  h_keys = static_cast<u64*>(pinned_alloc(h_keys_cap * kKeyWords * sizeof(u64), hipHostMallocDefault,
                                          "key staging"));
}

void DevicePipeline::wait_done(u32 seq, bool bounded_sync) {
  const u64 t0 = now_ns();
  while (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) != seq) {
    if (now_ns() - t0 > 2000000) {  // 2 ms
      if (bounded_sync) sync();
      break;
    }
    __builtin_ia32_pause();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
}

void DevicePipeline::enqueue_upload(const TextInput& in) {
  const u64 t0 = now_ns();
  prepare_upload(in);
  const u64 t1 = now_ns();
  enqueue_upload_device(in);
  if ((int)log_level() >= (int)LogLevel::kDebug)
    LOCUST_LOG_DEBUG("upload: mode %d, %zu pieces, host %.3f ms, enqueue %.3f ms",
                     (int)upload_mode, pieces.size(), (t1 - t0) * 1e-6, (now_ns() - t1) * 1e-6);
}

void DevicePipeline::prepare_upload(const TextInput& in) {
  ensure_h_text();
  map_text = d_text;
  pieces.clear();
  if (use_zero_copy(in)) {
    upload_mode = Upload::kZeroCopy;
    map_text = d_h_text;
  } else if (in.data != h_text && in.bytes && host_pinned(in.data)) {
    upload_mode = Upload::kDirect;
    plan_pieces(in);
    return;
  } else {
    upload_mode = Upload::kStaged;
  }
  if (in.data != h_text && in.bytes) std::memcpy(h_text, in.data, in.bytes);
  std::memset(h_text + in.bytes, 0, 16);
  plan_pieces(in);
}

void DevicePipeline::plan_pieces(const TextInput& in) {
  if (cfg.map_path != MapPath::kFast || !large_ordered || in.bytes < 2 * kPieceBytes) return;
  const u64 npieces = std::min<u64>(partial_slots_cap, kMaxPieces);
  const u64 piece = std::max<u64>({kPieceBytes, std::min<u64>(piece_target(), in.bytes / 4),
                                   div_up(in.bytes, npieces > 3 ? npieces - 3 : 1)});
  u64 pos = 0;
  while (pos < in.bytes && pieces.size() < npieces) {
    // Short first pieces start the map early, a short last piece keeps the work after
    // the final copy small: P/4, P/2, P, ..., P, (rest - P/4), P/4 (a P/8 tail measured
    // no better).  The last piece allowed takes the rest (line alignment shortens the
    // others).
    const u64 rest = in.bytes - pos, tail = piece / 4;
    u64 want = piece;
    if (pieces.size() == 0) want = piece / 4;
    else if (pieces.size() == 1) want = piece / 2;
    else if (rest <= tail + tail / 2) want = rest;
    else if (rest <= piece + tail) want = rest - tail;
    want = std::min(want, rest);
    u64 end = pieces.size() + 1 == npieces ? in.bytes : pos + want;
    if (end < in.bytes) {
      const void* nl = memrchr(in.data + pos, '\n', (size_t)(end - pos));
      if (!nl) {  // a line longer than a piece: no pieces at all
        pieces.clear();
        return;
      }
      end = (u64)(static_cast<const char*>(nl) - in.data) + 1;
    }
    pieces.emplace_back(pos, end - pos);
    pos = end;
  }
  if (pos < in.bytes) pieces.clear();
}

void DevicePipeline::ensure_piece_events(size_t n) {
  if (!cstream) LOCUST_HIP_CHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
  if (!cstream2) LOCUST_HIP_CHECK(hipStreamCreateWithFlags(&cstream2, hipStreamNonBlocking));
  if (!ev_fork) LOCUST_HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
  while (ev_piece.size() < n) {
    hipEvent_t e;
    LOCUST_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev_piece.push_back(e);
  }
}

void DevicePipeline::enqueue_upload_device(const TextInput& in) {
  if (!pieces.empty()) {
    // the pieces' copies go out first (outside a graph capture: there they need the fork
    // from `stream`, made in enqueue_map); their maps follow in enqueue_map
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    LOCUST_HIP_CHECK(hipStreamIsCapturing(stream, &cst));
    if (cst == hipStreamCaptureStatusNone)
      issue_piece_copies(upload_mode == Upload::kDirect ? in.data : h_text);
  } else if (upload_mode == Upload::kDirect) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_text, in.data, in.bytes, hipMemcpyHostToDevice, stream));
    LOCUST_HIP_CHECK(hipMemsetAsync(d_text + in.bytes, 0, 16, stream));
  } else if (upload_mode == Upload::kStaged) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_text, h_text, in.bytes + 16, hipMemcpyHostToDevice, stream));
  }
  if (!skip_sync_reset) LOCUST_HIP_CHECK(hipMemsetAsync(d_sync, 0, sync_bytes, stream));
}

bool DevicePipeline::use_job_graph(const TextInput& in) const {
  if (cfg.map_path == MapPath::kFast && large_ordered && in.bytes >= 2 * kPieceBytes) return false;
  if (cfg.graph < 0 && lean_job(in)) return false;  // auto: lean direct launches instead
  const bool radix_ok = cfg.sort_path == SortPath::kRadix && cfg.map_path == MapPath::kFast &&
                        table_tiles(in.bytes) > 0 && radix_mapped() && psort_enabled();
  if (cfg.graph >= 0) return cfg.graph > 0 && (cfg.sort_path == SortPath::kDict || radix_ok);
  return (cfg.sort_path == SortPath::kDict && cfg.map_path == MapPath::kFast) || radix_ok;
}

bool DevicePipeline::lean_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("LOCUST_LEAN");
    return !e || e[0] != '0';
  }();
  return on;
}

void DevicePipeline::launch_dict_graph(const TextInput& in, bool compat) {
  u64 sig = 0;
  for (const auto& pc : pieces) sig = (sig ^ pc.first) * 0x100000001b3ull;
  if (!pieces.empty()) sig |= 1;
  const GraphKey key{in.bytes, in.num_lines, upload_mode == Upload::kDirect ? in.data : nullptr,
                     map_text, upload_mode, d_out_mapped, skip_sync_reset, sig};
  const DictGraph* hit = nullptr;
  for (const auto& g : dict_graphs)
    if (g.key == key) hit = &g;
  if (!hit) {
    if (dict_graphs.size() >= 6) {  // shapes or buffers changed a lot: drop the oldest
      LOCUST_HIP_CHECK(hipGraphExecDestroy(dict_graphs.front().exec));
      dict_graphs.erase(dict_graphs.begin());
    }
    hipGraph_t g = nullptr;
    LOCUST_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
    enqueue_upload_device(in);
    enqueue_map(in);
    bool ordered;  // dictionary: the ordered kernel; radix: the partitioned sort
    if (cfg.sort_path == SortPath::kDict) {
      ordered = enqueue_dict_job((u32)in.num_lines, compat, false, nullptr, /*self_clean=*/true);
    } else {
      enqueue_radix_job((u32)in.num_lines, compat, nullptr, nullptr);
      ordered = psort_used;
      job_self_cleaned = false;
    }
    LOCUST_HIP_CHECK(hipStreamEndCapture(stream, &g));
    hipGraphExec_t exec = nullptr;
    LOCUST_HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    LOCUST_HIP_CHECK(hipGraphDestroy(g));
    dict_graphs.push_back({key, exec, ordered, job_self_cleaned, ordered && ord_compact});
    hit = &dict_graphs.back();
  }
  graph_ordered = hit->ordered;
  job_self_cleaned = hit->clean;
  ord_compact = hit->compact;
  if (cfg.sort_path == SortPath::kRadix) {  // what the replayed job took when it was captured
    psort_used = hit->ordered;
    process_path = psort_used ? kPathPsort : radix_path_name();
  }
  parts_ready = cfg.map_path == MapPath::kFast;  // what enqueue_map sets when not replaying
  part_tiles = cfg.map_path != MapPath::kFast ? 0u : pieces.empty() ? table_tiles(in.bytes)
                                                                       : piece_tiles();
  LOCUST_HIP_CHECK(hipGraphLaunch(hit->exec, stream));
}

void DevicePipeline::enqueue_map(const TextInput& in) {
  plan_pass = false;  // decided per pass (decide_plan) where the map can write occupancy
  parts_ready = cfg.map_path == MapPath::kFast;
  devplan_used = false;
  partial_nslots = 0;
  // combining needs the 4 KiB grouped map: upload pieces, or one launch past kMapLargeInput
  map_combined = combine_map && large_ordered && cfg.map_path == MapPath::kFast &&
                 (!pieces.empty() ? piece_tiles() > 0
                                  : in.bytes >= kMapLargeInput && table_tiles(in.bytes) > 0);
  if (cfg.map_path == MapPath::kCompat) {
    launch_line_index(d_text, in.bytes, d_nl, d_ctr, lb_line, stream);
    launch_map_compat(d_text, in.bytes, d_nl, (u32)in.num_lines, d_delims, cfg.emits_per_line,
                      cfg.max_key_len, slots, d_line_counts, d_ctr, stream);
  } else if (!pieces.empty()) {
    // piece k: H2D on the copy stream, then its map on the compute stream once it landed
    // (4 KiB tiles; the table rows of the pieces follow each other)
    ensure_piece_events(pieces.size());
    part_tiles = piece_tiles();
    const char* src = upload_mode == Upload::kDirect ? in.data : h_text;
    const DelimMask dm = make_delim_mask(cfg.delimiters.c_str());
    // The copies need no fork from `stream` outside a graph capture (nothing earlier in
    // the job touches d_text, and the previous job ended with a host sync).  A fork made
    // the first copy on a copy stream wait on the host for the compute queue's marker:
    // one job in ~8 stalled 8-9 ms inside hipMemcpyAsync (measured; none without it).
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    LOCUST_HIP_CHECK(hipStreamIsCapturing(stream, &cst));
    if (cst != hipStreamCaptureStatusNone) {
      LOCUST_HIP_CHECK(hipEventRecord(ev_fork, stream));
      LOCUST_HIP_CHECK(hipStreamWaitEvent(cstream, ev_fork, 0));
      LOCUST_HIP_CHECK(hipStreamWaitEvent(cstream2, ev_fork, 0));
    }
    // a combining large pass (run() / the shard engine take the two-kernel ordered build
    // next): aggregate each piece right after its map, into slot k -- on the same stream:
    // beside the next map on a third stream both kernels ran ~1.6x slower and every
    // cross-queue hand-off cost ~20 us (measured), while the copies leave room for both
    const bool agg = map_combined && large_ordered_ok() && pieces.size() <= partial_slots_cap;
    devplan_used = agg && devplan_env && !devplan_failed && !pm_tuned;
    if (devplan_used) {  // zeroed while piece 0 is on its way
      ensure_plan();
      LOCUST_HIP_CHECK(hipMemsetAsync(d_plan, 0, plan_zero_bytes, stream));
    }
    const u64 t_enq = now_ns();
    // the padding after the text: off the copy streams (a 16-byte fill at an unaligned
    // address is two blit kernels there, ~15 us in front of the last piece's event)
    LOCUST_HIP_CHECK(hipMemsetAsync(d_text + in.bytes, 0, 16, stream));
    u64 tile_off = 0;
    const bool issued = pieces_issued;
    pieces_issued = false;
    for (size_t k = 0; k < pieces.size(); ++k) {
      const u64 off = pieces[k].first, len = pieces[k].second;
      if (!issued) {
        hipStream_t cs = piece_stream(k);
        LOCUST_HIP_CHECK(hipMemcpyAsync(d_text + off, src + off, len, hipMemcpyHostToDevice, cs));
        LOCUST_HIP_CHECK(hipEventRecord(ev_piece[k], cs));
      }
      LOCUST_HIP_CHECK(hipStreamWaitEvent(stream, ev_piece[k], 0));
      if (k == 0 && devplan_used) enqueue_devplan(src, len, dm);
      launch_map_fast(d_text + off, len, dm, cfg.emits_per_line, cfg.max_key_len, tokens, d_parts,
                      cap, d_ctr, lb_map, stream, map_trace(),
                      part_tiles ? d_part_off + tile_off * kPartTable : nullptr, part_map(),
                      /*large_tiles=*/true, map_combined ? d_counts : nullptr, nullptr, nullptr,
                      cfg.ngram);
      const u64 t1 = tile_off + div_up(len, kMapTileBytesLarge);
      if (agg)
        launch_dict_partials(tokens, d_counts, d_part_off, (u32)tile_off, (u32)t1, 1, (u32)k,
                             (u32)pieces.size(), cap, d_partials, d_partial_n, stream,
                             partials_trace());
      tile_off = t1;
    }
    if ((int)log_level() >= (int)LogLevel::kDebug)
      LOCUST_LOG_DEBUG("piecewise map enqueued in %.3f ms", (now_ns() - t_enq) * 1e-6);
    if (agg) partial_nslots = (u32)pieces.size();
  } else {
    part_tiles = table_tiles(in.bytes);
    // A large pass in one launch (below the piecewise size): the same in-job plan as the
    // piecewise pass, from the first MiB of the text, before the map tags the tokens --
    // a first-letter map overflows the ordered kernel's LDS tables on ~80K distinct keys
    // (measured: 1/8 of synth1m, 5.7 ms first job with the HBM-table fallback).
    devplan_used = large_ordered && part_tiles && cfg.sort_path == SortPath::kDict &&
                   devplan_env && !devplan_failed && !pm_tuned;
    if (devplan_used) {
      ensure_plan();
      LOCUST_HIP_CHECK(hipMemsetAsync(d_plan, 0, plan_zero_bytes, stream));
      enqueue_devplan(upload_mode == Upload::kDirect || upload_mode == Upload::kZeroCopy ? in.data
                                                                                       : h_text,
                      in.bytes, make_delim_mask(cfg.delimiters.c_str()), map_text);
    }
    decide_plan(in.bytes);
    launch_map_fast(map_text, in.bytes, make_delim_mask(cfg.delimiters.c_str()),
                    cfg.emits_per_line, cfg.max_key_len, tokens, d_parts, cap, d_ctr, lb_map,
                    stream, map_trace(), part_tiles ? d_part_off : nullptr, part_map(), false,
                    map_combined ? d_counts : nullptr, plan_small() ? d_part_occ : nullptr,
                    plan_small() && plan_trigger ? d_plan_flag : nullptr, cfg.ngram);
  }
}

void DevicePipeline::enqueue_process(u32 num_lines, bool compat, bool with_counts, u64 host_n,
                       bool allow_psort) {
  ensure_radix_full();  // every token is sorted: a dictionary engine grows its buffers
  if (allow_psort && psort_ok(compat, with_counts)) {
    // one kernel, one workgroup per key range of the map's partition table (psort.hip)
    launch_psort(tokens, d_part_off, part_tiles, cap, sorted, d_ctr, d_pw, stream, ord_trace());
    psort_used = true;
    process_path = kPathPsort;
    return;
  }
  psort_used = false;
  process_path = radix_path_name();
  if (compat)
    launch_compact_slots(d_line_counts, num_lines, cfg.emits_per_line, slots, tokens, d_ctr,
                         lb_compact, stream);
  if (!cfg.sync_plan) {
    host_n = kUnknownCount;
  } else if (host_n == kUnknownCount) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_u64, &d_ctr->num_records, sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
    sync();
    host_n = *reinterpret_cast<const u32*>(h_u64);
  }
  radix_sort(tokens, &d_ctr->num_records, host_n, rx, with_counts ? d_counts : nullptr, sorted,
             with_counts ? d_sorted_counts : nullptr, d_perm, h_plan, stream);
}

void DevicePipeline::enqueue_radix_job(u32 num_lines, bool compat, hipEvent_t after_process,
                         hipEvent_t after_reduce) {
  ensure_radix_full();
  radix_fused = cfg.reduce_path == ReducePath::kLds &&
                radix_mapped() && psort_ok(compat, false);
  if (radix_fused) {
    // Process + Reduce in one kernel, records straight into the mapped output; it
    // re-zeroes its scratch and, in a lean job, tells the host itself (psort.hip)
    PsortReduceArgs ra;
    ra.out = d_out_mapped;
    ra.out_cap = h_out_cap;
    ra.ctr_out = d_ctr_mapped;
    ra.status = lb_dict.status;
    ra.done_counter = lb_dict.tile_counter + 1;  // the sync block's spare counter word
    ra.map_lb = lb_map;
    ra.map_words = (u32)(div_up(pass_bytes, kMapTileBytesMin) + 1);
    if (done_pending) {
      ra.host_done = d_done;
      ra.host_done_value = done_pending;
      done_pending = 0;
    }
    launch_psort_reduce(tokens, d_part_off, part_tiles, cap, d_ctr, d_pw, ra, stream, ord_trace());
    psort_used = true;
    process_path = kPathPsort;
    if (after_process) LOCUST_HIP_CHECK(hipEventRecord(after_process, stream));
    if (after_reduce) LOCUST_HIP_CHECK(hipEventRecord(after_reduce, stream));
    return;
  }
  enqueue_process(num_lines, compat, false, kUnknownCount, /*allow_psort=*/true);
  if (after_process) LOCUST_HIP_CHECK(hipEventRecord(after_process, stream));
  const bool mapped = radix_mapped();
  if (cfg.reduce_path == ReducePath::kLds) {
    // LDS path: mark + compact + adjacent difference + records in one kernel
    launch_reduce_fused(sorted, cap, d_ctr, mapped ? d_out_mapped : d_out, mapped ? h_out_cap : cap,
                        mapped ? d_ctr_mapped : nullptr, lb_heads, stream);
  } else {
    // global path: the reference's kernel sequence (kernFindUniqBool, partition,
    // kernGetCount) as separate launches
    enqueue_reduce_core(false);
    if (mapped)
      launch_pack_output(heads, d_head_val, d_head_count, cap, d_ctr, d_out_mapped, stream,
                         d_ctr_mapped);
    else
      enqueue_pack_output();
  }
  if (after_reduce) LOCUST_HIP_CHECK(hipEventRecord(after_reduce, stream));
}

void DevicePipeline::redo_radix_general(u32 num_lines) {
  redo_process_general(num_lines);
  LOCUST_HIP_CHECK(hipMemsetAsync(lb_heads.status, 0, 8 * (div_up(cap, kReduceTile) + 1), stream));
  LOCUST_HIP_CHECK(hipMemsetAsync(lb_heads.tile_counter, 0, 4, stream));
  enqueue_reduce_core(false);
  enqueue_pack_output();
}

void DevicePipeline::enqueue_reduce_core(bool with_counts) {
  ensure_radix_full();
  const u64* prefix = nullptr;
  if (with_counts) {
    launch_scan_counts(d_sorted_counts, cap, d_prefix, d_ctr, lb_scan, stream);
    prefix = d_prefix;
  }
  launch_mark_compact_heads(sorted, prefix, cap, cfg.reduce_path, heads, d_head_val, d_ctr,
                            lb_heads, stream);
  launch_adjacent_diff(d_head_val, cap, cfg.reduce_path, d_head_count, d_ctr, stream);
}

void DevicePipeline::enqueue_dict_insert(u32 num_lines, bool compat, bool with_counts) {
  if (compat)
    launch_compact_slots(d_line_counts, num_lines, cfg.emits_per_line, slots, tokens, d_ctr,
                         lb_compact, stream);
  if (!compat && parts_ready && cap <= kPartBuildMaxTokens) {
    launch_dict_part_build(tokens, with_counts ? d_counts : nullptr, d_parts,
                           &d_ctr->num_records, cap, dict, d_ctr, stream);
    return;
  }
  LOCUST_HIP_CHECK(hipMemsetAsync(dict.table, 0, dict_zero_bytes, stream));
  launch_dict_insert(tokens, with_counts ? d_counts : nullptr, &d_ctr->num_records, cap, dict,
                     d_ctr, stream);
}

void DevicePipeline::enqueue_partials() {
  if (partial_nslots) return;
  partial_nslots = kOrdWorkers;
  launch_dict_partials(tokens, map_combined ? d_counts : nullptr, d_part_off, 0, part_tiles,
                       kOrdWorkers, 0, kOrdWorkers, cap, d_partials, d_partial_n, stream,
                       partials_trace());
}

void DevicePipeline::set_tile_source(OrderedExtra& ex, bool with_counts) const {
  if (part_tiles && parts_ready && !with_counts) {
    ex.part_off = d_part_off;
    ex.part_tiles = part_tiles;
    // the in-job plan while the map is untuned (a retuned map is already balanced: the
    // plan would only add its ~2 us)
    if (plan_small()) ex.part_occ = d_part_occ;
    // ... and only when the map saw a crowded partition (plan_trigger)
    if (plan_small() && plan_trigger) ex.plan_flag = d_plan_flag;
  }
}

u64 DevicePipeline::retune_wanted() const {
  if (devplan_used && !pm_tuned) {  // a planned pass: hand over to the exact map
    if (const char* v = std::getenv("LOCUST_PART_TUNE"))
      if (v[0] == '0') return 0;
    return ~0ull / 8;
  }
  if (const char* v = std::getenv("LOCUST_PART_TUNE"))
    if (v[0] == '0') return 0;
  u64 sum = 0, mx = 0;
  for (int p = 0; p < kDictParts; ++p) {
    sum += h_pw[p];
    mx = std::max<u64>(mx, h_pw[p]);
  }
  if (sum < (1u << 13) || mx * kDictParts <= 2 * sum) return 0;  // small or balanced
  if (pm_predicted_max && mx * 4 <= pm_predicted_max * 5) return 0;  // as good as it gets
  return mx;
}

void DevicePipeline::force_retune(const EntryList& e) {
  if (warming) return;
  const u64 n = e.size();
  // a device-planned map overflowed: this engine keeps the host-side map from now on
  // (tuned from this output, or the default with tuning off) -- d_pmap holds the plan
  const bool planned = devplan_used;
  if (planned) {
    devplan_failed = true;
    devplan_used = false;
  }
  const char* v = std::getenv("LOCUST_PART_TUNE");
  const bool tune = n && !(v && v[0] == '0');
  PartMapTables t;
  u64 pred = 0;
  if (tune)
    pred = part_map_from_entries(e, &t);
  else
    part_map_default(&t);
  // The same map again (e.g. one first word with more distinct keys than an LDS table:
  // no cut can split it): a new upload would change nothing, so keep it.
  if (!planned && (!tune || std::memcmp(&t, h_pmap, sizeof(t)) == 0)) return;
  if (planned && !pred) return upload_pmap(t, 0);
  retune_with(~0ull / 8, pred, t);
}

void DevicePipeline::warm_first_job() {
  // small single-pass engines only: there the two-byte job launches the real job's kernels
  // (a large pass plans, pieces and aggregates differently)
  if (streaming || large_ordered || cfg.records_only || cfg.sort_path != SortPath::kDict ||
      cfg.map_path != MapPath::kFast || cap_bytes < 2 * (u64)cfg.ngram)
    return;
  TextInput in;
  in.data = ensure_h_text();
  in.bytes = 2 * (u64)cfg.ngram;  // one record: "a\n", or the n-gram "a a\n" / "a a a\n"
  in.num_lines = 1;
  if (!lean_job(in)) return;
  // one token: a byte outside the job's delimiter set
  char c = 0;
  for (const char* q = "aZ7xq"; *q && !c; ++q)
    if (cfg.delimiters.find(*q) == std::string::npos) c = *q;
  if (!c) return;
  for (int g = 0; g < cfg.ngram; ++g) {
    h_text[2 * g] = c;
    h_text[2 * g + 1] = g + 1 < cfg.ngram && !cfg.delimiters.empty() ? cfg.delimiters[0] : '\n';
  }
  // the engine's statistics describe the caller's jobs only
  const u64 fb = fallbacks, pp = planned_passes;
  warming = true;
  struct Reset {
    bool& w;
    ~Reset() { w = false; }
  } reset{warming};
  const WordCountResult r = run(in);
  if (r.num_unique != 1)
    LOCUST_LOG_INFO("engine warm-up job: %llu keys, expected 1", (unsigned long long)r.num_unique);
  fallbacks = fb;
  planned_passes = pp;
}

void DevicePipeline::maybe_retune(const EntryList& e) {
  if (warming) return;
  const u64 mx = retune_wanted();
  if (!mx || retune_pending) return;  // one at a time
  retune_pending = true;
  retune_task.mx = mx;
  retune_task.pred = 0;
  // a borrowed list: the copy shares the buffer (and its segments), not the entries
  retune_task.hold = out_pool[out_idx];
  retune_task.entries = e;
  retune_task.released.store(false, std::memory_order_relaxed);
  retune_task.t_submit = now_ns();
  retune_worker.submit([this] {
    RetuneTask& r = retune_task;
    r.t_start = now_ns();
    // the one pass over the output first, then the buffer is free for the next jobs
    part_map_groups(r.entries, &r.groups);
    r.entries = EntryList();
    r.hold.reset();
    r.t_released = now_ns();
    r.released.store(true, std::memory_order_release);
    r.pred = part_map_from_groups(r.groups, &r.t);
    r.t_done = now_ns();
  });
}

void DevicePipeline::poll_retune() {
  if (!retune_pending || !retune_worker.idle()) return;
  retune_pending = false;
  retune_worker.rethrow_error();  // a failed retune surfaces here, on the job's thread
  const RetuneTask& r = retune_task;
  LOCUST_LOG_DEBUG("retune on the worker: started %.3f ms after the job, output read in %.3f "
                   "ms, map built in %.3f ms (%zu first-word groups)",
                   (r.t_start - r.t_submit) * 1e-6, (r.t_released - r.t_start) * 1e-6,
                   (r.t_done - r.t_released) * 1e-6, r.groups.size());
  retune_with(retune_task.mx, retune_task.pred, retune_task.t);
}

void DevicePipeline::maybe_retune_records(const KeyCount* d_recs, u64 n, bool force) {
  const bool planned = force && devplan_used;
  if (planned) {  // as force_retune
    devplan_failed = true;
    devplan_used = false;
  }
  const u64 mx = force ? ~0ull / 8 : retune_wanted();
  if (planned && (!n || [] {
        const char* v = std::getenv("LOCUST_PART_TUNE");
        return v && v[0] == '0';
      }())) {
    PartMapTables t;
    part_map_default(&t);
    return upload_pmap(t, 0);
  }
  if (!mx || !n) return;
  std::vector<KeyCount> h(n);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h.data(), d_recs, n * sizeof(KeyCount), hipMemcpyDeviceToHost,
                                  stream));
  sync();
  std::vector<WordCountEntry> e(n);
  for (u64 i = 0; i < n; ++i) {
    for (int w = 0; w < kKeyWords; ++w) e[i].key.w[w] = h[i].w[w];
    e[i].count = h[i].count;
  }
  PartMapTables t;
  const u64 pred = part_map_from_entries(EntryList(std::move(e)), &t);
  if (force && !planned && std::memcmp(&t, h_pmap, sizeof(t)) == 0) return;  // as force_retune
  retune_with(mx, pred, t);
}

void DevicePipeline::retune_with(u64 mx, u64 pred, const PartMapTables& t) {
  if (!pred || pred * 5 >= mx * 4) {  // < 20 % better: keep the map, stop asking
    pm_predicted_max = mx;
    return;
  }
  upload_pmap(t, pred);
  ++pm_retunes;
  if (large_ordered) pm_tuned = true;
  LOCUST_LOG_DEBUG("partition map retuned (#%u): max partition work %llu -> %llu",
                   pm_retunes, (unsigned long long)mx, (unsigned long long)pred);
}

void DevicePipeline::enqueue_dict_ordered(bool with_counts, bool mapped, bool self_clean) {
  OrderedExtra ex;
  ex.pm = part_map();
  ex.part_w = d_pw;
  ex.split_min = split_min;
  if (self_clean) set_self_clean(ex);
  if (self_clean && done_pending) {  // the kernel itself tells the host it is done
    ex.host_done = d_done;
    ex.host_done_value = done_pending;
    done_pending = 0;
  }
  set_tile_source(ex, with_counts);
  set_compact_out(ex, mapped);
  launch_dict_ordered(tokens, with_counts ? d_counts : nullptr, d_parts, &d_ctr->num_records,
                      cap, d_ctr, mapped ? d_out_mapped : d_out, mapped ? d_ctr_mapped : nullptr,
                      lb_dict, stream, ord_trace(), ex);
}

u64* DevicePipeline::ord_trace() {
  static const bool on = std::getenv("LOCUST_ORD_TRACE") != nullptr;
  if (!on) return nullptr;
  if (!d_ord_trace) {
    LOCUST_HIP_CHECK(hipMalloc(&d_ord_trace, kDictParts * 32 * sizeof(u64)));
    LOCUST_HIP_CHECK(hipMemset(d_ord_trace, 0, kDictParts * 32 * sizeof(u64)));
  }
  return d_ord_trace;
}

u64* DevicePipeline::map_trace() {
  static const bool on = std::getenv("LOCUST_MAP_TRACE") != nullptr;
  if (!on) return nullptr;
  if (!d_map_trace) {
    LOCUST_HIP_CHECK(hipMalloc(&d_map_trace, 4096 * 8 * sizeof(u64)));
    LOCUST_HIP_CHECK(hipMemset(d_map_trace, 0, 4096 * 8 * sizeof(u64)));
  }
  return d_map_trace;
}

void DevicePipeline::print_map_trace() {
  if (!d_map_trace || warming) return;
  std::vector<u64> t(4096 * 8);
  LOCUST_HIP_CHECK(hipMemcpy(t.data(), d_map_trace, t.size() * 8, hipMemcpyDeviceToHost));
  u64 t0 = ~0ull;
  for (int i = 0; i < 4096; ++i)
    if (t[i * 8]) t0 = std::min(t0, t[i * 8]);
  for (int i = 0; i < 4096; ++i) {
    const u64* x = &t[i * 8];
    if (!x[0] || !x[5]) continue;
    // (small grouped tiles: 6 = wave 0's masks done, 7 = its keys packed and ranked, 3 =
    // the barrier after; large grouped tiles: 6 = records reserved)
    std::fprintf(stderr, "map tile=%4d entry=%6.2f acquired=%6.2f staged=%6.2f masks=%6.2f "
                 "prefix=%6.2f reserved=%6.2f done=%6.2f w0masks=%6.2f w0packed=%6.2f us\n", i,
                 (x[0] - t0) * 0.01, (x[1] - t0) * 0.01, (x[2] - t0) * 0.01, (x[3] - t0) * 0.01,
                 (x[4] - t0) * 0.01, x[6] ? (x[6] - t0) * 0.01 : 0.0, (x[5] - t0) * 0.01,
                 x[6] ? (x[6] - t0) * 0.01 : 0.0, x[7] ? (x[7] - t0) * 0.01 : 0.0);
  }
}

u64* DevicePipeline::partials_trace() {
  static const bool on = std::getenv("LOCUST_ORD_TRACE") != nullptr;
  if (!on) return nullptr;
  if (!d_partials_trace) {
    LOCUST_HIP_CHECK(hipMalloc(&d_partials_trace, (u64)kDictParts * kMaxPartialSlots * 8 * sizeof(u64)));
    LOCUST_HIP_CHECK(hipMemset(d_partials_trace, 0, (u64)kDictParts * kMaxPartialSlots * 8 * sizeof(u64)));
  }
  return d_partials_trace;
}

void DevicePipeline::print_partials_trace() {
  if (!d_partials_trace || warming) return;
  const u64 ns = std::max<u32>(partial_nslots, 1), nb = (u64)kDictParts * ns;
  std::vector<u64> t(nb * 8);  // slot b = p * ns + k
  LOCUST_HIP_CHECK(hipMemcpy(t.data(), d_partials_trace, t.size() * 8, hipMemcpyDeviceToHost));
  LOCUST_HIP_CHECK(hipMemset(d_partials_trace, 0, t.size() * 8));
  u64 t0 = ~0ull, t1 = 0, tok = 0;
  for (u64 b = 0; b < nb; ++b) {
    if (!t[b * 8]) continue;
    t0 = std::min(t0, t[b * 8]);
    t1 = std::max(t1, t[b * 8 + 3]);
    tok += t[b * 8 + 4];
  }
  std::fprintf(stderr, "partials span=%.2f us, tokens=%llu\n", (t1 - t0) * 0.01,
               (unsigned long long)tok);
  for (u64 b = 0; b < nb; ++b) {
    const u64* x = &t[b * 8];
    if (!x[0]) continue;
    std::fprintf(stderr, "partials b=%4llu p=%3llu k=%llu in=%7.2f clear=%6.2f insert=%7.2f "
                 "out=%7.2f tok=%7llu distinct=%5llu\n", (unsigned long long)b,
                 (unsigned long long)(b / ns), (unsigned long long)(b % ns),
                 (x[0] - t0) * 0.01, (x[1] - x[0]) * 0.01, (x[2] - x[1]) * 0.01,
                 (x[3] - t0) * 0.01, (unsigned long long)x[4], (unsigned long long)x[5]);
  }
}

void DevicePipeline::print_psort_trace() {
  if (!d_ord_trace) return;
  std::vector<u64> t(kDictParts * 16);
  LOCUST_HIP_CHECK(hipMemcpy(t.data(), d_ord_trace, t.size() * 8, hipMemcpyDeviceToHost));
  u64 first_in = ~0ull, last_out = 0;
  int last_p = -1;
  for (int p = 0; p < kDictParts; ++p) {
    const u64* x = &t[p * 16];
    if (!x[10]) continue;
    first_in = std::min(first_in, x[10]);
    if (x[11] > last_out) {
      last_out = x[11];
      last_p = p;
    }
  }
  if (last_p >= 0)
    std::fprintf(stderr, "psort span=%.2f us (first entry -> last exit), last p=%d m=%llu\n",
                 (last_out - first_in) * 0.01, last_p, (unsigned long long)t[last_p * 16 + 5]);
  for (int p = 0; p < kDictParts; ++p) {
    const u64* x = &t[p * 16];
    if (!x[0] || !x[4]) continue;
    auto d = [&](int a, int b) { return (unsigned long long)(x[a] && x[b] ? x[b] - x[a] : 0); };
    std::fprintf(stderr, "psort p=%3d m=%5llu passes=%2llu list=%6llu keys=%6llu sort=%6llu "
                 "write=%6llu | in=%6.2f out=%6.2f us\n", p, (unsigned long long)x[5],
                 (unsigned long long)x[6], d(0, 1), d(1, 2), d(2, 3), d(3, 4),
                 (x[10] - first_in) * 0.01, (x[11] - first_in) * 0.01);
  }
}

void DevicePipeline::print_ord_trace() {
  if (!d_ord_trace || warming) return;
  std::vector<u64> t(kDictParts * 32);
  LOCUST_HIP_CHECK(hipMemcpy(t.data(), d_ord_trace, t.size() * 8, hipMemcpyDeviceToHost));
  // stamps: 0 start, 1 built, 2 published, 8 histogram, 7 bucketed, 9 ranked, 3 sorted,
  // 4 prefix known, 5 written; 6 = distinct keys; 10 / 11 = entry / exit on the 100 MHz
  // device-wide clock (the kernel's critical path across workgroups)
  u64 first_in = ~0ull, last_out = 0;
  int last_p = -1;
  for (int p = 0; p < kDictParts; ++p) {
    const u64* x = &t[p * 32];
    if (!x[10]) continue;
    first_in = std::min(first_in, x[10]);
    if (x[11] > last_out) {
      last_out = x[11];
      last_p = p;
    }
  }
  if (last_p >= 0)
    std::fprintf(stderr, "ord span=%.2f us (first entry -> last exit), last p=%d m=%llu\n",
                 (last_out - first_in) * 0.01, last_p, (unsigned long long)t[last_p * 32 + 6]);
  {  // self-clean handshake: each workgroup's release + done count (25), the last one's
     // re-zeroing done (24; stale values from earlier jobs are older than this job's exits)
    u64 done_max = 0, clean = 0;
    for (int p = 0; p < kDictParts; ++p) {
      done_max = std::max(done_max, t[p * 32 + 25]);
      clean = std::max(clean, t[p * 32 + 24]);
    }
    if (last_p >= 0 && done_max >= last_out)
      std::fprintf(stderr, "ord tail: last exit -> last done count %.2f us, -> self-clean done %.2f us\n",
                   (done_max - last_out) * 0.01, clean >= last_out ? (clean - last_out) * 0.01 : -1.0);
  }

  for (int p = 0; p < kDictParts; ++p) {
    const u64* x = &t[p * 32];
    if (!x[0] || !x[6]) continue;
    auto d = [&](int a, int b) { return (unsigned long long)(x[a] && x[b] ? x[b] - x[a] : 0); };
    std::fprintf(stderr,
                 "ord p=%3d m=%5llu build=%6llu publish=%5llu sort=%6llu wait=%6llu write=%6llu"
                 " | hist=%5llu bucket=%5llu rank=%6llu scatter=%5llu | in=%6.2f out=%6.2f us"
                 " | clear=%5llu scan=%5llu fill=%5llu ld=%5llu srt=%5llu list=%5llu gather=%5llu lbk=%6llu rank0=%6llu cand=%6llu tie=%6llu ranks=%6llu"
                 " | waited=%6.2f us | counted=%6.2f us after exit\n",
                 p, (unsigned long long)x[6], d(0, 1), d(1, 2), d(2, 3), d(3, 4), d(4, 5),
                 d(2, 8), d(8, 7), d(7, 9), d(9, 3), (x[10] - first_in) * 0.01,
                 (x[11] - first_in) * 0.01, d(0, 14), d(14, 28), d(28, 26), d(26, 27), d(27, 12), d(14, 12), d(12, 13), d(2, 15), x[17] != ~0ull ? d(2, 17) : 0ull, d(2, 18), d(2, 19), d(2, 16),
                 x[20] ? (x[20] - x[10]) * 0.01 : 0.0,
                 x[25] >= x[11] ? (x[25] - x[11]) * 0.01 : -1.0);
  }
}

bool DevicePipeline::enqueue_dict_job(u32 num_lines, bool compat, bool with_counts, hipEvent_t after_process,
                        bool self_clean) {
  job_self_cleaned = false;
  if (!compat && ordered_ok()) {
    job_self_cleaned = self_clean && cfg.map_path == MapPath::kFast;
    enqueue_dict_ordered(with_counts, /*mapped=*/true, job_self_cleaned);
    if (after_process) LOCUST_HIP_CHECK(hipEventRecord(after_process, stream));
    return true;
  }
  if (!compat && !with_counts && large_ordered_ok()) {
    // large pass: per-slice partials (Process), then merge + sort + records (Reduce)
    enqueue_partials();
    if (after_process) LOCUST_HIP_CHECK(hipEventRecord(after_process, stream));
    OrderedExtra ex;
    ex.pm = part_map();
    ex.part_w = d_pw;
    ex.out_cap = h_out_cap;
    set_compact_out(ex, true);
    launch_dict_ordered_partials(d_partials, d_partial_n, partial_nslots, d_ctr, d_out_mapped,
                                 d_ctr_mapped,
                                 lb_dict, stream, ord_trace(), ex);
    return true;
  }
  enqueue_process_dict(num_lines, compat, with_counts);
  if (after_process) LOCUST_HIP_CHECK(hipEventRecord(after_process, stream));
  enqueue_emit_dict(/*mapped=*/true);
  return false;
}

void DevicePipeline::redo_dict_on_table(u32 num_lines, bool with_counts) {
  LOCUST_HIP_CHECK(hipMemsetAsync(&d_ctr->num_unique, 0, sizeof(u32), stream));
  LOCUST_HIP_CHECK(hipMemsetAsync(&d_ctr->flags, 0, sizeof(u32), stream));
  LOCUST_HIP_CHECK(hipMemsetAsync(dict.table, 0, dict_zero_bytes, stream));
  launch_dict_insert(tokens, with_counts ? d_counts : nullptr, &d_ctr->num_records, cap, dict,
                     d_ctr, stream);
  enqueue_rank();
  enqueue_emit_dict(/*mapped=*/true);
  sync();
  *h_ctr = *h_ctr_mapped;
}

void DevicePipeline::finish_dict_with_radix(u32 num_lines, bool with_counts) {
  if (h_ctr->flags & kCtrDictOverflow) {
    // table overflow: sort every record and reduce the reference way
    LOCUST_HIP_CHECK(hipMemsetAsync(lb_heads.status, 0, 8 * (div_up(cap, kReduceTile) + 1), stream));
    LOCUST_HIP_CHECK(hipMemsetAsync(lb_heads.tile_counter, 0, 4, stream));
    LOCUST_HIP_CHECK(hipMemsetAsync(lb_scan.status, 0, 8 * (div_up(cap, kReduceTile) + 1), stream));
    LOCUST_HIP_CHECK(hipMemsetAsync(lb_scan.tile_counter, 0, 4, stream));
    enqueue_process(num_lines, false, with_counts, h_ctr->num_records);
    enqueue_reduce_core(with_counts);
    enqueue_pack_output();
    return;
  }
  LOCUST_HIP_CHECK(hipMemsetAsync(lb_scan.status, 0, 8 * (div_up(cap, kReduceTile) + 1), stream));
  LOCUST_HIP_CHECK(hipMemsetAsync(lb_scan.tile_counter, 0, 4, stream));
  radix_sort(dict.ukeys, &d_ctr->num_unique, h_ctr->num_unique, rx, dict.ucount, sorted,
             d_sorted_counts, d_perm, h_plan, stream);
  enqueue_reduce_dict();
}

void DevicePipeline::download_output(WordCountResult& r, hipEvent_t done) {
  read_counters();
  const u64 u = h_ctr->num_unique;
  grow_host_out(u);
  if (u)
    launch_copy_to_mapped(d_out_mapped, d_out, u * sizeof(OutRecord), stream);
  if (done) LOCUST_HIP_CHECK(hipEventRecord(done, stream));
  sync();
  fill_counters(r);
  copy_out(r.entries, u);
}

void DevicePipeline::set_compact_out(OrderedExtra& ex, bool mapped) {
  ord_compact = mapped;
  if (!ord_compact) return;
  ex.cout = reinterpret_cast<u64*>(d_out_mapped);
  ex.ctab = d_ctab_mapped;
  ex.out_cap = std::min<u64>(ex.out_cap, h_out_cap);
}

void DevicePipeline::copy_out(EntryList& e, u64 u, bool compact) {
  static_assert(sizeof(WordCountEntry) == sizeof(OutRecord), "entry layout");
  static_assert(offsetof(WordCountEntry, count) == offsetof(OutRecord, count), "entry layout");
  LOCUST_CHECK_ARG(u <= h_out_cap, "output larger than its buffer");
  if (!compact) return e.adopt(out_pool[out_idx], reinterpret_cast<WordCountEntry*>(h_out), u);
  std::vector<EntrySegment> segs;
  segs.reserve(64);
  const u64* words = reinterpret_cast<const u64*>(h_out);
  u64 at = 0;  // entries so far
  for (int v = 0; v < kDictParts; ++v) {
    const u64 t = h_ctab[v];
    LOCUST_CHECK_ARG(t != ~0ull, "compact output: partition " + std::to_string(v) + " not written");
    const u64 m = t & 0xffffull, first = t >> 32;  // first: where its entries start
    LOCUST_CHECK_ARG(first + m <= h_out_cap, "compact output: partition " + std::to_string(v) +
                                                 " past the buffer");
    if (m) segs.push_back({words + kOutWords * first, m});
    at += m;
  }
  LOCUST_CHECK_ARG(at == u, "compact output: " + std::to_string(at) + " entries, expected " +
                                std::to_string(u));
  e.adopt_compact(out_pool[out_idx], std::move(segs), u);
}

void DevicePipeline::fill_counters(WordCountResult& r) const {
  r.num_tokens = h_ctr->total_count ? h_ctr->total_count : h_ctr->num_records;
  r.num_unique = h_ctr->num_unique;
  r.overflow_lines = h_ctr->overflow_lines;
  r.truncated = h_ctr->truncated;
  r.max_key_len = h_ctr->max_key_len;
}

WordCountResult DevicePipeline::run_ref_timed(const TextInput& in) {
  check_input(in);
  WordCountResult r;
  r.num_lines = in.num_lines;
  const bool compat = cfg.map_path == MapPath::kCompat;
  const bool dict_path = cfg.sort_path == SortPath::kDict;
  const u64 w0 = now_ns();
  enqueue_upload(in);
  sync();
  const u64 t0 = now_ns();
  enqueue_map(in);  // map timer: the launch only (main.cu:405-407)
  const u64 t1 = now_ns();
  if (dict_path) {
    enqueue_process_dict((u32)in.num_lines, compat);
  } else {
    enqueue_process((u32)in.num_lines, compat, false, kUnknownCount, /*allow_psort=*/true);
  }
  sync();  // process timer ends once the sort is done (thrust::sort returns)
  if (!dict_path && psort_used) {
    read_counters();
    if (h_ctr->flags & kCtrSortOverflow) {  // a partition outgrew the LDS sort
      redo_process_general((u32)in.num_lines);
      sync();
    }
  }
  const u64 t2 = now_ns();
  if (dict_path) {
    enqueue_emit_dict(/*mapped=*/true);  // the last reduce kernel: launch only (B4)
  } else {
    enqueue_reduce_core(false);
    enqueue_pack_output();
  }
  const u64 t3 = now_ns();
  if (dict_path) {
    sync();
    *h_ctr = *h_ctr_mapped;
    if (dict_fallback_needed()) {
      finish_dict_with_radix((u32)in.num_lines);
      download_output(r, nullptr);
    } else {
      fill_counters(r);
      copy_out(r.entries, h_ctr->num_unique);
    }
  } else {
    download_output(r, nullptr);
  }
  r.times.ref_map_ms = (t1 - t0) * 1e-6;
  r.times.ref_process_ms = (t2 - t1) * 1e-6;
  r.times.ref_reduce_ms = (t3 - t2) * 1e-6;
  r.times.wall_ms = (now_ns() - w0) * 1e-6;
  if (cfg.check) validate_result(r);
  return r;
}

WordCountResult DevicePipeline::run(const TextInput& in) {
  TraceRange tr("locust:job");
  const u64 tp = now_ns();
  poll_retune();
  const u64 tq = now_ns();
  select_out();  // the previous result may still hold the last output buffer
  if ((int)log_level() >= (int)LogLevel::kDebug)
    LOCUST_LOG_DEBUG("job prologue: retune adoption %.3f ms, output buffer %.3f ms",
                     (tq - tp) * 1e-6, (now_ns() - tq) * 1e-6);
  // The previous job left d_sync zeroed (self-cleaning ordered run): no reset this time.
  const bool clean_start = sync_clean;
  sync_clean = false;
  if (in.bytes > pass_bytes && cfg.sort_path == SortPath::kDict &&
      cfg.map_path == MapPath::kFast)
    return run_stream(in);
  if (cfg.ref_timers) return run_ref_timed(in);
  check_input(in);
  WordCountResult r;
  r.num_lines = in.num_lines;
  const u64 t0 = now_ns();
  const bool compat = cfg.map_path == MapPath::kCompat;
  const bool dict_path = cfg.sort_path == SortPath::kDict;
  struct ClearOnExit {  // only this entry point's dictionary pass combines in the map
    bool& f;
    ~ClearOnExit() { f = false; }
  } clear_combine{combine_map};
  combine_map = dict_path && !compat && large_ordered;
  const bool graphed = use_job_graph(in);
  // lean: a small single-pass job launched directly, no stage events, completion polled
  const bool lean = !graphed && lean_job(in);
  split_stages = !lean && !graphed;
  skip_sync_reset = clean_start && !compat;
  if (!lean) LOCUST_HIP_CHECK(hipEventRecord(ev[0], stream));
  const bool dbg = (int)log_level() >= (int)LogLevel::kDebug;
  u64 t_map = 0;
  if (lean) {
    enqueue_upload(in);
    enqueue_map(in);
    if (dbg) t_map = now_ns();
  } else if (graphed) {
    prepare_upload(in);
    launch_dict_graph(in, compat);
    LOCUST_HIP_CHECK(hipEventRecord(ev[5], stream));  // a replay has no stage split
    r.times.graph = true;
  } else {
    enqueue_upload(in);
    // Auto mode, piecewise pass: no stage markers between the kernels (the pass
    // interleaves Map and Process anyway); graph=0 keeps the split
    split_stages = pieces.empty() || cfg.graph == 0;
    if (split_stages) LOCUST_HIP_CHECK(hipEventRecord(ev[1], stream));
    enqueue_map(in);
    if (split_stages) {
      LOCUST_HIP_CHECK(hipEventRecord(ev[2], stream));
      // a piecewise pass interleaves Process (the per-piece partials) with Map: one
      // boundary, and no marker between the last partials and the ordered kernel
      if (!pieces.empty()) LOCUST_HIP_CHECK(hipEventRecord(ev[3], stream));
    }
  }
  if (dict_path) {
    bool ordered = graph_ordered;
    if (lean) {
      done_pending = ++done_seq;
      ordered = enqueue_dict_job((u32)in.num_lines, compat, false, nullptr,
                                 /*self_clean=*/true);
      if (done_pending) publish_done(done_seq);
      done_pending = 0;
    } else if (!graphed) {
      ordered = enqueue_dict_job((u32)in.num_lines, compat, false,
                                 split_stages && pieces.empty() ? ev[3] : nullptr,
                                 /*self_clean=*/true);
      if (split_stages) LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
      LOCUST_HIP_CHECK(hipEventRecord(ev[5], stream));
    }
    skip_sync_reset = false;
    const u64 t_launched = now_ns();
    if (dbg && lean)
      LOCUST_LOG_DEBUG("lean job: map launched +%.4f ms, ordered launched +%.4f ms",
                       (t_map - t0) * 1e-6, (t_launched - t0) * 1e-6);
    if (lean)
      wait_done(done_seq);
    else
      sync();  // the one host synchronisation of a dictionary run
    const u64 t_synced = now_ns();
    r.times.host_launch_ms = (t_launched - t0) * 1e-6;
    r.times.host_wait_ms = (t_synced - t_launched) * 1e-6;
    *h_ctr = *h_ctr_mapped;
    if (ordered && h_ctr->num_unique > h_out_cap) h_ctr->flags |= kCtrDictOverflow;  // no records
    const bool ordered_done = ordered && !(h_ctr->flags & kCtrDictOverflow);
    sync_clean = ordered_done && !compat && job_self_cleaned;  // the kernel re-zeroed its scratch
    if (ordered) print_ord_trace();
    print_partials_trace();
    print_map_trace();
    if (ordered && !ordered_done) ++fallbacks;
    if (devplan_used) ++planned_passes;
    if (ordered && !ordered_done) redo_dict_on_table((u32)in.num_lines, map_combined);
    if (!ordered_done && dict_fallback_needed()) {
      finish_dict_with_radix((u32)in.num_lines, map_combined);
      LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
      download_output(r, ev[5]);
      if (ordered) force_retune(r.entries);
    } else {
      fill_counters(r);
      copy_out(r.entries, h_ctr->num_unique, ordered_done && ord_compact);
      r.times.host_copy_ms = (now_ns() - t_synced) * 1e-6;
      if (ordered_done) maybe_retune(r.entries);
      else if (ordered) force_retune(r.entries);
    }
  } else {
    if (lean) {
      done_pending = ++done_seq;  // the fused kernel publishes it itself
      enqueue_radix_job((u32)in.num_lines, compat, nullptr, nullptr);
      if (done_pending) publish_done(done_seq);
      done_pending = 0;
    } else if (!graphed) {
      enqueue_radix_job((u32)in.num_lines, compat, ev[3], ev[4]);
    }
    skip_sync_reset = false;
    bool overflow;
    if (radix_mapped()) {  // records and counters already in host memory
      if (lean) {
        wait_done(done_seq);
      } else {
        if (!graphed) LOCUST_HIP_CHECK(hipEventRecord(ev[5], stream));
        sync();  // the one host synchronisation of a radix run
      }
      *h_ctr = *h_ctr_mapped;
      overflow = (h_ctr->flags & kCtrSortOverflow) != 0;
      // a fused run re-zeroed its scratch (not replayed from a graph: those reset it)
      sync_clean = lean && radix_fused && !overflow && !compat;
      if (psort_used) print_psort_trace();
      if (!overflow) {
        fill_counters(r);
        copy_out(r.entries, h_ctr->num_unique);
        if (psort_used) maybe_retune(r.entries);
      }
    } else {
      download_output(r, ev[5]);
      overflow = (h_ctr->flags & kCtrSortOverflow) != 0;
    }
    if (overflow) {  // a partition outgrew the LDS sort: the device-wide sort instead
      redo_radix_general((u32)in.num_lines);
      LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
      download_output(r, ev[5]);
    }
  }
  r.times.wall_ms = (now_ns() - t0) * 1e-6;
  r.times.lean = lean;
  if (lean) {  // no device timestamps: the job's wall time
    r.times.gpu_ms = r.times.wall_ms;
  } else {
    if (!graphed && split_stages) {
      r.times.h2d_ms = ms_between(ev[0], ev[1]);
      r.times.map_ms = ms_between(ev[1], ev[2]);
      r.times.process_ms = ms_between(ev[2], ev[3]);
      r.times.reduce_ms = ms_between(ev[3], ev[4]);
      r.times.d2h_ms = ms_between(ev[4], ev[5]);
    }
    r.times.gpu_ms = ms_between(ev[0], ev[5]);
  }
  if (cfg.check) validate_result(r);
  return r;
}

// =====================================================================================
// Top-K by count
// =====================================================================================
void DevicePipeline::ensure_topk(u64 n) {
  if (!h_top) {
    // first top job of this engine: the mapped top records (+ the word the final kernel
    // writes their number to) and the events
    h_top = static_cast<TopRecord*>(pinned_alloc((kTopKMax + 1) * sizeof(TopRecord),
                                                 hipHostMallocMapped | hipHostMallocCoherent,
                                                 "mapped top-k records"));
    LOCUST_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_top_mapped), h_top, 0));
    for (auto& e : ev_top) LOCUST_HIP_CHECK(hipEventCreate(&e));
  }
  if (topk.cap >= std::max<u64>(n, 1)) return;
  sync();  // nothing in flight may still use the workspace being replaced
  if (d_topk) LOCUST_HIP_CHECK(hipFree(d_topk));
  d_topk = nullptr;
  topk = TopKWorkspace{};
  // room for what this engine's passes can leave in d_out, at least for this job
  const u64 want = std::max<u64>({n, std::min<u64>(std::max(ucap, rcap), 1ull << 20), 1});
  const u64 bytes = topk_workspace_bytes(want);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("top-k selection workspace (" + std::to_string(bytes) + " B for " +
                std::to_string(want) + " records, plus " +
                std::to_string((kTopKMax + 1) * sizeof(TopRecord)) +
                " B of pinned top records) does not fit the free device memory (" +
                std::to_string(fr) + " B of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_topk), bytes));
  topk_bytes = bytes;
  topk_workspace_carve(d_topk, want, &topk);
}

void DevicePipeline::check_top_job(u32 k) const {
  LOCUST_CHECK_ARG(k >= 1, "top-k: k must be at least 1");
  LOCUST_CHECK_ARG(k <= kTopKMax,
                   "top-k: k = " + std::to_string(k) + " exceeds the device selection's limit "
                   "kTopKMax = " + std::to_string(kTopKMax) + "; take the full result and "
                   "select on the host (top_entries / Result.top)");
}

void DevicePipeline::enqueue_top_select(const OutRecord* recs, u64 n, u32 k) {
  TraceRange tr("locust:top_select");
  ensure_topk(n);
  LOCUST_HIP_CHECK(hipEventRecord(ev_top[0], stream));
  launch_top_select(recs, n, k, topk, d_top_mapped, reinterpret_cast<u32*>(d_top_mapped + kTopKMax),
                    stream);
  LOCUST_HIP_CHECK(hipEventRecord(ev_top[1], stream));
}

void DevicePipeline::collect_top(u64 n, u32 k, TopResult* t) {
  static_assert(offsetof(TopEntry, count) == offsetof(TopRecord, count) &&
                    offsetof(TopEntry, val) == offsetof(TopRecord, val),
                "entry layout");
  const u64 m = *reinterpret_cast<const u32*>(h_top + kTopKMax);
  LOCUST_CHECK_ARG(m == std::min<u64>(k, n), "top-k selection wrote " + std::to_string(m) +
                                                 " records, expected " +
                                                 std::to_string(std::min<u64>(k, n)));
  t->k = k;
  t->entries.resize(m);
  if (m) std::memcpy(t->entries.data(), h_top, m * sizeof(TopRecord));
  t->select_ms = ms_between(ev_top[0], ev_top[1]);
  t->wire_bytes = m * sizeof(TopRecord) + sizeof(u64);
}

void DevicePipeline::finish_top(u32 num_lines, u32 k, bool streamed, TopResult* t) {
  read_counters();  // (synchronises)
  if (streamed && (h_ctr->flags & kCtrDictOverflow))
    throw Error("streaming dictionary overflow: more than " + std::to_string(ucap) +
                " distinct keys; use a larger chunk size");
  if (dict_fallback_needed()) {
    // more distinct keys than the rank sort takes, or a full table: the radix path, which
    // also ends in d_out
    finish_dict_with_radix(num_lines);
    LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
    read_counters();
  }
  const u64 n = h_ctr->num_unique;
  LOCUST_CHECK_ARG(n <= rcap, "top-k: more distinct keys than the record buffer holds");
  enqueue_top_select(d_out, n, k);
  sync();
  collect_top(n, k, t);
  t->num_unique = n;
}

TopResult DevicePipeline::run_top(const TextInput& in, u32 k) {
  TraceRange tr("locust:top_job");
  LOCUST_CHECK_ARG(cfg.sort_path == SortPath::kDict,
                   "a top-k job needs a dictionary engine (sort=dict)");
  LOCUST_CHECK_ARG(!cfg.ref_timers, "a top-k job does not take ref_timers");
  LOCUST_CHECK_ARG(!cfg.records_only, "a records-only engine runs no text jobs");
  check_top_job(k);
  sync_clean = false;  // this entry point dirties d_sync
  const bool compat = cfg.map_path == MapPath::kCompat;
  TopResult t;
  t.num_lines = in.num_lines;
  const u64 t0 = now_ns();
  LOCUST_HIP_CHECK(hipEventRecord(ev[0], stream));
  if (in.bytes > pass_bytes && !compat) {
    // larger than a pass: every chunk into one dictionary, ranked and emitted once
    LOCUST_HIP_CHECK(hipEventRecord(ev[1], stream));
    const size_t nchunks = enqueue_stream_insert(in);
    LOCUST_HIP_CHECK(hipEventRecord(ev[2], stream));
    enqueue_rank();
    LOCUST_HIP_CHECK(hipEventRecord(ev[3], stream));
    enqueue_emit_dict(/*mapped=*/false);
    LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
    finish_top(0, k, true, &t);
    WordCountResult st;
    stream_stats(nchunks, st);
    t.num_tokens = st.num_tokens;
    t.overflow_lines = st.overflow_lines;
    t.truncated = st.truncated;
    t.max_key_len = st.max_key_len;
    t.chunks = st.chunks;
  } else {
    check_input(in);
    enqueue_upload(in);
    LOCUST_HIP_CHECK(hipEventRecord(ev[1], stream));
    enqueue_map(in);
    LOCUST_HIP_CHECK(hipEventRecord(ev[2], stream));
    enqueue_process_dict((u32)in.num_lines, compat);
    LOCUST_HIP_CHECK(hipEventRecord(ev[3], stream));
    enqueue_emit_dict(/*mapped=*/false);
    LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
    finish_top((u32)in.num_lines, k, false, &t);
    WordCountResult st;
    fill_counters(st);
    t.num_tokens = st.num_tokens;
    t.overflow_lines = st.overflow_lines;
    t.truncated = st.truncated;
    t.max_key_len = st.max_key_len;
    t.times.h2d_ms = ms_between(ev[0], ev[1]);
  }
  t.times.map_ms = ms_between(ev[1], ev[2]);
  t.times.process_ms = ms_between(ev[2], ev[3]);
  t.times.reduce_ms = ms_between(ev[3], ev[4]);
  t.times.gpu_ms = ms_between(ev[0], ev_top[1]);
  t.times.wall_ms = (now_ns() - t0) * 1e-6;
  if (cfg.check) validate_top(t);
  return t;
}

TopResult DevicePipeline::run_top_source(TextSource& src, u32 k) {
  TraceRange tr("locust:top_job");
  LOCUST_CHECK_ARG(cfg.sort_path == SortPath::kDict,
                   "a top-k job needs a dictionary engine (sort=dict)");
  LOCUST_CHECK_ARG(!cfg.ref_timers, "a top-k job does not take ref_timers");
  check_top_job(k);
  sync_clean = false;
  TopResult t;
  const u64 t0 = now_ns();
  LOCUST_HIP_CHECK(hipEventRecord(ev[0], stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev[1], stream));
  const size_t nchunks = enqueue_stream_source(src);
  LOCUST_HIP_CHECK(hipEventRecord(ev[2], stream));
  enqueue_rank();
  LOCUST_HIP_CHECK(hipEventRecord(ev[3], stream));
  enqueue_emit_dict(/*mapped=*/false);
  LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
  finish_top(0, k, true, &t);
  WordCountResult st;
  stream_stats(nchunks, st);
  t.num_lines = src.lines();
  t.num_tokens = st.num_tokens;
  t.overflow_lines = st.overflow_lines;
  t.truncated = st.truncated;
  t.max_key_len = st.max_key_len;
  t.chunks = st.chunks;
  t.times.map_ms = ms_between(ev[1], ev[2]);
  t.times.process_ms = ms_between(ev[2], ev[3]);
  t.times.reduce_ms = ms_between(ev[3], ev[4]);
  t.times.gpu_ms = ms_between(ev[0], ev_top[1]);
  t.times.wall_ms = (now_ns() - t0) * 1e-6;
  if (cfg.check) validate_top(t);
  return t;
}

TopResult DevicePipeline::top_counts(const KeyCount* recs, u64 n, u32 k) {
  static_assert(sizeof(KeyCount) == sizeof(OutRecord) &&
                    offsetof(KeyCount, count) == offsetof(OutRecord, count),
                "record layout");
  check_top_job(k);
  LOCUST_CHECK_ARG(n <= slot_records_cap(), "too many records for engine capacity");
  sync_clean = false;
  TopResult t;
  const u64 t0 = now_ns();
  if (n)
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_records, recs, n * sizeof(KeyCount), hipMemcpyHostToDevice,
                                    stream));
  enqueue_top_select(reinterpret_cast<const OutRecord*>(d_records), n, k);
  sync();
  collect_top(n, k, &t);
  t.num_unique = n;
  for (u64 i = 0; i < n; ++i) t.num_tokens += recs[i].count;
  t.times.gpu_ms = t.select_ms;
  t.times.wall_ms = (now_ns() - t0) * 1e-6;
  if (cfg.check) validate_top(t);
  return t;
}

// =====================================================================================
// Inverted index
// =====================================================================================
void DevicePipeline::ensure_index(u64 tokens, u64 n) {
  if (!h_ictr) {
    // first index job of this engine: the pinned counters and the events
    h_ictr = static_cast<IndexCounters*>(
        pinned_alloc(sizeof(IndexCounters), hipHostMallocDefault, "index counters"));
    for (auto& e : ev_index) LOCUST_HIP_CHECK(hipEventCreate(&e));
  }
  if (h_post_cap < tokens) {
    sync();  // (no copy into the old buffer is in flight: every job ends synchronised)
    pinned_free(h_post);
    h_post = nullptr;
    h_post_cap = align_up(std::max<u64>(tokens, 1), (u64)kSortTile);
    h_post = static_cast<u32*>(
        pinned_alloc(h_post_cap * sizeof(u32), hipHostMallocDefault, "index postings"));
  }
  if (index.pair_cap >= std::max<u64>(tokens, 1) && index.rec_cap >= std::max<u64>(n, 1)) return;
  sync();  // nothing in flight may still use the workspace being replaced
  if (d_index) LOCUST_HIP_CHECK(hipFree(d_index));
  d_index = nullptr;
  index = IndexWorkspace{};
  index_bytes = 0;
  // sized for this job (whole sort tiles: the sort zeroes its status words for the
  // capacity, not for the job) and for what this engine's passes can hold otherwise
  const u64 pair_cap = align_up(std::max<u64>(tokens, 1), (u64)kSortTile);
  const u64 rec_cap = std::max<u64>({n, std::min<u64>(std::max(ucap, rcap), 1ull << 20), 1});
  const u64 bytes = index_workspace_bytes(pair_cap, rec_cap, cap_lines, pass_bytes);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("index workspace (" + std::to_string(bytes) + " B needed for " +
                std::to_string(pair_cap) + " tokens, " + std::to_string(rec_cap) +
                " records and " + std::to_string(cap_lines) +
                " lines) does not fit the free device memory (" + std::to_string(fr) +
                " B free of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_index), bytes));
  index_bytes = bytes;
  index_workspace_carve(d_index, pair_cap, rec_cap, cap_lines, pass_bytes, &index);
  LOCUST_HIP_CHECK(hipMemsetAsync(index.zeros, 0, pair_cap * 8, stream));
}

void DevicePipeline::check_index_job(const TextInput& in) const {
  LOCUST_CHECK_ARG(cfg.sort_path == SortPath::kDict,
                   "an index job needs a dictionary engine (sort=dict), not sort=radix");
  LOCUST_CHECK_ARG(cfg.map_path != MapPath::kCompat,
                   "an index job needs the fast map (map_path fast): the compat map "
                   "overwrites the delimiters of the device text, which the index stage "
                   "tokenises again");
  LOCUST_CHECK_ARG(cfg.ngram == 1,
                   "an index job builds word keys only (ngram 1): run it without ngram");
  LOCUST_CHECK_ARG(!cfg.ref_timers, "an index job does not take ref_timers");
  LOCUST_CHECK_ARG(!cfg.records_only, "a records-only engine runs no text jobs");
  LOCUST_CHECK_ARG(!in.source && in.bytes <= pass_bytes,
                   "an index job takes one device pass (" + std::to_string(pass_bytes) +
                       " B here), not a streamed input of " + std::to_string(in.bytes) +
                       " B: use --backend cpu (the CPU engine indexes any size)");
}

void DevicePipeline::enqueue_index_job(const TextInput& in, WordCountResult& r,
                                       bool ship_postings, u64* n_out, u64* T_out) {
  check_index_job(in);
  check_input(in);
  LOCUST_CHECK_ARG(in.first_line + in.num_lines <= (1ull << 32),
                   "index: line numbers past 2^32 do not fit a u32 posting");
  select_out();        // the previous result may still hold the last output buffer
  sync_clean = false;  // this entry point dirties d_sync
  r.num_lines = in.num_lines;
  // the word job, its records left in d_out (as a top job)
  LOCUST_HIP_CHECK(hipEventRecord(ev[0], stream));
  enqueue_upload(in);
  LOCUST_HIP_CHECK(hipEventRecord(ev[1], stream));
  enqueue_map(in);
  LOCUST_HIP_CHECK(hipEventRecord(ev[2], stream));
  enqueue_process_dict((u32)in.num_lines, false);
  LOCUST_HIP_CHECK(hipEventRecord(ev[3], stream));
  enqueue_emit_dict(/*mapped=*/false);
  LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
  read_counters();  // (synchronises)
  if (dict_fallback_needed()) {
    // more distinct keys than the rank sort takes, or a full table: the radix path, which
    // also ends in d_out
    finish_dict_with_radix((u32)in.num_lines);
    LOCUST_HIP_CHECK(hipEventRecord(ev[4], stream));
    read_counters();
  }
  fill_counters(r);
  const u64 n = h_ctr->num_unique, T = r.num_tokens;
  LOCUST_CHECK_ARG(n <= rcap, "index: more distinct keys than the record buffer holds");
  LOCUST_CHECK_ARG(n < (1ull << 32) && T < (1ull << 32),
                   "index: " + std::to_string(n) + " words / " + std::to_string(T) +
                       " tokens do not fit the 32-bit halves of a pair word");
  // the index stage
  ensure_index(T, n);
  LOCUST_HIP_CHECK(hipEventRecord(ev_index[0], stream));
  // The text stays resident for phrase queries, and the resident copy must be the engine's
  // own: a zero-copy job's map read the pinned staging buffer, which the caller may refill
  // between jobs.  d_text is idle in that mode; the copy (with the 16 zero bytes behind the
  // text) runs inside the index stage's interval, so the word job's stage timers are as
  // they were.  Every other upload mode already ended in d_text.  The stage itself then reads
  // the copy too: three passes over device memory (line index, the map's count and pair
  // walks) instead of three over the host's.
  if (upload_mode == Upload::kZeroCopy)
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_text, h_text, in.bytes + 16, hipMemcpyHostToDevice, stream));
  IndexJob job;
  job.recs = d_out;
  job.n = n;
  job.tokens = T;
  job.text = d_text;
  job.bytes = in.bytes;
  job.num_lines = in.num_lines;
  job.first_line = in.first_line;
  job.dm = make_delim_mask(cfg.delimiters.c_str());
  job.emits_per_line = cfg.emits_per_line;
  job.max_key_len = cfg.max_key_len;
  launch_index(job, index, h_plan, stream);
  if (T && ship_postings)
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_post, index.postings, T * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ictr, index.ctr, sizeof(IndexCounters),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_index[1], stream));
  *n_out = n;
  *T_out = T;
}

void DevicePipeline::check_index_counters(u64 n, u64 T) const {
  const IndexCounters ic = *h_ictr;
  if (ic.miss)
    throw Error("index: " + std::to_string(ic.miss) + " of " + std::to_string(T) +
                " tokens have a key that is not among the " + std::to_string(n) +
                " records of the word job");
  if (ic.written != T || ic.total != T)
    throw Error("index: " + std::to_string(ic.written) + " pairs written, the records' counts "
                "add up to " + std::to_string(ic.total) + ", the word job emitted " +
                std::to_string(T) + " tokens");
  if (ic.misplaced)
    throw Error("index: " + std::to_string(ic.misplaced) + " of " + std::to_string(T) +
                " sorted pairs lie outside their word's range");
}

void DevicePipeline::keep_index(const TextInput& in, const WordCountResult& r, u64 n, u64 T) {
  idx_words = WordCountResult{};  // the statistics only
  idx_words.num_lines = r.num_lines;
  idx_words.num_tokens = r.num_tokens;
  idx_words.num_unique = n;
  idx_words.overflow_lines = r.overflow_lines;
  idx_words.truncated = r.truncated;
  idx_words.max_key_len = r.max_key_len;
  idx_view.recs = d_out;
  idx_view.val = index.val;
  idx_view.postings = index.postings;
  idx_view.n = (u32)n;
  idx_view.first_line = (u32)in.first_line;
  // the text view of the phrase kernel: the device copy, never the staging buffer
  idx_view.text = d_text;
  idx_view.bytes = in.bytes;
  idx_view.nl_pos = index.nl_pos;
  idx_view.lctr = index.lctr;
  idx_view.dm = make_delim_mask(cfg.delimiters.c_str());
  idx_view.emits_per_line = cfg.emits_per_line;
  idx_view.max_key_len = cfg.max_key_len;
  idx_num_lines = in.num_lines;
  idx_tokens = T;
  idx_in_store = false;  // (it lives in the pass buffers until an append moves it)
  idx_ends_nl = in.bytes == 0 || in.data[in.bytes - 1] == '\n';
  idx_segs.reset(in.first_line, in.num_lines);  // one file: "corpus"
  corpus_dirty = true;
  idx_resident = true;
}

IndexResult DevicePipeline::run_index(const TextInput& in) {
  TraceRange tr("locust:index_job");
  idx_resident = false;  // (until this job has left its index)
  IndexResult x;
  x.first_line = in.first_line;
  WordCountResult& r = x.words;
  const u64 t0 = now_ns();
  u64 n = 0, T = 0;
  enqueue_index_job(in, r, /*ship_postings=*/true, &n, &T);
  // the n records, as run()'s fallback paths deliver them
  grow_host_out(n);
  if (n) launch_copy_to_mapped(d_out_mapped, d_out, n * sizeof(OutRecord), stream);
  LOCUST_HIP_CHECK(hipEventRecord(ev[5], stream));
  sync();
  copy_out(r.entries, n);
  check_index_counters(n, T);
  x.postings.assign(h_post, h_post + T);
  x.index_ms = ms_between(ev_index[0], ev_index[1]);
  x.wire_bytes = T * sizeof(u32) + n * sizeof(OutRecord) + sizeof(IndexCounters);
  r.times.h2d_ms = ms_between(ev[0], ev[1]);
  r.times.map_ms = ms_between(ev[1], ev[2]);
  r.times.process_ms = ms_between(ev[2], ev[3]);
  r.times.reduce_ms = ms_between(ev[3], ev[4]);
  r.times.d2h_ms = ms_between(ev_index[1], ev[5]);
  r.times.gpu_ms = ms_between(ev[0], ev[5]);
  r.times.wall_ms = (now_ns() - t0) * 1e-6;
  keep_index(in, r, n, T);
  if (cfg.check) validate_index(x);
  return x;
}

// =====================================================================================
// Index search
// =====================================================================================
namespace {
constexpr u64 kSearchQT = (u64)kSearchMaxQueries * kSearchMaxTerms;
// the pinned result block: [SearchCounters (64 B) | t_len | offsets | q_hits (ranked)]
constexpr u64 kSearchResLen = 64;
constexpr u64 kSearchResOff = kSearchResLen + kSearchQT * sizeof(u32);
constexpr u64 kSearchResHits = kSearchResOff + ((u64)kSearchMaxQueries + 1) * sizeof(u64);
constexpr u64 kSearchResCorpus = kSearchResHits + (u64)kSearchMaxQueries * sizeof(u32);
constexpr u64 kSearchResBytes = kSearchResCorpus + 64;  // (CorpusCounters: "file sets")
}  // namespace

void DevicePipeline::ensure_search() {
  if (d_sbatch) return;
  // first search job of this engine: the batch arrays, the pinned buffers and the events
  const u64 bytes = search_batch_bytes();
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_sbatch), bytes));
  sbatch_bytes = bytes;
  search_batch_carve(d_sbatch, &sbatch);
  h_supload = static_cast<char*>(pinned_alloc(search_upload_bytes(kSearchMaxQueries, true),
                                              hipHostMallocDefault, "search queries"));
  h_sres = static_cast<char*>(pinned_alloc(kSearchResBytes, hipHostMallocDefault, "search result"));
  for (auto& e : ev_search) LOCUST_HIP_CHECK(hipEventCreate(&e));
}

void DevicePipeline::ensure_search_hits(u64 bound) {
  if (shits.cap >= std::max<u64>(bound, 1)) return;
  sync();  // nothing in flight may still use the workspace being replaced
  if (d_shits) LOCUST_HIP_CHECK(hipFree(d_shits));
  d_shits = nullptr;
  shits = SearchHits{};
  shits_bytes = 0;
  // whole sort tiles: the sort zeroes its status words for the capacity, not for the batch
  const u64 cap = align_up(std::max<u64>(bound, 1), (u64)kSortTile);
  const u64 bytes = search_hits_bytes(cap);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("search workspace (" + std::to_string(bytes) + " B needed for " +
                std::to_string(cap) + " list elements) does not fit the free device memory (" +
                std::to_string(fr) + " B free of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_shits), bytes));
  shits_bytes = bytes;
  search_hits_carve(d_shits, cap, &shits);
  LOCUST_HIP_CHECK(hipMemsetAsync(shits.zeros, 0, cap * 8, stream));
}

void DevicePipeline::ensure_search_merged(u64 elements) {
  if (sbatch.merged_cap >= elements) return;
  sync();  // nothing in flight may still read the lists being replaced
  if (d_smerged) LOCUST_HIP_CHECK(hipFree(d_smerged));
  d_smerged = nullptr;
  sbatch.merged = nullptr;
  sbatch.merged_cap = 0;
  const u64 cap = align_up(elements, (u64)kSortTile);
  const u64 bytes = cap * sizeof(u32);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("search workspace (" + std::to_string(bytes) + " B needed for the " +
                std::to_string(elements) + " list elements the batch's prefix terms merge) "
                "does not fit the free device memory (" + std::to_string(fr) + " B free of " +
                std::to_string(tot) + " B): split the batch");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_smerged), bytes));
  sbatch.merged = d_smerged;
  sbatch.merged_cap = cap;
}

void DevicePipeline::ensure_search_patterns() {
  if (d_spat) return;
  // first batch of this engine with a pattern term: the per-slot pattern arrays and the pinned
  // half that is uploaded (engines that never see a pattern keep their footprint)
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_spat), search_pattern_bytes()));
  h_spat = static_cast<u32*>(
      pinned_alloc(search_pattern_upload_bytes(), hipHostMallocDefault, "search patterns"));
}

void DevicePipeline::ensure_search_regex(u64 programs) {
  if (programs <= srx_cap) return;
  // first batch of this engine with a regex term, or one with more distinct programs than any
  // before: the program table and its pinned half, grown to what the batch holds (engines that
  // never see a regex keep their footprint; the batch before has drained)
  if (d_srx) LOCUST_HIP_CHECK(hipFree(d_srx));
  d_srx = nullptr;
  pinned_free(h_srx);
  h_srx = nullptr;
  srx_cap = 0;
  const u64 bytes = programs * kRegexWords * sizeof(u32);
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_srx), bytes));
  h_srx = static_cast<u32*>(pinned_alloc(bytes, hipHostMallocDefault, "search regex programs"));
  srx_cap = programs;
}

void DevicePipeline::ensure_search_expr() {
  if (d_sexpr) return;
  // first batch of this engine with an `expr` query (engines that never see one keep their
  // footprint)
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_sexpr), search_expr_bytes()));
  h_sexpr = static_cast<u32*>(pinned_alloc(search_expr_upload_bytes(kSearchMaxQueries),
                                           hipHostMallocDefault, "search expressions"));
}

void DevicePipeline::ensure_corpus(u64 segments, u64 sets) {
  if (d_corpus && scorpus.seg_cap >= segments && scorpus.set_cap >= sets) return;
  // first batch of this engine with a file set, or one that outgrows the arrays (engines that
  // never see one keep their footprint)
  sync();
  if (d_corpus) LOCUST_HIP_CHECK(hipFree(d_corpus));
  d_corpus = nullptr;
  pinned_free(h_corpus);
  h_corpus = nullptr;
  scorpus = CorpusSets{};
  corpus_bytes = 0;
  const u64 seg_cap = std::min<u64>(align_up(segments + segments / 2, (u64)1024), kCorpusMaxFiles);
  const u64 set_cap = std::min<u64>(align_up(sets, (u64)16), kSearchMaxQueries);
  const u64 bytes = corpus_sets_bytes(seg_cap, set_cap);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("search: the file-set arrays (" + std::to_string(bytes) + " B for " +
                std::to_string(seg_cap) + " segments and " + std::to_string(set_cap) +
                " sets) do not fit the free device memory (" + std::to_string(fr) + " B free of " +
                std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_corpus), bytes));
  corpus_bytes = bytes;
  corpus_sets_carve(d_corpus, seg_cap, set_cap, &scorpus);
  h_corpus = static_cast<u32*>(pinned_alloc(
      (2 * seg_cap + kSearchMaxQueries + set_cap * div_up(seg_cap, (u64)32)) * sizeof(u32),
      hipHostMallocDefault, "search file sets"));
  corpus_dirty = true;
}

void DevicePipeline::corpus_restrict(const std::vector<SearchQuery>& queries, u64 H) {
  const u32 Q = (u32)queries.size();
  const u64 S = idx_segs.segs.size();
  // one bitmap per distinct set of the batch
  std::map<std::vector<u32>, u32> set_index;
  std::vector<u32> row_of(Q, kCorpusNoSet);
  for (u32 q = 0; q < Q; ++q)
    if (!queries[q].files.empty())
      row_of[q] = set_index.emplace(queries[q].files, (u32)set_index.size()).first->second;
  const u64 D = set_index.size();
  ensure_corpus(S, D);
  const u64 words = div_up(S, (u64)32);
  u32* h_table = h_corpus;
  u32* h_qset = h_corpus + scorpus.seg_cap;
  u32* h_maps = h_qset + kSearchMaxQueries;
  (void)h_table;
  corpus_sync_table();
  std::copy(row_of.begin(), row_of.end(), h_qset);
  std::memset(h_maps, 0, (size_t)(D * words) * sizeof(u32));
  for (const auto& kv : set_index)
    for (const u32 id : kv.first) {  // (an id that is not resident has no bit)
      const size_t o = idx_segs.find(id);
      if (o < S) h_maps[(u64)kv.second * words + (o >> 5)] |= 1u << (o & 31);
    }
  LOCUST_HIP_CHECK(hipMemcpyAsync(scorpus.q_set, h_qset, (u64)Q * sizeof(u32),
                                  hipMemcpyHostToDevice, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(scorpus.bitmaps, h_maps, D * words * sizeof(u32),
                                  hipMemcpyHostToDevice, stream));
  launch_corpus_restrict(idx_view, sbatch, scorpus, (u32)S, (u32)D, Q, H, shits, stream);
}

void DevicePipeline::corpus_sync_table() {
  if (!corpus_dirty) return;
  const u64 S = idx_segs.segs.size();
  // (the ids' upload half: the words behind the bitmaps' part of the pinned buffer)
  u32* h_table = h_corpus;
  u32* h_ids = h_corpus + scorpus.seg_cap + kSearchMaxQueries +
               scorpus.set_cap * div_up(scorpus.seg_cap, (u64)32);
  for (u64 i = 0; i < S; ++i) {
    h_table[i] = (u32)idx_segs.segs[i].first_line;
    h_ids[i] = idx_segs.segs[i].id;
  }
  LOCUST_HIP_CHECK(hipMemcpyAsync(scorpus.table, h_table, S * sizeof(u32), hipMemcpyHostToDevice,
                                  stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(scorpus.ids, h_ids, S * sizeof(u32), hipMemcpyHostToDevice,
                                  stream));
  corpus_dirty = false;
}

void DevicePipeline::by_file_stage(u32 Q, const u64* offsets, u64 E, bool ranked, u32 by_file,
                                   SearchResult* r) {
  TraceRange tr("locust:by_file");
  const bool count_only = by_file == kByFileCount;
  r->by_file = by_file;
  const u64 S = idx_segs.segs.size();
  ensure_corpus(S, 0);
  if (!ev_byfile[0])
    for (auto& e : ev_byfile) LOCUST_HIP_CHECK(hipEventCreate(&e));
  if (!d_byfile || sbyfile.cap < E) {
    sync();
    if (d_byfile) LOCUST_HIP_CHECK(hipFree(d_byfile));
    d_byfile = nullptr;
    sbyfile = CorpusByFile{};
    byfile_bytes = 0;
    const u64 cap = align_up(std::max<u64>(E + E / 2, 1), (u64)kCorpusTile);
    u64 bytes = 0;
    corpus_by_file_carve(nullptr, cap, nullptr, &bytes);
    size_t fr = 0, tot = 0;
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if ((double)bytes > kHbmUsable * (double)fr)
      throw Error("by_file: the stage's arrays (" + std::to_string(bytes) + " B for " +
                  std::to_string(E) + " returned lines) do not fit the free device memory (" +
                  std::to_string(fr) + " B free of " + std::to_string(tot) + " B)");
    LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_byfile), bytes));
    byfile_bytes = bytes;
    corpus_by_file_carve(d_byfile, cap, &sbyfile);
  }
  constexpr u64 kHdr = 64 + ((u64)kSearchMaxQueries + 1) * sizeof(u64);
  // (room for the worst case: a run per returned line, and the two per-line arrays)
  const u64 need = kHdr + 4 * E * sizeof(u32);
  if (h_byfile_cap < need) {
    pinned_free(h_byfile);
    h_byfile = nullptr;
    h_byfile_cap = align_up(need, (u64)1 << 16);
    h_byfile = static_cast<char*>(pinned_alloc(h_byfile_cap, hipHostMallocDefault, "by-file answer"));
  }
  CorpusCounters* h_cc = reinterpret_cast<CorpusCounters*>(h_byfile);
  u64* h_foff = reinterpret_cast<u64*>(h_byfile + 64);
  u32* h_arr = reinterpret_cast<u32*>(h_byfile + kHdr);
  corpus_sync_table();
  LOCUST_HIP_CHECK(hipEventRecord(ev_byfile[0], stream));
  launch_corpus_by_file(scorpus, (u32)S, idx_segs.segs[0].base, offsets, Q, E, ranked, shits,
                        sbyfile, h_plan, stream);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_cc, sbyfile.ctr, sizeof(CorpusCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_foff, sbyfile.file_off, ((u64)Q + 1) * sizeof(u64),
                                  hipMemcpyDeviceToHost, stream));
  sync();
  const u64 F = h_cc->runs;
  if (h_cc->unlocated || F > E || (E != 0) != (F != 0) || h_foff[0] != 0 || h_foff[Q] != F)
    throw Error("by_file: " + std::to_string(F) + " (query, file) runs among " +
                std::to_string(E) + " returned lines, " + std::to_string(h_cc->unlocated) +
                " of them outside the table or their query; the offsets end at " +
                std::to_string(h_foff[Q]));
  u32* h_ids = h_arr;
  u32* h_cnt = h_arr + F;
  u32* h_lf = h_cnt + F;
  u32* h_ll = h_lf + E;
  if (F) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_ids, sbyfile.file_ids, F * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_cnt, sbyfile.file_counts, F * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
  }
  if (E && !count_only) {
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_lf, sbyfile.line_file, E * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_ll, sbyfile.line_local, E * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
  }
  LOCUST_HIP_CHECK(hipEventRecord(ev_byfile[1], stream));
  sync();
  r->file_off.assign(h_foff, h_foff + Q + 1);
  r->file_ids.assign(h_ids, h_ids + F);
  r->file_counts.assign(h_cnt, h_cnt + F);
  if (!count_only) {
    r->line_file.assign(h_lf, h_lf + E);
    r->line_local.assign(h_ll, h_ll + E);
  }
  r->by_file_ms = ms_between(ev_byfile[0], ev_byfile[1]);
  r->wire_bytes += sizeof(CorpusCounters) + ((u64)Q + 1) * sizeof(u64) + 2 * F * sizeof(u32) +
                   (count_only ? 0 : 2 * E * sizeof(u32));
}

IndexSegments DevicePipeline::segments() const {
  if (!idx_resident)
    throw Error("segments: the index on the device is stale -- this engine's last job was not "
                "a run_index, a run_search, an append_index or a drop_index; run one of them "
                "first");
  return idx_segs;
}

void DevicePipeline::check_search_batch(const std::vector<SearchQuery>& queries, u64 rank_k,
                                        bool ignore_case) const {
  LOCUST_CHECK_ARG(queries.size() <= (size_t)kSearchMaxQueries,
                   "search: a device batch holds at most kSearchMaxQueries = " +
                       std::to_string(kSearchMaxQueries) + " queries, not " +
                       std::to_string(queries.size()) + "; split the batch, or evaluate on the "
                       "host (search_index / IndexResult.search)");
  check_search_queries(queries, cfg);
  check_search_rank(rank_k, cfg, search_has_patterns(queries, ignore_case));
}

void DevicePipeline::show_stage(u32 Q, const u64* offsets, u64 E, u32 N, SearchResult* r) {
  TraceRange tr("locust:show");
  r->show_bytes = N;
  r->text_off.assign(1, 0);
  r->span_off.assign(1, 0);
  if (E == 0) return;  // nothing returned: nothing to show, nothing launched
  if (!ev_show[0])
    for (auto& e : ev_show) LOCUST_HIP_CHECK(hipEventCreate(&e));
  size_t fr = 0, tot = 0;
  if (sshow.cap_entries < E) {
    // (the stream is drained: search_stage has synchronised)
    if (d_show_entries) LOCUST_HIP_CHECK(hipFree(d_show_entries));
    d_show_entries = nullptr;
    sshow.cap_entries = 0;
    show_entry_cap_bytes = 0;
    const u64 cap = align_up(E, (u64)4096);
    const u64 bytes = show_entry_bytes(cap);
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if ((double)bytes > kHbmUsable * (double)fr)
      throw Error("show: the stage's per-entry arrays (" + std::to_string(bytes) + " B for " +
                  std::to_string(E) + " returned lines) do not fit the free device memory (" +
                  std::to_string(fr) + " B free of " + std::to_string(tot) +
                  " B): use --rank K to return fewer lines");
    LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_show_entries), bytes));
    show_entry_cap_bytes = bytes;
    show_entry_carve(d_show_entries, cap, &sshow);
  }
  LOCUST_HIP_CHECK(hipEventRecord(ev_show[0], stream));
  launch_show_measure(idx_view, sbatch, Q, shits.lines, offsets, E, N, sshow, stream);
  // the stage's one readback: the totals size, or refuse, the payload
  if (h_show_cap < sizeof(ShowCounters)) {
    h_show_cap = 1u << 20;
    h_show = static_cast<char*>(pinned_alloc(h_show_cap, hipHostMallocDefault, "show payload"));
  }
  ShowCounters* h_ctr = reinterpret_cast<ShowCounters*>(h_show);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ctr, sshow.ctr, sizeof(ShowCounters), hipMemcpyDeviceToHost,
                                  stream));
  sync();
  const u64 T = h_ctr->text, S = h_ctr->spans, cut = h_ctr->cut;
  if (T > E * (u64)N || cut > E)
    throw Error("show: the measure pass reports " + std::to_string(T) + " text bytes and " +
                std::to_string(cut) + " cut lines for " + std::to_string(E) + " entries of at "
                "most " + std::to_string(N) + " bytes");
  const u64 off_bytes = (E + 1) * sizeof(u64);
  const u64 payload = T + S * 3 * sizeof(u32) + 2 * off_bytes;
  const u64 need = align_up(sizeof(ShowCounters), 256) + align_up(2 * off_bytes, 256) +
                   align_up(S * 3 * sizeof(u32), 256) + T;
  if (payload > kShowMaxPayload)
    throw Error("show: the batch's payload (" + std::to_string(payload) + " B: " +
                std::to_string(T) + " text bytes and " + std::to_string(S) + " spans of " +
                std::to_string(E) + " returned lines) exceeds the pinned buffer's limit (" +
                std::to_string(kShowMaxPayload) + " B): use --rank K to return fewer lines, or "
                "a smaller --show N");
  if (sshow.cap_text < T || sshow.cap_spans < S) {
    const u64 cap_t = std::max<u64>(align_up(T, (u64)1 << 16), 1u << 16);
    const u64 cap_s = std::max<u64>(align_up(S, (u64)1 << 12), 1u << 12);
    if (sshow.cap_text < T) {
      if (d_show_text) LOCUST_HIP_CHECK(hipFree(d_show_text));
      d_show_text = nullptr;
      sshow.text = nullptr;
      sshow.cap_text = 0;
    }
    if (sshow.cap_spans < S) {
      if (d_show_spans) LOCUST_HIP_CHECK(hipFree(d_show_spans));
      d_show_spans = nullptr;
      sshow.spans = nullptr;
      sshow.cap_spans = 0;
    }
    const u64 bytes = (sshow.text ? 0 : cap_t) + (sshow.spans ? 0 : cap_s * 3 * sizeof(u32));
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if ((double)bytes > kHbmUsable * (double)fr)
      throw Error("show: the batch's payload (" + std::to_string(payload) + " B: " +
                  std::to_string(T) + " text bytes and " + std::to_string(S) + " spans of " +
                  std::to_string(E) + " returned lines) does not fit the free device memory (" +
                  std::to_string(fr) + " B free of " + std::to_string(tot) +
                  " B): use --rank K to return fewer lines, or a smaller --show N");
    if (!sshow.text) {
      LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_show_text), cap_t));
      sshow.text = d_show_text;
      sshow.cap_text = cap_t;
    }
    if (!sshow.spans) {
      LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_show_spans), cap_s * 3 * sizeof(u32)));
      sshow.spans = d_show_spans;
      sshow.cap_spans = cap_s;
    }
  }
  if (h_show_cap < need) {
    pinned_free(h_show);
    h_show = nullptr;
    h_show_cap = 0;
    const u64 cap = align_up(need, (u64)1 << 20);
    h_show = static_cast<char*>(pinned_alloc(cap, hipHostMallocDefault, "show payload"));
    h_show_cap = cap;
    h_ctr = reinterpret_cast<ShowCounters*>(h_show);
  }
  launch_show_write(idx_view, sbatch, Q, shits.lines, offsets, E, sshow, stream);
  u64* h_toff = reinterpret_cast<u64*>(h_show + align_up(sizeof(ShowCounters), 256));
  u64* h_soff = h_toff + (E + 1);
  u32* h_spans =
      reinterpret_cast<u32*>(reinterpret_cast<char*>(h_toff) + align_up(2 * off_bytes, 256));
  char* h_text = reinterpret_cast<char*>(h_spans) + align_up(S * 3 * sizeof(u32), 256);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_toff, sshow.text_off, off_bytes, hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_soff, sshow.span_off, off_bytes, hipMemcpyDeviceToHost,
                                  stream));
  if (S)
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_spans, sshow.spans, S * 3 * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
  if (T) LOCUST_HIP_CHECK(hipMemcpyAsync(h_text, sshow.text, T, hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ctr, sshow.ctr, sizeof(ShowCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_show[1], stream));
  sync();
  if (h_ctr->mismatch || h_ctr->text != T || h_ctr->spans != S || h_toff[E] != T || h_soff[E] != S)
    throw Error("show: the write pass disagrees with the measure pass on " +
                std::to_string(h_ctr->mismatch) + " of " + std::to_string(E) + " entries (" +
                std::to_string(h_soff[E]) + " of " + std::to_string(S) + " spans, " +
                std::to_string(h_toff[E]) + " of " + std::to_string(T) + " text bytes)");
  r->text_off.assign(h_toff, h_toff + E + 1);
  r->span_off.assign(h_soff, h_soff + E + 1);
  r->spans.assign(h_spans, h_spans + S * 3);
  r->text.assign(h_text, (size_t)T);
  r->cut_lines = cut;
  r->show_ms = ms_between(ev_show[0], ev_show[1]);
  r->wire_bytes += payload + 2 * sizeof(ShowCounters);
}

void DevicePipeline::tally_stage(u32 Q, const u64* offsets, u64 E, u32 K, SearchResult* r) {
  TraceRange tr("locust:tally");
  r->tally_k = K;
  r->tally_off.assign((size_t)Q + 1, 0);
  r->tally_words.assign((size_t)Q, 0);
  r->tally_tokens.assign((size_t)Q, 0);
  if (E == 0) return;  // nothing returned: nothing to tally, nothing launched
  if (!ev_tally[0])
    for (auto& e : ev_tally) LOCUST_HIP_CHECK(hipEventCreate(&e));
  size_t fr = 0, tot = 0;
  if (stally.cap_entries < E) {
    // (the stream is drained: search_stage, or show_stage, has synchronised)
    if (d_tally_entries) LOCUST_HIP_CHECK(hipFree(d_tally_entries));
    d_tally_entries = nullptr;
    stally.cap_entries = 0;
    tally_entry_cap_bytes = 0;
    const u64 cap = align_up(E, (u64)4096);
    const u64 bytes = tally_entry_bytes(cap);
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if ((double)bytes > kHbmUsable * (double)fr)
      throw Error("tally: the stage's per-entry arrays (" + std::to_string(bytes) + " B for " +
                  std::to_string(E) + " returned lines) do not fit the free device memory (" +
                  std::to_string(fr) + " B free of " + std::to_string(tot) +
                  " B): use --rank K to return fewer lines, or fewer queries");
    LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_tally_entries), bytes));
    tally_entry_cap_bytes = bytes;
    tally_entry_carve(d_tally_entries, cap, &stally);
  }
  // the pinned answer: [counters | q_words | words | tokens | out_off | the winners' records]
  const u64 kHdr = sizeof(TallyCounters) + (u64)kSearchMaxQueries * sizeof(u32) +
                   (3 * (u64)kSearchMaxQueries + 1) * sizeof(u64);
  if (h_tally_cap < kHdr) {
    h_tally_cap = 1u << 20;
    h_tally = static_cast<char*>(pinned_alloc(h_tally_cap, hipHostMallocDefault, "tally answer"));
  }
  TallyCounters* h_ctr = reinterpret_cast<TallyCounters*>(h_tally);
  LOCUST_HIP_CHECK(hipEventRecord(ev_tally[0], stream));
  launch_tally_measure(idx_view, shits.lines, E, stally, stream);
  // the stage's sizing readback: the pair words size, or refuse, the workspace and fix the key
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ctr, stally.ctr, sizeof(TallyCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_tally[1], stream));
  sync();
  const u64 T = h_ctr->tokens;
  if (T > E * (u64)cfg.emits_per_line)
    throw Error("tally: the measure pass reports " + std::to_string(T) + " tokens for " +
                std::to_string(E) + " entries of at most " + std::to_string(cfg.emits_per_line));
  r->wire_bytes += sizeof(TallyCounters);
  if (T == 0) {  // empty lines only: every query's answer is 0, 0 and no word
    r->tally_ms = ms_between(ev_tally[0], ev_tally[1]);
    return;
  }
  const TallyKeySplit ks = tally_key_split(idx_view.n, T);
  const u64 out_need = std::min<u64>(T, (u64)Q * std::min<u64>(K, idx_view.n));
  if (stally.cap_pairs < T || stally.cap_out < out_need) {
    if (d_tally_pairs) LOCUST_HIP_CHECK(hipFree(d_tally_pairs));
    d_tally_pairs = nullptr;
    stally.cap_pairs = stally.cap_out = 0;
    stally.rx.cap = 0;
    tally_pair_cap_bytes = 0;
    const u64 cap_p = align_up(T, (u64)kSortTile);
    const u64 cap_o = align_up(out_need, (u64)4096);
    const u64 bytes = tally_pair_bytes(cap_p, cap_o);
    LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
    if ((double)bytes > kHbmUsable * (double)fr)
      throw Error("tally: the batch's workspace (" + std::to_string(bytes) + " B: " +
                  std::to_string(T) + " tokens on " + std::to_string(E) +
                  " returned lines) does not fit the free device memory (" + std::to_string(fr) +
                  " B free of " + std::to_string(tot) +
                  " B): use --rank K to return fewer lines, or fewer queries");
    LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_tally_pairs), bytes));
    tally_pair_cap_bytes = bytes;
    tally_pair_carve(d_tally_pairs, cap_p, cap_o, &stally);
    LOCUST_HIP_CHECK(hipMemsetAsync(stally.zeros, 0, cap_p * sizeof(u64), stream));
  }
  launch_tally_map(idx_view, Q, shits.lines, offsets, E, T, ks, stally, h_plan, stream);
  // U and the words per query: the second sort takes its regime from U, and they size what
  // comes back
  u32* h_qw = reinterpret_cast<u32*>(h_tally + sizeof(TallyCounters));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ctr, stally.zero, sizeof(TallyCounters) + (u64)Q * sizeof(u32),
                                  hipMemcpyDeviceToHost, stream));
  sync();
  if (h_ctr->miss || h_ctr->mismatch || h_ctr->sort_n != T || h_ctr->tokens != T)
    throw Error("tally: the map pass disagrees with the index (" + std::to_string(h_ctr->miss) +
                " tokens whose key it does not hold) or with the measure pass (" +
                std::to_string(h_ctr->mismatch) + " of " + std::to_string(E) + " entries; " +
                std::to_string(h_ctr->sort_n) + " of " + std::to_string(T) + " pair words sorted)");
  const u64 U = h_ctr->runs;
  u64 W = 0, R = 0;
  for (u32 q = 0; q < Q; ++q) {
    W += h_qw[q];
    R += std::min<u64>(h_qw[q], K);
  }
  if (U < 1 || U > T || W != U || h_ctr->misplaced || R > out_need)
    throw Error("tally: " + std::to_string(U) + " runs among " + std::to_string(T) +
                " sorted pair words, " + std::to_string(W) + " of them counted for the queries, " +
                std::to_string(h_ctr->misplaced) + " naming no query, word or count");
  const u64 need = align_up(kHdr, 256) + R * sizeof(OutRecord);
  if (h_tally_cap < need) {
    std::vector<u32> keep(h_qw, h_qw + Q);
    pinned_free(h_tally);
    h_tally = nullptr;
    h_tally_cap = 0;
    const u64 cap = align_up(need, (u64)1 << 20);
    h_tally = static_cast<char*>(pinned_alloc(cap, hipHostMallocDefault, "tally answer"));
    h_tally_cap = cap;
    h_ctr = reinterpret_cast<TallyCounters*>(h_tally);
    h_qw = reinterpret_cast<u32*>(h_tally + sizeof(TallyCounters));
    std::copy(keep.begin(), keep.end(), h_qw);
  }
  launch_tally_top(idx_view, Q, offsets, U, K, ks, stally, h_plan, stream);
  u64* h_words = reinterpret_cast<u64*>(h_qw + kSearchMaxQueries);
  u64* h_tokens = h_words + kSearchMaxQueries;
  u64* h_off = h_tokens + kSearchMaxQueries;
  OutRecord* h_recs = reinterpret_cast<OutRecord*>(h_tally + align_up(kHdr, 256));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_words, stally.words, (u64)Q * sizeof(u64),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_tokens, stally.tokens, (u64)Q * sizeof(u64),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_off, stally.out_off, ((u64)Q + 1) * sizeof(u64),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_recs, stally.out, R * sizeof(OutRecord),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_ctr, stally.ctr, sizeof(TallyCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_tally[1], stream));
  sync();
  u64 tok_sum = 0;
  bool agree = h_off[Q] == R && h_off[0] == 0;
  for (u32 q = 0; q < Q; ++q) {
    agree &= h_words[q] == h_qw[q] && h_off[q + 1] - h_off[q] == std::min<u64>(h_qw[q], K);
    tok_sum += h_tokens[q];
  }
  if (h_ctr->misplaced || !agree || tok_sum != T)
    throw Error("tally: " + std::to_string(h_ctr->misplaced) + " of " + std::to_string(U) +
                " sorted rank keys lie outside their query's range or name no word; the output "
                "offsets end at " + std::to_string(h_off[Q]) + " (the runs give " +
                std::to_string(R) + "), the queries' tokens add up to " + std::to_string(tok_sum) +
                " of " + std::to_string(T));
  r->tally_off.assign(h_off, h_off + Q + 1);
  r->tally_words.assign(h_words, h_words + Q);
  r->tally_tokens.assign(h_tokens, h_tokens + Q);
  r->tally_keys.resize((size_t)R);
  r->tally_counts.resize((size_t)R);
  for (u64 i = 0; i < R; ++i) {
    std::memcpy(r->tally_keys[i].w, h_recs[i].w, sizeof(PackedKey));
    r->tally_counts[i] = h_recs[i].count;
  }
  r->tallied = T;
  r->tally_ms = ms_between(ev_tally[0], ev_tally[1]);
  r->wire_bytes += R * sizeof(OutRecord) + (3 * (u64)Q + 1) * sizeof(u64) +
                   (u64)Q * sizeof(u32) + 2 * sizeof(TallyCounters);
}

void DevicePipeline::search_stage(const std::vector<SearchQuery>& queries, u64 rank_k,
                                  bool ignore_case, u32 show, u32 tally, u32 by_file,
                                  SearchResult* r) {
  TraceRange tr("locust:search");
  const u32 Q = (u32)queries.size();
  r->queries = queries;
  r->first_line = idx_view.first_line;
  r->num_lines = idx_words.num_lines;
  r->num_tokens = idx_words.num_tokens;
  r->num_unique = idx_words.num_unique;
  r->overflow_lines = idx_words.overflow_lines;
  r->truncated = idx_words.truncated;
  r->max_key_len = idx_words.max_key_len;
  r->rank_k = rank_k;
  r->ignore_case = ignore_case;
  r->emits_per_line = (u64)cfg.emits_per_line;
  r->segments = idx_segs.segs;
  r->offsets.assign((size_t)Q + 1, 0);
  r->matches.assign((size_t)Q, 0);
  r->term_counts.assign((size_t)Q * kSearchMaxTerms, 0);
  ensure_search();
  // a batch with a pattern term (engine.hpp "pattern terms") drives the pattern stages; every
  // other batch runs what it ran before they existed
  const bool patterns = Q != 0 && search_has_patterns(queries, ignore_case);
  if (patterns) ensure_search_patterns();
  sbatch.pat = patterns ? d_spat : nullptr;
  // ... and one with a fuzzy term (engine.hpp "fuzzy terms") the kernels compiled with both
  // matchers (kernels.hpp "fuzzy.hip"): per batch, so the next one is routed afresh
  sbatch.fuzzy = patterns && search_has_fuzzy(queries);
  // ... and one with a regex term (engine.hpp "regex terms") the kernels compiled with all three
  // (kernels.hpp "regex.hip") and the batch's compiled programs: set below, per batch
  sbatch.regex = nullptr;
  std::map<std::string, u32> rx_index;  // a source's program in the batch's table
  std::vector<u32> rx_progs;            // the distinct programs, in index order
  // a regex term's slot: its program's index (identical sources share one), which is its meta
  // word and, behind the tag, its key words
  const auto regex_slot = [&](SearchPattern* sp) {
    if (!sp->regex) return;
    const auto it = rx_index.emplace(sp->src, (u32)rx_index.size());
    if (it.second) rx_progs.insert(rx_progs.end(), sp->rx.begin(), sp->rx.end());
    sp->meta = it.first->second;
    sp->p = PackedKey{};
    sp->p.w[0] = kRegexKeyTag;
    sp->p.w[1] = it.first->second;
  };
  // ... and one with an `expr` query (engine.hpp "boolean expressions") the plan and the hit
  // kernel of kernels.hpp "expr.hip"; a batch without one launches what it always launched
  bool exprs = false;
  for (const SearchQuery& sq : queries) exprs |= sq.mode == SearchMode::kExpr;
  if (exprs) ensure_search_expr();
  sbatch.expr = exprs ? d_sexpr : nullptr;
  LOCUST_HIP_CHECK(hipEventRecord(ev_search[0], stream));
  if (Q == 0) {
    LOCUST_HIP_CHECK(hipEventRecord(ev_search[1], stream));
    sync();
    if (show) show_stage(0, nullptr, 0, show, r);
    if (tally) tally_stage(0, nullptr, 0, tally, r);
    if (by_file) {  // no query: an empty CSR
      r->by_file = by_file;
      r->file_off.assign(1, 0);
    }
    return;
  }
  // the batch: q_meta | the terms' keys, packed exactly as the map packs them | the windows,
  // only when a near query needs them
  u32* meta = reinterpret_cast<u32*>(h_supload);
  u64* keys = reinterpret_cast<u64*>(h_supload + (u64)kSearchMaxQueries * sizeof(u32));
  u32* within = search_within(keys, Q);
  bool verify = false;  // the batch has a phrase of two or more terms: the phrase kernel runs
  bool near = false;    // ... a near query of two or more terms and W < emits_per_line: the
                        // near kernel runs (a wider window holds every line: answered as `all`)
  std::memset(keys, 0, (size_t)Q * kSearchMaxTerms * sizeof(PackedKey));
  if (patterns) std::memset(h_spat, 0, search_pattern_upload_bytes());
  for (u32 q = 0; q < Q; ++q) {
    const SearchQuery& sq = queries[q];
    // (the modes see the positive terms only; the exclusion terms stand behind them)
    const size_t npos = sq.positives();
    const bool qnear = sq.mode == SearchMode::kNear && npos >= 2 &&
                       sq.within < (u64)cfg.emits_per_line;
    meta[q] = (u32)sq.terms.size() | (sq.mode == SearchMode::kAny      ? kSearchAny
                                      : sq.mode == SearchMode::kExpr   ? kSearchAny | kSearchExpr
                                      : sq.mode == SearchMode::kPhrase ? kSearchPhrase
                                      : qnear                          ? kSearchNear
                                                                       : 0u);
    within[q] = qnear ? (u32)sq.within : 0u;
    verify |= sq.mode == SearchMode::kPhrase && npos >= 2;
    near |= qnear;
    for (size_t t = 0; t < sq.terms.size(); ++t) {
      if (t >= npos) meta[q] |= 1u << (kSearchExcludeShift + (int)t);
      // a prefix term's flag; its length needs no word: the key's non-zero bytes are it
      SearchPattern sp;
      if (search_term_pattern(sq, t, cfg, ignore_case, &sp)) {
        // a pattern slot: the flag and the map in the pattern upload, the pattern's bytes in
        // the slot's key words (q_meta's prefix bit stays clear: a prefix term under
        // ignore_case is the pattern p*)
        h_spat[q] |= (1u << t) | (ignore_case ? kSearchFold : 0u);
        // (a regex term: the tag and its program's index in the key words, the index as the map)
        if (sp.regex) {
          h_spat[q] |= 1u << (kSearchRegexShift + (int)t);
          regex_slot(&sp);
        } else if (sp.budget) {
          // (a fuzzy term: its word in the key words, kFuzzyMeta | its budget as the map)
          h_spat[q] |= 1u << (kSearchFuzzyShift + (int)t);
        }
        h_spat[kSearchPatMeta + (u64)q * kSearchMaxTerms + t] = sp.meta;
        std::memcpy(keys + ((u64)q * kSearchMaxTerms + t) * kKeyWords, sp.p.w, sizeof(PackedKey));
        continue;
      }
      if (search_term_prefix(sq, t, cfg)) meta[q] |= 1u << (kSearchPrefixShift + (int)t);
      const PackedKey k = search_term_key(sq.terms[t], cfg);
      std::memcpy(keys + ((u64)q * kSearchMaxTerms + t) * kKeyWords, k.w, sizeof(PackedKey));
    }
    if (!exprs) continue;
    // the expression arrays' upload: the truth table, and which pattern slots are the same term
    // (equal patterns, as the lookup's identity rule compares them)
    u32 alias = 0;
    u32* truth = h_sexpr + kExprTruth + (u64)q * kSearchMaxTerms;
    std::memset(truth, 0, kSearchMaxTerms * sizeof(u32));
    if (sq.mode == SearchMode::kExpr) {
      std::memcpy(truth, sq.truth.data(), kSearchMaxTerms * sizeof(u32));
      SearchPattern pats[kSearchMaxTerms];
      for (size_t t = 0; t < sq.terms.size(); ++t) {
        if (!search_term_pattern(sq, t, cfg, ignore_case, &pats[t])) continue;
        size_t first = t;
        for (size_t i = 0; i < t && first == t; ++i)
          if (((alias >> (24 + i)) & 1u) && pats[i].same(pats[t])) first = i;
        alias |= (1u << (24 + (int)t)) | ((u32)first << (3 * (int)t));
      }
    }
    h_sexpr[kExprAlias + q] = alias;
  }
  LOCUST_HIP_CHECK(hipMemcpyAsync(sbatch.upload, h_supload, search_upload_bytes(Q, near),
                                  hipMemcpyHostToDevice, stream));
  if (patterns)
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_spat, h_spat, search_pattern_upload_bytes(),
                                    hipMemcpyHostToDevice, stream));
  if (!rx_progs.empty()) {  // the programs in use, and nothing more
    ensure_search_regex(rx_index.size());
    std::memcpy(h_srx, rx_progs.data(), rx_progs.size() * sizeof(u32));
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_srx, h_srx, rx_progs.size() * sizeof(u32),
                                    hipMemcpyHostToDevice, stream));
    sbatch.regex = d_srx;
  }
  if (exprs)
    LOCUST_HIP_CHECK(hipMemcpyAsync(d_sexpr, h_sexpr, search_expr_upload_bytes(Q),
                                    hipMemcpyHostToDevice, stream));
  // lookup (behind the match stage, in a pattern batch): the terms' lists and the bound on the
  // hits
  launch_search_lookup(idx_view, sbatch, Q, stream);
  SearchCounters* h_sc = reinterpret_cast<SearchCounters*>(h_sres);
  u32* h_tlen = reinterpret_cast<u32*>(h_sres + kSearchResLen);
  u64* h_off = reinterpret_cast<u64*>(h_sres + kSearchResOff);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_sc, sbatch.ctr, sizeof(SearchCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_tlen, sbatch.t_len, (u64)Q * kSearchMaxTerms * sizeof(u32),
                                  hipMemcpyDeviceToHost, stream));
  sync();
  // B: what search_hit_kernel walks; E: what expr_hit_kernel walks (0 without an `expr` query;
  // saturated at 2^32 - 1, which the second check below refuses)
  const u64 B = h_sc->bound, E = exprs ? (u64)h_sc->ebound : 0;
  if (h_sc->anyover)
    throw Error("search: " + std::to_string(h_sc->anyover) + " `any` queries of the batch walk "
                "2^32 list elements or more each (their pattern terms' lists overlap): split "
                "the queries");
  if (B >= (1ull << 32))
    throw Error("search: the batch's " + std::to_string(Q) + " queries walk " + std::to_string(B) +
                " list elements, which does not fit the 32-bit slot counter (2^32): split "
                "the batch");
  // (E == 2^32 - 1: saturated -- the expressions alone walk that many elements or more)
  if (E == 0xffffffffull || B + E >= (1ull << 32))
    throw Error("search: the batch's " + std::to_string(Q) + " queries walk " +
                (E == 0xffffffffull ? "2^32 - 1 or more" : std::to_string(B + E)) +
                " list elements, " + (E == 0xffffffffull ? "at least " : "") + std::to_string(E) +
                " of them for its expressions, which does not fit the 32-bit slot counter "
                "(2^32): split the batch");
  // X: the list elements of the prefix terms that cover two or more words (0: no such term,
  // and nothing below differs from a batch without prefix terms)
  const u64 X = h_sc->merge;
  check_search_merge(Q, X);
  ensure_search_hits(std::max(B + E, X));  // (the expand stage's scratch: idle until the hits)
  if (X) {
    // expand: the merged lists, which the hit, phrase and score kernels read as any list
    ensure_search_merged(X);
    launch_search_expand(idx_view, sbatch, Q, X, shits, h_plan, stream);
  }
  r->merged = X;
  r->walked = B + E;
  // hits; a phrase's and a near query's candidates are verified against the resident text
  // behind them.  The `expr` queries' hits come first: the seal behind the others closes both
  if (E) launch_expr_hits(idx_view, sbatch, Q, E, shits, stream);
  launch_search_hits(idx_view, sbatch, Q, B, verify, near, shits, stream);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_sc, sbatch.ctr, sizeof(SearchCounters), hipMemcpyDeviceToHost,
                                  stream));
  u32* h_hits = reinterpret_cast<u32*>(h_sres + kSearchResHits);
  if (rank_k)  // the matches: they size what comes back
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_hits, sbatch.q_hits, (u64)Q * sizeof(u32),
                                    hipMemcpyDeviceToHost, stream));
  sync();
  u64 H = h_sc->written;
  const u64 C = h_sc->cands, NC = h_sc->ncands;
  if (h_sc->merge_n != (u32)X || h_sc->unmerged)
    throw Error("search: " + std::to_string(h_sc->merge_n) + " of " + std::to_string(X) +
                " list elements of prefix terms merged, " + std::to_string(h_sc->unmerged) +
                " of them outside their term's range");
  if (H > B + E || h_sc->sort_n != H)
    throw Error("search: " + std::to_string(H) + " hits written, the lists hold " +
                std::to_string(B + E) + " elements");
  if (C > B || h_sc->verified != C || (C && !verify))
    throw Error("search: " + std::to_string(C) + " phrase candidates, " +
                std::to_string(h_sc->verified) + " of them verified, the lists hold " +
                std::to_string(B) + " elements");
  if (C + NC > B || h_sc->nverified != NC || (NC && !near))
    throw Error("search: " + std::to_string(NC) + " near candidates, " +
                std::to_string(h_sc->nverified) + " of them verified, the lists hold " +
                std::to_string(B) + " elements");
  // "file sets": a batch in which a query names one keeps the pairs of its files only, before
  // anything is sorted or scored; every other batch goes on as it always did
  bool restrict = false;
  for (const SearchQuery& sq : queries) restrict |= !sq.files.empty();
  u64 corpus_wire = 0;
  if (restrict) {
    const u64 H0 = H;
    corpus_restrict(queries, H0);
    CorpusCounters* h_cc = reinterpret_cast<CorpusCounters*>(h_sres + kSearchResCorpus);
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_sc, sbatch.ctr, sizeof(SearchCounters),
                                    hipMemcpyDeviceToHost, stream));
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_cc, scorpus.ctr, sizeof(CorpusCounters),
                                    hipMemcpyDeviceToHost, stream));
    if (rank_k)
      LOCUST_HIP_CHECK(hipMemcpyAsync(h_hits, sbatch.q_hits, (u64)Q * sizeof(u32),
                                      hipMemcpyDeviceToHost, stream));
    sync();
    H = h_sc->written;
    if (h_cc->stray || h_cc->kept != H || H > H0 || h_sc->sort_n != H)
      throw Error("search: the restrict stage kept " + std::to_string(h_cc->kept) + " of " +
                  std::to_string(H0) + " hits (" + std::to_string(h_sc->sort_n) +
                  " handed to the sort), " + std::to_string(h_cc->stray) +
                  " of them naming no query or no segment");
    r->restricted = H0 - H;
    corpus_wire = sizeof(SearchCounters) + sizeof(CorpusCounters) +
                  (rank_k ? (u64)Q * sizeof(u32) : 0);
  }
  // ranked: R lines and R scores come back, R = the sum of min(matches, K)
  u64 R = 0, M = 0;
  if (rank_k)
    for (u32 q = 0; q < Q; ++q) {
      R += std::min<u64>(h_hits[q], rank_k);
      M += h_hits[q];
    }
  if (rank_k && M != H)
    throw Error("search: the per-query hit counts add up to " + std::to_string(M) +
                ", the hit kernel wrote " + std::to_string(H));
  const u64 need = rank_k ? 2 * R : H;
  if (h_slines_cap < need) {
    pinned_free(h_slines);
    h_slines = nullptr;
    h_slines_cap = align_up(need, (u64)kSortTile);
    h_slines = static_cast<u32*>(
        pinned_alloc(h_slines_cap * sizeof(u32), hipHostMallocDefault, "search lines"));
  }
  if (rank_k) {
    // offsets + score + order + top: only the winners and their scores cross
    launch_search_rank(idx_view, sbatch, Q, H, (u32)rank_k, shits, h_plan, stream);
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_off, sbatch.out_off, ((u64)Q + 1) * sizeof(u64),
                                    hipMemcpyDeviceToHost, stream));
    if (R) {
      LOCUST_HIP_CHECK(hipMemcpyAsync(h_slines, shits.lines, R * sizeof(u32),
                                      hipMemcpyDeviceToHost, stream));
      LOCUST_HIP_CHECK(hipMemcpyAsync(h_slines + R, search_rank_scores(shits), R * sizeof(u32),
                                      hipMemcpyDeviceToHost, stream));
    }
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_sc, sbatch.ctr, sizeof(SearchCounters),
                                    hipMemcpyDeviceToHost, stream));
    LOCUST_HIP_CHECK(hipEventRecord(ev_search[1], stream));
    sync();
    if (h_sc->misplaced)
      throw Error("search: " + std::to_string(h_sc->misplaced) + " of " + std::to_string(H) +
                  " sorted hits lie outside their query's range");
    if (h_sc->unscored)
      throw Error("search: " + std::to_string(h_sc->unscored) + " of " + std::to_string(H) +
                  " hits score 0 or more than 32 * emits_per_line" + (patterns ? " * 8" : ""));
    if (h_off[Q] != R)
      throw Error("search: the output offsets end at " + std::to_string(h_off[Q]) +
                  ", the hit counts and K give " + std::to_string(R));
    r->offsets.assign(h_off, h_off + Q + 1);
    r->matches.assign(h_hits, h_hits + Q);
    r->lines.assign(h_slines, h_slines + R);
    r->scores.assign(h_slines + R, h_slines + 2 * R);
    for (u64 i = 0; i < (u64)Q * kSearchMaxTerms; ++i) r->term_counts[i] = h_tlen[i];
    r->wire_bytes = ((u64)Q + 1) * sizeof(u64) + (u64)Q * sizeof(u32) + 2 * R * sizeof(u32) +
                    (u64)Q * kSearchMaxTerms * sizeof(u32) + 3 * sizeof(SearchCounters) +
                    corpus_wire;
    if (by_file) by_file_stage(Q, sbatch.out_off, R, true, by_file, r);
    if (show) show_stage(Q, sbatch.out_off, R, show, r);
    if (tally) tally_stage(Q, sbatch.out_off, R, tally, r);
    return;
  }
  // order + emit
  launch_search_order(idx_view, sbatch, Q, H, shits, h_plan, stream);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_off, sbatch.offsets, ((u64)Q + 1) * sizeof(u64),
                                  hipMemcpyDeviceToHost, stream));
  const bool count_only = by_file == kByFileCount;  // (the lines stay on the device)
  if (H && !count_only)
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_slines, shits.lines, H * sizeof(u32), hipMemcpyDeviceToHost,
                                    stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_sc, sbatch.ctr, sizeof(SearchCounters), hipMemcpyDeviceToHost,
                                  stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_search[1], stream));
  sync();
  if (h_sc->misplaced)
    throw Error("search: " + std::to_string(h_sc->misplaced) + " of " + std::to_string(H) +
                " sorted hits lie outside their query's range");
  if (h_off[Q] != H)
    throw Error("search: the per-query hit counts add up to " + std::to_string(h_off[Q]) +
                ", the hit kernel wrote " + std::to_string(H));
  for (u32 q = 0; q < Q; ++q) r->matches[q] = h_off[q + 1] - h_off[q];
  if (!count_only) {
    r->offsets.assign(h_off, h_off + Q + 1);
    r->lines.assign(h_slines, h_slines + H);
  }
  for (u64 i = 0; i < (u64)Q * kSearchMaxTerms; ++i) r->term_counts[i] = h_tlen[i];
  r->wire_bytes = ((u64)Q + 1) * sizeof(u64) + (count_only ? 0 : H * sizeof(u32)) +
                  (u64)Q * kSearchMaxTerms * sizeof(u32) + 3 * sizeof(SearchCounters) +
                  corpus_wire;
  if (by_file) by_file_stage(Q, sbatch.offsets, H, false, by_file, r);
  if (show) show_stage(Q, sbatch.offsets, H, show, r);
  if (tally) tally_stage(Q, sbatch.offsets, H, tally, r);
}

SearchResult DevicePipeline::run_search(const TextInput& in,
                                        const std::vector<SearchQuery>& queries, u64 rank_k,
                                        bool ignore_case, u64 show, u64 tally, u32 by_file) {
  TraceRange tr("locust:search_job");
  check_search_by_file(by_file, rank_k, show, tally);
  check_search_batch(queries, rank_k, ignore_case);  // (a refused batch starts nothing)
  check_search_show(show, in.bytes);
  check_search_tally(tally);
  idx_resident = false;         // (until this job has left its index)
  SearchResult r;
  WordCountResult w;
  const u64 t0 = now_ns();
  u64 n = 0, T = 0;
  enqueue_index_job(in, w, /*ship_postings=*/false, &n, &T);
  sync();
  check_index_counters(n, T);
  keep_index(in, w, n, T);
  search_stage(queries, rank_k, ignore_case, (u32)show, (u32)tally, by_file, &r);
  r.index_ms = ms_between(ev_index[0], ev_index[1]);
  r.search_ms = ms_between(ev_search[0], ev_search[1]);
  r.wire_bytes += sizeof(IndexCounters) + sizeof(MapCounters);
  r.times.h2d_ms = ms_between(ev[0], ev[1]);
  r.times.map_ms = ms_between(ev[1], ev[2]);
  r.times.process_ms = ms_between(ev[2], ev[3]);
  r.times.reduce_ms = ms_between(ev[3], ev[4]);
  r.times.gpu_ms = ms_between(ev[0], ev_search[1]) + r.show_ms + r.tally_ms + r.by_file_ms;
  r.times.wall_ms = (now_ns() - t0) * 1e-6;
  if (cfg.check) validate_search(r);
  return r;
}

SearchResult DevicePipeline::search_resident(const std::vector<SearchQuery>& queries,
                                             u64 rank_k, bool ignore_case, u64 show,
                                             u64 tally, u32 by_file) {
  TraceRange tr("locust:search_resident");
  check_search_by_file(by_file, rank_k, show, tally);
  check_search_batch(queries, rank_k, ignore_case);
  check_search_show(show, idx_view.bytes);
  check_search_tally(tally);
  if (!idx_resident)
    throw Error("search_resident: the index on the device is stale -- this engine's last job "
                "was not a run_index or a run_search (any other job, a refused one included, "
                "overwrites what the index reads); run one of them first");
  SearchResult r;
  const u64 t0 = now_ns();
  search_stage(queries, rank_k, ignore_case, (u32)show, (u32)tally, by_file, &r);
  r.search_ms = ms_between(ev_search[0], ev_search[1]);
  r.times.gpu_ms = r.search_ms + r.show_ms + r.tally_ms + r.by_file_ms;
  r.times.wall_ms = (now_ns() - t0) * 1e-6;
  if (cfg.check) validate_search(r);
  return r;
}

// =====================================================================================
// Index store and append
// =====================================================================================
void DevicePipeline::ensure_store_half(int h, u64 recs, u64 posts, u64 text_bytes, u64 lines) {
  IndexStoreHalf& st = store[h];
  if (st.base && st.rec_cap >= recs && st.post_cap >= posts && st.text_cap >= text_bytes &&
      st.line_cap >= lines)
    return;
  sync();  // nothing in flight may still use the half being replaced
  if (st.base) LOCUST_HIP_CHECK(hipFree(st.base));
  st = IndexStoreHalf{};
  // half as much again as this merge needs: the destination is rewritten whole, so growing
  // copies nothing, and a run of appends reallocates a half only every few merges
  const auto grow = [](u64 need) { return std::max<u64>(need + need / 2, 1); };
  const u64 rec_cap = grow(recs), post_cap = grow(posts), text_cap = grow(text_bytes),
            line_cap = grow(lines);
  u64 off[7];
  u64 b = 0;
  int k = 0;
  for (const u64 part : {rec_cap * sizeof(OutRecord), (rec_cap + 1) * 8, post_cap * 4,
                         text_cap + 16, (line_cap + 1) * 8, (u64)64}) {
    b = align_up(b, 256);
    off[k++] = b;
    b += part;
  }
  const u64 bytes = align_up(b, 256);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("index store (" + std::to_string(bytes) + " B needed for " +
                std::to_string(rec_cap) + " records, " + std::to_string(post_cap) +
                " postings, " + std::to_string(text_cap) + " text bytes and " +
                std::to_string(line_cap) + " lines) does not fit the free device memory (" +
                std::to_string(fr) + " B free of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st.base), bytes));
  st.bytes = bytes;
  st.ix.recs = reinterpret_cast<OutRecord*>(st.base + off[0]);
  st.ix.val = reinterpret_cast<u64*>(st.base + off[1]);
  st.ix.postings = reinterpret_cast<u32*>(st.base + off[2]);
  st.ix.text = st.base + off[3];
  st.ix.nl_pos = reinterpret_cast<u64*>(st.base + off[4]);
  st.ix.lctr = reinterpret_cast<MapCounters*>(st.base + off[5]);
  st.rec_cap = rec_cap;
  st.post_cap = post_cap;
  st.text_cap = text_cap;
  st.line_cap = line_cap;
}

void DevicePipeline::ensure_append_scratch(u64 recs_a, u64 recs_b) {
  if (!h_actr) {
    // first append of this engine: the pinned counters and the events
    h_actr = static_cast<AppendCounters*>(
        pinned_alloc(sizeof(AppendCounters), hipHostMallocDefault, "append counters"));
    for (auto& e : ev_append) LOCUST_HIP_CHECK(hipEventCreate(&e));
  }
  if (d_append && append_ws.rec_cap_a >= recs_a && append_ws.rec_cap_b >= recs_b) return;
  sync();
  if (d_append) LOCUST_HIP_CHECK(hipFree(d_append));
  d_append = nullptr;
  append_ws = AppendScratch{};
  append_bytes = 0;
  const u64 cap_a = std::max<u64>(recs_a + recs_a / 2, 1), cap_b = std::max<u64>(recs_b + recs_b / 2, 1);
  const u64 bytes = append_scratch_bytes(cap_a, cap_b);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("append scratch (" + std::to_string(bytes) + " B needed for " +
                std::to_string(cap_a) + " + " + std::to_string(cap_b) +
                " records) does not fit the free device memory (" + std::to_string(fr) +
                " B free of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_append), bytes));
  append_bytes = bytes;
  append_scratch_carve(d_append, cap_a, cap_b, &append_ws);
}

void DevicePipeline::ensure_line_index(u64 bytes, u64 n, u64 T) {
  if (bytes == 0 || (n != 0 && T != 0)) return;  // launch_index built it (or there is no text)
  LOCUST_HIP_CHECK(hipMemsetAsync(index.zero, 0, index.zero_bytes, stream));
  launch_line_index(d_text, bytes, index.nl_pos, index.lctr, index.lb, stream);
}

AppendIndex DevicePipeline::resident_as_append() const {
  AppendIndex a;
  a.recs = const_cast<OutRecord*>(idx_view.recs);
  a.val = const_cast<u64*>(idx_view.val);
  a.postings = const_cast<u32*>(idx_view.postings);
  a.text = const_cast<char*>(idx_view.text);
  a.nl_pos = const_cast<u64*>(idx_view.nl_pos);
  a.lctr = const_cast<MapCounters*>(idx_view.lctr);
  a.n = idx_view.n;
  a.tokens = idx_tokens;
  a.bytes = idx_view.bytes;
  a.lines = idx_num_lines;
  return a;
}

IndexAppend DevicePipeline::append_index(const TextInput& in, bool new_file) {
  TraceRange tr("locust:index_append");
  // ---- refusals: nothing is enqueued, the resident index stays as it is ----
  if (!idx_resident)
    throw Error("append_index: the index on the device is stale -- this engine's last job "
                "was not a run_index, a run_search or an append_index (any other job, a refused "
                "one included, overwrites what the index reads); run one of them first");
  const u64 next_line = (u64)idx_view.first_line + idx_num_lines;
  LOCUST_CHECK_ARG(in.first_line == next_line,
                   "append_index: the block starts at line " + std::to_string(in.first_line) +
                       ", the resident index ends before line " + std::to_string(next_line));
  LOCUST_CHECK_ARG(!in.source && in.bytes <= pass_bytes && in.num_lines <= cap_lines,
                   "append_index: a block (" + std::to_string(in.bytes) + " B, " +
                       std::to_string(in.num_lines) + " lines) is indexed in one device pass (" +
                       std::to_string(pass_bytes) + " B, " + std::to_string(cap_lines) +
                       " lines here): append smaller blocks");
  check_index_job(in);
  LOCUST_CHECK_ARG(idx_view.bytes == 0 || idx_ends_nl,
                   "append_index: the resident text does not end in a newline -- the block's "
                   "first line would continue its last one");
  LOCUST_CHECK_ARG(next_line + in.num_lines <= (1ull << 32),
                   "index: line numbers past 2^32 do not fit a u32 posting");
  LOCUST_CHECK_ARG(!new_file || idx_segs.segs.size() < kCorpusMaxFiles,
                   "append_index: the index holds " + std::to_string(idx_segs.segs.size()) +
                       " files, the most it takes (kCorpusMaxFiles = " +
                       std::to_string(kCorpusMaxFiles) + "): drop the oldest first");
  IndexAppend out;
  const u64 t0 = now_ns();
  if (!idx_in_store) {
    // the resident index lives in the pass buffers, which the block's job overwrites: into a
    // half first.  (A refusal of the allocation still leaves it where it was.)
    const AppendIndex a = resident_as_append();
    ensure_store_half(0, a.n, a.tokens, a.bytes, a.lines);
    ensure_line_index(a.bytes, a.n, a.tokens);
    AppendIndex& d = store[0].ix;
    const auto d2d = [&](void* dst, const void* src, u64 bytes) {
      if (bytes) LOCUST_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    };
    d2d(d.recs, a.recs, a.n * sizeof(OutRecord));
    d2d(d.val, a.val, (a.n + 1) * 8);
    d2d(d.postings, a.postings, a.tokens * 4);
    d2d(d.text, a.text, a.bytes);
    LOCUST_HIP_CHECK(hipMemsetAsync(d.text + a.bytes, 0, 16, stream));
    d2d(d.nl_pos, a.nl_pos, std::min<u64>(a.lines, index.line_cap) * 8);
    d2d(d.lctr, a.lctr, sizeof(MapCounters));
    sync();
    d.n = a.n;
    d.tokens = a.tokens;
    d.bytes = a.bytes;
    d.lines = a.lines;
    idx_view.recs = d.recs;
    idx_view.val = d.val;
    idx_view.postings = d.postings;
    idx_view.text = d.text;
    idx_view.nl_pos = d.nl_pos;
    idx_view.lctr = d.lctr;
    store_cur = 0;
    idx_in_store = true;
  }
  // ---- the block's own index, in the pass buffers ----
  idx_resident = false;  // (until the merged index stands: any failure from here leaves it stale)
  WordCountResult w;
  u64 nb = 0, tb = 0;
  enqueue_index_job(in, w, /*ship_postings=*/false, &nb, &tb);
  sync();
  check_index_counters(nb, tb);
  ensure_line_index(in.bytes, nb, tb);
  const AppendIndex a = store[store_cur].ix;
  LOCUST_CHECK_ARG(a.n + nb < (1ull << 32) && a.tokens + tb < (1ull << 32),
                   "index: " + std::to_string(a.n + nb) + " words / " +
                       std::to_string(a.tokens + tb) +
                       " tokens do not fit the 32-bit halves of a pair word");
  AppendIndex b;
  b.recs = d_out;
  b.val = index.val;
  b.postings = index.postings;
  b.text = d_text;
  b.nl_pos = index.nl_pos;
  b.lctr = index.lctr;
  b.n = nb;
  b.tokens = tb;
  b.bytes = in.bytes;
  b.lines = in.num_lines;
  // ---- the merge, into the other half ----
  const int dst = 1 - store_cur;
  ensure_store_half(dst, a.n + nb, a.tokens + tb, a.bytes + b.bytes, a.lines + b.lines);
  ensure_append_scratch(a.n, nb);
  AppendIndex c = store[dst].ix;
  c.n = store[dst].rec_cap;
  c.tokens = store[dst].post_cap;
  c.bytes = store[dst].text_cap + 16;
  c.lines = store[dst].line_cap;
  LOCUST_HIP_CHECK(hipEventRecord(ev_append[0], stream));
  launch_append(a, b, c, append_ws, stream);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_actr, append_ws.ctr, sizeof(AppendCounters),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_append[1], stream));
  sync();
  const AppendCounters ac = *h_actr;
  if (ac.misplaced)
    throw Error("append: " + std::to_string(ac.misplaced) +
                " records or postings misplaced (a position outside the merged index, or keys "
                "out of order)");
  if (ac.moved != a.tokens + tb)
    throw Error("append: " + std::to_string(ac.moved) + " postings moved, the two indexes hold " +
                std::to_string(a.tokens + tb));
  if (ac.fresh > nb || ac.records != a.n + ac.fresh)
    throw Error("append: " + std::to_string(ac.records) + " records written, expected " +
                std::to_string(a.n) + " + " + std::to_string(ac.fresh) + " fresh words");
  // ---- the merged index is the resident one ----
  AppendIndex& m = store[dst].ix;
  m.n = a.n + ac.fresh;
  m.tokens = a.tokens + tb;
  m.bytes = a.bytes + b.bytes;
  m.lines = a.lines + b.lines;
  store_cur = dst;
  idx_view.recs = m.recs;
  idx_view.val = m.val;
  idx_view.postings = m.postings;
  idx_view.n = (u32)m.n;
  idx_view.text = m.text;
  idx_view.bytes = m.bytes;
  idx_view.nl_pos = m.nl_pos;
  idx_view.lctr = m.lctr;
  idx_num_lines = m.lines;
  idx_tokens = m.tokens;
  idx_words.num_lines = m.lines;
  idx_words.num_tokens = m.tokens;
  idx_words.num_unique = m.n;
  idx_words.overflow_lines += w.overflow_lines;
  idx_words.truncated += w.truncated;
  idx_words.max_key_len = std::max(idx_words.max_key_len, w.max_key_len);
  if (in.bytes) idx_ends_nl = in.data[in.bytes - 1] == '\n';
  idx_segs.append(in.num_lines, new_file);
  corpus_dirty |= new_file;  // (the mirror holds first lines only: a longer last file changes none)
  idx_resident = true;
  out.files = idx_segs.segs.size();
  out.block_lines = in.num_lines;
  out.block_tokens = tb;
  out.block_unique = nb;
  out.num_lines = m.lines;
  out.num_tokens = m.tokens;
  out.num_unique = m.n;
  out.fresh_words = ac.fresh;
  out.index_ms = ms_between(ev_index[0], ev_index[1]);
  out.append_ms = ms_between(ev_append[0], ev_append[1]);
  out.times.h2d_ms = ms_between(ev[0], ev[1]);
  out.times.map_ms = ms_between(ev[1], ev[2]);
  out.times.process_ms = ms_between(ev[2], ev[3]);
  out.times.reduce_ms = ms_between(ev[3], ev[4]);
  out.times.gpu_ms = ms_between(ev[0], ev_index[1]) + out.append_ms;
  out.times.wall_ms = (now_ns() - t0) * 1e-6;
  out.store_bytes = store_bytes();
  return out;
}

void DevicePipeline::ensure_drop_scratch(u64 recs) {
  if (!h_dctr) {
    // first drop of this engine: the pinned counters and the events
    h_dctr = static_cast<DropCounters*>(
        pinned_alloc(sizeof(DropCounters), hipHostMallocDefault, "drop counters"));
    for (auto& e : ev_drop) LOCUST_HIP_CHECK(hipEventCreate(&e));
  }
  if (d_drop && drop_ws.rec_cap >= recs) return;
  sync();
  if (d_drop) LOCUST_HIP_CHECK(hipFree(d_drop));
  d_drop = nullptr;
  drop_ws = DropScratch{};
  drop_bytes = 0;
  const u64 cap = std::max<u64>(recs + recs / 2, 1);
  const u64 bytes = drop_scratch_bytes(cap);
  size_t fr = 0, tot = 0;
  LOCUST_HIP_CHECK(hipMemGetInfo(&fr, &tot));
  if ((double)bytes > kHbmUsable * (double)fr)
    throw Error("drop scratch (" + std::to_string(bytes) + " B needed for " +
                std::to_string(cap) + " records) does not fit the free device memory (" +
                std::to_string(fr) + " B free of " + std::to_string(tot) + " B)");
  LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_drop), bytes));
  drop_bytes = bytes;
  drop_scratch_carve(d_drop, cap, &drop_ws);
}

IndexDrop DevicePipeline::drop_index(u64 lines) {
  TraceRange tr("locust:index_drop");
  // ---- refusals: nothing is enqueued, the resident index stays as it is ----
  if (!idx_resident)
    throw Error("drop_index: the index on the device is stale -- this engine's last job "
                "was not a run_index, a run_search, an append_index or a drop_index (any other "
                "job, a refused one included, overwrites what the index reads); run one of them "
                "first");
  LOCUST_CHECK_ARG(lines <= idx_num_lines,
                   "drop_index: " + std::to_string(lines) + " lines to drop, the resident index "
                       "holds " + std::to_string(idx_num_lines));
  const u64 cut_line = (u64)idx_view.first_line + lines;
  LOCUST_CHECK_ARG(cut_line < (1ull << 32),
                   "index: line numbers past 2^32 do not fit a u32 posting");
  IndexDrop out;
  const auto report = [&] {
    out.first_line = idx_view.first_line;
    out.num_lines = idx_num_lines;
    out.num_tokens = idx_tokens;
    out.num_unique = idx_view.n;
    out.store_bytes = store_bytes();
  };
  if (lines == 0) {  // a no-op: nothing is enqueued or allocated
    report();
    return out;
  }
  // ---- the source where it lives, the destination the other half ----
  const AppendIndex a = idx_in_store ? store[store_cur].ix : resident_as_append();
  const int dst = idx_in_store ? 1 - store_cur : 0;
  ensure_store_half(dst, a.n, a.tokens, a.bytes, a.lines - lines);
  ensure_drop_scratch(a.n);
  idx_resident = false;  // (until the compacted index stands: any failure from here leaves it stale)
  if (!idx_in_store) ensure_line_index(a.bytes, a.n, a.tokens);
  AppendIndex c = store[dst].ix;
  c.n = store[dst].rec_cap;
  c.tokens = store[dst].post_cap;
  c.bytes = store[dst].text_cap + 16;
  c.lines = store[dst].line_cap;
  DropRules rules;
  rules.dm = idx_view.dm;
  rules.emits_per_line = idx_view.emits_per_line;
  rules.max_key_len = idx_view.max_key_len;
  LOCUST_HIP_CHECK(hipEventRecord(ev_drop[0], stream));
  launch_drop(a, c, (u32)cut_line, lines, rules, drop_ws, stream);
  LOCUST_HIP_CHECK(hipMemcpyAsync(h_dctr, drop_ws.ctr, sizeof(DropCounters),
                                  hipMemcpyDeviceToHost, stream));
  LOCUST_HIP_CHECK(hipEventRecord(ev_drop[1], stream));
  sync();
  const DropCounters dc = *h_dctr;
  if (dc.misplaced)
    throw Error("drop: " + std::to_string(dc.misplaced) +
                " records or postings misplaced (a position outside the index that is left, keys "
                "out of order, or offsets that do not ascend)");
  if (dc.moved + dc.dropped != a.tokens)
    throw Error("drop: " + std::to_string(dc.moved) + " postings moved and " +
                std::to_string(dc.dropped) + " dropped, the index holds " +
                std::to_string(a.tokens));
  if ((u64)dc.records + dc.vanished != a.n || dc.records != dc.nc)
    throw Error("drop: " + std::to_string(dc.records) + " records written and " +
                std::to_string(dc.vanished) + " words emptied, the index holds " +
                std::to_string(a.n));
  if (dc.cut_byte > a.bytes || dc.overflow_lines > idx_words.overflow_lines ||
      dc.truncated > idx_words.truncated)
    throw Error("drop: the dropped lines hold " + std::to_string(dc.cut_byte) + " bytes, " +
                std::to_string(dc.overflow_lines) + " lines over the emit cap and " +
                std::to_string(dc.truncated) + " truncated tokens, more than the index (" +
                std::to_string(a.bytes) + ", " + std::to_string(idx_words.overflow_lines) + ", " +
                std::to_string(idx_words.truncated) + ")");
  // ---- the compacted index is the resident one ----
  AppendIndex& m = store[dst].ix;
  m.n = dc.nc;
  m.tokens = dc.moved;
  m.bytes = a.bytes - dc.cut_byte;
  m.lines = a.lines - lines;
  store_cur = dst;
  idx_in_store = true;
  idx_view.recs = m.recs;
  idx_view.val = m.val;
  idx_view.postings = m.postings;
  idx_view.n = (u32)m.n;
  idx_view.first_line = (u32)cut_line;
  idx_view.text = m.text;
  idx_view.bytes = m.bytes;
  idx_view.nl_pos = m.nl_pos;
  idx_view.lctr = m.lctr;
  idx_num_lines = m.lines;
  idx_tokens = m.tokens;
  idx_words.num_lines = m.lines;
  idx_words.num_tokens = m.tokens;
  idx_words.num_unique = m.n;
  idx_words.overflow_lines -= dc.overflow_lines;
  idx_words.truncated -= dc.truncated;
  if (m.bytes == 0) idx_ends_nl = true;
  out.dropped_files = idx_segs.drop(lines);
  corpus_dirty = true;
  idx_resident = true;
  out.dropped_lines = lines;
  out.dropped_tokens = dc.dropped;
  out.dropped_words = dc.vanished;
  out.dropped_bytes = dc.cut_byte;
  out.dropped_overflow_lines = dc.overflow_lines;
  out.dropped_truncated = dc.truncated;
  out.drop_ms = ms_between(ev_drop[0], ev_drop[1]);
  report();
  return out;
}

IndexResult DevicePipeline::index_resident() {
  if (!idx_resident)
    throw Error("index_resident: the index on the device is stale -- this engine's last job "
                "was not a run_index, a run_search or an append_index (any other job, a refused "
                "one included, overwrites what the index reads); run one of them first");
  IndexResult x;
  x.first_line = idx_view.first_line;
  x.words = idx_words;  // the statistics
  const u64 n = idx_view.n, T = idx_tokens;
  grow_host_out(n);
  if (n) launch_copy_to_mapped(d_out_mapped, idx_view.recs, n * sizeof(OutRecord), stream);
  x.postings.resize(T);
  sync();
  if (T)
    LOCUST_HIP_CHECK(hipMemcpy(x.postings.data(), idx_view.postings, T * sizeof(u32),
                               hipMemcpyDeviceToHost));
  copy_out(x.words.entries, n);
  x.wire_bytes = T * sizeof(u32) + n * sizeof(OutRecord);
  x.segments = idx_segs.segs;
  if (cfg.check) validate_index(x);
  return x;
}

bool DevicePipeline::host_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: clear the sticky error
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

void DevicePipeline::ensure_stream_buffers(bool staging, u64 nchunks) {
  if (!cstream) {
    LOCUST_HIP_CHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
      LOCUST_HIP_CHECK(hipEventCreateWithFlags(&ev_copied[b], hipEventDisableTiming));
      LOCUST_HIP_CHECK(hipEventCreateWithFlags(&ev_consumed[b], hipEventDisableTiming));
    }
    size_t got = 0;  // the process-wide block cache, like the arena
    d_text_alt = static_cast<char*>(dev_block_alloc(cap_bytes + 64, &got));
    d_text_alt_block = got;
    LOCUST_HIP_CHECK(hipMalloc(&d_dctr, sizeof(MapCounters)));
  }
  if (staging && !h_stage[0])
    for (int b = 0; b < 2; ++b)
      h_stage[b] = static_cast<char*>(pinned_alloc(cap_bytes + 64, hipHostMallocDefault, "chunk staging"));
  // per-window counter snapshots (folded when full: at most 4096 pinned)
  nchunks = std::min<u64>(std::max<u64>(nchunks, 64), 4096);
  if (nchunks > h_chunk_cap) {
    if (h_chunk_ctr) LOCUST_HIP_CHECK(hipHostFree(h_chunk_ctr));
    h_chunk_cap = nchunks;
    LOCUST_HIP_CHECK(hipHostMalloc(&h_chunk_ctr, h_chunk_cap * sizeof(MapCounters),
                                   hipHostMallocDefault));
  }
}

u64 DevicePipeline::stream_ring_piece() const {
  return std::min<u64>(cap_bytes, cfg.ring_piece_bytes ? cfg.ring_piece_bytes : kRingPieceMax);
}

void DevicePipeline::ensure_read_ring(u64 piece) {
  if (ring_piece == piece) return;
  for (int i = 0; i < kRingPieces; ++i) {
    pinned_free(h_ring[i]);
    h_ring[i] = static_cast<char*>(pinned_alloc(piece + 64, hipHostMallocDefault, "read ring piece"));
    if (!ev_ring[i]) LOCUST_HIP_CHECK(hipEventCreateWithFlags(&ev_ring[i], hipEventDisableTiming));
  }
  ring_piece = piece;
}

char* DevicePipeline::ensure_h_text() {
  if (h_text) return h_text;
  h_text = static_cast<char*>(pinned_alloc(cap_bytes + 64, hipHostMallocDefault, "input text buffer"));
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&d_h_text), h_text, 0) != hipSuccess) {
    (void)hipGetLastError();
    d_h_text = nullptr;  // not device-visible: always DMA
  }
  return h_text;
}

std::vector<std::pair<u64, u64>> DevicePipeline::plan_chunks(const TextInput& in) const {
  std::vector<std::pair<u64, u64>> out;
  u64 pos = 0;
  while (pos < in.bytes) {
    u64 end = std::min<u64>(pos + cap_bytes, in.bytes);
    if (end < in.bytes) {
      const void* nl = memrchr(in.data + pos, '\n', (size_t)(end - pos));
      if (!nl)
        throw Error("a line longer than the engine's chunk size (" + std::to_string(cap_bytes) +
                    " B) at byte " + std::to_string(pos));
      end = (u64)(static_cast<const char*>(nl) - in.data) + 1;
    }
    out.emplace_back(pos, end - pos);
    pos = end;
  }
  return out;
}

size_t DevicePipeline::enqueue_stream_insert(const TextInput& in) {
  const auto chunks = plan_chunks(in);
  const bool pinned = host_pinned(in.data);
  size_t k = 0;
  return enqueue_stream_chunks(!pinned, chunks.size(), [&](int b, const char** src) -> u64 {
    if (k >= chunks.size()) return 0;
    const u64 off = chunks[k].first, len = chunks[k].second;
    ++k;
    *src = in.data + off;
    if (!pinned) {  // pageable input: host copy into the pinned half
      std::memcpy(h_stage[b], in.data + off, len);
      *src = h_stage[b];
    }
    return len;
  });
}

void DevicePipeline::snapshot_window_counters() {
  if (win_pending == h_chunk_cap) {  // full: fold the snapshots so far (one host sync)
    sync();
    for (u64 k = 0; k < win_pending; ++k) {
      const MapCounters& c = h_chunk_ctr[k];
      win_acc.num_records += c.num_records;
      win_acc.overflow_lines += c.overflow_lines;
      win_acc.truncated += c.truncated;
      win_acc.max_key_len = std::max(win_acc.max_key_len, c.max_key_len);
    }
    win_pending = 0;
  }
  LOCUST_HIP_CHECK(hipMemcpyAsync(&h_chunk_ctr[win_pending], d_ctr, sizeof(MapCounters),
                                  hipMemcpyDeviceToHost, stream));
  ++win_pending;
}

void DevicePipeline::enqueue_map_window(const char* dtext, u64 len, const DelimMask& dm) {
  LOCUST_HIP_CHECK(hipMemsetAsync(d_sync, 0, sync_bytes, stream));
  launch_map_fast(dtext, len, dm, cfg.emits_per_line, cfg.max_key_len, tokens, nullptr, cap,
                  d_ctr, lb_map, stream, nullptr, nullptr, PartMap{}, false, nullptr, nullptr,
                  nullptr, cfg.ngram);
  snapshot_window_counters();
  launch_dict_insert(tokens, nullptr, &d_ctr->num_records, cap, dict, d_dctr, stream);
}

u64 DevicePipeline::window_len(const char* p, u64 n) const {
  if (n <= map_window) return n;
  const void* nl = memrchr(p, '\n', (size_t)map_window);
  if (nl) return (u64)(static_cast<const char*>(nl) - p) + 1;
  // one line longer than a window: it alone (its tokens are capped at emits_per_line)
  nl = std::memchr(p + map_window, '\n', (size_t)(n - map_window));
  return nl ? (u64)(static_cast<const char*>(nl) - p) + 1 : n;
}

size_t DevicePipeline::enqueue_stream_source(TextSource& src_text) {
  LOCUST_CHECK_ARG(cfg.sort_path == SortPath::kDict && cfg.map_path == MapPath::kFast,
                   "inputs larger than the engine capacity stream through the dictionary "
                   "path with the fast map (sort=dict, map=fast)");
  const u64 piece = stream_ring_piece();
  // a map window closes before a piece would overflow it: windows >= map_window - piece
  const u64 min_window = map_window > piece ? map_window - piece : std::max<u64>(map_window / 2, 1);
  const u64 t_setup = now_ns();
  ensure_stream_buffers(false, div_up(std::max<u64>(src_text.size(), 1), min_window) + 2);
  const u64 t_bufs = now_ns();
  reset_window_counters();
  ensure_read_ring(piece);
  if ((int)log_level() >= (int)LogLevel::kDebug)
    LOCUST_LOG_DEBUG("stream setup: copy stream / second chunk / counters %.2f ms, read ring %.2f ms",
                     (t_bufs - t_setup) * 1e-6, (now_ns() - t_bufs) * 1e-6);
  const DelimMask dm = make_delim_mask(cfg.delimiters.c_str());
  LOCUST_HIP_CHECK(hipMemsetAsync(dict.table, 0, dict_zero_bytes, stream));
  LOCUST_HIP_CHECK(hipMemsetAsync(d_dctr, 0, sizeof(MapCounters), stream));
  // the copy stream must not overwrite a text buffer before the reset is queued
  LOCUST_HIP_CHECK(hipEventRecord(ev_copied[1], stream));
  LOCUST_HIP_CHECK(hipStreamWaitEvent(cstream, ev_copied[1], 0));
  size_t k = 0;     // chunks closed
  u64 fill = 0;     // bytes in chunk k
  u64 mapped = 0;   // bytes of chunk k already mapped (the windows so far)
  int last_slot = -1;  // the ring slot of the last piece copied into chunk k
  auto chunk_text = [&](size_t c) { return (c & 1) ? d_text_alt : d_text; };
  // Map + insert chunk k's bytes [mapped, fill) as one window, once their copies landed.
  auto map_pending = [&] {
    if (fill == mapped) return;
    LOCUST_HIP_CHECK(hipStreamWaitEvent(stream, ev_ring[last_slot], 0));
    enqueue_map_window(chunk_text(k) + mapped, fill - mapped, dm);
    mapped = fill;
  };
  auto close_chunk = [&] {
    const int b = (int)(k & 1);
    map_pending();
    // the chunk buffer is free for its refill two chunks on once its last map ran
    LOCUST_HIP_CHECK(hipEventRecord(ev_consumed[b], stream));
    ++k;
    fill = mapped = 0;
  };
  for (u64 r = 0;; ++r) {
    const int slot = (int)(r % kRingPieces);
    // the slot's previous H2D must have drained before the source refills it
    if (r >= (u64)kRingPieces) LOCUST_HIP_CHECK(hipEventSynchronize(ev_ring[slot]));
    const u64 n = src_text.next(h_ring[slot], piece);
    if (!n) break;
    if (fill + n > cap_bytes)
      close_chunk();
    else if (fill - mapped + n > map_window)
      map_pending();  // the window so far, before this piece would overflow it
    // a chunk buffer is refilled only after the maps two chunks back consumed it
    if (fill == 0 && k >= 2)
      LOCUST_HIP_CHECK(hipStreamWaitEvent(cstream, ev_consumed[k & 1], 0));
    LOCUST_HIP_CHECK(hipMemcpyAsync(chunk_text(k) + fill, h_ring[slot], n, hipMemcpyHostToDevice,
                                    cstream));
    LOCUST_HIP_CHECK(hipEventRecord(ev_ring[slot], cstream));
    last_slot = slot;
    fill += n;
  }
  if (fill) close_chunk();
  // hand the dictionary's counters to the single-pass stages that follow
  LOCUST_HIP_CHECK(hipMemcpyAsync(&d_ctr->num_unique, &d_dctr->num_unique, sizeof(u32),
                                  hipMemcpyDeviceToDevice, stream));
  LOCUST_HIP_CHECK(hipMemcpyAsync(&d_ctr->flags, &d_dctr->flags, sizeof(u32),
                                  hipMemcpyDeviceToDevice, stream));
  return k;
}

void DevicePipeline::stream_stats(size_t nchunks, WordCountResult& r) const {
  r.num_tokens = win_acc.num_records;
  r.overflow_lines = win_acc.overflow_lines;
  r.truncated = win_acc.truncated;
  r.max_key_len = win_acc.max_key_len;
  for (u64 k = 0; k < win_pending; ++k) {
    const MapCounters& c = h_chunk_ctr[k];
    r.num_tokens += c.num_records;
    r.overflow_lines += c.overflow_lines;
    r.truncated += c.truncated;
    r.max_key_len = std::max<u64>(r.max_key_len, c.max_key_len);
  }
  r.chunks = nchunks;
}

WordCountResult DevicePipeline::run_source(TextSource& src) {
  sync_clean = false;
  select_out();
  WordCountResult r = finish_stream(0, [&] { return enqueue_stream_source(src); });
  r.num_lines = src.lines();
  return r;
}

void DevicePipeline::download_keys(const KeysSoA& src, u64 n, std::vector<PackedKey>* out) {
  out->resize(n);
  if (!n) return;
  grow_host_keys(n);
  for (int w = 0; w < kKeyWords; ++w)
    LOCUST_HIP_CHECK(hipMemcpyAsync(h_keys + (u64)w * n, src.w[w], n * sizeof(u64),
                                    hipMemcpyDeviceToHost, stream));
  sync();
  for (u64 i = 0; i < n; ++i)
    for (int w = 0; w < kKeyWords; ++w) (*out)[i].w[w] = h_keys[(u64)w * n + i];
}

void DevicePipeline::set_num_records(u64 n) {
  LOCUST_CHECK_ARG(n <= cap, "too many records for engine capacity");
  LOCUST_HIP_CHECK(hipMemsetAsync(d_sync, 0, sync_bytes, stream));
  h_u64[0] = n;  // little endian: low 32 bits == num_records
  LOCUST_HIP_CHECK(hipMemcpyAsync(&d_ctr->num_records, h_u64, sizeof(u32),
                                  hipMemcpyHostToDevice, stream));
}

void DevicePipeline::upload_keys(const KeysSoA& dst, const PackedKey* keys, u64 n) {
  grow_host_keys(n);
  for (u64 i = 0; i < n; ++i)
    for (int w = 0; w < kKeyWords; ++w) h_keys[(u64)w * n + i] = keys[i].w[w];
  if (n)
    for (int w = 0; w < kKeyWords; ++w)
      LOCUST_HIP_CHECK(hipMemcpyAsync(dst.w[w], h_keys + (u64)w * n, n * sizeof(u64),
                                      hipMemcpyHostToDevice, stream));
}

}  // namespace detail

DevicePassPlan plan_device_pass(const JobConfig& cfg, u64 max_bytes, u64 max_lines,
                                u64 cap_records, u64 free_bytes) {
  using detail::DevicePipeline;
  const u64 E = (u64)std::max(cfg.emits_per_line, 1);
  const u64 share = (u64)std::max(cfg.hbm_share, 1);
  const u64 budget = (u64)((long double)free_bytes * kHbmUsable) / share;
  auto make = [&](bool stream, u64 chunk) {
    DevicePassPlan p;
    p.streaming = stream;
    if (stream) {
      p.chunk_bytes = std::max<u64>(chunk, 1);
      p.map_window = std::min<u64>(p.chunk_bytes, kStreamMapWindow);
      p.pass_bytes = p.map_window;
      p.cap_lines = p.map_window;
      // a window's tokens (a byte in two); the dictionary of a streamed input collects
      // the distinct keys of ALL windows: room for 2^20 of them even in small windows
      p.cap = std::max<u64>(p.map_window / 2 + 1, 1ull << 20);
    } else {
      p.chunk_bytes = std::max<u64>(max_bytes, 1);
      p.pass_bytes = p.chunk_bytes;
      p.map_window = p.chunk_bytes;  // (an input streamed through it anyway: chunk-sized maps)
      p.cap_lines = std::max<u64>(max_lines, 1);
      p.cap = cap_records ? cap_records : std::min<u64>(p.cap_lines * E, p.chunk_bytes / 2 + 1);
    }
    p.cap = std::max<u64>(p.cap, 1);
    // dense distinct-key capacity: every key of a pass, at most 16M (a 2^25-slot table)
    p.ucap = std::min<u64>(p.cap, 1ull << 24);
    // a dictionary engine's sort / reduce buffers hold its distinct keys (every ordered and
    // table path emits <= ucap of them); a receiver (cap_records) or a radix engine sorts
    // every record
    p.rcap = cfg.sort_path == SortPath::kDict && !cap_records ? p.ucap : p.cap;
    p.device_bytes = DevicePipeline::shape_arena(cfg, p, DevicePipeline::small_pass_limit()).arena_bytes;
    if (stream) p.device_bytes += p.chunk_bytes + 64;  // the second chunk buffer
    p.budget_bytes = budget;
    return p;
  };
  const bool streamable = !cap_records && cfg.sort_path == SortPath::kDict &&
                          cfg.map_path == MapPath::kFast;
  const bool asked = cfg.chunk_bytes && max_bytes > cfg.chunk_bytes && !cap_records;
  DevicePassPlan p = make(asked, cfg.chunk_bytes);
  if (!asked && streamable) {
    std::string why;
    if (p.cap >= (1ull << 30))
      why = "more than 2^30 tokens in one pass";
    else if (free_bytes && p.device_bytes > budget)
      why = "one pass would need " + std::to_string(p.device_bytes >> 20) + " MiB of the " +
            std::to_string(budget >> 20) + " MiB of HBM this engine may use";
    if (!why.empty()) {
      // the chunk asked for covers the whole input, and one pass of it does not fit
      LOCUST_CHECK_ARG(!cfg.chunk_bytes,
                       "--chunk-mb " + std::to_string(cfg.chunk_bytes >> 20) +
                           " asks for one device pass of the whole " +
                           std::to_string(max_bytes) + " B input: " + why +
                           "; use a smaller --chunk-mb (LOCUST_CHUNK_MB)");
      if (max_bytes > kDefaultStreamChunk) {
        p = make(true, kDefaultStreamChunk);
        p.why = why;
      }
    }
  }
  LOCUST_CHECK_ARG(p.cap < (1ull << 30),
                   "more than 2^30 records per GPU call (" + std::to_string(p.cap) +
                       "); inputs this large stream on the dictionary path with the fast map");
  if (free_bytes && p.device_bytes > budget) {
    char msg[512];
    std::snprintf(msg, sizeof(msg),
                  "device pass of %llu B needs %.2f GiB of HBM but this engine may use %.2f GiB "
                  "(%.2f GiB free x %.2f / %d engine(s) on the GPU)%s",
                  (unsigned long long)p.chunk_bytes, p.device_bytes / 1073741824.0,
                  budget / 1073741824.0, free_bytes / 1073741824.0, kHbmUsable,
                  std::max(cfg.hbm_share, 1),
                  p.streaming ? ": use a smaller --chunk-mb (LOCUST_CHUNK_MB)"
                              : ": stream it with --chunk-mb (dictionary path, fast map)");
    throw Error(msg);
  }
  return p;
}

}  // namespace locust
