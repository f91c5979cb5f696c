// Inverted index: word -> the lines it occurs on (kernels.hpp "index.hip"; the semantics
// are engine.hpp "inverted index").
//
// The word job has left its n = num_unique records in key order in device memory.  Each
// record's val -- the exclusive prefix of the counts -- is the CSR offset of the word's
// postings list, so the index is the line number of every emitted token, ordered by (word
// rank, line).  This stage re-tokenises the text the map read, one wave per line, finds
// every emitted token's rank by a binary search among the n records, writes one pair word
// rank << 32 | line per token in arbitrary order and sorts the pair words: the low halves
// of the sorted words, offset by first_line, are the postings.
//
// Shape (gfx950, wave64):
//  * offsets: per-tile count sums, a one-workgroup scan of the tile array, a workgroup scan
//    inside each tile (topk.hip's shape for tile_val): val[0 .. n] and the total;
//  * line starts: launch_line_index (map.hip) over the same text;
//  * index_map_kernel: a wave walks its line 64 bytes per step.  The step's bytes (and the
//    32 behind them) are staged in the wave's LDS row, ballots give the token starts, the
//    lanes that own an emitting start pack their key from LDS -- bit-identical to the map's
//    packing (kv.hpp) -- and search it.  The slots come from one wave-level atomic per
//    group of up to 64 consecutive lines, whose emitted tokens the wave counts first.  A
//    line far longer than 64 bytes is walked by its one wave, step after step: slow for a
//    single-line file, but correct;
//  * order: the device-wide radix_sort() on a one-word key (words 1..3 are a zero buffer,
//    whose digit positions are constant and skipped);
//  * index_emit_kernel: postings[j] = first_line + low32(sorted[j]), and a check that j
//    lies inside the CSR range of the word the pair names.
// Data crosses between workgroups only at kernel boundaries (the existing line index and
// radix sort keep their own look-back); this file adds no polled word.
#include <algorithm>

#include "locust/device/linetok.hpp"
#include "locust/device/rank.hpp"
#include "locust/device/wave.hpp"
#include "locust/dstring.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kIdxMapBlock = 256;
constexpr int kIdxMapWaves = kIdxMapBlock / 64;
constexpr int kIdxMapMaxBlocks = 2048;  // 8 workgroups per CU
constexpr int kIdxRow = dev::kLineRow;  // a step's bytes + the 32 behind them

// tile_val[tile] = the tile's count sum.
__global__ __launch_bounds__(kIndexBlock) void index_tile_sum_kernel(
    const OutRecord* __restrict__ recs, u32 n, u64* __restrict__ tile_val) {
  __shared__ u64 s_sum[kIndexBlock / 64];
  const u64 base = (u64)blockIdx.x * kIndexTile;
  u64 sum = 0;
#pragma unroll
  for (int j = 0; j < kIndexItems; ++j) {
    const u64 i = base + (u64)j * kIndexBlock + threadIdx.x;
    if (i < n) sum += recs[i].count;
  }
  sum = dev::wave_reduce_sum(sum);
  if (dev::lane_id() == 0) s_sum[dev::wave_id()] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < kIndexBlock / 64; ++w) t += s_sum[w];
    tile_val[blockIdx.x] = t;
  }
}

// One workgroup: exclusive scan of the tile sums, in place; the total to val[n] and ctr.
__global__ __launch_bounds__(kIndexBlock) void index_tile_scan_kernel(
    u64* __restrict__ tile_val, u32 tiles, u64* __restrict__ val, u32 n,
    IndexCounters* __restrict__ ctr) {
  __shared__ u64 s_scan[kIndexBlock / 64 + 1];
  u64 carry = 0;
  for (u32 base = 0; base < tiles; base += kIndexBlock) {
    const u32 i = base + threadIdx.x;
    const u64 v = i < tiles ? tile_val[i] : 0;
    u64 tv;
    const u64 ev = dev::block_exclusive_scan<u64, kIndexBlock>(v, s_scan, &tv);
    if (i < tiles) tile_val[i] = carry + ev;
    carry += tv;
  }
  if (threadIdx.x == 0) {
    val[n] = carry;
    ctr->total = carry;
  }
}

// val[i] = exclusive prefix of the counts (blocked: a thread's items are neighbours).
__global__ __launch_bounds__(kIndexBlock) void index_val_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ tile_val,
    u64* __restrict__ val) {
  __shared__ u64 s_scan[kIndexBlock / 64 + 1];
  const u64 first = (u64)blockIdx.x * kIndexTile + (u64)threadIdx.x * kIndexItems;
  u64 c[kIndexItems];
  u64 sum = 0;
#pragma unroll
  for (int t = 0; t < kIndexItems; ++t) {
    c[t] = first + t < n ? recs[first + t].count : 0;
    sum += c[t];
  }
  u64 tot;
  u64 at = dev::block_exclusive_scan<u64, kIndexBlock>(sum, s_scan, &tot) + tile_val[blockIdx.x];
#pragma unroll
  for (int t = 0; t < kIndexItems; ++t) {
    if (first + t < n) val[first + t] = at;
    at += c[t];
  }
}

// One wave per line; a wave takes `group` consecutive lines at a time, grid-stride over the
// groups.  It first counts the group's emitted tokens (ballots only), reserves their slots
// with ONE atomic -- every wave of the grid adds to the same word, and such atomics
// complete one after the other: one per line was the whole kernel's time on 10^6 lines --
// and then walks the lines again (their bytes are cached by then) to build, search and
// write the pairs.
__global__ __launch_bounds__(kIdxMapBlock) void index_map_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const OutRecord* __restrict__ recs, u32 n, u64* __restrict__ pairs, u64 pair_cap,
    IndexCounters* __restrict__ ctr) {
  __shared__ unsigned char s_row[kIdxMapWaves][kIdxRow];
  const int lane = dev::lane_id();
  unsigned char* row = s_row[dev::wave_id()];
  const u64 num_nl = lctr->num_newlines;
  // the text's lines: one per newline, and what follows the last newline (empty when the
  // text ends with its newline: no tokens)
  const u64 num_lines = bytes ? num_nl + 1 : 0;
  const u64 wave = (u64)blockIdx.x * kIdxMapWaves + dev::wave_id();
  const u64 nwaves = (u64)gridDim.x * kIdxMapWaves;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 E = (u32)emits_per_line;
  for (u64 g0 = wave * group; g0 < num_lines; g0 += nwaves * group) {
    const u64 g1 = g0 + group < num_lines ? g0 + group : num_lines;
    // ---- the group's emitted tokens ----
    u32 total = 0;
    for (u64 line = g0; line < g1; ++line) {
      const u64 start = line ? nl_pos[line - 1] + 1 : 0;
      const u64 end = line < num_nl ? nl_pos[line] : bytes;
      u32 seen = 0;
      u64 carry = 0;
      for (u64 pos = start; pos < end && seen < E; pos += 64) {
        const u64 p = pos + lane;
        const unsigned c = p < end ? (unsigned char)text[p] : 0u;
        bool last;
        seen += (u32)__popcll(dev::step_starts(c, dm, &carry, &last));
        if (last) break;
      }
      total += seen < E ? seen : E;
    }
    if (total == 0) continue;  // (wave-uniform)
    u32 at = 0;  // the group's first slot
    if (lane == 0) at = atomicAdd(&ctr->written, total);
    at = (u32)__shfl((int)at, 0, 64);
    // ---- the pairs ----
    for (u64 line = g0; line < g1; ++line) {
      const u64 start = line ? nl_pos[line - 1] + 1 : 0;
      const u64 end = line < num_nl ? nl_pos[line] : bytes;
      u32 seen = 0;   // token starts of this line before the current step
      u64 carry = 0;
      for (u64 pos = start; pos < end && seen < E; pos += 64) {
        const u64 p = pos + lane;
        const unsigned c = p < end ? (unsigned char)text[p] : 0u;
        const u64 p2 = pos + 64 + lane;
        const unsigned c2 = (lane < 32 && p2 < end) ? (unsigned char)text[p2] : 0u;
        __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
        row[lane] = (unsigned char)c;
        if (lane < 32) row[64 + lane] = (unsigned char)c2;
        __builtin_amdgcn_wave_barrier();
        bool last;
        const u64 starts = dev::step_starts(c, dm, &carry, &last);
        const u32 ord = seen + (u32)__popcll(starts & below);
        const bool emit = ((starts >> lane) & 1ull) && ord < E;
        const u64 em = dev::ballot(emit);
        bool found = false;
        if (emit) {
          u64 w0, w1, w2, w3;
          dev::pack_row_key(row, lane, dm, max_key_len, &w0, &w1, &w2, &w3);
          const u32 rank = dev::find_rank(recs, n, w0, w1, w2, w3);
          found = rank < n;
          const u64 slot = (u64)at + (u32)__popcll(em & below);
          if (found && slot < pair_cap) pairs[slot] = ((u64)rank << 32) | (u64)(u32)line;
        }
        const u64 mm = dev::ballot(emit && !found);
        if (mm && lane == __ffsll((unsigned long long)mm) - 1)
          atomicAdd(&ctr->miss, (u32)__popcll(mm));
        at += (u32)__popcll(em);
        seen += (u32)__popcll(starts);
        if (last) break;  // a NUL, or the line end, inside this step
      }
    }
  }
}

// One thread, between the map and the sort: the sort takes its length from device memory,
// and only the expected number of pairs is ever sorted -- a tokeniser that disagreed with
// the word job's (the host then throws) must not run the sort past its buffers.
__global__ void index_seal_kernel(IndexCounters* __restrict__ ctr, u32 expect) {
  ctr->sort_n = ctr->written == expect ? expect : 0u;
}

// postings[j] = first_line + the pair's line; a pair outside its word's CSR range counts
// as misplaced.
__global__ __launch_bounds__(256) void index_emit_kernel(const u64* __restrict__ sorted, u64 T,
                                                         const u64* __restrict__ val, u32 n,
                                                         u32 first_line, u32* __restrict__ postings,
                                                         IndexCounters* __restrict__ ctr) {
  if (ctr->sort_n != (u32)T) return;  // nothing was sorted (workgroup-uniform)
  u32 bad = 0;
  for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < T; j += (u64)gridDim.x * 256) {
    const u64 w = sorted[j];
    const u32 r = (u32)(w >> 32);
    postings[j] = first_line + (u32)w;
    if (r >= n || j < val[r] || j >= val[r + 1]) ++bad;
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->misplaced, bad);
  }
}

u64 lb_words(u64 text_cap) { return div_up(std::max<u64>(text_cap, 1), (u64)kLineIdxTile) + 1; }

// The workspace's parts in order; `take` is called once per part with its byte size.
template <class Take>
void index_layout(u64 pair_cap, u64 rec_cap, u64 line_cap, u64 text_cap, Take&& take) {
  const u64 tiles = div_up(std::max<u64>(rec_cap, 1), (u64)kIndexTile);
  take(index_zero_bytes(text_cap));                                       // zeroed per job
  take(pair_cap * 8);                                                     // pairs
  take(pair_cap * 8);                                                     // zeros
  take(pair_cap * 8);                                                     // sorted
  take(pair_cap * 8);                                                     // spare
  take(pair_cap * 4);                                                     // postings
  take((rec_cap + 1) * 8);                                                // val
  take(tiles * 8);                                                        // tile_val
  take((line_cap + 1) * 8);                                               // nl_pos
  take(radix_zero_bytes(pair_cap));                                       // rx counters + status
  take((u64)radix_hist_blocks(pair_cap) * kNumPositions * 256 * 4);       // rx hist_part
  take(sizeof(SortPlan));                                                 // rx plan
  take(pair_cap * 8);                                                     // rx keys[0]
  take(pair_cap * 8);                                                     // rx keys[1]
  take(pair_cap * 4);                                                     // rx vals[0]
  take(pair_cap * 4);                                                     // rx vals[1]
}

}  // namespace

u64 index_zero_bytes(u64 text_cap) { return 256 + 8 * lb_words(text_cap); }

u64 index_workspace_bytes(u64 pair_cap, u64 rec_cap, u64 line_cap, u64 text_cap) {
  u64 b = 0;
  index_layout(pair_cap, rec_cap, line_cap, text_cap,
               [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void index_workspace_carve(char* base, u64 pair_cap, u64 rec_cap, u64 line_cap, u64 text_cap,
                           IndexWorkspace* ws) {
  char* part[16];
  int k = 0;
  u64 b = 0;
  index_layout(pair_cap, rec_cap, line_cap, text_cap, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  // zero block: [MapCounters | IndexCounters @64 | tile counter @128 | status words @256]
  static_assert(sizeof(MapCounters) <= 64 && sizeof(IndexCounters) <= 64, "zero block layout");
  ws->zero = part[0];
  ws->zero_bytes = index_zero_bytes(text_cap);
  ws->lctr = reinterpret_cast<MapCounters*>(part[0]);
  ws->ctr = reinterpret_cast<IndexCounters*>(part[0] + 64);
  ws->lb.tile_counter = reinterpret_cast<u32*>(part[0] + 128);
  ws->lb.status = reinterpret_cast<u64*>(part[0] + 256);
  ws->pairs = reinterpret_cast<u64*>(part[1]);
  ws->zeros = reinterpret_cast<u64*>(part[2]);
  ws->sorted = reinterpret_cast<u64*>(part[3]);
  ws->spare = reinterpret_cast<u64*>(part[4]);
  ws->postings = reinterpret_cast<u32*>(part[5]);
  ws->val = reinterpret_cast<u64*>(part[6]);
  ws->tile_val = reinterpret_cast<u64*>(part[7]);
  ws->nl_pos = reinterpret_cast<u64*>(part[8]);
  ws->rx.tile_counters = reinterpret_cast<u32*>(part[9]);
  ws->rx.status = ws->rx.tile_counters + kNumPositions;
  ws->rx.hist_part = reinterpret_cast<u32*>(part[10]);
  ws->rx.plan = reinterpret_cast<SortPlan*>(part[11]);
  ws->rx.keys[0] = reinterpret_cast<u64*>(part[12]);
  ws->rx.keys[1] = reinterpret_cast<u64*>(part[13]);
  ws->rx.vals[0] = reinterpret_cast<u32*>(part[14]);
  ws->rx.vals[1] = reinterpret_cast<u32*>(part[15]);
  ws->rx.cap = pair_cap;
  ws->pair_cap = pair_cap;
  ws->rec_cap = rec_cap;
  ws->line_cap = line_cap;
  ws->text_cap = text_cap;
}

void launch_index(const IndexJob& job, IndexWorkspace& ws, SortPlan* h_plan, hipStream_t s) {
  const u64 n = job.n, T = job.tokens;
  LOCUST_CHECK_ARG(n < (1ull << 32) && n <= ws.rec_cap,
                   "index: " + std::to_string(n) + " records exceed the workspace (" +
                       std::to_string(ws.rec_cap) + ")");
  LOCUST_CHECK_ARG(T < (1ull << 32) && T <= ws.pair_cap,
                   "index: " + std::to_string(T) + " tokens exceed the workspace (" +
                       std::to_string(ws.pair_cap) + ")");
  LOCUST_CHECK_ARG(job.bytes <= ws.text_cap && job.num_lines <= ws.line_cap,
                   "index: the text exceeds the workspace");
  LOCUST_CHECK_ARG(job.first_line + job.num_lines <= (1ull << 32),
                   "index: line numbers past 2^32 do not fit a u32 posting");
  // the counters and the line index's look-back words
  LOCUST_HIP_CHECK(hipMemsetAsync(ws.zero, 0, ws.zero_bytes, s));
  // a. offsets
  const u32 tiles = (u32)div_up(std::max<u64>(n, 1), (u64)kIndexTile);
  index_tile_sum_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(job.recs, (u32)n, ws.tile_val);
  LOCUST_HIP_LAUNCH_CHECK();
  index_tile_scan_kernel<<<dim3(1), dim3(kIndexBlock), 0, s>>>(ws.tile_val, tiles, ws.val, (u32)n,
                                                              ws.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
  index_val_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(job.recs, (u32)n, ws.tile_val, ws.val);
  LOCUST_HIP_LAUNCH_CHECK();
  if (job.bytes == 0 || n == 0 || T == 0) return;  // nothing to index
  // b. line starts
  launch_line_index(job.text, job.bytes, ws.nl_pos, ws.lctr, ws.lb, s);
  // c. one pair word per emitted token
  // lines per slot reservation: one while the lines are few (every line its own wave),
  // up to 64 when each wave of a full grid has many lines to walk anyway
  const u64 lines = std::max<u64>(job.num_lines, 1);
  const u32 group = (u32)std::min<u64>(div_up(lines, (u64)kIdxMapMaxBlocks), 64);
  const u32 blocks = (u32)std::min<u64>(div_up(div_up(lines, (u64)group), (u64)kIdxMapWaves),
                                        (u64)kIdxMapMaxBlocks);
  index_map_kernel<<<dim3(blocks), dim3(kIdxMapBlock), 0, s>>>(
      job.text, job.bytes, ws.nl_pos, ws.lctr, job.dm, job.emits_per_line, job.max_key_len, group,
      job.recs, (u32)n, ws.pairs, ws.pair_cap, ws.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
  index_seal_kernel<<<dim3(1), dim3(1), 0, s>>>(ws.ctr, (u32)T);
  LOCUST_HIP_LAUNCH_CHECK();
  // d. order: the pair words ascending = (word rank, line)
  ConstKeysSoA keys;
  KeysSoA sorted;
  keys.w[0] = ws.pairs;
  sorted.w[0] = ws.sorted;
  for (int j = 1; j < kKeyWords; ++j) {
    keys.w[j] = ws.zeros;
    sorted.w[j] = ws.spare;  // the gather's copies of the zero words
  }
  radix_sort(keys, &ws.ctr->sort_n, T, ws.rx, nullptr, sorted, nullptr, nullptr, h_plan, s);
  // e. postings
  const u32 eblocks = (u32)std::min<u64>(div_up(T, 256), 4096);
  index_emit_kernel<<<dim3(eblocks), dim3(256), 0, s>>>(ws.sorted, T, ws.val, (u32)n,
                                                        (u32)job.first_line, ws.postings, ws.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_index() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&index_map_kernel));
}

}  // namespace locust
