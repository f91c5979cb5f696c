// The restrict stage of a search batch over a corpus (kernels.hpp "corpus.hip"; the rules are
// engine.hpp "corpus" and "file sets"): the hit and verify kernels have left H unsorted pair
// words query << 32 | (line - first_line) in `pairs`; a batch in which at least one query names a
// file set keeps, of those, the pairs whose line lies in a segment of its query's set.
//   restrict  one pass in tiles of kCorpusTile over the H pair words.  A pair's segment is the
//             last one whose first line is <= first_line + low32(pair): a binary search of the
//             device table, S u32 first lines (S >= 1, table[0] == first_line).  Its ordinal's
//             bit is tested in the query's set (a bitmap over the resident ordinals, one per
//             distinct set of the batch; a query without a set keeps everything).  Inside a
//             tile the kept pairs' positions come from a workgroup scan of the threads' counts;
//             the tile's base from one atomic per tile on `kept`.  The pairs were in arbitrary
//             order before, and the sort behind the stage decides the order of the answer, so
//             the order of the tiles does not matter.  The kept pairs go to `out` (the hit
//             workspace's `cands`, idle at that point), never past out_cap; the per-query hit
//             counts are rebuilt as commit_hits builds them: one atomic per wave, step and
//             distinct query.  A pair that names no query of the batch or a line in front of the
//             table counts in `stray` (the host throws) and is dropped.
//   seal      one thread: written = sort_n = kept, so the order and rank stages see the
//             restricted pairs exactly as they see a hit kernel's.
// Data crosses between workgroups at the kernel boundary alone; no word is polled.
// Behind it in this file: the by-file stage of a batch that asks for answers by file (kernels.hpp
// launch_corpus_by_file states the kernels): resolve, the heads' three-kernel scan, offsets.
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {

namespace {

// The ordinal of the last segment whose first line is <= line, or S when table[0] > line.
// (Never reads outside table[0 .. S).)
__device__ __forceinline__ u32 corpus_locate(const u32* __restrict__ table, u32 S, u32 line) {
  u32 lo = 0, hi = S;  // the number of first lines <= line lies in [lo, hi]
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (table[mid] <= line)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : S;
}

}  // namespace

__global__ __launch_bounds__(kCorpusBlock) void corpus_restrict_kernel(
    const u64* __restrict__ pairs, u64 H, u32 first_line, const u32* __restrict__ table, u32 S,
    const u32* __restrict__ q_set, const u32* __restrict__ bitmaps, u32 set_words, u32 sets, u32 Q,
    u64* __restrict__ out, u64 out_cap, u32* __restrict__ q_hits,
    CorpusCounters* __restrict__ cc) {
  __shared__ u32 s_scan[kCorpusBlock / 64 + 1];
  __shared__ u32 s_base;
  const int lane = dev::lane_id();
  u32 stray = 0;
  for (u64 tile = blockIdx.x; tile * kCorpusTile < H; tile += gridDim.x) {  // (uniform)
    u64 w[kCorpusItems];
    u32 keep = 0;  // bit j: item j stays
#pragma unroll
    for (int j = 0; j < kCorpusItems; ++j) {
      const u64 e = tile * kCorpusTile + (u64)j * kCorpusBlock + threadIdx.x;
      w[j] = 0;
      if (e >= H) continue;
      w[j] = pairs[e];
      const u32 q = (u32)(w[j] >> 32);
      const u32 ord = corpus_locate(table, S, first_line + (u32)w[j]);
      if (q >= Q || ord >= S) {
        ++stray;
        continue;
      }
      const u32 set = q_set[q];
      bool in = set == kCorpusNoSet;
      if (!in && set < sets)
        in = (bitmaps[(u64)set * set_words + (ord >> 5)] >> (ord & 31u)) & 1u;
      keep |= (u32)in << j;
    }
    u32 total;
    u32 at = dev::block_exclusive_scan<u32, kCorpusBlock>((u32)__popc(keep), s_scan, &total);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(&cc->kept, total) : 0u;
    __syncthreads();
    const u64 base = s_base;
#pragma unroll
    for (int j = 0; j < kCorpusItems; ++j) {
      const bool hit = (keep >> j) & 1u;
      if (hit) {
        const u64 slot = base + at++;
        if (slot < out_cap) out[slot] = w[j];
      }
      // per query: one atomic for all of the wave's kept pairs of that query
      const u32 q = (u32)(w[j] >> 32);
      u64 rem = dev::ballot(hit);
      while (rem) {  // (wave-uniform)
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const u32 ql = (u32)__shfl((int)q, leader, 64);
        const u64 same = dev::ballot(hit && q == ql);
        if (lane == leader) atomicAdd(&q_hits[ql], (u32)__popcll(same));
        rem &= ~same;
      }
    }
    __syncthreads();  // (s_base is read: the next tile may write it)
  }
  const u64 sm = dev::ballot(stray != 0);
  if (sm) {
    stray = dev::wave_reduce_sum(stray);
    if (lane == 0) atomicAdd(&cc->stray, stray);
  }
}

__global__ void corpus_seal_kernel(const CorpusCounters* __restrict__ cc, u64 out_cap,
                                   SearchCounters* __restrict__ ctr) {
  const u32 kept = cc->kept;
  ctr->written = kept;
  ctr->sort_n = (u64)kept <= out_cap ? kept : 0u;
}

// ---- answers by file ----
__global__ __launch_bounds__(kCorpusBlock) void corpus_resolve_kernel(
    const u32* __restrict__ lines, u64 E, const u64* __restrict__ offsets, u32 Q,
    const u32* __restrict__ table, const u32* __restrict__ ids, u32 S, u64 base0,
    u32* __restrict__ line_file, u32* __restrict__ line_local, u64* __restrict__ keys,
    CorpusCounters* __restrict__ cc) {
  __shared__ u32 s_table[kCorpusLdsSegs];
  const bool staged = S <= (u32)kCorpusLdsSegs;  // (uniform)
  if (staged) {
    for (u32 i = threadIdx.x; i < S; i += kCorpusBlock) s_table[i] = table[i];
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) cc->sort_n = (u32)E;
  u32 bad = 0;
  for (u64 j = (u64)blockIdx.x * kCorpusBlock + threadIdx.x; j < E;
       j += (u64)gridDim.x * kCorpusBlock) {
    // the query: the last q < Q with offsets[q] <= j (an empty query owns no j)
    u32 lo = 0, hi = Q;
    while (lo < hi) {
      const u32 mid = lo + ((hi - lo) >> 1);
      if (offsets[mid] <= j)
        lo = mid + 1;
      else
        hi = mid;
    }
    const u32 line = lines[j];
    u32 ord = staged ? corpus_locate(s_table, S, line) : corpus_locate(table, S, line);
    u32 q = lo ? lo - 1 : 0;
    if (lo == 0 || ord >= S || j >= offsets[q + 1]) {
      ++bad;
      ord = 0;
    }
    const u32 first = staged ? s_table[ord] : table[ord];
    line_file[j] = ids[ord];
    line_local[j] = line - first + (ord == 0 ? (u32)base0 : 0u);
    keys[j] = ((u64)q << 32) | (u64)ord;
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&cc->unlocated, bad);
  }
}

// tile_val[tile] = the heads among the tile's keys.
__global__ __launch_bounds__(kCorpusBlock) void corpus_head_sum_kernel(
    const u64* __restrict__ keys, u64 E, u64* __restrict__ tile_val) {
  __shared__ u32 s_sum[kCorpusBlock / 64];
  const u64 first = (u64)blockIdx.x * kCorpusTile + (u64)threadIdx.x * kCorpusItems;
  u32 c = 0;
#pragma unroll
  for (int t = 0; t < kCorpusItems; ++t) {
    const u64 j = first + t;
    if (j < E) c += j == 0 || keys[j] != keys[j - 1];
  }
  c = dev::wave_reduce_sum(c);
  if (dev::lane_id() == 0) s_sum[dev::wave_id()] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 t = 0;
#pragma unroll
    for (int w = 0; w < kCorpusBlock / 64; ++w) t += s_sum[w];
    tile_val[blockIdx.x] = t;
  }
}

// One workgroup: exclusive scan of the tile sums, in place; the total to cc->runs.
__global__ __launch_bounds__(kCorpusBlock) void corpus_head_scan_kernel(
    u64* __restrict__ tile_val, u32 tiles, CorpusCounters* __restrict__ cc) {
  __shared__ u64 s_scan[kCorpusBlock / 64 + 1];
  u64 carry = 0;
  for (u32 base = 0; base < tiles; base += kCorpusBlock) {  // (uniform)
    const u32 i = base + threadIdx.x;
    const u64 v = i < tiles ? tile_val[i] : 0;
    u64 tv;
    const u64 ev = dev::block_exclusive_scan<u64, kCorpusBlock>(v, s_scan, &tv);
    if (i < tiles) tile_val[i] = carry + ev;
    carry += tv;
  }
  if (threadIdx.x == 0) cc->runs = (u32)carry;
}

// Every head writes its run: (id, count) and the key, at the tile's base + its rank in the tile
// (blocked: a thread's keys are neighbours, so the runs keep the keys' order).
__global__ __launch_bounds__(kCorpusBlock) void corpus_head_emit_kernel(
    const u64* __restrict__ keys, u64 E, const u64* __restrict__ tile_val,
    const u32* __restrict__ ids, u32 S, u64 out_cap, u64* __restrict__ run_keys,
    u32* __restrict__ file_ids, u32* __restrict__ file_counts) {
  __shared__ u32 s_scan[kCorpusBlock / 64 + 1];
  const u64 first = (u64)blockIdx.x * kCorpusTile + (u64)threadIdx.x * kCorpusItems;
  u32 heads = 0;  // bit t: key first + t heads a run
#pragma unroll
  for (int t = 0; t < kCorpusItems; ++t) {
    const u64 j = first + t;
    if (j < E && (j == 0 || keys[j] != keys[j - 1])) heads |= 1u << t;
  }
  u32 total;
  u64 at = tile_val[blockIdx.x] +
           dev::block_exclusive_scan<u32, kCorpusBlock>((u32)__popc(heads), s_scan, &total);
#pragma unroll 1
  for (int t = 0; t < kCorpusItems; ++t) {
    if (!((heads >> t) & 1u)) continue;
    const u64 j = first + t, key = keys[j];
    u64 lo = j + 1, hi = E;  // the run's end: the first key behind j that differs
    while (lo < hi) {
      const u64 mid = lo + ((hi - lo) >> 1);
      if (keys[mid] == key)
        lo = mid + 1;
      else
        hi = mid;
    }
    const u32 ord = (u32)key;
    if (at < out_cap) {
      run_keys[at] = key;
      file_ids[at] = ord < S ? ids[ord] : 0u;
      file_counts[at] = (u32)(lo - j);
    }
    ++at;
  }
}

// file_off[q] = the runs of the queries in front of q, q <= Q.
__global__ __launch_bounds__(kCorpusBlock) void corpus_off_kernel(
    const u64* __restrict__ run_keys, const CorpusCounters* __restrict__ cc, u64 out_cap, u32 Q,
    u64* __restrict__ file_off) {
  const u32 q = blockIdx.x * kCorpusBlock + threadIdx.x;
  if (q > Q) return;
  const u64 want = (u64)q << 32;
  u64 lo = 0, hi = cc->runs <= out_cap ? cc->runs : out_cap;
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (run_keys[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  file_off[q] = lo;
}

void corpus_by_file_carve(char* base, u64 cap, CorpusByFile* f, u64* bytes) {
  const u64 tiles = div_up(cap, (u64)kCorpusTile) + 1;
  u64 off[10];
  u64 b = 0;
  int k = 0;
  for (const u64 part : {(u64)64, cap * 8, cap * 8, cap * 8, tiles * 8,
                         ((u64)kSearchMaxQueries + 1) * 8, cap * 4, cap * 4, cap * 4, cap * 4}) {
    b = align_up(b, 256);
    off[k++] = b;
    b += part;
  }
  if (bytes) *bytes = align_up(b, 256);
  if (!f) return;
  f->ctr = reinterpret_cast<CorpusCounters*>(base + off[0]);
  f->keys = reinterpret_cast<u64*>(base + off[1]);
  f->sorted = reinterpret_cast<u64*>(base + off[2]);
  f->run_keys = reinterpret_cast<u64*>(base + off[3]);
  f->tile_val = reinterpret_cast<u64*>(base + off[4]);
  f->file_off = reinterpret_cast<u64*>(base + off[5]);
  f->line_file = reinterpret_cast<u32*>(base + off[6]);
  f->line_local = reinterpret_cast<u32*>(base + off[7]);
  f->file_ids = reinterpret_cast<u32*>(base + off[8]);
  f->file_counts = reinterpret_cast<u32*>(base + off[9]);
  f->cap = cap;
}

void launch_corpus_by_file(const CorpusSets& c, u32 segments, u64 base0, const u64* offsets,
                           u32 queries, u64 lines, bool ranked, SearchHits& h, CorpusByFile& f,
                           SortPlan* h_plan, hipStream_t s) {
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && lines <= f.cap &&
                       lines <= h.cap && lines < (1ull << 32) && segments >= 1 &&
                       segments <= c.seg_cap,
                   "search: " + std::to_string(lines) + " returned lines in " +
                       std::to_string(segments) + " files exceed the by-file arrays (" +
                       std::to_string(f.cap) + ", " + std::to_string(c.seg_cap) + ")");
  LOCUST_HIP_CHECK(hipMemsetAsync(f.ctr, 0, sizeof(CorpusCounters), s));
  const u64* keys = f.keys;
  if (lines) {
    const u32 rblocks = (u32)std::min<u64>(div_up(lines, (u64)kCorpusBlock), (u64)kCorpusMaxBlocks);
    corpus_resolve_kernel<<<dim3(rblocks), dim3(kCorpusBlock), 0, s>>>(
        h.lines, lines, offsets, queries, c.table, c.ids, segments, base0, f.line_file,
        f.line_local, f.keys, f.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
    if (ranked) {  // the winners stand in rank order: their files alternate
      ConstKeysSoA in;
      KeysSoA out;
      in.w[0] = f.keys;
      out.w[0] = f.sorted;
      for (int j = 1; j < kKeyWords; ++j) {
        in.w[j] = h.zeros;
        out.w[j] = h.spare;  // the gather's copies of the zero words
      }
      radix_sort(in, &f.ctr->sort_n, lines, h.rx, nullptr, out, nullptr, nullptr, h_plan, s);
      keys = f.sorted;
    }
    const u32 tiles = (u32)div_up(lines, (u64)kCorpusTile);
    corpus_head_sum_kernel<<<dim3(tiles), dim3(kCorpusBlock), 0, s>>>(keys, lines, f.tile_val);
    LOCUST_HIP_LAUNCH_CHECK();
    corpus_head_scan_kernel<<<dim3(1), dim3(kCorpusBlock), 0, s>>>(f.tile_val, tiles, f.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
    corpus_head_emit_kernel<<<dim3(tiles), dim3(kCorpusBlock), 0, s>>>(
        keys, lines, f.tile_val, c.ids, segments, f.cap, f.run_keys, f.file_ids, f.file_counts);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  corpus_off_kernel<<<dim3((u32)div_up((u64)queries + 1, (u64)kCorpusBlock)), dim3(kCorpusBlock),
                      0, s>>>(f.run_keys, f.ctr, f.cap, queries, f.file_off);
  LOCUST_HIP_LAUNCH_CHECK();
}

u64 corpus_sets_bytes(u64 seg_cap, u64 set_cap) {
  u64 b = 0;
  corpus_sets_carve(nullptr, seg_cap, set_cap, nullptr, &b);
  return b;
}

void corpus_sets_carve(char* base, u64 seg_cap, u64 set_cap, CorpusSets* c, u64* bytes) {
  const u64 words = div_up(seg_cap, (u64)32);
  u64 off[5];
  u64 b = 0;
  int k = 0;
  for (const u64 part : {(u64)64, seg_cap * 4, (u64)kSearchMaxQueries * 4, set_cap * words * 4,
                         seg_cap * 4}) {
    b = align_up(b, 256);
    off[k++] = b;
    b += part;
  }
  if (bytes) *bytes = align_up(b, 256);
  if (!c) return;
  c->ctr = reinterpret_cast<CorpusCounters*>(base + off[0]);
  c->table = reinterpret_cast<u32*>(base + off[1]);
  c->q_set = reinterpret_cast<u32*>(base + off[2]);
  c->bitmaps = reinterpret_cast<u32*>(base + off[3]);
  c->ids = reinterpret_cast<u32*>(base + off[4]);
  c->seg_cap = seg_cap;
  c->set_cap = set_cap;
}

void launch_corpus_restrict(const SearchIndex& ix, const SearchBatch& b, const CorpusSets& c,
                            u32 segments, u32 sets, u32 queries, u64 hits, SearchHits& h,
                            hipStream_t s) {
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && hits <= h.cap &&
                       hits < (1ull << 32),
                   "search: " + std::to_string(hits) + " hits to restrict exceed the workspace (" +
                       std::to_string(h.cap) + ")");
  LOCUST_CHECK_ARG(segments >= 1 && segments <= c.seg_cap && sets <= c.set_cap,
                   "search: " + std::to_string(segments) + " segments and " +
                       std::to_string(sets) + " file sets exceed the corpus arrays (" +
                       std::to_string(c.seg_cap) + ", " + std::to_string(c.set_cap) + ")");
  LOCUST_HIP_CHECK(hipMemsetAsync(c.ctr, 0, sizeof(CorpusCounters), s));
  LOCUST_HIP_CHECK(hipMemsetAsync(b.q_hits, 0, (u64)queries * sizeof(u32), s));
  if (hits) {
    const u32 blocks = (u32)std::min<u64>(div_up(hits, (u64)kCorpusTile), (u64)kCorpusMaxBlocks);
    // (the bitmaps' row length follows the resident segments, not the arrays' capacity)
    corpus_restrict_kernel<<<dim3(blocks), dim3(kCorpusBlock), 0, s>>>(
        h.pairs, hits, ix.first_line, c.table, segments, c.q_set, c.bitmaps,
        (u32)div_up((u64)segments, (u64)32), sets, queries, h.cands, h.cap, b.q_hits, c.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  corpus_seal_kernel<<<dim3(1), dim3(1), 0, s>>>(c.ctr, h.cap, b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
  // the kept pairs are the batch's pairs from here on; what held them before is the idle array
  std::swap(h.pairs, h.cands);
}

void warm_module_corpus() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&corpus_restrict_kernel));
}

}  // namespace locust
