// The tally stage of a search batch (kernels.hpp "tally.hip"; the rule is engine.hpp "tally: the
// words of the returned lines"): for every query the K most frequent index words of its returned
// lines.  The text, the line starts, the key-ordered records and the returned lines are all
// resident beside the index; only the winners' records, three per-query arrays and the counters
// cross PCIe.
//
// Shape (gfx950, wave64): the show kernels' skeleton over index.hip's walk.  One wave per entry,
// up to 64 consecutive entries per wave and round; lane i keeps entry i's line and (map) finds
// its query by a binary search in the per-query offsets.  Two walks with a scan between them:
//  * measure: ballots only, per entry the emitted tokens;
//  * tally_scan_kernel: one workgroup, the exclusive u64 scan of the counts;
//  * map: the step's bytes (and the 32 behind them) staged in the wave's LDS row, the lanes that
//    own an emitting start pack their key (device/linetok.hpp), search it (device/rank.hpp) and
//    write q << 32 | rank at tok_off[i] + the token's ordinal.  No atomics on the output.
// Then two device-wide sorts with a run-length pass between them: the pair words sorted are
// (query, rank) runs; a run's head finds its end by binary search and writes one rank key
// query << 54 | (cmask - count) << r | rank; those sorted are, per query, the words by (count
// descending, rank = key ascending).  One workgroup finds the queries' segments, one thread per
// key writes the winners' records.  Data crosses between workgroups only at kernel boundaries
// (the radix sort keeps its own look-back); this file adds no polled word.
#include <algorithm>

#include "locust/device/linetok.hpp"
#include "locust/device/rank.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTallyBlock = 256;
constexpr int kTallyWaves = kTallyBlock / 64;
constexpr int kTallyMaxBlocks = 2048;  // 8 workgroups per CU, as the show kernels
constexpr int kScanBlock = 512;
constexpr int kScanItems = 8;  // consecutive entries per thread and tile
constexpr int kOffBlock = 256;

// What a walk reads and writes (one kernel argument).
struct TallyJob {
  const char* text;
  u64 bytes;
  const u64* nl_pos;
  const MapCounters* lctr;
  DelimMask dm;
  int emits_per_line, max_key_len;
  u32 group, Q, first_line, n;
  const OutRecord* recs;
  const u32* lines;    // [E] the returned lines, global numbers
  const u64* offsets;  // [Q + 1] their per-query segments
  u64 E;
  TallyCounters* ctr;
  u32* n_tok;          // measure writes, the scan reads
  const u64* tok_off;  // map reads
  u64* pairs;
  u64 pair_cap;
};

// The walk of both kernels: measure counts entry i's emitted tokens, map writes their pair words.
template <bool kMap>
__device__ __forceinline__ void tally_body(unsigned char* row, const TallyJob& j) {
  const char* __restrict__ text = j.text;
  const u64* __restrict__ nl_pos = j.nl_pos;
  const u32* __restrict__ lines = j.lines;
  const u64* __restrict__ offsets = j.offsets;
  const u64* __restrict__ tok_off = j.tok_off;
  const DelimMask& dm = j.dm;
  const int lane = dev::lane_id();
  const u64 bytes = j.bytes;
  const u64 num_nl = j.lctr->num_newlines;
  const u64 E = j.E;
  const u32 Q = j.Q, group = j.group, n = j.n;
  const u32 EM = (u32)j.emits_per_line;
  const u32 wave = blockIdx.x * kTallyWaves + dev::wave_id();
  // a round of all waves: at most kTallyMaxBlocks * kTallyWaves * 64 = 2^19 entries
  const u32 stride = gridDim.x * kTallyWaves * group;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  for (u64 g0 = (u64)wave * group; g0 < E; g0 += stride) {  // (wave-uniform)
    const u32 cnt = (u32)(g0 + group < E ? group : E - g0);
    // lane i: entry i -- its line, and (map) its query: offsets[q] <= e < offsets[q + 1]
    u32 myq = 0, myline = 0;
    if ((u32)lane < cnt) {
      const u64 e = g0 + lane;
      myline = lines[e] - j.first_line;
      if (kMap) {
        u32 lo = 0, hi = Q;
        while (hi - lo > 1) {
          const u32 mid = lo + ((hi - lo) >> 1);
          if (offsets[mid] <= e)
            lo = mid;
          else
            hi = mid;
        }
        myq = lo;
      }
    }
    u32 my_n = 0;  // measure: lane i keeps entry i's tokens
    u32 bad = 0;   // map: entries whose tokens do not number what measure counted
    for (u32 i = 0; i < cnt; ++i) {
      const u64 line = (u32)__shfl((int)myline, (int)i, 64);
      const u32 q = (u32)__shfl((int)myq, (int)i, 64);
      u32 seen = 0;  // token starts of this line before the current step
      // (a line past the text never comes from the search's own lines: no tokens)
      if (line <= num_nl) {
        const u64 start = line ? nl_pos[line - 1] + 1 : 0;
        const u64 end = line < num_nl ? nl_pos[line] : bytes;
        u64 at = 0, at_end = 0;  // map: where the entry's pair words go
        if (kMap) {
          at = tok_off[g0 + i];
          at_end = tok_off[g0 + i + 1];
        }
        u64 carry = 0;
        for (u64 pos = start; pos < end && seen < EM; pos += 64) {
          const u64 p = pos + lane;
          const unsigned c = p < end ? (unsigned char)text[p] : 0u;
          if (kMap) {
            const u64 p2 = pos + 64 + lane;
            const unsigned c2 = (lane < 32 && p2 < end) ? (unsigned char)text[p2] : 0u;
            __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
            row[lane] = (unsigned char)c;
            if (lane < 32) row[64 + lane] = (unsigned char)c2;
            __builtin_amdgcn_wave_barrier();
          }
          bool last;
          const u64 starts = dev::step_starts(c, dm, &carry, &last);
          if (kMap) {
            const u32 ord = seen + (u32)__popcll(starts & below);
            const bool emit = ((starts >> lane) & 1ull) && ord < EM;
            bool found = false;
            if (emit) {
              u64 w0, w1, w2, w3;
              dev::pack_row_key(row, lane, dm, j.max_key_len, &w0, &w1, &w2, &w3);
              const u32 rank = dev::find_rank(j.recs, n, w0, w1, w2, w3);
              found = rank < n;
              const u64 slot = at + ord;
              if (found && slot < at_end && slot < j.pair_cap)
                j.pairs[slot] = ((u64)q << 32) | (u64)rank;
            }
            const u64 mm = dev::ballot(emit && !found);
            if (mm && lane == __ffsll((unsigned long long)mm) - 1)
              atomicAdd(&j.ctr->miss, (u32)__popcll(mm));
          }
          seen += (u32)__popcll(starts);
          if (last) break;  // a NUL, or the line end, inside this step
        }
        seen = seen < EM ? seen : EM;
        if (kMap) bad += at + seen != at_end ? 1u : 0u;
      }
      if (!kMap && (u32)lane == i) my_n = seen;
    }
    if (kMap) {
      if (bad && lane == 0) atomicAdd(&j.ctr->mismatch, bad);
    } else if ((u32)lane < cnt) {
      j.n_tok[g0 + lane] = my_n;
    }
  }
}

__global__ __launch_bounds__(kTallyBlock) void tally_measure_kernel(TallyJob j) {
  tally_body<false>(nullptr, j);
}

__global__ __launch_bounds__(kTallyBlock) void tally_map_kernel(TallyJob j) {
  __shared__ unsigned char s_row[kTallyWaves][dev::kLineRow];
  tally_body<true>(s_row[dev::wave_id()], j);
}

// One workgroup: tok_off[0 .. E] = the exclusive scan of n_tok, kScanItems consecutive entries
// per thread and tile, kept in registers; the total also to the counters.
__global__ __launch_bounds__(kScanBlock) void tally_scan_kernel(const u32* __restrict__ n_tok,
                                                                u64 E, u64* __restrict__ tok_off,
                                                                TallyCounters* __restrict__ ctr) {
  __shared__ u64 s_scan[kScanBlock / 64 + 1];
  u64 carry = 0;
  for (u64 base = 0; base < E; base += (u64)kScanBlock * kScanItems) {  // (workgroup-uniform)
    const u64 first = base + (u64)threadIdx.x * kScanItems;
    u32 nt[kScanItems];
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      nt[k] = first + k < E ? n_tok[first + k] : 0u;
      v += nt[k];
    }
    u64 tot;
    u64 ex = carry + dev::block_exclusive_scan<u64, kScanBlock>(v, s_scan, &tot);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
      if (first + k < E) {
        tok_off[first + k] = ex;
        ex += nt[k];
      }
    carry += tot;
  }
  if (threadIdx.x == 0) {
    tok_off[E] = carry;
    ctr->tokens = carry;
  }
}

// One thread, between the map and the sort: the sort takes its length from device memory, and
// only pair words that were all written are ever sorted -- a walk that disagreed with the
// measure pass or the index (the host then throws) must not hand the sort unwritten words.
__global__ void tally_seal_kernel(TallyCounters* __restrict__ ctr, u32 expect) {
  ctr->sort_n = (ctr->tokens == expect && ctr->miss == 0 && ctr->mismatch == 0) ? expect : 0u;
}

// One thread per sorted pair word: the heads of the (query, rank) runs write the rank keys.
__global__ __launch_bounds__(256) void tally_runs_kernel(const u64* __restrict__ sorted,
                                                         TallyCounters* __restrict__ ctr, u32 r,
                                                         u64 cmask, u32 Q, u32 n,
                                                         u64* __restrict__ keys, u64 key_cap,
                                                         u32* __restrict__ q_words) {
  const u32 T = ctr->sort_n;
  const int lane = dev::lane_id();
  for (u64 base = (u64)blockIdx.x * 256; base < T; base += (u64)gridDim.x * 256) {
    const u64 jj = base + threadIdx.x;
    bool head = false;
    u64 s = 0;
    if (jj < T) {
      s = sorted[jj];
      head = jj == 0 || sorted[jj - 1] != s;
    }
    u64 key = ~0ull;
    u32 q = 0;
    bool ok = false;
    if (head) {
      // the run's end: the first word above s behind jj (the words are sorted)
      u32 lo = (u32)jj + 1, hi = T;
      while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] <= s)
          lo = mid + 1;
        else
          hi = mid;
      }
      const u64 count = (u64)lo - jj;
      q = (u32)(s >> 32);
      const u32 rank = (u32)s;
      ok = q < Q && rank < n && count <= cmask;
      if (ok) key = ((u64)q << 54) | ((cmask - count) << r) | (u64)rank;
    }
    const u64 hm = dev::ballot(head);
    if (hm == 0) continue;  // (wave-uniform)
    const int first = __ffsll((unsigned long long)hm) - 1;
    u32 slot0 = 0;
    if (lane == first) slot0 = atomicAdd(&ctr->runs, (u32)__popcll(hm));
    slot0 = (u32)__shfl((int)slot0, first, 64);
    const u64 slot = (u64)slot0 + dev::lanes_below(hm);
    if (head && slot < key_cap) keys[slot] = key;
    const u64 bm = dev::ballot(head && !ok);
    if (bm && lane == __ffsll((unsigned long long)bm) - 1)
      atomicAdd(&ctr->misplaced, (u32)__popcll(bm));
    // the queries' words: one atomic per distinct query of the wave's heads (sorted by query:
    // one or two, mostly)
    u64 left = dev::ballot(head && ok);
    while (left) {  // (wave-uniform)
      const int lead = __ffsll((unsigned long long)left) - 1;
      const u32 lq = (u32)__shfl((int)q, lead, 64);
      const u64 same = dev::ballot(head && ok && q == lq);
      if (lane == lead) atomicAdd(&q_words[lq], (u32)__popcll(same));
      left &= ~same;
    }
  }
}

// One workgroup: the queries' segments of the sorted rank keys, their words and tokens, and where
// their winners go.
__global__ __launch_bounds__(kOffBlock) void tally_offsets_kernel(
    const u64* __restrict__ skeys, u32 U, u32 Q, u32 K, const u64* __restrict__ offsets,
    const u64* __restrict__ tok_off, u64* __restrict__ run_off, u64* __restrict__ words,
    u64* __restrict__ tokens, u64* __restrict__ out_off) {
  __shared__ u64 s_run[kSearchMaxQueries + 1];
  __shared__ u64 s_scan[kOffBlock / 64 + 1];
  for (u32 q = threadIdx.x; q <= Q; q += kOffBlock) {
    u32 lo = 0, hi = U;
    if (q == Q) lo = U;  // (Q << 54 may not fit the key: the end is the end)
    const u64 want = (u64)q << 54;
    while (lo < hi) {  // lower bound
      const u32 mid = lo + ((hi - lo) >> 1);
      if (skeys[mid] < want)
        lo = mid + 1;
      else
        hi = mid;
    }
    s_run[q] = lo;
    run_off[q] = lo;
  }
  __syncthreads();
  u64 carry = 0;
  for (u32 base = 0; base < Q; base += kOffBlock) {  // (workgroup-uniform)
    const u32 q = base + threadIdx.x;
    u64 w = 0;
    if (q < Q) {
      w = s_run[q + 1] - s_run[q];
      words[q] = w;
      tokens[q] = tok_off[offsets[q + 1]] - tok_off[offsets[q]];
    }
    const u64 m = w < (u64)K ? w : (u64)K;
    u64 tot;
    const u64 ex = carry + dev::block_exclusive_scan<u64, kOffBlock>(m, s_scan, &tot);
    if (q < Q) out_off[q] = ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out_off[Q] = carry;
}

// One thread per sorted rank key: the first K of every query become records.
__global__ __launch_bounds__(256) void tally_top_kernel(
    const u64* __restrict__ skeys, u32 U, u32 r, u64 cmask, u32 Q, u32 K, u32 n,
    const OutRecord* __restrict__ recs, const u64* __restrict__ run_off,
    const u64* __restrict__ out_off, OutRecord* __restrict__ out, u64 out_cap,
    TallyCounters* __restrict__ ctr) {
  const u64 rmask = r ? (~0ull >> (64 - r)) : 0ull;
  u32 bad = 0;
  for (u64 jj = (u64)blockIdx.x * 256 + threadIdx.x; jj < U; jj += (u64)gridDim.x * 256) {
    const u64 key = skeys[jj];
    const u32 q = (u32)(key >> 54);
    const u64 rank = key & rmask;
    const u64 count = cmask - ((key >> r) & cmask);
    if (q >= Q || rank >= n || count == 0 || jj < run_off[q] || jj >= run_off[q + 1]) {
      ++bad;
      continue;
    }
    const u64 pos = jj - run_off[q];
    if (pos >= K) continue;
    const u64 o = out_off[q] + pos;
    if (o >= out_cap) {
      ++bad;
      continue;
    }
    OutRecord rec;
#pragma unroll
    for (int w = 0; w < kKeyWords; ++w) rec.w[w] = recs[rank].w[w];
    rec.count = count;
    out[o] = rec;
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->misplaced, bad);
  }
}

template <class Take>
void entry_layout(u64 entries, Take&& take) {
  take(sizeof(TallyCounters) + (u64)kSearchMaxQueries * 4);  // ctr | q_words: zeroed per batch
  take(entries * 4);                                         // n_tok
  take((entries + 1) * 8);                                   // tok_off
  take(((u64)kSearchMaxQueries + 1) * 8);                    // run_off
  take((u64)kSearchMaxQueries * 8);                          // words
  take((u64)kSearchMaxQueries * 8);                          // tokens
  take(((u64)kSearchMaxQueries + 1) * 8);                    // out_off
}

template <class Take>
void pair_layout(u64 pairs, u64 out, Take&& take) {
  take(pairs * 8);                                                // pairs
  take(pairs * 8);                                                // zeros
  take(pairs * 8);                                                // sorted
  take(pairs * 8);                                                // spare
  take(out * sizeof(OutRecord));                                  // out
  take(radix_zero_bytes(pairs));                                  // rx counters + status
  take((u64)radix_hist_blocks(pairs) * kNumPositions * 256 * 4);  // rx hist_part
  take(sizeof(SortPlan));                                         // rx plan
  take(pairs * 8);                                                // rx keys[0]
  take(pairs * 8);                                                // rx keys[1]
  take(pairs * 4);                                                // rx vals[0]
  take(pairs * 4);                                                // rx vals[1]
}

TallyJob make_job(const SearchIndex& ix, u32 queries, const u32* lines, const u64* offsets,
                  u64 entries, const TallyBuffers& tb, u32* blocks) {
  LOCUST_CHECK_ARG(ix.text && ix.nl_pos && ix.lctr && ix.recs && ix.n >= 1 &&
                       ix.emits_per_line > 0 && ix.max_key_len > 0 &&
                       ix.max_key_len <= kKeyBytes && ix.bytes >= 1,
                   "tally: the stage needs the index's text view and its records");
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && entries >= 1 &&
                       entries <= tb.cap_entries && entries < (1ull << 32),
                   "tally: " + std::to_string(entries) + " entries of " + std::to_string(queries) +
                       " queries exceed the workspace (" + std::to_string(tb.cap_entries) +
                       " entries)");
  TallyJob j{};
  j.text = ix.text;
  j.bytes = ix.bytes;
  j.nl_pos = ix.nl_pos;
  j.lctr = ix.lctr;
  j.dm = ix.dm;
  j.emits_per_line = ix.emits_per_line;
  j.max_key_len = ix.max_key_len;
  // one entry per wave while they are few, up to 64 per wave and round (as the show kernels)
  j.group = (u32)std::min<u64>(div_up(entries, (u64)kTallyMaxBlocks), 64);
  *blocks = (u32)std::min<u64>(div_up(div_up(entries, (u64)j.group), (u64)kTallyWaves),
                               (u64)kTallyMaxBlocks);
  j.Q = queries;
  j.first_line = ix.first_line;
  j.n = ix.n;
  j.recs = ix.recs;
  j.lines = lines;
  j.offsets = offsets;
  j.E = entries;
  j.ctr = tb.ctr;
  j.n_tok = tb.n_tok;
  j.tok_off = tb.tok_off;
  j.pairs = tb.pairs;
  j.pair_cap = tb.cap_pairs;
  return j;
}

// The sort of tb's one-word keys at `keys` into `sorted` (words 1..3: the zero buffer).
void sort_words(const u64* keys, const u32* d_n, u64 host_n, TallyBuffers& tb, u64* sorted,
                SortPlan* h_plan, hipStream_t s) {
  ConstKeysSoA in;
  KeysSoA out;
  in.w[0] = keys;
  out.w[0] = sorted;
  for (int j = 1; j < kKeyWords; ++j) {
    in.w[j] = tb.zeros;
    out.w[j] = tb.spare;  // the gather's copies of the zero words
  }
  radix_sort(in, d_n, host_n, tb.rx, nullptr, out, nullptr, nullptr, h_plan, s);
}

}  // namespace

u64 tally_entry_bytes(u64 entries) {
  u64 b = 0;
  entry_layout(entries, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void tally_entry_carve(char* base, u64 entries, TallyBuffers* tb) {
  char* part[7];
  int k = 0;
  u64 b = 0;
  entry_layout(entries, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  tb->zero = part[0];
  tb->zero_bytes = sizeof(TallyCounters) + (u64)kSearchMaxQueries * 4;
  tb->ctr = reinterpret_cast<TallyCounters*>(part[0]);
  tb->q_words = reinterpret_cast<u32*>(part[0] + sizeof(TallyCounters));
  tb->n_tok = reinterpret_cast<u32*>(part[1]);
  tb->tok_off = reinterpret_cast<u64*>(part[2]);
  tb->run_off = reinterpret_cast<u64*>(part[3]);
  tb->words = reinterpret_cast<u64*>(part[4]);
  tb->tokens = reinterpret_cast<u64*>(part[5]);
  tb->out_off = reinterpret_cast<u64*>(part[6]);
  tb->cap_entries = entries;
}

u64 tally_pair_bytes(u64 pairs, u64 out) {
  u64 b = 0;
  pair_layout(pairs, out, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void tally_pair_carve(char* base, u64 pairs, u64 out, TallyBuffers* tb) {
  char* part[12];
  int k = 0;
  u64 b = 0;
  pair_layout(pairs, out, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  tb->pairs = reinterpret_cast<u64*>(part[0]);
  tb->zeros = reinterpret_cast<u64*>(part[1]);
  tb->sorted = reinterpret_cast<u64*>(part[2]);
  tb->spare = reinterpret_cast<u64*>(part[3]);
  tb->out = reinterpret_cast<OutRecord*>(part[4]);
  tb->rx.tile_counters = reinterpret_cast<u32*>(part[5]);
  tb->rx.status = tb->rx.tile_counters + kNumPositions;
  tb->rx.hist_part = reinterpret_cast<u32*>(part[6]);
  tb->rx.plan = reinterpret_cast<SortPlan*>(part[7]);
  tb->rx.keys[0] = reinterpret_cast<u64*>(part[8]);
  tb->rx.keys[1] = reinterpret_cast<u64*>(part[9]);
  tb->rx.vals[0] = reinterpret_cast<u32*>(part[10]);
  tb->rx.vals[1] = reinterpret_cast<u32*>(part[11]);
  tb->rx.cap = pairs;
  tb->cap_pairs = pairs;
  tb->cap_out = out;
}

void launch_tally_measure(const SearchIndex& ix, const u32* lines, u64 entries,
                          const TallyBuffers& tb, hipStream_t s) {
  u32 blocks = 0;
  // (measure finds no query: one, and no offsets)
  const TallyJob j = make_job(ix, 1, lines, nullptr, entries, tb, &blocks);
  LOCUST_HIP_CHECK(hipMemsetAsync(tb.zero, 0, tb.zero_bytes, s));
  tally_measure_kernel<<<dim3(blocks), dim3(kTallyBlock), 0, s>>>(j);
  LOCUST_HIP_LAUNCH_CHECK();
  tally_scan_kernel<<<dim3(1), dim3(kScanBlock), 0, s>>>(tb.n_tok, entries, tb.tok_off, tb.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_tally_map(const SearchIndex& ix, u32 queries, const u32* lines, const u64* offsets,
                      u64 entries, u64 tokens, const TallyKeySplit& ks, TallyBuffers& tb,
                      SortPlan* h_plan, hipStream_t s) {
  u32 blocks = 0;
  const TallyJob j = make_job(ix, queries, lines, offsets, entries, tb, &blocks);
  LOCUST_CHECK_ARG(offsets && tb.pairs && tokens >= 1 && tokens <= tb.cap_pairs &&
                       tokens < (1ull << 32),
                   "tally: " + std::to_string(tokens) + " pair words exceed the workspace (" +
                       std::to_string(tb.cap_pairs) + ")");
  tally_map_kernel<<<dim3(blocks), dim3(kTallyBlock), 0, s>>>(j);
  LOCUST_HIP_LAUNCH_CHECK();
  tally_seal_kernel<<<dim3(1), dim3(1), 0, s>>>(tb.ctr, (u32)tokens);
  LOCUST_HIP_LAUNCH_CHECK();
  // order: the pair words ascending = (query, rank)
  sort_words(tb.pairs, &tb.ctr->sort_n, tokens, tb, tb.sorted, h_plan, s);
  // runs: the rank keys, into the words the pairs have left
  const u32 rblocks = (u32)std::min<u64>(div_up(tokens, 256), 4096);
  tally_runs_kernel<<<dim3(rblocks), dim3(256), 0, s>>>(tb.sorted, tb.ctr, ks.r, ks.cmask, queries,
                                                        ix.n, tb.pairs, tb.cap_pairs, tb.q_words);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_tally_top(const SearchIndex& ix, u32 queries, const u64* offsets, u64 runs, u32 k,
                      const TallyKeySplit& ks, TallyBuffers& tb, SortPlan* h_plan, hipStream_t s) {
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && offsets && runs >= 1 &&
                       runs <= tb.cap_pairs && runs < (1ull << 32) && k >= 1 && k <= kTopKMax,
                   "tally: " + std::to_string(runs) + " rank keys exceed the workspace (" +
                       std::to_string(tb.cap_pairs) + ")");
  // order: (query, count descending, rank ascending); the runs kernel wrote exactly `runs` keys
  sort_words(tb.pairs, &tb.ctr->runs, runs, tb, tb.sorted, h_plan, s);
  tally_offsets_kernel<<<dim3(1), dim3(kOffBlock), 0, s>>>(tb.sorted, (u32)runs, queries, k,
                                                           offsets, tb.tok_off, tb.run_off,
                                                           tb.words, tb.tokens, tb.out_off);
  LOCUST_HIP_LAUNCH_CHECK();
  const u32 blocks = (u32)std::min<u64>(div_up(runs, 256), 4096);
  tally_top_kernel<<<dim3(blocks), dim3(256), 0, s>>>(tb.sorted, (u32)runs, ks.r, ks.cmask,
                                                      queries, k, ix.n, ix.recs, tb.run_off,
                                                      tb.out_off, tb.out, tb.cap_out, tb.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_tally() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&tally_measure_kernel));
}

}  // namespace locust
