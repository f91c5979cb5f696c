// Dropping the oldest lines of the index in device memory (kernels.hpp "drop.hip"; the
// semantics are engine.hpp "dropping the oldest lines").
//
// A is the resident index over the lines [F, F + N) and cut_line = F + d.  Every postings list
// is non-decreasing in the line number, so what word w loses is a prefix of its list, k_w
// elements long; a word whose list empties leaves the dictionary.  Nothing is renumbered and
// nothing is sorted: the survivors compact by a scan, the CSR offsets are scanned anew, every
// kept posting moves once, and the text and the line starts lose a prefix.
//
// Shape (gfx950, wave64):
//  * cut: one thread per record, a lower bound of cut_line in the word's own list;
//  * scans: device/tile_scan.hpp's three kernels (shared with append.hip) over the survive
//    flags, then over the counts of C's records.  C's length is known on the device only
//    (DropCounters::nc), so the second scan takes it from there and its grid from the host's
//    bound nA;
//  * records: a survivor writes its record at its scanned position and leaves its source word
//    there (src_of);
//  * postings: the work is spread by tiles of kAppendTile DESTINATION elements, never by words.
//    Destination tiles were chosen over source tiles because the work is then proportional to
//    what survives -- a drop of nearly everything launches workgroups that leave after one
//    load -- and because every store of a tile is contiguous, whatever was cut between its
//    words; the loads are contiguous within a word's run, as in the merge.  The host knows only
//    the bound TA, which sizes the grid.  A tile's words are a contiguous range of C found by
//    two binary searches in valC; their offsets and their shifts to the source (val_w + k_w -
//    valC_p) are staged in LDS (at most one word per element: every kept count is >= 1), and
//    an element finds its word by a binary search there;
//  * lines and text: the cut byte B is read on the device by every thread that needs it (one
//    scalar load), so no stage waits for the host: nl_posC[k] = nl_posA[d + k] - B, and the
//    text is copied from B in 8-byte words funnelled from two aligned loads;
//  * stats: one wave per dropped line, device/linetok.hpp's step_starts as index.hip walks a
//    line, up to the token behind the emit cap.
// Data crosses between workgroups only at kernel boundaries; no output array is written with
// atomics, and every output word has one writer.  The counters (DropCounters) take one
// wave-reduced atomic per wave.
#include <algorithm>

#include "locust/device/linetok.hpp"
#include "locust/device/tile_scan.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr u64 kBadShift = 1ull << 63;  // a word whose source range is inconsistent

__device__ __forceinline__ bool rec_less(const OutRecord* a, const OutRecord* b) {
#pragma unroll
  for (int j = 0; j < kKeyWords; ++j)
    if (a->w[j] != b->w[j]) return a->w[j] < b->w[j];
  return false;
}

__device__ __forceinline__ void count_u32(u32* word, u32 v) {
  if (dev::ballot(v != 0)) {  // (wave-uniform)
    v = dev::wave_reduce_sum(v);
    if (dev::lane_id() == 0) atomicAdd(word, v);
  }
}

__device__ __forceinline__ void count_u64(u64* word, u64 v) {
  if (dev::ballot(v != 0)) {  // (wave-uniform)
    v = dev::wave_reduce_sum(v);
    if (dev::lane_id() == 0) atomicAdd((unsigned long long*)word, (unsigned long long)v);
  }
}

// The byte behind the newline of line d - 1: what the first d lines hold.  d - 1 == num_nl is
// the last, unterminated line: all of the bytes.
__device__ __forceinline__ u64 cut_byte(const u64* __restrict__ nl_pos, u64 num_nl, u64 d,
                                        u64 bytes) {
  if (d == 0) return 0;
  const u64 b = d - 1 < num_nl ? nl_pos[d - 1] + 1 : bytes;
  return b < bytes ? b : bytes;
}

// k[w] = the postings of word w below cut_line, keep[w] = some are left.
__global__ __launch_bounds__(kAppendBlock) void drop_cut_kernel(
    const u64* __restrict__ val, const u32* __restrict__ post, u32 n, u64 T, u32 cut_line,
    u32* __restrict__ k, u64* __restrict__ keep, DropCounters* __restrict__ ctr) {
  const u64 t = (u64)blockIdx.x * kAppendBlock + threadIdx.x;
  u64 gone = 0;
  u32 emptied = 0, bad = 0;
  if (t < n) {
    const u64 lo = val[t], hi = val[t + 1];
    u32 kw = 0;
    u64 left = 0;
    if (lo < hi && hi <= T) {  // (every count is >= 1)
      u64 a = lo, b = hi;      // the first posting >= cut_line
      while (a < b) {
        const u64 mid = a + ((b - a) >> 1);
        if (post[mid] < cut_line)
          a = mid + 1;
        else
          b = mid;
      }
      kw = (u32)(a - lo);
      left = hi - a;
      gone = a - lo;
      emptied = left == 0;
    } else {
      ++bad;  // val does not ascend
    }
    k[t] = kw;
    keep[t] = left ? 1 : 0;
  }
  count_u64(&ctr->dropped, gone);
  count_u32(&ctr->vanished, emptied);
  count_u32(&ctr->misplaced, bad);
}

// C's records: survivor w at pos[w] with what is left of its count; src_of[pos[w]] = w.
__global__ __launch_bounds__(kAppendBlock) void drop_records_kernel(
    const OutRecord* __restrict__ ra, const u64* __restrict__ val, u32 n,
    const u32* __restrict__ k, const u64* __restrict__ keep, const u64* __restrict__ pos,
    OutRecord* __restrict__ rc, u32* __restrict__ src_of, DropCounters* __restrict__ ctr) {
  const u64 nc = ctr->nc;
  const u64 t = (u64)blockIdx.x * kAppendBlock + threadIdx.x;
  u32 wrote = 0, bad = 0;
  if (t < n) {
    const OutRecord* r = ra + t;
    if (t && !rec_less(r - 1, r)) ++bad;  // A's keys ascend strictly
    if (keep[t]) {
      const u64 p = pos[t];
      if (p >= nc || p >= n) {
        ++bad;
      } else {
        OutRecord o = *r;
        o.count = val[t + 1] - val[t] - k[t];
        rc[p] = o;
        src_of[p] = (u32)t;
        wrote = 1;
      }
    }
  }
  count_u32(&ctr->records, wrote);
  count_u32(&ctr->misplaced, bad);
}

// The largest w in [0, n) with val[w] <= x (n >= 1, val[0] == 0).
__device__ __forceinline__ u32 word_of(const u64* __restrict__ val, u32 n, u64 x) {
  u32 lo = 0, hi = n - 1;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo + 1) >> 1);
    if (val[mid] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Every kept posting to its place in C, by tiles of C's elements: word p of C, source word
// w = src_of[p], takes [val_w + k_w, val_(w+1)) to [valC[p], valC[p + 1]).
__global__ __launch_bounds__(kAppendBlock) void drop_postings_kernel(
    const u64* __restrict__ val_a, const u32* __restrict__ post_a, u32 n, u64 T,
    const u32* __restrict__ k, const u32* __restrict__ src_of, const u64* __restrict__ val_c,
    u32* __restrict__ post_c, u64 post_cap, DropCounters* __restrict__ ctr) {
  __shared__ u64 s_val[kAppendTile + 1];
  __shared__ u64 s_shift[kAppendTile];
  const u32 nc = ctr->nc;
  if (nc == 0 || nc > n) return;  // (workgroup-uniform; nc > n: the records kernel counted it)
  const u64 tc = val_c[nc];
  if (tc > T || tc > post_cap) {  // C's counts exceed A's (workgroup-uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&ctr->misplaced, 1u);
    return;
  }
  const u64 base = (u64)blockIdx.x * kAppendTile;
  if (base >= tc) return;  // (workgroup-uniform)
  const u64 end = base + kAppendTile < tc ? base + kAppendTile : tc;
  // the words of C the tile's elements belong to
  const u32 w_lo = word_of(val_c, nc, base);
  const u32 w_hi = word_of(val_c, nc, end - 1);
  const u32 nw = w_hi - w_lo + 1;
  if (w_hi < w_lo || nw > (u32)kAppendTile) {  // valC does not ascend (workgroup-uniform)
    if (threadIdx.x == 0) atomicAdd(&ctr->misplaced, (u32)(end - base));
    return;
  }
  for (u32 j = threadIdx.x; j < nw; j += kAppendBlock) {
    const u32 p = w_lo + j;
    const u64 v = val_c[p], vnext = val_c[p + 1];
    const u32 w = src_of[p];
    u64 shift = kBadShift;
    if (w < n && vnext >= v) {
      const u64 s0 = val_a[w] + k[w], s1 = val_a[w + 1];
      if (s1 >= s0 && s1 <= T && s1 - s0 == vnext - v && s0 >= v) shift = s0 - v;
    }
    s_val[j] = v;
    s_shift[j] = shift;
    if (j == nw - 1) s_val[nw] = vnext;
  }
  __syncthreads();
  u32 moved = 0, bad = 0;
#pragma unroll
  for (int it = 0; it < kAppendItems; ++it) {
    const u64 e = base + (u64)it * kAppendBlock + threadIdx.x;
    if (e >= end) continue;
    u32 lo = 0, hi = nw - 1;  // the largest j with s_val[j] <= e
    while (lo < hi) {
      const u32 mid = lo + ((hi - lo + 1) >> 1);
      if (s_val[mid] <= e)
        lo = mid;
      else
        hi = mid - 1;
    }
    const u64 shift = s_shift[lo];
    const u64 src = e + shift;
    // inside the word's destination range, so inside its source run, which ends within A
    if (shift != kBadShift && s_val[lo] <= e && e < s_val[lo + 1] && src < T) {
      post_c[e] = post_a[src];
      ++moved;
    } else {
      ++bad;
    }
  }
  count_u32(&ctr->misplaced, bad);
  count_u64(&ctr->moved, (u64)moved);
}

// nl_posC[k] = nl_posA[d + k] - B; num_newlines = nlA - min(d, nlA); the cut byte to the
// counters.
__global__ __launch_bounds__(256) void drop_lines_kernel(
    const u64* __restrict__ nl_a, const MapCounters* __restrict__ lctr_a, u64 cap_a, u64 d,
    u64 bytes_a, u64* __restrict__ nl_c, u64 cap_c, MapCounters* __restrict__ lctr_c,
    DropCounters* __restrict__ ctr) {
  const u64 na = lctr_a->num_newlines < cap_a ? lctr_a->num_newlines : cap_a;
  const u64 B = cut_byte(nl_a, na, d, bytes_a);
  u64 nc = na - (d < na ? d : na);
  if (nc > cap_c) nc = cap_c;
  for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < nc; j += (u64)gridDim.x * 256)
    nl_c[j] = nl_a[d + j] - B;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    lctr_c->num_newlines = (u32)nc;
    ctr->cut_byte = B;
  }
}

// out[0 .. bytes_a - B + 16) = text[B .. bytes_a) and 16 zero bytes.  `text` and `out` are
// 8-byte aligned and text[bytes_a .. bytes_a + 16) is readable (zero, as everywhere): a word of
// the output is funnelled from the two aligned words of the source that hold it.
__global__ __launch_bounds__(256) void drop_text_kernel(
    const char* __restrict__ text, u64 bytes_a, const u64* __restrict__ nl_a,
    const MapCounters* __restrict__ lctr_a, u64 cap_a, u64 d, char* __restrict__ out,
    u64 out_cap) {
  const u64 na = lctr_a->num_newlines < cap_a ? lctr_a->num_newlines : cap_a;
  const u64 B = cut_byte(nl_a, na, d, bytes_a);
  const u64 left = bytes_a - B;
  const u64 total = left + 16 < out_cap ? left + 16 : out_cap;
  const u64* __restrict__ src = reinterpret_cast<const u64*>(text) + (B >> 3);
  const u32 sh = (u32)(B & 7) * 8;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i * 8 < total; i += (u64)gridDim.x * 256) {
    const u64 o = i * 8;
    u64 v = 0;
    if (o < left) {  // the source words end before bytes_a + 15
      v = src[i];
      if (sh) v = (v >> sh) | (src[i + 1] << (64 - sh));
      if (left - o < 8) v &= (1ull << (8 * (u32)(left - o))) - 1;
    }
    if (o + 8 <= total) {
      *reinterpret_cast<u64*>(out + o) = v;
    } else {
      for (u64 b = o; b < total; ++b) out[b] = (char)(v >> (8 * (b - o)));
    }
  }
}

// The word job's statistics of the dropped lines: a wave takes one line at a time, grid-stride,
// and walks it 64 bytes per step until the token behind the emit cap (one more than the index
// walk: that token makes the line an overflow line).  A token among the first emits_per_line
// is longer than max_key_len when the max_key_len + 1 bytes from its start all belong to it;
// they lie inside the staged row.
__global__ __launch_bounds__(kDropStatWaves * 64) void drop_stats_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, u64 nl_cap, u64 d, DelimMask dm, int emits_per_line,
    int max_key_len, DropCounters* __restrict__ ctr) {
  __shared__ unsigned char s_row[kDropStatWaves][dev::kLineRow];
  const int lane = dev::lane_id();
  unsigned char* row = s_row[dev::wave_id()];
  const u64 num_nl = lctr->num_newlines < nl_cap ? lctr->num_newlines : nl_cap;
  const u64 wave = (u64)blockIdx.x * kDropStatWaves + dev::wave_id();
  const u64 nwaves = (u64)gridDim.x * kDropStatWaves;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 E = (u32)emits_per_line;
  u32 over = 0, trunc = 0;
  for (u64 line = wave; line < d && line <= num_nl; line += nwaves) {
    const u64 start = line ? nl_pos[line - 1] + 1 : 0;
    u64 end = line < num_nl ? nl_pos[line] : bytes;
    if (end > bytes) end = bytes;
    u32 seen = 0;  // token starts of this line before the current step
    u64 carry = 0;
    for (u64 pos = start; pos < end && seen <= E; pos += 64) {
      const u64 p = pos + lane;
      const unsigned c = p < end ? (unsigned char)text[p] : 0u;
      const u64 p2 = pos + 64 + lane;
      const unsigned c2 = (lane < 32 && p2 < end) ? (unsigned char)text[p2] : 0u;
      __builtin_amdgcn_wave_barrier();  // the previous step's row reads are done
      row[lane] = (unsigned char)c;
      if (lane < 32) row[64 + lane] = (unsigned char)c2;
      __builtin_amdgcn_wave_barrier();
      bool last;
      const u64 starts = dev::step_starts(c, dm, &carry, &last);
      const u32 ord = seen + (u32)__popcll(starts & below);
      if (((starts >> lane) & 1ull) && ord < E) {
        bool longer = true;
        for (int len = 1; len <= max_key_len; ++len) {
          const unsigned ch = row[lane + len];
          if (ch == 0u || mask_is_delim(dm, ch)) {
            longer = false;
            break;
          }
        }
        trunc += longer ? 1u : 0u;
      }
      seen += (u32)__popcll(starts);
      if (last) break;  // a NUL, or the line end, inside this step
    }
    over += seen > E ? 1u : 0u;  // (wave-uniform)
  }
  count_u32(&ctr->truncated, trunc);
  if (lane == 0 && over) atomicAdd(&ctr->overflow_lines, over);
}

// The scratch's parts in order; `take` is called once per part with its byte size.
template <class Take>
void drop_layout(u64 rec_cap, Take&& take) {
  const u64 n = std::max<u64>(rec_cap, 1);
  take(sizeof(DropCounters));                         // ctr
  take(n * 4);                                        // k
  take(n * 8);                                        // keep
  take((n + 1) * 8);                                  // pos
  take(n * 4);                                        // src_of
  take((div_up(n, (u64)kIndexTile) + 1) * 8);         // tile_val
}

}  // namespace

u64 drop_scratch_bytes(u64 rec_cap) {
  u64 b = 0;
  drop_layout(rec_cap, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void drop_scratch_carve(char* base, u64 rec_cap, DropScratch* ws) {
  char* part[6];
  int j = 0;
  u64 b = 0;
  drop_layout(rec_cap, [&](u64 bytes) {
    b = align_up(b, 256);
    part[j++] = base + b;
    b += bytes;
  });
  ws->ctr = reinterpret_cast<DropCounters*>(part[0]);
  ws->k = reinterpret_cast<u32*>(part[1]);
  ws->keep = reinterpret_cast<u64*>(part[2]);
  ws->pos = reinterpret_cast<u64*>(part[3]);
  ws->src_of = reinterpret_cast<u32*>(part[4]);
  ws->tile_val = reinterpret_cast<u64*>(part[5]);
  ws->rec_cap = rec_cap;
}

void launch_drop(const AppendIndex& a, const AppendIndex& c, u32 cut_line, u64 d,
                 const DropRules& rules, DropScratch& ws, hipStream_t s) {
  const u64 n = a.n, T = a.tokens;
  LOCUST_CHECK_ARG(n <= ws.rec_cap, "drop: " + std::to_string(n) +
                                        " records exceed the drop's scratch (" +
                                        std::to_string(ws.rec_cap) + ")");
  LOCUST_CHECK_ARG(d >= 1 && d <= a.lines, "drop: " + std::to_string(d) + " lines of " +
                                               std::to_string(a.lines));
  LOCUST_CHECK_ARG(n < (1ull << 32) && T < (1ull << 32),
                   "index: " + std::to_string(n) + " words / " + std::to_string(T) +
                       " tokens do not fit the 32-bit halves of a pair word");
  LOCUST_CHECK_ARG(c.n >= n && c.tokens >= T && c.bytes >= a.bytes + 16 &&
                       c.lines >= a.lines - d,
                   "drop: the index that is left exceeds its destination");
  LOCUST_CHECK_ARG(rules.emits_per_line >= 1 && rules.max_key_len >= 1 &&
                       rules.max_key_len <= dev::kLineRow - 64,
                   "drop: token rules outside the line walk's row");
  LOCUST_HIP_CHECK(hipMemsetAsync(ws.ctr, 0, sizeof(DropCounters), s));
  LOCUST_HIP_CHECK(hipMemsetAsync(c.lctr, 0, sizeof(MapCounters), s));
  const u32 rec_blocks = (u32)div_up(n, (u64)kAppendBlock);
  const u32 tiles = (u32)div_up(std::max<u64>(n, 1), (u64)kIndexTile);
  // a. cut
  if (rec_blocks) {
    drop_cut_kernel<<<dim3(rec_blocks), dim3(kAppendBlock), 0, s>>>(a.val, a.postings, (u32)n, T,
                                                                   cut_line, ws.k, ws.keep, ws.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // b. pos = exclusive scan of keep; ctr->nc = pos[n]
  append_tile_sum_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(ws.keep, 1, (u32)n, nullptr,
                                                                  ws.tile_val);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_scan_kernel<<<dim3(1), dim3(kIndexBlock), 0, s>>>(ws.tile_val, tiles, ws.pos, (u32)n,
                                                               nullptr, &ws.ctr->nc);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_apply_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(ws.keep, 1, (u32)n, nullptr,
                                                                    ws.tile_val, ws.pos);
  LOCUST_HIP_LAUNCH_CHECK();
  // c. records
  if (rec_blocks) {
    drop_records_kernel<<<dim3(rec_blocks), dim3(kAppendBlock), 0, s>>>(
        a.recs, a.val, (u32)n, ws.k, ws.keep, ws.pos, c.recs, ws.src_of, ws.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // d. valC = exclusive scan of C's counts; nC = ctr->nc lives on the device
  const u64* counts = &c.recs->count;
  append_tile_sum_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(counts, kOutWords, 0u,
                                                                  &ws.ctr->nc, ws.tile_val);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_scan_kernel<<<dim3(1), dim3(kIndexBlock), 0, s>>>(ws.tile_val, tiles, c.val, 0u,
                                                               &ws.ctr->nc, nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_apply_kernel<<<dim3(tiles), dim3(kIndexBlock), 0, s>>>(
      counts, kOutWords, 0u, &ws.ctr->nc, ws.tile_val, c.val);
  LOCUST_HIP_LAUNCH_CHECK();
  // e. postings: the grid is the bound TA, the tiles are C's
  const u32 ptiles = (u32)div_up(T, (u64)kAppendTile);
  if (ptiles) {
    drop_postings_kernel<<<dim3(ptiles), dim3(kAppendBlock), 0, s>>>(
        a.val, a.postings, (u32)n, T, ws.k, ws.src_of, c.val, c.postings, c.tokens, ws.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // f. lines and text
  const u32 lblocks = (u32)std::min<u64>(div_up(std::max<u64>(a.lines - d, 1), 256), 2048);
  drop_lines_kernel<<<dim3(lblocks), dim3(256), 0, s>>>(a.nl_pos, a.lctr, a.lines, d, a.bytes,
                                                       c.nl_pos, c.lines, c.lctr, ws.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
  const u32 tblocks = (u32)std::min<u64>(div_up(a.bytes + 16, (u64)256 * 8), 4096);
  drop_text_kernel<<<dim3(tblocks), dim3(256), 0, s>>>(a.text, a.bytes, a.nl_pos, a.lctr, a.lines,
                                                      d, c.text, c.bytes);
  LOCUST_HIP_LAUNCH_CHECK();
  // g. the statistics of the dropped lines
  const u32 sblocks = (u32)std::min<u64>(div_up(d, (u64)kDropStatWaves), 4096);
  drop_stats_kernel<<<dim3(sblocks), dim3(kDropStatWaves * 64), 0, s>>>(
      a.text, a.bytes, a.nl_pos, a.lctr, a.lines, d, rules.dm, rules.emits_per_line,
      rules.max_key_len, ws.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_drop() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&drop_postings_kernel));
}

}  // namespace locust
