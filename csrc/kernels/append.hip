// Appending to the index: the merge of two indexes in device memory (kernels.hpp "append.hip";
// the semantics are engine.hpp "appending to the index").
//
// A is the resident index, B what launch_index left for a block whose lines are numbered behind
// all of A's: B's postings are global, and for every word the merged list is A's followed by
// B's.  So nothing is sorted here: the key-ordered records of the two sides merge by binary
// searches and a scan, and every posting moves once, to a place computed from the three CSR
// offset arrays.
//
// Shape (gfx950, wave64):
//  * locate: one thread per record, a lower bound among the other side's records (device/
//    rank.hpp's four-word compare);
//  * scans: index.hip's three-kernel shape (tile sums, a one-workgroup scan of the tile array, a
//    workgroup scan inside each tile; device/tile_scan.hpp, shared with drop.hip) over a
//    strided u64 source: the fresh flags, then the counts of C's records.  C's length is known
//    on the device only (nA + fresh), so the second scan takes it from the counters and its
//    grid from the host's bound nA + nB;
//  * records: position = own index + the other side's records below; the A thread coalesces;
//  * postings: the work is spread by tiles of kAppendTile SOURCE elements, never by words: a
//    word with thousands of postings is moved by several workgroups, a thousand words with one
//    posting each by one.  A tile's words are a contiguous range found by two binary searches
//    in the source val; their offsets and destination shifts are staged in LDS (at most one
//    word per element: every count is >= 1), and an element finds its word by a binary search
//    there -- no step at all for a tile inside one long list.  Loads and stores are coalesced
//    within a word's run;
//  * lines: nl_posC = nl_posA ++ (nl_posB + bytesA).
// Data crosses between workgroups only at kernel boundaries; no output array is written with
// atomics, and every output word has one writer.  The counters (AppendCounters) take one
// wave-reduced atomic per wave.
#include <algorithm>

#include "locust/device/rank.hpp"
#include "locust/device/tile_scan.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr u32 kNoPos = 0xffffffffu;      // a record whose position fell outside C
constexpr u64 kBadShift = 1ull << 63;    // a word whose destination range is inconsistent

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

// b_pos[j] = the lower bound of B[j] among A's records, fresh[j] = its key is absent there;
// a_pos[i] = the lower bound of A[i] among B's records.
__global__ __launch_bounds__(kAppendBlock) void append_locate_kernel(
    const OutRecord* __restrict__ ra, u32 na, const OutRecord* __restrict__ rb, u32 nb,
    u32* __restrict__ a_pos, u32* __restrict__ b_pos, u64* __restrict__ fresh) {
  const u64 t = (u64)blockIdx.x * kAppendBlock + threadIdx.x;
  bool eq;
  if (t < nb) {
    const OutRecord* r = rb + t;
    b_pos[t] = dev::lower_rank(ra, na, r->w[0], r->w[1], r->w[2], r->w[3], &eq);
    fresh[t] = eq ? 0 : 1;
  } else if (t - nb < na) {
    const u64 i = t - nb;
    const OutRecord* r = ra + i;
    a_pos[i] = dev::lower_rank(rb, nb, r->w[0], r->w[1], r->w[2], r->w[3], &eq);
  }
}

// C's records, and every source record's position in C (a_pos, b_pos: in place of the lower
// bounds).  The A thread writes the coalesced record, a B thread only a fresh key: one writer
// per record.
__global__ __launch_bounds__(kAppendBlock) void append_records_kernel(
    const OutRecord* __restrict__ ra, u32 na, const OutRecord* __restrict__ rb, u32 nb,
    const u64* __restrict__ sb, u32* __restrict__ a_pos, u32* __restrict__ b_pos,
    OutRecord* __restrict__ rc, AppendCounters* __restrict__ ctr) {
  const u64 nc = (u64)na + ctr->fresh;
  const u64 t = (u64)blockIdx.x * kAppendBlock + threadIdx.x;
  u32 wrote = 0, bad = 0;
  if (t < nb) {
    const OutRecord* r = rb + t;
    const u64 s = sb[t];
    const bool is_fresh = sb[t + 1] != s;
    const u64 p = (u64)b_pos[t] + s;
    if (t && !rec_less(r - 1, r)) ++bad;  // B's keys ascend strictly
    if (p >= nc) {
      ++bad;
      b_pos[t] = kNoPos;
    } else {
      b_pos[t] = (u32)p;
      if (is_fresh) {
        rc[p] = *r;
        wrote = 1;
      }
    }
  } else if (t - nb < na) {
    const u64 i = t - nb;
    const OutRecord* r = ra + i;
    const u32 lb = a_pos[i];  // <= nb
    const u64 p = i + sb[lb];
    if (i && !rec_less(r - 1, r)) ++bad;  // A's keys ascend strictly
    if (p >= nc) {
      ++bad;
      a_pos[i] = kNoPos;
    } else {
      OutRecord o = *r;
      if (lb < nb) {
        const OutRecord* q = rb + lb;
        if (!rec_less(r, q) && !rec_less(q, r)) o.count += q->count;
      }
      a_pos[i] = (u32)p;
      rc[p] = o;
      wrote = 1;
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

// Every posting to its place in C: workgroups [0, tiles_a) take A's tiles, the rest B's.
// Word w of A at position p of C goes to [valC[p], valC[p] + countA), word w of B to
// [valC[p + 1] - countB, valC[p + 1]).
__global__ __launch_bounds__(kAppendBlock) void append_postings_kernel(
    const u64* __restrict__ val_a, const u32* __restrict__ post_a, u32 na, u64 ta,
    const u32* __restrict__ a_pos, const u64* __restrict__ val_b,
    const u32* __restrict__ post_b, u32 nb, u64 tb, const u32* __restrict__ b_pos, u32 tiles_a,
    const u64* __restrict__ val_c, u32* __restrict__ post_c, AppendCounters* __restrict__ ctr) {
  __shared__ u64 s_val[kAppendTile + 1];
  __shared__ u64 s_shift[kAppendTile];
  const bool side_b = blockIdx.x >= tiles_a;
  const u64* __restrict__ val = side_b ? val_b : val_a;
  const u32* __restrict__ post = side_b ? post_b : post_a;
  const u32* __restrict__ pos = side_b ? b_pos : a_pos;
  const u32 n = side_b ? nb : na;
  const u64 T = side_b ? tb : ta;
  const u64 nc = (u64)na + ctr->fresh;
  const u64 tc = ta + tb;
  const u64 base = (u64)(blockIdx.x - (side_b ? tiles_a : 0u)) * kAppendTile;
  if (n == 0 || base >= T) return;  // (workgroup-uniform)
  const u64 end = base + kAppendTile < T ? base + kAppendTile : T;
  // the words the tile's elements belong to
  const u32 w_lo = word_of(val, n, base);
  const u32 w_hi = word_of(val, n, end - 1);
  const u32 nw = w_hi - w_lo + 1;
  if (w_hi < w_lo || nw > (u32)kAppendTile) {  // val does not ascend (workgroup-uniform)
    if (threadIdx.x == 0) atomicAdd(&ctr->misplaced, (u32)(end - base));
    return;
  }
  for (u32 k = threadIdx.x; k < nw; k += kAppendBlock) {
    const u32 w = w_lo + k;
    const u64 v = val[w], vnext = val[w + 1];
    const u32 p = pos[w];
    u64 shift = kBadShift;
    if (p < nc && vnext >= v) {
      const u64 lo = val_c[p], hi = val_c[p + 1], len = vnext - v;
      if (hi >= lo && hi <= tc && len <= hi - lo) shift = (side_b ? hi - len : lo) - v;
    }
    s_val[k] = v;
    s_shift[k] = shift;
    if (k == nw - 1) s_val[nw] = vnext;
  }
  __syncthreads();
  u32 moved = 0, bad = 0;
#pragma unroll
  for (int it = 0; it < kAppendItems; ++it) {
    const u64 e = base + (u64)it * kAppendBlock + threadIdx.x;
    if (e >= end) continue;
    u32 lo = 0, hi = nw - 1;  // the largest k with s_val[k] <= e
    while (lo < hi) {
      const u32 mid = lo + ((hi - lo + 1) >> 1);
      if (s_val[mid] <= e)
        lo = mid;
      else
        hi = mid - 1;
    }
    const u64 shift = s_shift[lo];
    const u64 d = e + shift;
    // inside the word's source run, so inside its destination range, which ends within C
    if (shift != kBadShift && s_val[lo] <= e && e < s_val[lo + 1] && d < tc) {
      post_c[d] = post[e];
      ++moved;
    } else {
      ++bad;
    }
  }
  count_u32(&ctr->misplaced, bad);
  if (dev::ballot(moved != 0)) {
    const u64 m = dev::wave_reduce_sum((u64)moved);
    if (dev::lane_id() == 0) atomicAdd((unsigned long long*)&ctr->moved, (unsigned long long)m);
  }
}

// nl_posC = nl_posA ++ (nl_posB + bytes_a); num_newlines = nlA + nlB.
__global__ __launch_bounds__(256) void append_lines_kernel(
    const u64* __restrict__ nl_a, const MapCounters* __restrict__ lctr_a, u64 cap_a,
    const u64* __restrict__ nl_b, const MapCounters* __restrict__ lctr_b, u64 cap_b, u64 bytes_a,
    u64* __restrict__ nl_c, u64 cap_c, MapCounters* __restrict__ lctr_c) {
  const u64 na = lctr_a->num_newlines < cap_a ? lctr_a->num_newlines : cap_a;
  u64 nb = lctr_b->num_newlines < cap_b ? lctr_b->num_newlines : cap_b;
  if (na + nb > cap_c) nb = cap_c > na ? cap_c - na : 0;
  const u64 nc = na + nb < cap_c ? na + nb : cap_c;
  for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < nc; k += (u64)gridDim.x * 256)
    nl_c[k] = k < na ? nl_a[k] : nl_b[k - na] + bytes_a;
  if (blockIdx.x == 0 && threadIdx.x == 0) lctr_c->num_newlines = (u32)nc;
}

// The scratch's parts in order; `take` is called once per part with its byte size.
template <class Take>
void append_layout(u64 rec_cap_a, u64 rec_cap_b, Take&& take) {
  take(sizeof(AppendCounters));                                                // ctr
  take(std::max<u64>(rec_cap_a, 1) * 4);                                       // a_pos
  take(std::max<u64>(rec_cap_b, 1) * 4);                                       // b_pos
  take(std::max<u64>(rec_cap_b, 1) * 8);                                       // fresh
  take((rec_cap_b + 1) * 8);                                                   // sb
  take((div_up(std::max<u64>(rec_cap_a + rec_cap_b, 1), (u64)kIndexTile) + 1) * 8);  // tile_val
}

}  // namespace

u64 append_scratch_bytes(u64 rec_cap_a, u64 rec_cap_b) {
  u64 b = 0;
  append_layout(rec_cap_a, rec_cap_b, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void append_scratch_carve(char* base, u64 rec_cap_a, u64 rec_cap_b, AppendScratch* ws) {
  char* part[6];
  int k = 0;
  u64 b = 0;
  append_layout(rec_cap_a, rec_cap_b, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  ws->ctr = reinterpret_cast<AppendCounters*>(part[0]);
  ws->a_pos = reinterpret_cast<u32*>(part[1]);
  ws->b_pos = reinterpret_cast<u32*>(part[2]);
  ws->fresh = reinterpret_cast<u64*>(part[3]);
  ws->sb = reinterpret_cast<u64*>(part[4]);
  ws->tile_val = reinterpret_cast<u64*>(part[5]);
  ws->rec_cap_a = rec_cap_a;
  ws->rec_cap_b = rec_cap_b;
}

void launch_append(const AppendIndex& a, const AppendIndex& b, const AppendIndex& c,
                   AppendScratch& ws, hipStream_t s) {
  const u64 na = a.n, nb = b.n, ta = a.tokens, tb = b.tokens;
  LOCUST_CHECK_ARG(na <= ws.rec_cap_a && nb <= ws.rec_cap_b,
                   "append: " + std::to_string(na) + " + " + std::to_string(nb) +
                       " records exceed the merge's scratch (" + std::to_string(ws.rec_cap_a) +
                       " + " + std::to_string(ws.rec_cap_b) + ")");
  LOCUST_CHECK_ARG(na + nb < (1ull << 32) && ta + tb < (1ull << 32),
                   "index: " + std::to_string(na + nb) + " words / " + std::to_string(ta + tb) +
                       " tokens do not fit the 32-bit halves of a pair word");
  LOCUST_CHECK_ARG(c.n >= na + nb && c.tokens >= ta + tb && c.bytes >= a.bytes + b.bytes + 16 &&
                       c.lines >= a.lines + b.lines,
                   "append: the merged index exceeds its destination");
  LOCUST_HIP_CHECK(hipMemsetAsync(ws.ctr, 0, sizeof(AppendCounters), s));
  LOCUST_HIP_CHECK(hipMemsetAsync(c.lctr, 0, sizeof(MapCounters), s));
  const u32 rec_blocks = (u32)div_up(na + nb, (u64)kAppendBlock);
  // a. locate
  if (rec_blocks) {
    append_locate_kernel<<<dim3(rec_blocks), dim3(kAppendBlock), 0, s>>>(
        a.recs, (u32)na, b.recs, (u32)nb, ws.a_pos, ws.b_pos, ws.fresh);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // b. sB = exclusive scan of fresh; ctr->fresh = sB[nB]
  const u32 tiles_b = (u32)div_up(std::max<u64>(nb, 1), (u64)kIndexTile);
  append_tile_sum_kernel<<<dim3(tiles_b), dim3(kIndexBlock), 0, s>>>(ws.fresh, 1, (u32)nb, nullptr,
                                                                    ws.tile_val);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_scan_kernel<<<dim3(1), dim3(kIndexBlock), 0, s>>>(ws.tile_val, tiles_b, ws.sb, (u32)nb,
                                                               nullptr, &ws.ctr->fresh);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_apply_kernel<<<dim3(tiles_b), dim3(kIndexBlock), 0, s>>>(ws.fresh, 1, (u32)nb, nullptr,
                                                                      ws.tile_val, ws.sb);
  LOCUST_HIP_LAUNCH_CHECK();
  // c. records
  if (rec_blocks) {
    append_records_kernel<<<dim3(rec_blocks), dim3(kAppendBlock), 0, s>>>(
        a.recs, (u32)na, b.recs, (u32)nb, ws.sb, ws.a_pos, ws.b_pos, c.recs, ws.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // d. valC = exclusive scan of C's counts; nC = nA + ctr->fresh lives on the device
  const u32 tiles_c = (u32)div_up(std::max<u64>(na + nb, 1), (u64)kIndexTile);
  const u64* counts = &c.recs->count;
  append_tile_sum_kernel<<<dim3(tiles_c), dim3(kIndexBlock), 0, s>>>(counts, kOutWords, (u32)na,
                                                                    &ws.ctr->fresh, ws.tile_val);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_scan_kernel<<<dim3(1), dim3(kIndexBlock), 0, s>>>(ws.tile_val, tiles_c, c.val, (u32)na,
                                                               &ws.ctr->fresh, nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  append_tile_apply_kernel<<<dim3(tiles_c), dim3(kIndexBlock), 0, s>>>(
      counts, kOutWords, (u32)na, &ws.ctr->fresh, ws.tile_val, c.val);
  LOCUST_HIP_LAUNCH_CHECK();
  // e. postings
  const u32 tiles_a = (u32)div_up(ta, (u64)kAppendTile);
  const u32 tiles_pb = (u32)div_up(tb, (u64)kAppendTile);
  if (tiles_a + tiles_pb) {
    append_postings_kernel<<<dim3(tiles_a + tiles_pb), dim3(kAppendBlock), 0, s>>>(
        a.val, a.postings, (u32)na, ta, ws.a_pos, b.val, b.postings, (u32)nb, tb, ws.b_pos, tiles_a,
        c.val, c.postings, ws.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  // f. lines and text
  const u32 lblocks = (u32)std::min<u64>(div_up(std::max<u64>(a.lines + b.lines, 1), 256), 2048);
  append_lines_kernel<<<dim3(lblocks), dim3(256), 0, s>>>(a.nl_pos, a.lctr, a.lines, b.nl_pos,
                                                         b.lctr, b.lines, a.bytes, c.nl_pos,
                                                         c.lines, c.lctr);
  LOCUST_HIP_LAUNCH_CHECK();
  if (a.bytes)
    LOCUST_HIP_CHECK(hipMemcpyAsync(c.text, a.text, a.bytes, hipMemcpyDeviceToDevice, s));
  if (b.bytes)
    LOCUST_HIP_CHECK(
        hipMemcpyAsync(c.text + a.bytes, b.text, b.bytes, hipMemcpyDeviceToDevice, s));
  LOCUST_HIP_CHECK(hipMemsetAsync(c.text + a.bytes + b.bytes, 0, 16, s));
}

void warm_module_append() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&append_postings_kernel));
}

}  // namespace locust
