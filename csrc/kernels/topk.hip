// Top-K by count: exact device-side selection over the key-ordered output records
// (kernels.hpp "topk.hip"; the semantics are engine.hpp "top-K words by count").
//
// The job's full output already sits in device memory as 40-B {key, count} records in key
// order.  Ranking it on the host means shipping every record across PCIe and a partial
// sort there; here a radix select finds the k-th largest count T, and only the records
// above it (plus the first `quota` records equal to it, in key order) are gathered,
// ordered in one workgroup's LDS and written out -- at most kTopKMax 48-B records travel.
//
// Shape (gfx950, wave64):
//  * the counts are read once from the 40-B stride into a dense u64 array; every later
//    pass streams that array (8 B per record, coalesced);
//  * the select runs most significant byte first, one kernel per byte.  A kernel's
//    workgroups each re-derive the digits chosen so far from the earlier passes' finished
//    histograms (a 256-bin suffix scan per pass, all in LDS), so the threshold prefix and
//    the remaining quota never leave the device and no workgroup ever waits for another:
//    data crosses workgroups only at kernel boundaries.  Bytes above the largest count's
//    top byte are skipped (their kernels exit on one load);
//  * histograms are built in LDS, a wave whose matching lanes all hold one digit (the
//    common case: most words occur once) adds its ballot's popcount with one LDS atomic,
//    and a workgroup issues one global atomic per non-empty bin;
//  * val is the exact u64 exclusive prefix of the counts: per-tile sums, a one-workgroup
//    scan of the tile array between passes, a workgroup scan inside the tile.
// The launch function zeroes the accumulated words (largest count, histograms) on every
// call; everything else is fully rewritten before it is read.
#include <algorithm>

#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kFinalBlock = 1024;
constexpr u32 kPadSlot = 0xFFFFFFFFu;

__device__ __forceinline__ int top_byte(u64 m) { return m ? (63 - __clzll(m)) >> 3 : 0; }

__device__ __forceinline__ const u32* sel_hist(const u64* sel) {
  return reinterpret_cast<const u32*>(sel + 1);
}

// The select's state after the passes for bytes tb .. b_stop + 1: the chosen digits (at
// their byte positions) and how many of the k are still to be found among the counts that
// match them.  Derived by every workgroup on its own from the finished histograms.
// b_stop = -1: the whole threshold T and the quota of records equal to it.
struct Sel {
  u64 prefix;
  u32 kk;
};
template <int kBlock>
__device__ __forceinline__ Sel resolve_digits(const u64* __restrict__ sel, u32 k_eff, int b_stop,
                                              u32* s_scan, u32* s_pick) {
  const u32* hist = sel_hist(sel);
  const int tb = top_byte(sel[0]);
  const u32 t = threadIdx.x;
  if (t == 0) {
    s_pick[0] = 0;
    s_pick[1] = 1;
  }
  Sel r;
  r.prefix = 0;
  r.kk = k_eff;
  for (int q = tb; q > b_stop; --q) {
    // thread t holds digit 255 - t: the exclusive scan counts the larger digits
    const u32 h = t < 256 ? hist[q * 256 + (255 - t)] : 0u;
    u32 total;
    const u32 above = dev::block_exclusive_scan<u32, kBlock>(h, s_scan, &total);
    if (t < 256 && above < r.kk && r.kk <= above + h) {
      s_pick[0] = 255 - t;
      s_pick[1] = r.kk - above;
    }
    __syncthreads();
    r.prefix |= (u64)s_pick[0] << (8 * q);
    r.kk = s_pick[1];
  }
  return r;
}

// counts[i] = recs[i].count; tile_val[tile] = the tile's count sum; sel[0] = max count.
__global__ __launch_bounds__(kTopKBlock) void topk_extract_kernel(
    const OutRecord* __restrict__ recs, u32 n, u64* __restrict__ counts,
    u64* __restrict__ tile_val, u64* __restrict__ sel) {
  __shared__ u64 s_sum[kTopKBlock / 64], s_max[kTopKBlock / 64];
  const u64 base = (u64)blockIdx.x * kTopKTile;
  u64 sum = 0, mx = 0;
#pragma unroll
  for (int j = 0; j < kTopKItems; ++j) {
    const u64 i = base + (u64)j * kTopKBlock + threadIdx.x;
    if (i < n) {
      const u64 c = recs[i].count;
      counts[i] = c;
      sum += c;
      mx = c > mx ? c : mx;
    }
  }
  sum = dev::wave_reduce_sum(sum);
  mx = dev::wave_reduce_max(mx);
  if (dev::lane_id() == 0) {
    s_sum[dev::wave_id()] = sum;
    s_max[dev::wave_id()] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 ts = 0, tm = 0;
#pragma unroll
    for (int w = 0; w < kTopKBlock / 64; ++w) {
      ts += s_sum[w];
      tm = s_max[w] > tm ? s_max[w] : tm;
    }
    tile_val[blockIdx.x] = ts;
    if (tm) atomicMax(reinterpret_cast<unsigned long long*>(sel), (unsigned long long)tm);
  }
}

// Histogram of byte b over the counts matching the digits chosen for the bytes above it.
__global__ __launch_bounds__(kTopKBlock) void topk_digit_kernel(const u64* __restrict__ counts,
                                                                u32 n, u32 k_eff, int b,
                                                                u64* __restrict__ sel) {
  __shared__ u32 s_hist[256];
  __shared__ u32 s_scan[kTopKBlock / 64 + 1];
  __shared__ u32 s_pick[2];
  if (b > top_byte(sel[0])) return;  // every count is zero up here (workgroup-uniform)
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const Sel r = resolve_digits<kTopKBlock>(sel, k_eff, b, s_scan, s_pick);
  const int sh = 8 * (b + 1);
  const u64 want = sh < 64 ? r.prefix >> sh : 0;
  const u64 base = (u64)blockIdx.x * kTopKTile;
  const int lane = dev::lane_id();
#pragma unroll
  for (int j = 0; j < kTopKItems; ++j) {
    const u64 i = base + (u64)j * kTopKBlock + threadIdx.x;
    const u64 c = i < n ? counts[i] : 0;
    const bool m = i < n && (sh < 64 ? c >> sh : 0) == want;
    const u32 d = (u32)(c >> (8 * b)) & 255u;
    const u64 mm = dev::ballot(m);
    if (mm) {  // wave-uniform
      const int first = __ffsll((unsigned long long)mm) - 1;
      const u32 d0 = (u32)__shfl((int)d, first, 64);
      const u64 same = dev::ballot(m && d == d0);
      if (same == mm) {
        if (lane == first) atomicAdd(&s_hist[d0], (u32)__popcll(mm));
      } else if (m) {
        atomicAdd(&s_hist[d], 1u);
      }
    }
  }
  __syncthreads();
  const u32 h = s_hist[threadIdx.x];
  if (h) atomicAdd(reinterpret_cast<u32*>(sel + 1) + b * 256 + threadIdx.x, h);
}

// tile_ge[tile] = (#records above T) << 32 | #records equal to T.
__global__ __launch_bounds__(kTopKBlock) void topk_tile_count_kernel(
    const u64* __restrict__ counts, u32 n, u32 k_eff, const u64* __restrict__ sel,
    u64* __restrict__ tile_ge) {
  __shared__ u32 s_scan[kTopKBlock / 64 + 1];
  __shared__ u32 s_pick[2];
  __shared__ u64 s_ge[kTopKBlock / 64];
  const u64 T = resolve_digits<kTopKBlock>(sel, k_eff, -1, s_scan, s_pick).prefix;
  const u64 base = (u64)blockIdx.x * kTopKTile;
  u64 ge = 0;
#pragma unroll
  for (int j = 0; j < kTopKItems; ++j) {
    const u64 i = base + (u64)j * kTopKBlock + threadIdx.x;
    if (i < n) {
      const u64 c = counts[i];
      ge += c > T ? 1ull << 32 : (c == T ? 1ull : 0ull);
    }
  }
  ge = dev::wave_reduce_sum(ge);
  if (dev::lane_id() == 0) s_ge[dev::wave_id()] = ge;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < kTopKBlock / 64; ++w) t += s_ge[w];
    tile_ge[blockIdx.x] = t;
  }
}

// One workgroup: exclusive scans of the tile arrays, in place.  (Both halves of tile_ge
// stay below 2^32 -- n does -- so the packed sum never carries between them.)
__global__ __launch_bounds__(kTopKBlock) void topk_scan_kernel(u64* __restrict__ tile_val,
                                                               u64* __restrict__ tile_ge,
                                                               u32 tiles) {
  __shared__ u64 s_scan[kTopKBlock / 64 + 1];
  u64 carry_v = 0, carry_g = 0;
  for (u32 base = 0; base < tiles; base += kTopKBlock) {
    const u32 i = base + threadIdx.x;
    const u64 v = i < tiles ? tile_val[i] : 0;
    const u64 g = i < tiles ? tile_ge[i] : 0;
    u64 tv, tg;
    const u64 ev = dev::block_exclusive_scan<u64, kTopKBlock>(v, s_scan, &tv);
    const u64 eg = dev::block_exclusive_scan<u64, kTopKBlock>(g, s_scan, &tg);
    if (i < tiles) {
      tile_val[i] = carry_v + ev;
      tile_ge[i] = carry_g + eg;
    }
    carry_v += tv;
    carry_g += tg;
  }
}

// The winners into their candidate slots: the records above T take slots [0, #gt) in key
// order, the first `quota` records equal to T the slots behind them.
__global__ __launch_bounds__(kTopKBlock) void topk_scatter_kernel(
    const u64* __restrict__ counts, u32 n, u32 k_eff, const u64* __restrict__ sel,
    const u64* __restrict__ tile_val, const u64* __restrict__ tile_ge,
    u64* __restrict__ cand_count, u32* __restrict__ cand_idx, u64* __restrict__ cand_val) {
  __shared__ u32 s_scan[kTopKBlock / 64 + 1];
  __shared__ u32 s_pick[2];
  __shared__ u64 s_scan64[kTopKBlock / 64 + 1];
  const Sel r = resolve_digits<kTopKBlock>(sel, k_eff, -1, s_scan, s_pick);
  const u64 T = r.prefix;
  const u32 quota = r.kk;
  const u32 gt_total = k_eff - quota;
  // blocked: a thread's items are neighbours in key order
  const u64 first = (u64)blockIdx.x * kTopKTile + (u64)threadIdx.x * kTopKItems;
  u64 c[kTopKItems];
  u64 sum = 0, ge = 0;
#pragma unroll
  for (int t = 0; t < kTopKItems; ++t) {
    c[t] = first + t < n ? counts[first + t] : 0;
    sum += c[t];
    if (first + t < n) ge += c[t] > T ? 1ull << 32 : (c[t] == T ? 1ull : 0ull);
  }
  u64 tot;
  u64 val = dev::block_exclusive_scan<u64, kTopKBlock>(sum, s_scan64, &tot);
  u64 at = dev::block_exclusive_scan<u64, kTopKBlock>(ge, s_scan64, &tot);
  if (ge == 0) return;  // (after the scans' barriers)
  val += tile_val[blockIdx.x];
  at += tile_ge[blockIdx.x];
  u32 g = (u32)(at >> 32), e = (u32)at;
#pragma unroll
  for (int t = 0; t < kTopKItems; ++t) {
    if (first + t < n) {
      u32 slot = kPadSlot;
      if (c[t] > T) {
        slot = g++;
      } else if (c[t] == T) {
        if (e < quota) slot = gt_total + e;
        ++e;
      }
      if (slot < kTopKMax) {
        cand_count[slot] = c[t];
        cand_idx[slot] = (u32)(first + t);
        cand_val[slot] = val;
      }
    }
    val += c[t];
  }
}

// One workgroup: bitonic sort of the m candidates (padded to P, a power of two) by (count
// descending, slot ascending) in LDS, then the TopRecords.  Slot order is index order
// wherever counts tie: ties happen only inside the group above T or inside the group
// equal to it, and both were filled in key order.
__global__ __launch_bounds__(kFinalBlock) void topk_final_kernel(
    const OutRecord* __restrict__ recs, u32 n, u32 m, u32 P, const u64* __restrict__ cand_count,
    const u32* __restrict__ cand_idx, const u64* __restrict__ cand_val,
    TopRecord* __restrict__ out, u32* __restrict__ out_n) {
  __shared__ u64 s_c[kTopKMax];
  __shared__ u32 s_s[kTopKMax];
  for (u32 i = threadIdx.x; i < P; i += kFinalBlock) {
    s_c[i] = i < m ? cand_count[i] : 0;
    s_s[i] = i < m ? i : kPadSlot;
  }
  __syncthreads();
  for (u32 size = 2; size <= P; size <<= 1) {
    for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
      for (u32 t = threadIdx.x; t < P / 2; t += kFinalBlock) {
        const u32 lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const u64 ca = s_c[lo], cb = s_c[hi];
        const u32 sa = s_s[lo], sb = s_s[hi];
        const bool b_first = cb > ca || (cb == ca && sb < sa);
        if (b_first == up) {
          s_c[lo] = cb;
          s_c[hi] = ca;
          s_s[lo] = sb;
          s_s[hi] = sa;
        }
      }
      __syncthreads();
    }
  }
  for (u32 j = threadIdx.x; j < m; j += kFinalBlock) {
    const u32 slot = s_s[j];
    if (slot >= m) continue;  // (never: the pads sort behind every candidate)
    const u32 idx = cand_idx[slot];
    if (idx >= n) continue;  // (never: every slot below m was filled from a record)
    const OutRecord src = recs[idx];
    TopRecord r;
#pragma unroll
    for (int q = 0; q < kKeyWords; ++q) r.w[q] = src.w[q];
    r.count = s_c[j];
    r.val = cand_val[slot];
    out[j] = r;
  }
  if (threadIdx.x == 0) *out_n = m;
}

}  // namespace

u64 topk_workspace_bytes(u64 cap) {
  const u64 tiles = div_up(std::max<u64>(cap, 1), kTopKTile);
  u64 b = 0;
  for (u64 part : {cap * 8, tiles * 8, tiles * 8, kTopKSelWords * 8, (u64)kTopKMax * 8,
                   (u64)kTopKMax * 8, (u64)kTopKMax * 4})
    b = align_up(b, 256) + part;
  return align_up(b, 256);
}

void topk_workspace_carve(char* base, u64 cap, TopKWorkspace* ws) {
  const u64 tiles = div_up(std::max<u64>(cap, 1), kTopKTile);
  u64 b = 0;
  auto take = [&](u64 bytes) {
    b = align_up(b, 256);
    char* p = base + b;
    b += bytes;
    return p;
  };
  ws->counts = reinterpret_cast<u64*>(take(cap * 8));
  ws->tile_val = reinterpret_cast<u64*>(take(tiles * 8));
  ws->tile_ge = reinterpret_cast<u64*>(take(tiles * 8));
  ws->sel = reinterpret_cast<u64*>(take(kTopKSelWords * 8));
  ws->cand_count = reinterpret_cast<u64*>(take((u64)kTopKMax * 8));
  ws->cand_val = reinterpret_cast<u64*>(take((u64)kTopKMax * 8));
  ws->cand_idx = reinterpret_cast<u32*>(take((u64)kTopKMax * 4));
  ws->cap = cap;
}

void launch_top_select(const OutRecord* recs, u64 n, u32 k, const TopKWorkspace& ws,
                       TopRecord* out, u32* out_n, hipStream_t s) {
  LOCUST_CHECK_ARG(k >= 1 && k <= kTopKMax, "top-k selection: k must be in [1, " +
                                                std::to_string(kTopKMax) + "]");
  LOCUST_CHECK_ARG(n <= ws.cap && n < (1ull << 32), "top-k selection: " + std::to_string(n) +
                                                        " records exceed the workspace (" +
                                                        std::to_string(ws.cap) + ")");
  const u32 m = (u32)std::min<u64>(k, n);
  if (n) {
    const u32 tiles = (u32)div_up(n, kTopKTile);
    const dim3 grid(tiles), block(kTopKBlock);
    // the words the kernels accumulate into: the largest count and the digit histograms
    LOCUST_HIP_CHECK(hipMemsetAsync(ws.sel, 0, kTopKSelWords * 8, s));
    topk_extract_kernel<<<grid, block, 0, s>>>(recs, (u32)n, ws.counts, ws.tile_val, ws.sel);
    LOCUST_HIP_LAUNCH_CHECK();
    for (int b = 7; b >= 0; --b) {
      topk_digit_kernel<<<grid, block, 0, s>>>(ws.counts, (u32)n, m, b, ws.sel);
      LOCUST_HIP_LAUNCH_CHECK();
    }
    topk_tile_count_kernel<<<grid, block, 0, s>>>(ws.counts, (u32)n, m, ws.sel, ws.tile_ge);
    LOCUST_HIP_LAUNCH_CHECK();
    topk_scan_kernel<<<dim3(1), block, 0, s>>>(ws.tile_val, ws.tile_ge, tiles);
    LOCUST_HIP_LAUNCH_CHECK();
    topk_scatter_kernel<<<grid, block, 0, s>>>(ws.counts, (u32)n, m, ws.sel, ws.tile_val,
                                               ws.tile_ge, ws.cand_count, ws.cand_idx,
                                               ws.cand_val);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  u32 P = 2;
  while (P < m) P <<= 1;
  topk_final_kernel<<<dim3(1), dim3(kFinalBlock), 0, s>>>(recs, (u32)n, m, P, ws.cand_count, ws.cand_idx,
                                                          ws.cand_val, out, out_n);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_topk() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&topk_extract_kernel));
}

}  // namespace locust
