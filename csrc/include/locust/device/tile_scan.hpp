// The three-kernel exclusive scan of the index merge and the index drop (append.hip, drop.hip):
// tile sums, a one-workgroup scan of the tile array, a workgroup scan inside each tile, over a
// strided u64 source whose length may be known on the device only.  Data crosses between
// workgroups at the kernel boundaries alone.  The kernels are file-local (static): every .hip
// file that includes this header gets its own copies in its own code object.
#pragma once

#include "locust/device/wave.hpp"
#include "locust/kernels.hpp"

namespace locust {

// The scans read src[i * stride] for i < n = n_base + *n_more (n_more: optional).
// tile_val[tile] = the tile's sum.
static __global__ __launch_bounds__(kIndexBlock) void append_tile_sum_kernel(
    const u64* __restrict__ src, u32 stride, u32 n_base, const u32* __restrict__ n_more,
    u64* __restrict__ tile_val) {
  __shared__ u64 s_sum[kIndexBlock / 64];
  const u64 n = (u64)n_base + (n_more ? *n_more : 0u);
  const u64 base = (u64)blockIdx.x * kIndexTile;
  u64 sum = 0;
#pragma unroll
  for (int j = 0; j < kIndexItems; ++j) {
    const u64 i = base + (u64)j * kIndexBlock + threadIdx.x;
    if (i < n) sum += src[i * stride];
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

// One workgroup: exclusive scan of the tile sums, in place; the total to out[n] and, if given,
// to *total32.
static __global__ __launch_bounds__(kIndexBlock) void append_tile_scan_kernel(
    u64* __restrict__ tile_val, u32 tiles, u64* __restrict__ out, u32 n_base,
    const u32* __restrict__ n_more, u32* __restrict__ total32) {
  __shared__ u64 s_scan[kIndexBlock / 64 + 1];
  const u64 n = (u64)n_base + (n_more ? *n_more : 0u);
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
    out[n] = carry;
    if (total32) *total32 = (u32)carry;
  }
}

// out[i] = exclusive prefix of the source (blocked: a thread's items are neighbours).
static __global__ __launch_bounds__(kIndexBlock) void append_tile_apply_kernel(
    const u64* __restrict__ src, u32 stride, u32 n_base, const u32* __restrict__ n_more,
    const u64* __restrict__ tile_val, u64* __restrict__ out) {
  __shared__ u64 s_scan[kIndexBlock / 64 + 1];
  const u64 n = (u64)n_base + (n_more ? *n_more : 0u);
  const u64 first = (u64)blockIdx.x * kIndexTile + (u64)threadIdx.x * kIndexItems;
  u64 c[kIndexItems];
  u64 sum = 0;
#pragma unroll
  for (int t = 0; t < kIndexItems; ++t) {
    c[t] = first + t < n ? src[(first + t) * stride] : 0;
    sum += c[t];
  }
  u64 tot;
  u64 at = dev::block_exclusive_scan<u64, kIndexBlock>(sum, s_scan, &tot) + tile_val[blockIdx.x];
#pragma unroll
  for (int t = 0; t < kIndexItems; ++t) {
    if (first + t < n) out[first + t] = at;
    at += c[t];
  }
}

}  // namespace locust
