// Rank lookup among a word job's key-ordered records (index.hip, search.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "locust/kernels.hpp"

namespace locust {
namespace dev {

// The rank of key (w0..w3) among the n sorted, distinct records; n when it is absent.
__device__ __forceinline__ u32 find_rank(const OutRecord* __restrict__ recs, u32 n, u64 w0, u64 w1,
                                         u64 w2, u64 w3) {
  u32 lo = 0, hi = n;
  while (lo < hi) {  // lower bound
    const u32 mid = lo + ((hi - lo) >> 1);
    const OutRecord* r = recs + mid;
    bool less;  // recs[mid] < key
    const u64 a0 = r->w[0];
    if (a0 != w0) {
      less = a0 < w0;
    } else {
      const u64 a1 = r->w[1];
      if (a1 != w1) {
        less = a1 < w1;
      } else {
        const u64 a2 = r->w[2];
        if (a2 != w2) {
          less = a2 < w2;
        } else {
          less = r->w[3] < w3;
        }
      }
    }
    if (less)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < n) {
    const OutRecord* r = recs + lo;
    if (r->w[0] == w0 && r->w[1] == w1 && r->w[2] == w2 && r->w[3] == w3) return lo;
  }
  return n;
}

}  // namespace dev
}  // namespace locust
