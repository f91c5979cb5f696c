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

// The lower bound of key (w0..w3) among the n sorted, distinct records: the number of records
// below it (append.hip); *equal: the record there holds the key.
__device__ __forceinline__ u32 lower_rank(const OutRecord* __restrict__ recs, u32 n, u64 w0, u64 w1,
                                          u64 w2, u64 w3, bool* equal) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
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
  *equal = false;
  if (lo < n) {
    const OutRecord* r = recs + lo;
    *equal = r->w[0] == w0 && r->w[1] == w1 && r->w[2] == w2 && r->w[3] == w3;
  }
  return lo;
}

// The rank range [*lo, *hi) of the records whose key starts with the prefix p = the non-zero
// bytes of (w0..w3) (a key holds no NUL before its padding): *lo is the lower bound of p
// padded with 0x00, which is (w0..w3) itself, *hi the upper bound of p padded with 0xff to
// kKeyBytes.  The keys are in unsigned-byte order, so exactly the ranks between start with
// p; *lo == *hi when none does.
__device__ __forceinline__ void find_prefix_range(const OutRecord* __restrict__ recs, u32 n,
                                                  u64 w0, u64 w1, u64 w2, u64 w3, u32* lo_out,
                                                  u32* hi_out) {
  const u64 lw[kKeyWords] = {w0, w1, w2, w3};
  u64 hw[kKeyWords];
#pragma unroll
  for (int j = 0; j < kKeyWords; ++j) hw[j] = lw[j] | ~key_word_mask(lw[j]);
  u32 lo = 0, hi = n;
  while (lo < hi) {  // lower bound: the first record >= lw
    const u32 mid = lo + ((hi - lo) >> 1);
    const OutRecord* r = recs + mid;
    bool less = false;  // recs[mid] < lw
#pragma unroll
    for (int j = 0; j < kKeyWords; ++j) {
      const u64 a = r->w[j];
      if (a != lw[j]) {
        less = a < lw[j];
        break;
      }
    }
    if (less)
      lo = mid + 1;
    else
      hi = mid;
  }
  *lo_out = lo;
  hi = n;  // (lw <= hw: the upper bound lies at or behind the lower one)
  while (lo < hi) {  // upper bound: the first record > hw
    const u32 mid = lo + ((hi - lo) >> 1);
    const OutRecord* r = recs + mid;
    bool above = false;  // recs[mid] > hw
#pragma unroll
    for (int j = 0; j < kKeyWords; ++j) {
      const u64 a = r->w[j];
      if (a != hw[j]) {
        above = a > hw[j];
        break;
      }
    }
    if (above)
      hi = mid;
    else
      lo = mid + 1;
  }
  *hi_out = lo;
}

}  // namespace dev
}  // namespace locust
