// What the kernels that walk a line against a query's terms share (search.hip: the phrase and
// near kernels; show.hip: the show kernels): the term mask of one token, and the register-file
// hint their pattern siblings use.
#pragma once

#include "locust/device/fuzzy.hpp"
#include "locust/device/glob.hpp"
#include "locust/device/linetok.hpp"
#include "locust/device/regex.hpp"
#include "locust/kernels.hpp"

namespace locust {

// A pointer kept in vector registers from here on.  The verify kernels' walk keeps 97 scalar
// registers live, and the matcher's divergent loop needs about twenty more for its masks: their
// glob siblings move the pointers they rarely use out of the scalar file instead of spilling.
template <class T>
__device__ __forceinline__ T* in_vgprs(T* p) {
  u64 v = reinterpret_cast<u64>(p);
  asm volatile("" : "+v"(v));
  return reinterpret_cast<T*>(v);
}

// A value kept in vector registers from here on: in_vgprs for what is no pointer.
template <class T>
__device__ __forceinline__ T value_in_vgprs(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// A wave-uniform u32 parked in a vector register (kPark), and read back where a uniform branch
// needs it: a long-lived scalar register for one v_readfirstlane per use.  Without kPark both
// are the value itself.
template <bool kPark>
__device__ __forceinline__ u32 parked(u32 v) {
  if (kPark) asm volatile("" : "+v"(v));
  return v;
}
template <bool kPark>
__device__ __forceinline__ u32 unparked(u32 v) {
  return kPark ? (u32)__builtin_amdgcn_readfirstlane((int)v) : v;
}

// The lane number behind a barrier the compiler does not look through (kOpaque): a compare
// with it is made where it stands, not hoisted out of the walk into a scalar register pair that
// then lives through the whole kernel.  For the rare sites: a round's atomics, a query's keys.
template <bool kOpaque>
__device__ __forceinline__ int lane_here(int lane) {
  if (kOpaque) asm volatile("" : "+v"(lane));
  return lane;
}

// parked / unparked for a wave-uniform u64.
template <bool kPark>
__device__ __forceinline__ u64 parked64(u64 v) {
  if (kPark) asm volatile("" : "+v"(v));
  return v;
}
template <bool kPark>
__device__ __forceinline__ u64 unparked64(u64 v) {
  if (!kPark) return v;
  const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
  const u32 hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// A wave-uniform pointer that lives in vector registers, read back into the scalar file where
// scalar loads need it.
template <class T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) {
  const u64 v = reinterpret_cast<u64>(p);
  const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
  const u32 hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32));
  return reinterpret_cast<const T*>(((u64)hi << 32) | lo);
}

// Bit j: the token that starts at row[at] matches term j of the m keys at qk -- it equals
// the key, or (pre bit j: a prefix term) starts with the key's bytes.  kMatch 1 (a batch with
// pattern terms): or (pt bit j: a pattern term) the key is a pattern that matches the token's
// cut key, qm[j] its metacharacter map and pt's kSearchFold the batch's fold.  kMatch 2 (a
// batch with a fuzzy term): or (pt bit kSearchFuzzyShift + j as well) the key is a word within
// qm[j]'s budget of the token's cut key (device/fuzzy.hpp), under the same fold.  The fuzzy
// terms have a loop of their own behind the others': the pattern matcher's backtracking loop
// holds the scalar file to its last register, and nothing of the second matcher is live in it.
// kMatch 3 (a batch with a regex term): or (pt bit kSearchRegexShift + j as well) qm[j] is the
// index of the term's program in the table rx, and the program matches the token's cut key
// (device/regex.hpp; the fold is compiled in).  The regex terms have a third loop, for the same
// reason.
template <int kMatch>
__device__ __forceinline__ u32 token_term_mask(const unsigned char* row, int at,
                                               const DelimMask& dm, int max_key_len,
                                               const u64* qk, u32 m, u32 pre, u32 pt,
                                               const u32* qm, const u32* rx = nullptr) {
  u64 w0, w1, w2, w3;
  dev::pack_row_key(row, at, dm, max_key_len, &w0, &w1, &w2, &w3);
  u32 eq = 0;
  for (u32 j = 0; j < m; ++j) {
    const u64* k = qk + j * kKeyWords;
    if (kMatch >= 2 && ((pt >> (kSearchFuzzyShift + j)) & 1u)) continue;  // (wave-uniform) below
    if (kMatch == 3 && ((pt >> (kSearchRegexShift + j)) & 1u)) continue;  // (wave-uniform) below
    if (kMatch && ((pt >> j) & 1u)) {  // (wave-uniform)
      eq |= (u32)glob_match(k[0], k[1], k[2], k[3], qm[j], w0, w1, w2, w3,
                            (pt & kSearchFold) != 0)
            << j;
      continue;
    }
    if ((pre >> j) & 1u) {  // (wave-uniform) the token starts with the term's bytes
      eq |= (u32)(k[0] == (w0 & key_word_mask(k[0])) && k[1] == (w1 & key_word_mask(k[1])) &&
                  k[2] == (w2 & key_word_mask(k[2])) && k[3] == (w3 & key_word_mask(k[3])))
            << j;
      continue;
    }
    eq |= (u32)(k[0] == w0 && k[1] == w1 && k[2] == w2 && k[3] == w3) << j;
  }
  if (kMatch >= 2) {
    // (wave-uniform) the query's fuzzy terms among its m positive ones
    for (u32 fm = (pt >> kSearchFuzzyShift) & ((1u << m) - 1u); fm; fm &= fm - 1u) {
      const u32 j = (u32)__ffs((int)fm) - 1u;
      const u64* k = qk + j * kKeyWords;
      eq |= (u32)fuzzy_match(k[0], k[1], k[2], k[3], qm[j] & kFuzzyBudgetMask, w0, w1, w2, w3,
                             (pt & kSearchFold) != 0)
            << j;
    }
  }
  if (kMatch == 3) {
    // (wave-uniform) the query's regex terms among its m positive ones
    for (u32 j = 0; j < m; ++j) {
      if (!((pt >> (kSearchRegexShift + j)) & 1u)) continue;
      // (the index comes out of LDS: uniform, and now the compiler knows -- scalar loads below)
      const u32 pi = (u32)__builtin_amdgcn_readfirstlane((int)qm[j]);
      eq |= (u32)regex_match(uniform_ptr(rx + (u64)pi * kRegexWords), w0, w1, w2, w3) << j;
    }
  }
  return eq;
}

}  // namespace locust
