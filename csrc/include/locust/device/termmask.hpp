// What the kernels that walk a line against a query's terms share (search.hip: the phrase and
// near kernels; show.hip: the show kernels): the term mask of one token, and the register-file
// hint their pattern siblings use.
#pragma once

#include "locust/device/fuzzy.hpp"
#include "locust/device/glob.hpp"
#include "locust/device/linetok.hpp"
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

// Bit j: the token that starts at row[at] matches term j of the m keys at qk -- it equals
// the key, or (pre bit j: a prefix term) starts with the key's bytes.  kMatch 1 (a batch with
// pattern terms): or (pt bit j: a pattern term) the key is a pattern that matches the token's
// cut key, qm[j] its metacharacter map and pt's kSearchFold the batch's fold.  kMatch 2 (a
// batch with a fuzzy term): or (pt bit kSearchFuzzyShift + j as well) the key is a word within
// qm[j]'s budget of the token's cut key (device/fuzzy.hpp), under the same fold.  The fuzzy
// terms have a loop of their own behind the others': the pattern matcher's backtracking loop
// holds the scalar file to its last register, and nothing of the second matcher is live in it.
template <int kMatch>
__device__ __forceinline__ u32 token_term_mask(const unsigned char* row, int at,
                                               const DelimMask& dm, int max_key_len,
                                               const u64* qk, u32 m, u32 pre, u32 pt,
                                               const u32* qm) {
  u64 w0, w1, w2, w3;
  dev::pack_row_key(row, at, dm, max_key_len, &w0, &w1, &w2, &w3);
  u32 eq = 0;
  for (u32 j = 0; j < m; ++j) {
    const u64* k = qk + j * kKeyWords;
    if (kMatch == 2 && ((pt >> (kSearchFuzzyShift + j)) & 1u)) continue;  // (wave-uniform) below
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
  if (kMatch == 2) {
    // (wave-uniform) the query's fuzzy terms among its m positive ones
    for (u32 fm = (pt >> kSearchFuzzyShift) & ((1u << m) - 1u); fm; fm &= fm - 1u) {
      const u32 j = (u32)__ffs((int)fm) - 1u;
      const u64* k = qk + j * kKeyWords;
      eq |= (u32)fuzzy_match(k[0], k[1], k[2], k[3], qm[j] & kFuzzyBudgetMask, w0, w1, w2, w3,
                             (pt & kSearchFold) != 0)
            << j;
    }
  }
  return eq;
}

}  // namespace locust
