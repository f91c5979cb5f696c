// The dictionary scan of a batch that has a pattern term (kernels.hpp "search.hip": match,
// scatter): the bodies of its two kernels, compiled per matcher level -- search.hip's kernels
// with the pattern matcher (kMatch 1), fuzzy.hip's with the fuzzy matcher beside it (kMatch 2),
// regex.hip's with the regex matcher as well (kMatch 3).
//
// The walk the match and the scatter kernel share: grid x strides over the records in tiles
// of kSearchBlock, one record per thread; grid y takes every gridDim.y-th query.  A tile's
// waves are whole (the tail's dead lanes match nothing), so every ballot below is converged.
#pragma once

#include <algorithm>

#include "locust/device/fuzzy.hpp"
#include "locust/device/glob.hpp"
#include "locust/device/regex.hpp"
#include "locust/device/wave.hpp"
#include "locust/kernels.hpp"

namespace locust {

constexpr u32 kMatchMaxBlocks = 1024;  // the grid: x * y workgroups at most

// The dictionary scan's grid: x over the record tiles, y over the queries while there are few
// tiles (a small dictionary would otherwise leave most of the device idle).
inline dim3 match_grid(u32 n, u32 queries) {
  const u32 x = (u32)std::min<u64>(div_up((u64)std::max(n, 1u), (u64)kSearchBlock), kMatchMaxBlocks);
  const u32 y = std::min(queries, std::max(1u, kMatchMaxBlocks / x));
  return dim3(x, y);
}

// Does the key match pattern slot `slot` of a query whose flag word is fl?  (All but the key
// wave-uniform.)  kMatch 2: a slot with its fuzzy bit holds a word and, in its meta word, a
// budget.  kMatch 3: a slot with its regex bit holds, in its meta word, the index of its program
// in the table rx.
template <int kMatch>
__device__ __forceinline__ bool slot_match(const u64* __restrict__ p, u32 fl, u32 slot, bool fold,
                                           u32 meta, u64 k0, u64 k1, u64 k2, u64 k3,
                                           const u32* __restrict__ rx = nullptr) {
  if (kMatch == 3 && ((fl >> (kSearchRegexShift + slot % kSearchMaxTerms)) & 1u))  // (uniform)
    return regex_match(rx + (u64)meta * kRegexWords, k0, k1, k2, k3);
  if (kMatch >= 2 && ((fl >> (kSearchFuzzyShift + slot % kSearchMaxTerms)) & 1u))  // (uniform)
    return fuzzy_match(p[0], p[1], p[2], p[3], meta & kFuzzyBudgetMask, k0, k1, k2, k3, fold);
  return glob_match(p[0], p[1], p[2], p[3], meta, k0, k1, k2, k3, fold);
}

// words[slot] += the records the slot's pattern matches, len[slot] += their counts, rank[slot]
// = one of them (pw: words | len | rank, zeroed per batch).
template <int kMatch>
__device__ __forceinline__ void search_match_body(const OutRecord* __restrict__ recs, u32 n,
                                                  const u64* __restrict__ keys,
                                                  const u32* __restrict__ pq, u32 Q,
                                                  u32* __restrict__ pw,
                                                  const u32* __restrict__ rx = nullptr) {
  constexpr u32 kTerms = kSearchMaxTerms;
  const int lane = dev::lane_id();
  for (u32 base = blockIdx.x * kSearchBlock; base < n; base += gridDim.x * kSearchBlock) {
    const u32 rank = base + threadIdx.x;
    const bool live = rank < n;
    u64 k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    u32 cnt = 0;
    if (live) {
      k0 = recs[rank].w[0];
      k1 = recs[rank].w[1];
      k2 = recs[rank].w[2];
      k3 = recs[rank].w[3];
      cnt = (u32)recs[rank].count;  // (the index holds < 2^32 postings in all)
    }
    for (u32 q = blockIdx.y; q < Q; q += gridDim.y) {  // (uniform)
      const u32 fl = pq[q];
      const bool fold = (fl & kSearchFold) != 0;
      for (u32 pm = fl & 0xffu; pm; pm &= pm - 1u) {  // (uniform) the query's pattern terms
        const u32 slot = q * kTerms + (u32)__ffs((int)pm) - 1u;
        const u64* p = keys + (u64)slot * kKeyWords;
        const bool m = live && slot_match<kMatch>(p, fl, slot, fold, pq[kSearchPatMeta + slot],
                                                  k0, k1, k2, k3, rx);
        const u64 bm = dev::ballot(m);
        if (bm == 0) continue;  // (wave-uniform)
        const u32 sum = dev::wave_reduce_sum(m ? cnt : 0u);
        if (lane == __ffsll((unsigned long long)bm) - 1) {
          atomicAdd(&pw[slot], (u32)__popcll(bm));
          atomicAdd(&pw[kSearchSlots + slot], sum);
          pw[2 * kSearchSlots + slot] = rank;
        }
      }
    }
  }
}

// The wide pattern slots' part of the keys (x_len != 0 and a pattern slot): the match kernel's
// walk and match; the matching words of a wave and pattern take consecutive room in the slot's
// part of [0, X) -- a wave prefix sum of their counts behind one atomic on the slot's cursor --
// and the wave copies their postings word by word, 64 elements per step.  Reads stay inside
// the CSR (a word's val range), writes inside [x_start[slot], x_start[slot + 1]), whatever
// the cursor says: a slot that does not fill exactly counts as unmerged in the strip.
template <int kMatch>
__device__ __forceinline__ void search_scatter_body(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ val,
    const u32* __restrict__ postings, u32 first_line, const u64* __restrict__ pkeys,
    const u32* __restrict__ pq, u32 Q, const u32* __restrict__ x_len,
    const u64* __restrict__ x_start, u64 X, u64 cap, u32* __restrict__ cursor,
    u64* __restrict__ keys, const u32* __restrict__ rx = nullptr) {
  constexpr u32 kTerms = kSearchMaxTerms;
  if (x_start[Q * kTerms] != X || X > cap) return;  // (uniform; as the gather kernel)
  const int lane = dev::lane_id();
  for (u32 base = blockIdx.x * kSearchBlock; base < n; base += gridDim.x * kSearchBlock) {
    const u32 rank = base + threadIdx.x;
    const bool live = rank < n;
    u64 k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    u32 src = 0, cnt = 0;
    if (live) {
      k0 = recs[rank].w[0];
      k1 = recs[rank].w[1];
      k2 = recs[rank].w[2];
      k3 = recs[rank].w[3];
      src = (u32)val[rank];  // (the index holds < 2^32 postings in all)
      cnt = (u32)(val[rank + 1] - val[rank]);
    }
    for (u32 q = blockIdx.y; q < Q; q += gridDim.y) {  // (uniform)
      const u32 fl = pq[q];
      const bool fold = (fl & kSearchFold) != 0;
      for (u32 pm = fl & 0xffu; pm; pm &= pm - 1u) {  // (uniform) the query's pattern terms
        const u32 slot = q * kTerms + (u32)__ffs((int)pm) - 1u;
        if (x_len[slot] == 0u) continue;  // (uniform) not wide: nothing to merge
        const u64* p = pkeys + (u64)slot * kKeyWords;
        const bool m = live && slot_match<kMatch>(p, fl, slot, fold, pq[kSearchPatMeta + slot],
                                                  k0, k1, k2, k3, rx);
        u64 bm = dev::ballot(m);
        if (bm == 0) continue;  // (wave-uniform)
        const u32 mine = m ? cnt : 0u;
        const u32 incl = dev::wave_inclusive_scan(mine);
        const u32 total = (u32)__shfl((int)incl, 63, 64);
        u32 at = 0;
        if (lane == 0) at = atomicAdd(&cursor[slot], total);
        at = (u32)__shfl((int)at, 0, 64) + incl - mine;  // this lane's word, inside the slot
        const u64 lo = x_start[slot], hi = x_start[slot + 1];
        for (; bm; bm &= bm - 1) {  // (wave-uniform) word by word, the whole wave copying
          const int l = __ffsll((unsigned long long)bm) - 1;
          const u32 wsrc = (u32)__shfl((int)src, l, 64);
          const u32 wcnt = (u32)__shfl((int)cnt, l, 64);
          const u64 dst = lo + (u32)__shfl((int)at, l, 64);
          for (u32 i = (u32)lane; i < wcnt; i += 64u)
            if (dst + i < hi)
              keys[dst + i] = ((u64)slot << 32) | (u64)(postings[wsrc + i] - first_line);
        }
      }
    }
  }
}

}  // namespace locust
