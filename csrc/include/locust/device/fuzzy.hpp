// The fuzzy-term matcher (engine.hpp "fuzzy terms"): one function, the same on the device
// (kernels/fuzzy.hip) and on the host (engine/common.cpp).
//
// A fuzzy term is a word w of at most kKeyBytes - 1 bytes, packed exactly as kv.hpp packs a
// key, and a budget d of 1 or 2.  A key k -- an index key or a token's cut key, its length the
// bytes before the NUL padding -- matches when the Levenshtein distance over bytes lev(w, k)
// is at most d: an insertion, a deletion or a substitution of one byte costs 1, there is no
// transposition, and two bytes are equal as glob_byte_eq says (the batch's fold).
//
// The lengths decide first: |len(k) - len(w)| > d is no match.  Behind that filter the only
// cells of the distance matrix that can hold a value <= 2 lie on the five diagonals j - i in
// [-2, 2], so a row is five cells in registers -- for either budget: the band of 2 is exact
// wherever the distance is at most 2, and never below the distance anywhere -- and the five key
// bytes beside them slide along, one new byte per row.  The loop runs len(w) rows and its trip
// count depends on the word alone; bytes come off the top of the packed words by shifts: no
// byte array, no indexing, nothing that could land in scratch.
#pragma once

#include <cstdint>

#include "locust/device/glob.hpp"
#include "locust/kv.hpp"

namespace locust {

// A fuzzy term's `meta` word (SearchPattern::meta, the pattern arrays' meta part): this bit, which
// no metacharacter map has (a pattern holds at most kKeyBytes - 1 bytes), and the budget below it.
constexpr uint32_t kFuzzyMeta = 1u << 31;
constexpr uint32_t kFuzzyBudgetMask = 3u;
constexpr uint32_t kFuzzyMaxBudget = 2;

// The bytes of a packed key before its NUL padding.
LOCUST_HD inline int fuzzy_len(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
  const int nw = w3 ? 4 : w2 ? 3 : w1 ? 2 : 1;
  const uint64_t last = w3 ? w3 : w2 ? w2 : w1 ? w1 : w0;
  return last ? 8 * nw - (__builtin_ctzll(last) >> 3) : 0;
}

// The byte as the comparison sees it: under the fold an ASCII capital becomes its small letter,
// every other byte stays.  Two bytes are equal here exactly when glob_byte_eq says so -- letters
// match either case, `@` and `[`, 0x80 and above only themselves -- but a cell then compares
// with one xor, and the fold itself is arithmetic: no lane mask stays alive in the row update.
LOCUST_HD inline uint32_t fuzzy_fold_byte(uint32_t c, uint32_t fold) {
  const uint32_t t = c - 0x41u;                 // 0 .. 25 for A .. Z
  const uint32_t upper = ~(t | (25u - t)) >> 31;  // both differences non-negative
  return c | ((upper & fold) << 5);
}

// 1 when two (folded) bytes differ, 0 when they are equal: (x + 255) >> 8 for x = a ^ b < 256.
LOCUST_HD inline uint32_t fuzzy_ne(uint32_t a, uint32_t b) { return ((a ^ b) + 255u) >> 8; }

// Is lev(w, k) <= d?  (p: the word w, d: 1 or 2.)  On the device the word must be the same in
// every lane of the wave, as it is wherever a batch's term meets the wave's keys: the row loop
// then runs on a scalar counter and keeps no per-lane loop mask alive.
LOCUST_HD inline bool fuzzy_match(uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3, uint32_t d,
                                  uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, bool fold) {
  int la = fuzzy_len(p0, p1, p2, p3);
#if defined(__HIP_DEVICE_COMPILE__)
  la = __builtin_amdgcn_readfirstlane(la);  // (wave-uniform already: now the compiler knows)
#endif
  const int diff = fuzzy_len(k0, k1, k2, k3) - la;
  const bool near = (uint32_t)(diff + (int)d) <= 2u * d;  // the length filter: |diff| <= d
  const uint32_t f = fold ? 1u : 0u;
  // c_t = D[i][i + t - 2], the cell of row i (i bytes of w) and column i + t - 2 (bytes of k).
  // A column below 0 holds kInf, which only grows: at most kKeyBytes rows add one each.
  constexpr uint32_t kInf = 64;
  uint32_t c0 = kInf, c1 = kInf, c2 = 0, c3 = 1, c4 = 2;
  // b_t = k[i + t - 2]: the key byte a step along diagonal t consumes (0 outside the key: no
  // byte of w equals it, and a cell behind the key's end is never read back)
  uint32_t b0 = 0, b1 = 0, b2 = fuzzy_fold_byte((uint32_t)(k0 >> 56), f),
           b3 = fuzzy_fold_byte((uint32_t)(k0 >> 48) & 0xffu, f),
           b4 = fuzzy_fold_byte((uint32_t)(k0 >> 40) & 0xffu, f);
  // the words go by in order: w's bytes from the top of pw, the key's from byte 3 on from the
  // top of kw (the key shifted by three bytes, word by word)
  const uint64_t pws[kKeyWords] = {p0, p1, p2, p3};
  const uint64_t kws[kKeyWords] = {(k0 << 24) | (k1 >> 40), (k1 << 24) | (k2 >> 40),
                                   (k2 << 24) | (k3 >> 40), k3 << 24};
  int i = 0;
#pragma unroll
  for (int j = 0; j < kKeyWords; ++j) {  // (static: pws and kws stay in registers)
    uint64_t pw = pws[j], kw = kws[j];
    const int rows = la < 8 * (j + 1) ? la : 8 * (j + 1);  // this word's bytes of w
    for (; i < rows; ++i) {
      const uint32_t a = fuzzy_fold_byte((uint32_t)(pw >> 56), f);
      pw <<= 8;
      // row i + 1: along the diagonal (a substitution, or equal bytes), from the cell above
      // (w's byte deleted: c_{t+1}), from the cell to the left (k's byte inserted: the new
      // c_{t-1})
      uint32_t n0 = c0 + fuzzy_ne(a, b0);
      n0 = n0 < c1 + 1u ? n0 : c1 + 1u;
      uint32_t n1 = c1 + fuzzy_ne(a, b1);
      n1 = n1 < c2 + 1u ? n1 : c2 + 1u;
      n1 = n1 < n0 + 1u ? n1 : n0 + 1u;
      uint32_t n2 = c2 + fuzzy_ne(a, b2);
      n2 = n2 < c3 + 1u ? n2 : c3 + 1u;
      n2 = n2 < n1 + 1u ? n2 : n1 + 1u;
      uint32_t n3 = c3 + fuzzy_ne(a, b3);
      n3 = n3 < c4 + 1u ? n3 : c4 + 1u;
      n3 = n3 < n2 + 1u ? n3 : n2 + 1u;
      uint32_t n4 = c4 + fuzzy_ne(a, b4);
      n4 = n4 < n3 + 1u ? n4 : n3 + 1u;
      c0 = n0, c1 = n1, c2 = n2, c3 = n3, c4 = n4;
      b0 = b1, b1 = b2, b2 = b3, b3 = b4;
      b4 = fuzzy_fold_byte((uint32_t)(kw >> 56), f);
      kw <<= 8;
    }
  }
  // D[len(w)][len(k)]: the cell on diagonal diff, picked by a shift (every cell is below 128;
  // a diff outside the band has failed the filter already)
  const uint64_t cells = (uint64_t)c0 | ((uint64_t)c1 << 8) | ((uint64_t)c2 << 16) |
                         ((uint64_t)c3 << 24) | ((uint64_t)c4 << 32);
  const uint32_t dist = (uint32_t)(cells >> (8u * ((uint32_t)(diff + 2) & 7u))) & 0xffu;
  return near && dist <= d;
}

// Does the key match the term a `meta` word describes: a fuzzy term's word within its budget,
// or a pattern (device/glob.hpp)?
LOCUST_HD inline bool term_match(const uint64_t* p, uint32_t meta, const uint64_t* k, bool fold) {
  if (meta & kFuzzyMeta)
    return fuzzy_match(p[0], p[1], p[2], p[3], meta & kFuzzyBudgetMask, k[0], k[1], k[2], k[3],
                       fold);
  return glob_match(p[0], p[1], p[2], p[3], meta, k[0], k[1], k[2], k[3], fold);
}

}  // namespace locust
