// The pattern-term matcher (engine.hpp "pattern terms"): one function, the same on the
// device (kernels/search.hip) and on the host (engine/common.cpp).
//
// A pattern is at most kKeyBytes bytes, packed exactly as kv.hpp packs a key (big-endian
// words, NUL padded), and a 32-bit map of its metacharacters: bit i set means that byte i,
// a `*` or a `?`, is one; a clear bit makes the byte literal whatever it is.  (A plain term
// that is evaluated as a pattern under ignore_case may hold a literal `*`, so the bytes
// alone cannot say.)  The key is an index key or a token's cut key: its length is the bytes
// before the NUL padding.
//
// The match is iterative with one backtrack point -- the last star and the key position
// tried behind it -- and reads bytes out of the words by shifts and selects: no byte array,
// nothing that could land in scratch.
#pragma once

#include <cstdint>

#include "locust/kv.hpp"

namespace locust {

// Byte i of a packed key or pattern; 0 (the padding) for i >= kKeyBytes.
LOCUST_HD inline uint32_t glob_byte(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, int i) {
  if (i >= kKeyBytes) return 0u;
  const uint64_t w = i < 8 ? w0 : i < 16 ? w1 : i < 24 ? w2 : w3;
  return (uint32_t)(w >> (56 - 8 * (i & 7))) & 0xffu;
}

// Does the literal pattern byte p match the key byte k?  fold: ASCII letters match either
// case; every other byte -- `@`, `[`, 0x80 and above -- matches only itself.
LOCUST_HD inline bool glob_byte_eq(uint32_t p, uint32_t k, bool fold) {
  if (p == k) return true;
  if (!fold || (p ^ k) != 0x20u) return false;
  const uint32_t l = p | 0x20u;
  return l >= (uint32_t)'a' && l <= (uint32_t)'z';
}

// Does the whole key k match the pattern p?  `*` matches any run of bytes, the empty one
// included; `?` exactly one byte, never the padding; every other byte itself.
LOCUST_HD inline bool glob_match(uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3,
                                 uint32_t meta, uint64_t k0, uint64_t k1, uint64_t k2,
                                 uint64_t k3, bool fold) {
  int pi = 0, ki = 0;
  int star = -1, mark = 0;  // the last star's position, and the key position tried behind it
  for (;;) {                // (ends: ki and mark only grow, and the key ends by kKeyBytes)
    const uint32_t kc = glob_byte(k0, k1, k2, k3, ki);
    const uint32_t pc = glob_byte(p0, p1, p2, p3, pi);
    const bool m = pi < kKeyBytes && ((meta >> pi) & 1u);
    if (m && pc == (uint32_t)'*') {  // (at the key's end too: what is left must be stars)
      star = pi++;
      mark = ki;
      continue;
    }
    if (kc == 0u) return pc == 0u;  // the key's end: the pattern's end, or no match
    if (pc != 0u && (m || glob_byte_eq(pc, kc, fold))) {  // (a meta byte here is a `?`)
      ++pi;
      ++ki;
      continue;
    }
    if (star < 0) return false;
    pi = star + 1;  // the star takes one byte more
    ki = ++mark;
  }
}

LOCUST_HD inline bool glob_match(const uint64_t* p, uint32_t meta, const uint64_t* k, bool fold) {
  return glob_match(p[0], p[1], p[2], p[3], meta, k[0], k[1], k[2], k[3], fold);
}

}  // namespace locust
