// Ping-pong parity of the radix sort's pass schedule (radix_sort.hip), from the 32-bit mask
// of live digit positions (bit p = position p).  Words run 3..0; passes of word w run bytes
// 7..0 and alternate buffers starting at buffer 0 (the word's prepare kernel writes it);
// buffer 2 = identity permutation.  Host and device: the kernels of a device-planned sort
// call these to pick their buffers, and the bindings expose them to the schedule test.
#pragma once

#include "locust/common.hpp"
#include "locust/kv.hpp"

namespace locust {

LOCUST_HD inline u32 word_bits(u32 act, int w) { return (act >> (8 * w)) & 0xffu; }
LOCUST_HD inline u32 popc32(u32 x) {
  u32 c = 0;
  for (; x; x &= x - 1) ++c;
  return c;
}
LOCUST_HD inline u32 pass_src(u32 act, int pos) {
  const int w = pos / 8, b = pos % 8;
  return popc32(word_bits(act, w) >> (b + 1)) & 1u;  // live passes of this word before it
}
LOCUST_HD inline u32 word_src(u32 act, int w) {  // buffer holding the permutation at word start
  for (int v = w + 1; v < kKeyWords; ++v)
    if (word_bits(act, v))  // the nearest higher live word ran last: ended in popc & 1
      return popc32(word_bits(act, v)) & 1u;
  return 2u;
}
LOCUST_HD inline u32 final_src(u32 act) {
  for (int v = 0; v < kKeyWords; ++v)
    if (word_bits(act, v)) return popc32(word_bits(act, v)) & 1u;
  return 2u;
}

}  // namespace locust
