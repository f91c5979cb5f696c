// The wave-per-line tokeniser's per-step pieces (index.hip, search.hip): a wave walks a line
// 64 bytes per step, stages the step's bytes and the 32 behind them in its LDS row, takes
// the token starts from ballots and packs the keys from the row -- bit-identical to the
// map's packing (kv.hpp).
#pragma once

#include "locust/common.hpp"
#include "locust/device/wave.hpp"
#include "locust/dstring.hpp"
#include "locust/kv.hpp"

namespace locust {
namespace dev {

constexpr int kLineRow = 64 + 32;  // a step's bytes + the 32 behind them (keys <= 31 bytes)
static_assert(kKeyBytes <= 32, "a key that starts in lane 63 ends inside the staged row");

// The token starts of one 64-byte step of a line (c: this lane's byte, 0 past the line end;
// carry: the previous step's last byte belonged to a token).  *last: a NUL, or the line
// end, lies inside the step.
__device__ __forceinline__ u64 step_starts(unsigned c, const DelimMask& dm, u64* carry,
                                           bool* last) {
  // bytes past the line end were loaded as 0: they end the tokens like a NUL
  const u64 z = ballot(c == 0u);
  u64 m = ballot(c != 0u && !mask_is_delim(dm, c));
  if (z) m &= (z & (~z + 1)) - 1;  // nothing at or behind the first NUL (or the end)
  const u64 starts = m & ~((m << 1) | *carry);
  *carry = m >> 63;
  *last = z != 0;
  return starts;
}

// The key of the token that starts at row[at] (at < 64): its first max_key_len bytes, up to
// a delimiter or a 0 byte.
__device__ __forceinline__ void pack_row_key(const unsigned char* row, int at, const DelimMask& dm,
                                             int max_key_len, u64* w0, u64* w1, u64* w2, u64* w3) {
  u64 k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  for (int len = 0; len < max_key_len; ++len) {
    const unsigned ch = row[at + len];
    if (ch == 0u || mask_is_delim(dm, ch)) break;
    const u64 v = (u64)ch << (56 - 8 * (len & 7));
    const int wi = len >> 3;
    k0 |= wi == 0 ? v : 0ull;
    k1 |= wi == 1 ? v : 0ull;
    k2 |= wi == 2 ? v : 0ull;
    k3 |= wi == 3 ? v : 0ull;
  }
  *w0 = k0;
  *w1 = k1;
  *w2 = k2;
  *w3 = k3;
}

}  // namespace dev
}  // namespace locust
