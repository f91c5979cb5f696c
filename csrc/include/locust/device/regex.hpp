// The regex-term matcher (engine.hpp "regex terms"): the layout of a compiled program and one
// function, the same on the device (kernels/regex.hip) and on the host (engine/common.cpp).
//
// A regex term is compiled on the host (compile_regex, engine/common.cpp) into the Glushkov
// position automaton of its expression: at most kRegexMaxPos = 32 positions -- one per literal,
// `.` or class of the source -- so a set of positions is one u32.  A program is kRegexWords u32
// words:
//   [kRegexFirst]     the positions a match may start at
//   [kRegexLast]      the positions a match may end at
//   [kRegexNullable]  non-zero: the expression matches the empty key
//   [kRegexNpos]      the number of positions
//   [kRegexFollow + i], i < 32   the positions that may follow position i
//   [kRegexB + c], c < 256       bit i: position i accepts the byte c.  The batch's fold is
//                     compiled in (engine.hpp: a position's set closed under the ASCII case swap
//                     before a class's negation), and B[0] is 0: nothing accepts the padding.
//
// A key k -- an index key or a token's cut key, its length the bytes before the NUL padding --
// matches when the automaton, started at its first byte, holds a last position at its end:
//   S = first & B[k[0]];  S = (OR of follow[i] over the bits i of S) & B[k[j]], j = 1, 2, ...
// anchored at both ends.  The OR runs as a loop over the program's positions, not over the set
// bits of S: on the device the program is the same in every lane of the wave, so follow[i] is a
// scalar load and the loop a scalar counter, where a walk over each lane's own bits would be a
// chain of dependent divergent loads.  Only B is indexed per lane, by the lane's own byte.  Key
// bytes come off the top of the packed words by shifts: no byte array, no scratch.
#pragma once

#include <cstdint>

#include "locust/kv.hpp"

namespace locust {

constexpr int kRegexMaxPos = 32;
constexpr int kRegexFirst = 0;
constexpr int kRegexLast = 1;
constexpr int kRegexNullable = 2;
constexpr int kRegexNpos = 3;
constexpr int kRegexFollow = 4;
constexpr int kRegexB = kRegexFollow + kRegexMaxPos;
constexpr int kRegexWords = kRegexB + 256;  // 292

// In the device's pattern arrays a regex slot's meta word is its program's index in the batch's
// table, and its key words are kRegexKeyTag and that index: a first key word whose top byte is
// NUL, which no pattern's and no fuzzy term's bytes give.  (No bit of a meta word marks a regex
// term: a pattern of max_key_len <= 31 bytes may use every bit of its map below bit 31.  The
// slot's flag bit does, and on the host SearchPattern::regex.)
constexpr uint64_t kRegexKeyTag = 0x52454758ull;  // "REGX" below a NUL top byte

// Does the whole key k match the program?  (On the device `prog` must be the same in every lane
// of the wave, as it is wherever a batch's term meets the wave's keys.)
LOCUST_HD inline bool regex_match(const uint32_t* __restrict__ prog, uint64_t k0, uint64_t k1,
                                  uint64_t k2, uint64_t k3) {
  const uint32_t c0 = (uint32_t)(k0 >> 56);
  uint32_t npos = prog[kRegexNpos];
#if defined(__HIP_DEVICE_COMPILE__)
  npos = (uint32_t)__builtin_amdgcn_readfirstlane((int)npos);  // (wave-uniform already)
#endif
  // (an empty key: B[0] is 0, so S is; the answer below is `nullable`)
  uint32_t S = prog[kRegexFirst] & prog[kRegexB + c0];
  // run: non-zero while this key goes on and its state is alive.  The byte loop runs on a
  // scalar counter until no lane of the wave has anything left, and a lane whose key has ended
  // keeps its state by a select: no per-lane loop mask stays alive.  The four words shift along
  // as one register of 32 bytes, so the next byte always stands on top of k0: no word is
  // selected, no shift count computed.
  uint32_t run = S;
#pragma unroll 1
  for (;;) {  // (ends: after kKeyBytes - 1 shifts at the latest every byte is 0, and run with it)
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_amdgcn_ballot_w64(run != 0u) == 0ull) break;  // (wave-uniform)
#else
    if (run == 0u) break;
#endif
    k0 = (k0 << 8) | (k1 >> 56);
    k1 = (k1 << 8) | (k2 >> 56);
    k2 = (k2 << 8) | (k3 >> 56);
    k3 <<= 8;
    const uint32_t c = (uint32_t)(k0 >> 56);  // (0: the key has ended, and stays ended)
    uint32_t T = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < npos; ++i)  // (uniform) bit i of S set: its followers
      T |= (0u - ((S >> i) & 1u)) & prog[kRegexFollow + i];
    const uint32_t N = T & prog[kRegexB + c];
    S = c ? N : S;
    run = c ? N : 0u;
  }
  return c0 ? (S & prog[kRegexLast]) != 0u : prog[kRegexNullable] != 0u;
}

LOCUST_HD inline bool regex_match(const uint32_t* prog, const uint64_t* k) {
  return regex_match(prog, k[0], k[1], k[2], k[3]);
}

}  // namespace locust
