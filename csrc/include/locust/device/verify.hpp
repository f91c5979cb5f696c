// The verify stage of a search batch (kernels.hpp "search.hip": phrase, near): the bodies of the
// two kernels that walk a candidate line against its query's terms, compiled per matcher level
// -- search.hip's kernels without a matcher (kMatch 0) and with the pattern matcher (1),
// fuzzy.hip's with the fuzzy matcher beside it (2), regex.hip's with the regex matcher as well
// (3) -- how a converged wave commits its hits, and how the hit kernels (search.hip, expr.hip)
// read a term's list.
#pragma once

#include <algorithm>

#include "locust/device/linetok.hpp"
#include "locust/device/termmask.hpp"
#include "locust/device/wave.hpp"
#include "locust/kernels.hpp"

namespace locust {

constexpr int kPhraseBlock = 256;
constexpr int kPhraseWaves = kPhraseBlock / 64;
constexpr int kPhraseMaxBlocks = 2048;  // 8 workgroups per CU

// The hits of one converged wave step (hit: this lane has one, of query q on local line
// rel_line): one atomic reserves the step's slots in `pairs`, one atomic per distinct query
// of the wave adds to its hit count.
__device__ __forceinline__ void commit_hits(bool hit, u32 q, u32 rel_line, u64* __restrict__ pairs,
                                            u64 pair_cap, u32* __restrict__ q_hits,
                                            SearchCounters* __restrict__ ctr) {
  const int lane = dev::lane_id();
  const u64 hm = dev::ballot(hit);
  if (hm == 0) return;  // (wave-uniform)
  const int first = __ffsll((unsigned long long)hm) - 1;
  u32 at = 0;
  if (lane == first) at = atomicAdd(&ctr->written, (u32)__popcll(hm));
  at = (u32)__shfl((int)at, first, 64);
  if (hit) {
    const u64 slot = (u64)at + dev::lanes_below(hm);
    if (slot < pair_cap) pairs[slot] = ((u64)q << 32) | (u64)rel_line;
  }
  // per query: one atomic for all of the wave's hits of that query
  u64 rem = hm;
  while (rem) {  // (wave-uniform)
    const int leader = __ffsll((unsigned long long)rem) - 1;
    const u32 ql = (u32)__shfl((int)q, leader, 64);
    const u64 same = dev::ballot(hit && q == ql);
    if (lane == leader) atomicAdd(&q_hits[ql], (u32)__popcll(same));
    rem &= ~same;
  }
}

// Is `line` among the len sorted postings at p?  (Never reads outside [p, p + len).)
__device__ __forceinline__ bool list_has(const u32* __restrict__ p, u32 len, u32 line) {
  u32 lo = 0, hi = len;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (p[mid] < line)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < len && p[lo] == line;
}

// A term's list: at its CSR offset in the postings, or (kSearchMerged, a prefix term of two
// or more words behind the expand stage) at its offset in `merged`.  Either way t_len
// elements, and list_has / list_tf stay inside them.
__device__ __forceinline__ const u32* term_list(const u32* __restrict__ postings,
                                                const u32* __restrict__ merged, u64 tv) {
  return ((tv & kSearchMerged) ? merged : postings) + (tv & ~kSearchMerged);
}

// One wave per candidate; a wave takes `group` (<= 64) consecutive candidates per round,
// grid-stride over the rounds.  The candidates' number comes from device memory (the hit
// kernel's counter): no host round trip between the two kernels.  Lane i keeps candidate
// i's verdict, so a round ends like a step of the hit kernel: ONE atomic for its slots and
// one per distinct query -- one atomic per verified line would serialise on ctr->written as
// index_map_kernel's comment (index.hip) records for 10^6 lines.
template <int kMatch>
__device__ __forceinline__ void search_phrase_body(
    unsigned char* row, u64* qk, u32* qm, const u32* __restrict__ pq,
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, const DelimMask& dm, int emits_per_line,
    int max_key_len, u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys,
    u32 Q, const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr,
    const u32* __restrict__ rx = nullptr) {
  constexpr int kTerms = (int)kSearchMaxTerms;
  // row, qk, qm: this wave's LDS -- the line step, the query's term keys and (kMatch) its
  // pattern terms' metacharacter maps; pq: the batch's pattern flags and maps (kMatch)
  if (kMatch) {  // (in_vgprs: room in the scalar file for the matcher)
    pq = in_vgprs(pq);
    nl_pos = in_vgprs(nl_pos);
    q_meta = in_vgprs(q_meta);
    keys = in_vgprs(keys);
    cands = in_vgprs(cands);
    pairs = in_vgprs(pairs);
    q_hits = in_vgprs(q_hits);
    ctr = in_vgprs(ctr);
    lctr = in_vgprs(lctr);
  }
  if (kMatch >= 2) {  // (two matchers in the term loop: more room still)
    text = in_vgprs(text);
  }
  if (kMatch == 3) rx = in_vgprs(rx);  // (three: the program table leaves the scalar file, too)
  const int lane = dev::lane_id();
  const u64 num_nl = lctr->num_newlines;
  const u64 num_lines = bytes ? num_nl + 1 : 0;
  const u64 C = ctr->cands <= pair_cap ? ctr->cands : 0;  // (an overflow: the host throws)
  if (kMatch >= 2) {  // (from here on only lanes compare with pair_cap; Q is read back)
    pair_cap = value_in_vgprs(pair_cap);
    Q = parked<true>(Q);
  }
  const u64 wave = (u64)blockIdx.x * kPhraseWaves + dev::wave_id();
  const u64 nwaves = (u64)gridDim.x * kPhraseWaves;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 E = parked<kMatch >= 2>((u32)emits_per_line);  // (the fuzzy siblings park the cap)
  // Level 3 parks what only a round reads -- its stride, its end, its group size -- in vector
  // registers and reads them back once per round (parked64 / unparked64, device/termmask.hpp);
  // below level 3 these are the values themselves.  Only this body does: without it the level-3
  // phrase kernel spills scalar registers, while the near body, whose per-term state lives in
  // lanes, compiles without spills as it stands (profiles/regex/resources.txt).
  const u64 stride_p = parked64<kMatch == 3>(nwaves * group), end_p = parked64<kMatch == 3>(C);
  const u32 group_p = parked<kMatch == 3>(group);
  if (kMatch == 3) max_key_len = value_in_vgprs(max_key_len);
  for (u64 g0 = wave * group; g0 < unparked64<kMatch == 3>(end_p);
       g0 += unparked64<kMatch == 3>(stride_p)) {  // (wave-uniform)
    const u64 round_end = unparked64<kMatch == 3>(end_p);
    const u32 round_group = unparked<kMatch == 3>(group_p);
    const u32 cnt = (u32)(g0 + round_group < round_end ? round_group : round_end - g0);
    const u64 mine = (u32)lane < cnt ? cands[g0 + lane] : 0ull;  // lane i: candidate i
    bool hit = false;
    u32 q_loaded = ~0u;  // the query whose term keys the wave's LDS row holds
    for (u32 i = 0; i < cnt; ++i) {
      const u32 q = (u32)__shfl((int)(u32)(mine >> 32), (int)i, 64);
      const u64 line = (u32)__shfl((int)(u32)mine, (int)i, 64);
      // (wave-uniform; never: the hit kernel's words)
      if (q >= unparked<kMatch >= 2>(Q) || line >= num_lines) continue;
      const u32 meta = q_meta[q];
      // the positive terms, which stand first: exclusion terms are no part of the match
      const u32 m = (meta & 0xffu) - (u32)__popc(meta >> kSearchExcludeShift);
      if (m == 0 || m > (u32)kTerms) continue;    // (never: the host checked the batch)
      const u32 pre = (meta >> kSearchPrefixShift) & 0xffu;  // bit j: term j is a prefix term
      const u32 pt = kMatch ? pq[q] : 0u;  // bit j: term j is a pattern term | kSearchFold
      if (q != q_loaded) {  // (wave-uniform) neighbours mostly share their query
        __builtin_amdgcn_wave_barrier();  // the previous candidate's key reads are done
        const int ql = lane_here<kMatch == 3>(lane);
        if (ql < kTerms * kKeyWords) qk[ql] = keys[(u64)q * kTerms * kKeyWords + ql];
        if (kMatch && ql < kTerms) qm[ql] = pq[kSearchPatMeta + (u64)q * kTerms + ql];
        __builtin_amdgcn_wave_barrier();
        q_loaded = q;
      }
      const u64 start = line ? nl_pos[line - 1] + 1 : 0;
      const u64 end = line < num_nl ? nl_pos[line] : bytes;
      const u32 accept = 1u << (m - 1);
      u32 seen = 0;   // token starts of this line before the current step
      u32 state = 0;  // bit j: the last j + 1 tokens equal terms 0 .. j
      u64 carry = 0;
      bool match = false;
      for (u64 pos = start; pos < end && seen < unparked<kMatch >= 2>(E) && !match; pos += 64) {
        const u64 p = pos + lane;
        const unsigned c = p < end ? (unsigned char)text[p] : 0u;
        const u64 p2 = pos + 64 + lane;
        const int sl = lane_here<kMatch == 3>(lane);  // (a step's own compares with 32)
        const unsigned c2 = (sl < 32 && p2 < end) ? (unsigned char)text[p2] : 0u;
        __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
        row[lane] = (unsigned char)c;
        if (sl < 32) row[64 + lane] = (unsigned char)c2;
        __builtin_amdgcn_wave_barrier();
        bool last;
        const u64 starts = dev::step_starts(c, dm, &carry, &last);
        const u32 ord = seen + (u32)__popcll(starts & below);
        const bool emit = ((starts >> lane) & 1ull) && ord < E;
        u32 eq = 0;  // bit j: this lane's token equals term j
        if (emit) eq = token_term_mask<kMatch>(row, lane, dm, max_key_len, qk, m, pre, pt, qm, rx);
        // the automaton over the step's emitted tokens in order (all wave-uniform)
        u64 em = dev::ballot(emit);
        if (dev::ballot(eq != 0u) == 0) {
          if (em) state = 0;  // no token of this step equals any term
        } else {
          while (em) {
            const int tl = __ffsll((unsigned long long)em) - 1;
            const u32 e = (u32)__shfl((int)eq, tl, 64);
            state = ((state << 1) | 1u) & e;
            if (state & accept) {
              match = true;
              break;
            }
            em &= em - 1;
          }
        }
        seen += (u32)__popcll(starts);
        if (last) break;  // a NUL, or the line end, inside this step
      }
      if ((u32)lane == i) hit = match;
    }
    if (lane_here<kMatch == 3>(lane) == 0) atomicAdd(&ctr->verified, cnt);
    commit_hits(hit, (u32)(mine >> 32), (u32)mine, pairs, pair_cap, q_hits, ctr);
  }
}

// The phrase kernel's sibling for `near` queries (engine.hpp "index search"): the same rounds
// over the near candidates, which the hit kernel wrote from cands[pair_cap - 1] downwards,
// the same walk and the same token masks.  In place of the automaton: per term the ordinal
// of the last token that matched it.  Lane j < 8 keeps term j's in one register (updated by
// a select: no indexing, no scratch; 0: not seen yet); eight scalars and a set of seen terms
// instead cost 104 SGPRs and a wave of occupancy.  Only the step's tokens whose mask is
// non-zero are walked, in order; behind each, the minimum over lanes 0 .. 7 (three DPP
// steps) tells whether every term has been seen and where the shortest covering window that
// ends there starts: the line matches when ord - min < W.  (A minimal covering window always
// ends at a matching token.)  The state carries across the 64-byte steps; ordinals and W
// are full u32.
template <int kMatch>
__device__ __forceinline__ void search_near_body(
    unsigned char* row, u64* qk, u32* qm, const u32* __restrict__ pq,
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, const DelimMask& dm, int emits_per_line,
    int max_key_len, u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys,
    u32 Q, const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr,
    const u32* __restrict__ rx = nullptr) {
  constexpr int kTerms = (int)kSearchMaxTerms;
  // row, qk, qm: this wave's LDS -- the line step, the query's term keys and (kMatch) its
  // pattern terms' metacharacter maps; pq: the batch's pattern flags and maps (kMatch)
  if (kMatch) {  // (in_vgprs: room in the scalar file for the matcher)
    pq = in_vgprs(pq);
    nl_pos = in_vgprs(nl_pos);
    q_meta = in_vgprs(q_meta);
    keys = in_vgprs(keys);
    cands = in_vgprs(cands);
    pairs = in_vgprs(pairs);
    q_hits = in_vgprs(q_hits);
    ctr = in_vgprs(ctr);
    lctr = in_vgprs(lctr);
  }
  if (kMatch >= 2) {  // (two matchers in the term loop: more room still)
    text = in_vgprs(text);
  }
  if (kMatch == 3) rx = in_vgprs(rx);  // (three: the program table leaves the scalar file, too)
  const int lane = dev::lane_id();
  const u64 num_nl = lctr->num_newlines;  // (bytes > 0, the launch's check: num_nl + 1 lines)
  const u32 C = ctr->ncands <= pair_cap ? ctr->ncands : 0u;  // (an overflow: the host throws)
  if (kMatch >= 2) pair_cap = value_in_vgprs(pair_cap);  // (from here on only lanes read it)
  const u32 wave = blockIdx.x * kPhraseWaves + dev::wave_id();
  // a round of all waves: at most kPhraseMaxBlocks * kPhraseWaves * 64 = 2^19 candidates
  const u32 stride = gridDim.x * kPhraseWaves * group;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 E = parked<kMatch >= 2>((u32)emits_per_line);  // (the fuzzy siblings park the cap)
  for (u64 g0 = (u64)wave * group; g0 < C; g0 += stride) {  // (wave-uniform)
    const u32 cnt = (u32)(g0 + group < C ? group : C - g0);
    // lane i: candidate i (g0 + lane < C <= pair_cap: inside cands)
    const u64 mine = (u32)lane < cnt ? cands[pair_cap - 1 - (g0 + lane)] : 0ull;
    bool hit = false;
    u32 q_loaded = ~0u;  // the query whose term keys the wave's LDS row holds
    for (u32 i = 0; i < cnt; ++i) {
      const u32 q = (u32)__shfl((int)(u32)(mine >> 32), (int)i, 64);
      const u64 line = (u32)__shfl((int)(u32)mine, (int)i, 64);
      if (q >= Q || line > num_nl) continue;  // (wave-uniform; never: the hit kernel's words)
      const u32 meta = q_meta[q];
      // the positive terms, which stand first: exclusion terms are no part of the match
      const u32 m = (meta & 0xffu) - (u32)__popc(meta >> kSearchExcludeShift);
      if (m == 0 || m > (u32)kTerms) continue;    // (never: the host checked the batch)
      const u32 pre = (meta >> kSearchPrefixShift) & 0xffu;  // bit j: term j is a prefix term
      const u32 pt = kMatch ? pq[q] : 0u;  // bit j: term j is a pattern term | kSearchFold
      // the batch's windows stand behind its keys (search_within)
      const u32 W = reinterpret_cast<const u32*>(keys + (u64)Q * kTerms * kKeyWords)[q];
      if (q != q_loaded) {  // (wave-uniform) neighbours mostly share their query
        __builtin_amdgcn_wave_barrier();  // the previous candidate's key reads are done
        const int ql = lane_here<kMatch == 3>(lane);
        if (ql < kTerms * kKeyWords) qk[ql] = keys[(u64)q * kTerms * kKeyWords + ql];
        if (kMatch && ql < kTerms) qm[ql] = pq[kSearchPatMeta + (u64)q * kTerms + ql];
        __builtin_amdgcn_wave_barrier();
        q_loaded = q;
      }
      const u64 start = line ? nl_pos[line - 1] + 1 : 0;
      const u64 end = line < num_nl ? nl_pos[line] : bytes;
      u32 seen = 0;  // token starts of this line before the current step
      // lane j < 8: 1 + the ordinal of the last token that matched term min(j, m - 1) (the
      // lanes behind the query's terms repeat its last one), 0: none yet
      const u32 term = min((u32)(lane & 7), m - 1u);
      u32 lastv = 0;
      u64 carry = 0;
      bool match = false;
      for (u64 pos = start; pos < end && seen < unparked<kMatch >= 2>(E) && !match; pos += 64) {
        const u64 p = pos + lane;
        const unsigned c = p < end ? (unsigned char)text[p] : 0u;
        const u64 p2 = pos + 64 + lane;
        const int sl = lane_here<kMatch == 3>(lane);  // (a step's own compares with 32)
        const unsigned c2 = (sl < 32 && p2 < end) ? (unsigned char)text[p2] : 0u;
        __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
        row[lane] = (unsigned char)c;
        if (sl < 32) row[64 + lane] = (unsigned char)c2;
        __builtin_amdgcn_wave_barrier();
        bool last;
        const u64 starts = dev::step_starts(c, dm, &carry, &last);
        const u32 ord = seen + (u32)__popcll(starts & below);
        const bool emit = ((starts >> lane) & 1ull) && ord < E;
        u32 eq = 0;  // bit j: this lane's token matches term j
        if (emit) eq = token_term_mask<kMatch>(row, lane, dm, max_key_len, qk, m, pre, pt, qm, rx);
        // the step's matching tokens in order (all wave-uniform)
        u64 mm = dev::ballot(eq != 0u);
        while (mm) {
          const int tl = __ffsll((unsigned long long)mm) - 1;
          const u32 e = (u32)__builtin_amdgcn_readlane((int)eq, tl);
          const u32 o = (u32)__builtin_amdgcn_readlane((int)ord, tl);  // its ordinal
          lastv = ((e >> term) & 1u) ? o + 1u : lastv;  // (lanes >= 8: never read)
          // lane 7: the minimum over lanes 0 .. 7 (row_shr 1, 2, 4; a lane without a source
          // reads 0, which never reaches lane 7)
          u32 x = lastv;
          x = min(x, dev::dpp_mov<0x111, 0xf>(x));
          x = min(x, dev::dpp_mov<0x112, 0xf>(x));
          x = min(x, dev::dpp_mov<0x114, 0xf>(x));
          const u32 first = (u32)__builtin_amdgcn_readlane((int)x, 7);
          // every term seen, and the tokens first - 1 .. o are at most W
          if (first != 0u && o + 1u - first < W) {
            match = true;
            break;
          }
          mm &= mm - 1;
        }
        seen += (u32)__popcll(starts);
        if (last) break;  // a NUL, or the line end, inside this step
      }
      if ((u32)lane == i) hit = match;
    }
    if (lane_here<kMatch == 3>(lane) == 0) atomicAdd(&ctr->nverified, cnt);
    commit_hits(hit, (u32)(mine >> 32), (u32)mine, pairs, pair_cap, q_hits, ctr);
  }
}

// The grid of a verify kernel over at most `bound` candidates: one per wave while they are
// few, up to 64 per wave and round when every wave of a full grid has many to walk anyway (as
// launch_index).
inline u32 verify_grid(u64 bound, u32* group) {
  *group = (u32)std::min<u64>(div_up(bound, (u64)kPhraseMaxBlocks), 64);
  return (u32)std::min<u64>(div_up(div_up(bound, (u64)*group), (u64)kPhraseWaves),
                            (u64)kPhraseMaxBlocks);
}

}  // namespace locust
