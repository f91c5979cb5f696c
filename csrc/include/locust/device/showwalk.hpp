// The show stage's walk (kernels.hpp "show.hip": measure, write): the body of its kernels,
// compiled per matcher level -- show.hip's kernels without a matcher (kMatch 0) and with the
// pattern matcher (1), fuzzy.hip's with the fuzzy matcher beside it (2), regex.hip's with the
// regex matcher as well (3; they take the program table beside it) -- and the one argument they
// take.
#pragma once

#include "locust/device/termmask.hpp"
#include "locust/device/wave.hpp"
#include "locust/kernels.hpp"

namespace locust {

constexpr int kShowBlock = 256;
constexpr int kShowWaves = kShowBlock / 64;
constexpr int kShowMaxBlocks = 2048;  // 8 workgroups per CU, as the verify kernels

// What a show kernel reads and writes (one kernel argument).
struct ShowJob {
  const char* text;
  u64 bytes;
  const u64* nl_pos;
  const MapCounters* lctr;
  DelimMask dm;
  int emits_per_line, max_key_len;
  u32 group, Q, first_line, show;
  const u32* q_meta;
  const u64* keys;
  const u32* pq;       // the batch's pattern flags and maps (the glob and fuzzy siblings)
  const u32* lines;    // [E] the returned lines, global numbers
  const u64* offsets;  // [Q + 1] their per-query segments
  u64 E;
  ShowCounters* ctr;
  u32* n_spans;        // measure writes, the scan reads
  u32* t_len;
  const u64* span_off;  // write reads
  const u64* text_off;
  u32* spans;
  char* out;
};

// fuzzy.hip's siblings of the show kernels (kernels.hpp "fuzzy.hip"): the measure or the write
// walk of job j over `blocks` workgroups, for a batch that has a fuzzy term.
void launch_fuzzy_show(const ShowJob& j, u32 blocks, bool write, hipStream_t s);
// regex.hip's (kernels.hpp "regex.hip"), for a batch that has a regex term; rx: its program table.
void launch_regex_show(const ShowJob& j, const u32* rx, u32 blocks, bool write, hipStream_t s);

template <int kMatch, bool kWrite>
__device__ __forceinline__ void show_body(unsigned char* row, u64* qk, u32* qm, const ShowJob& j,
                                          const u32* __restrict__ rx = nullptr) {
  constexpr int kTerms = (int)kSearchMaxTerms;
  // row, qk, qm: this wave's LDS -- the line step, the query's term keys and (kMatch) its
  // pattern terms' metacharacter maps
  const char* __restrict__ text = j.text;
  const u64* __restrict__ nl_pos = j.nl_pos;
  const u32* __restrict__ q_meta = j.q_meta;
  const u64* __restrict__ keys = j.keys;
  const u32* __restrict__ pq = j.pq;
  const u32* __restrict__ lines = j.lines;
  const u64* __restrict__ offsets = j.offsets;
  const u64* __restrict__ span_off = j.span_off;
  const u64* __restrict__ text_off = j.text_off;
  u32* __restrict__ spans = j.spans;
  char* __restrict__ out = j.out;
  u32* __restrict__ n_spans = j.n_spans;
  u32* __restrict__ t_len = j.t_len;
  ShowCounters* __restrict__ ctr = j.ctr;
  if (kMatch) {  // (in_vgprs: room in the scalar file for the matcher)
    pq = in_vgprs(pq);
    nl_pos = in_vgprs(nl_pos);
    q_meta = in_vgprs(q_meta);
    keys = in_vgprs(keys);
    lines = in_vgprs(lines);
    offsets = in_vgprs(offsets);
    span_off = in_vgprs(span_off);
    text_off = in_vgprs(text_off);
    spans = in_vgprs(spans);
    out = in_vgprs(out);
    n_spans = in_vgprs(n_spans);
    t_len = in_vgprs(t_len);
    ctr = in_vgprs(ctr);
  }
  int max_key_len = j.max_key_len;
  u32 first_line = j.first_line;
  if (kMatch >= 2) {  // (two matchers in the term loop: more room still)
    text = in_vgprs(text);
    max_key_len = value_in_vgprs(max_key_len);
    first_line = value_in_vgprs(first_line);
  }
  if (kMatch == 3) rx = in_vgprs(rx);  // (three: the program table leaves the scalar file, too)
  const DelimMask& dm = j.dm;
  const int lane = dev::lane_id();
  const u32 bytes = (u32)j.bytes;  // (a window holds < 2^32 bytes: the launch's check)
  // (line numbers are u32, and the launch checked bytes > 0: num_nl + 1 lines)
  const u32 num_nl = (u32)j.lctr->num_newlines;
  const u64 E = j.E;
  // (the fuzzy siblings park N and the emit cap, too)
  const u32 Q = j.Q, group = j.group, N = parked<kMatch >= 2>(j.show);
  const u32 wave = blockIdx.x * kShowWaves + dev::wave_id();
  // a round of all waves: at most kShowMaxBlocks * kShowWaves * 64 = 2^19 entries
  const u32 stride = gridDim.x * kShowWaves * group;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 EM = parked<kMatch >= 2>((u32)j.emits_per_line);
  for (u64 g0 = (u64)wave * group; g0 < E; g0 += stride) {  // (wave-uniform)
    const u32 cnt = (u32)(g0 + group < E ? group : E - g0);
    // lane i: entry i -- its line, and its query: offsets[q] <= e < offsets[q + 1]
    u32 myq = Q, myline = 0;
    if ((u32)lane < cnt) {
      const u64 e = g0 + lane;
      myline = lines[e] - first_line;
      u32 lo = 0, hi = Q;
      while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= e)
          lo = mid;
        else
          hi = mid;
      }
      myq = lo;
    }
    u32 my_spans = 0, my_len = 0;  // measure: lane i keeps entry i's figures
    bool my_cut = false;
    u32 bad = 0;           // write: entries whose spans do not number what measure counted
    u32 q_loaded = ~0u;    // the query whose term keys the wave's LDS row holds
    for (u32 i = 0; i < cnt; ++i) {
      const u32 q = (u32)__shfl((int)myq, (int)i, 64);
      const u32 line = (u32)__shfl((int)myline, (int)i, 64);
      if (q >= Q || line > num_nl) continue;  // (wave-uniform; never: the search's own lines)
      const u32 meta = q_meta[q];
      // the positive terms, which stand first: exclusion terms never produce a span
      const u32 m = (meta & 0xffu) - (u32)__popc(meta >> kSearchExcludeShift);
      if (m == 0 || m > (u32)kTerms) continue;  // (never: the host checked the batch)
      const u32 pre = (meta >> kSearchPrefixShift) & 0xffu;  // bit j: term j is a prefix term
      const u32 pt = kMatch ? pq[q] : 0u;  // bit j: term j is a pattern term | kSearchFold
      if (q != q_loaded) {  // (wave-uniform) neighbours mostly share their query
        __builtin_amdgcn_wave_barrier();  // the previous entry's key reads are done
        const int ql = lane_here<kMatch == 3>(lane);
        if (ql < kTerms * kKeyWords) qk[ql] = keys[(u64)q * kTerms * kKeyWords + ql];
        if (kMatch && ql < kTerms) qm[ql] = pq[kSearchPatMeta + (u64)q * kTerms + ql];
        __builtin_amdgcn_wave_barrier();
        q_loaded = q;
      }
      const u32 start = line ? (u32)nl_pos[line - 1] + 1u : 0u;
      const u32 end = line < num_nl ? (u32)nl_pos[line] : bytes;
      // write: where the entry's spans and bytes go, and how many measure counted
      u64 s_at = 0, s_end = 0, t_at = 0;
      u32 tl = 0;
      if (kWrite) {
        s_at = span_off[g0 + i];
        s_end = span_off[g0 + i + 1];
        t_at = text_off[g0 + i];
        tl = (u32)(text_off[g0 + i + 1] - t_at);  // (<= N)
      }
      u32 len = end - start;  // the line's length, unless a NUL (or the early end) cuts it
      u32 seen = 0;           // token starts of this line before the current step
      u32 nsp = 0;            // spans of this line before the current step
      u64 carry = 0;
      bool open = false;  // a matching token of an earlier step has not ended yet:
      u32 open_len = 0;   // its bytes so far,
      u64 open_at = 0;    // and its triple
      for (u32 pos = start; pos < end; pos += 64u) {
        const u32 left = end - pos;  // (>= 1)
        const unsigned c = (u32)lane < left ? (unsigned char)text[(u64)pos + lane] : 0u;
        const int sl = lane_here<kMatch == 3>(lane);  // (a step's own compares with 32)
        const unsigned c2 =
            (sl < 32 && 64u + (u32)lane < left) ? (unsigned char)text[(u64)pos + 64 + lane] : 0u;
        const u32 off = pos - start + (u32)lane;
        // (below t_len every byte is the line's: t_len <= its length, which ends at a NUL)
        if (kWrite && off < tl) out[t_at + off] = (char)c;
        __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
        row[lane] = (unsigned char)c;
        if (sl < 32) row[64 + lane] = (unsigned char)c2;
        __builtin_amdgcn_wave_barrier();
        // dev::step_starts, with the token bytes kept: they give the tokens' ends
        const u64 z = dev::ballot(c == 0u);
        u64 tm = dev::ballot(c != 0u && !mask_is_delim(dm, c));
        if (z) tm &= (z & (~z + 1)) - 1;  // nothing at or behind the first NUL (or the end)
        const u64 starts = tm & ~((tm << 1) | carry);
        carry = tm >> 63;
        if (open) {  // (wave-uniform) the open token goes on for the step's leading token bytes
          const u32 lead = tm == ~0ull ? 64u : (u32)__ffsll((unsigned long long)~tm) - 1u;
          open_len += lead;
          if (lead < 64u) {
            if (kWrite && lane == 0 && open_at < s_end) spans[open_at * 3 + 1] = open_len;
            open = false;
          }
        }
        const u32 ord = seen + (u32)__popcll(starts & below);
        const bool emit = ((starts >> lane) & 1ull) && ord < EM;
        u32 eq = 0;  // bit t: this lane's token matches term t
        if (emit) eq = token_term_mask<kMatch>(row, lane, dm, max_key_len, qk, m, pre, pt, qm, rx);
        const u64 mm = dev::ballot(eq != 0u);
        if (mm) {  // (wave-uniform)
          // the token's end: the first byte at or behind its start that is no token byte
          const u64 rest = ~tm & (~0ull << lane);
          if (kWrite && eq != 0u) {
            const u64 at = s_at + nsp + dev::lanes_below(mm);
            if (at < s_end) {
              spans[at * 3] = off;
              // (a token that reaches the step's last byte: the closing step writes its length)
              if (rest) spans[at * 3 + 1] = (u32)__ffsll((unsigned long long)rest) - 1u - (u32)lane;
              spans[at * 3 + 2] = eq;
            }
          }
          // the step's last matching token is open when token bytes fill the step behind it
          const int hl = 63 - __clzll((long long)mm);
          if ((tm >> hl) == (~0ull >> hl)) {
            open = true;
            open_len = 64u - (u32)hl;
            open_at = s_at + nsp + (u32)__popcll(mm) - 1u;
          }
          nsp += (u32)__popcll(mm);
        }
        seen += (u32)__popcll(starts);
        if (z) {  // a NUL, or the line end, inside this step
          len = pos - start + (u32)__ffsll((unsigned long long)z) - 1u;
          break;
        }
        // every token that can match has ended, and enough of the line is known: measure
        // needs byte N to tell a cut line, write the bytes below t_len
        if (left <= 64u) break;  // the line ends with the step
        const u32 walked = pos - start + 64u;
        if (seen >= unparked<kMatch >= 2>(EM) && !open &&
            (kWrite ? walked >= tl : walked > unparked<kMatch >= 2>(N))) {
          len = walked;  // (N < walked < the line's length: the line is cut)
          break;
        }
      }
      // the line ended with the open token
      if (kWrite && open && lane == 0 && open_at < s_end) spans[open_at * 3 + 1] = open_len;
      if (kWrite) {
        bad += s_at + nsp != s_end ? 1u : 0u;
      } else if ((u32)lane == i) {
        my_spans = nsp;
        my_len = (u32)(len < N ? len : N);
        my_cut = len > N;
      }
    }
    if (kWrite) {
      if (bad && lane_here<kMatch == 3>(lane) == 0) atomicAdd(&ctr->mismatch, bad);
    } else {
      if ((u32)lane < cnt) {
        n_spans[g0 + lane] = my_spans;
        t_len[g0 + lane] = my_len;
      }
      const u64 cm = dev::ballot(my_cut);
      if (cm && lane_here<kMatch == 3>(lane) == 0) atomicAdd(&ctr->cut, (u32)__popcll(cm));
    }
  }
}

}  // namespace locust
