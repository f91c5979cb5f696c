// The show stage of a search batch (kernels.hpp "show.hip"; the rule is engine.hpp "show"):
// for every returned line of every query, the line's first N bytes and the byte spans of its
// emitted tokens that match a positive term of that entry's query.  The text, the line starts,
// the batch's keys and the returned lines are all resident beside the index; only the gathered
// lines and spans cross PCIe.
//
// Shape (gfx950, wave64): the verify kernels' skeleton (search.hip).  One wave per entry, up to
// 64 consecutive entries per wave and round; lane i keeps entry i's line and finds its query
// by a binary search in the per-query offsets.  The wave walks the line 64 bytes per step
// with index.hip's tokeniser (device/linetok.hpp) and asks token_term_mask
// (device/termmask.hpp) of every emitted token.  Two walks with a scan between them:
//  * measure: per entry the number of spans (ballot + popcount per step) and min(length, N);
//  * show_scan_kernel: one workgroup, exclusive u64 scans of both arrays;
//  * write: the same walk.  The step's matching lanes write their triples at span_off[i] +
//    (spans so far) + lanes_below, the step's bytes go out as the wave loaded them.  A token
//    that reaches the step's last byte stays open -- wave-uniform state: where its triple
//    lies and its length so far -- and the step that holds its end (a ballot's trailing ones)
//    or the line's end writes its length.  No per-lane byte loop, no atomics on the output.
// A batch with a pattern term runs the siblings compiled with the matcher.
#include <algorithm>

#include "locust/device/termmask.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;
constexpr int kShowBlock = 256;
constexpr int kShowWaves = kShowBlock / 64;
constexpr int kShowMaxBlocks = 2048;  // 8 workgroups per CU, as the verify kernels
constexpr int kScanBlock = 512;
constexpr int kScanItems = 8;  // consecutive entries per thread and tile

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
  const u32* pq;       // the batch's pattern flags and maps (the glob siblings)
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

template <bool kGlob, bool kWrite>
__device__ __forceinline__ void show_body(unsigned char* row, u64* qk, u32* qm, const ShowJob& j) {
  // row, qk, qm: this wave's LDS -- the line step, the query's term keys and (kGlob) its
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
  if (kGlob) {  // (in_vgprs: room in the scalar file for the matcher)
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
  const DelimMask& dm = j.dm;
  const int lane = dev::lane_id();
  const u32 bytes = (u32)j.bytes;  // (a window holds < 2^32 bytes: the launch's check)
  // (line numbers are u32, and the launch checked bytes > 0: num_nl + 1 lines)
  const u32 num_nl = (u32)j.lctr->num_newlines;
  const u64 E = j.E;
  const u32 Q = j.Q, group = j.group, N = j.show;
  const u32 wave = blockIdx.x * kShowWaves + dev::wave_id();
  // a round of all waves: at most kShowMaxBlocks * kShowWaves * 64 = 2^19 entries
  const u32 stride = gridDim.x * kShowWaves * group;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;  // the lanes below this one
  const u32 EM = (u32)j.emits_per_line;
  for (u64 g0 = (u64)wave * group; g0 < E; g0 += stride) {  // (wave-uniform)
    const u32 cnt = (u32)(g0 + group < E ? group : E - g0);
    // lane i: entry i -- its line, and its query: offsets[q] <= e < offsets[q + 1]
    u32 myq = Q, myline = 0;
    if ((u32)lane < cnt) {
      const u64 e = g0 + lane;
      myline = lines[e] - j.first_line;
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
      const u32 pt = kGlob ? pq[q] : 0u;  // bit j: term j is a pattern term | kSearchFold
      if (q != q_loaded) {  // (wave-uniform) neighbours mostly share their query
        __builtin_amdgcn_wave_barrier();  // the previous entry's key reads are done
        if (lane < kTerms * kKeyWords) qk[lane] = keys[(u64)q * kTerms * kKeyWords + lane];
        if (kGlob && lane < kTerms) qm[lane] = pq[kSearchPatMeta + (u64)q * kTerms + lane];
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
        const unsigned c2 =
            (lane < 32 && 64u + (u32)lane < left) ? (unsigned char)text[(u64)pos + 64 + lane] : 0u;
        const u32 off = pos - start + (u32)lane;
        // (below t_len every byte is the line's: t_len <= its length, which ends at a NUL)
        if (kWrite && off < tl) out[t_at + off] = (char)c;
        __builtin_amdgcn_wave_barrier();  // the previous step's key reads are done
        row[lane] = (unsigned char)c;
        if (lane < 32) row[64 + lane] = (unsigned char)c2;
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
        if (emit) eq = token_term_mask<kGlob>(row, lane, dm, j.max_key_len, qk, m, pre, pt, qm);
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
        if (seen >= EM && !open && (kWrite ? walked >= tl : walked > N)) {
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
      if (bad && lane == 0) atomicAdd(&ctr->mismatch, bad);
    } else {
      if ((u32)lane < cnt) {
        n_spans[g0 + lane] = my_spans;
        t_len[g0 + lane] = my_len;
      }
      const u64 cm = dev::ballot(my_cut);
      if (cm && lane == 0) atomicAdd(&ctr->cut, (u32)__popcll(cm));
    }
  }
}

// The show kernels: the body above, measuring or writing, without and with the matcher.
__global__ __launch_bounds__(kShowBlock) void show_measure_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  show_body<false, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, j);
}

__global__ __launch_bounds__(kShowBlock) void show_write_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  show_body<false, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, j);
}

// ... of a batch that has a pattern term (j.pq: its pattern flags and maps).
__global__ __launch_bounds__(kShowBlock) void show_globmeasure_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<true, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
}

__global__ __launch_bounds__(kShowBlock) void show_globwrite_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<true, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
}

// One workgroup: span_off[0 .. E] and text_off[0 .. E] = the exclusive scans of n_spans and
// t_len, kScanItems consecutive entries per thread and tile, kept in registers; the totals
// also to the counters.  A thread's whole run of entries moves as 16-byte words (every array
// starts 256-byte aligned, a run at a multiple of kScanItems): one workgroup has to hide the
// memory latency of a million entries by itself.
__global__ __launch_bounds__(kScanBlock) void show_scan_kernel(const u32* __restrict__ n_spans,
                                                               const u32* __restrict__ t_len,
                                                               u64 E, u64* __restrict__ span_off,
                                                               u64* __restrict__ text_off,
                                                               ShowCounters* __restrict__ ctr) {
  static_assert(kScanItems == 8, "two 16-byte loads and four 16-byte stores per array and run");
  __shared__ u64 s_scan[kScanBlock / 64 + 1];
  u64 carry_s = 0, carry_t = 0;
  for (u64 base = 0; base < E; base += (u64)kScanBlock * kScanItems) {  // (workgroup-uniform)
    const u64 first = base + (u64)threadIdx.x * kScanItems;
    const bool whole = first + kScanItems <= E;
    u32 ns[kScanItems], tl[kScanItems];
    if (whole) {
      const uint4 a0 = *reinterpret_cast<const uint4*>(n_spans + first);
      const uint4 a1 = *reinterpret_cast<const uint4*>(n_spans + first + 4);
      const uint4 b0 = *reinterpret_cast<const uint4*>(t_len + first);
      const uint4 b1 = *reinterpret_cast<const uint4*>(t_len + first + 4);
      ns[0] = a0.x, ns[1] = a0.y, ns[2] = a0.z, ns[3] = a0.w;
      ns[4] = a1.x, ns[5] = a1.y, ns[6] = a1.z, ns[7] = a1.w;
      tl[0] = b0.x, tl[1] = b0.y, tl[2] = b0.z, tl[3] = b0.w;
      tl[4] = b1.x, tl[5] = b1.y, tl[6] = b1.z, tl[7] = b1.w;
    } else {
#pragma unroll
      for (int k = 0; k < kScanItems; ++k) {
        ns[k] = first + k < E ? n_spans[first + k] : 0u;
        tl[k] = first + k < E ? t_len[first + k] : 0u;
      }
    }
    u64 vs = 0, vt = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      vs += ns[k];
      vt += tl[k];
    }
    u64 ts, tt;
    u64 es = carry_s + dev::block_exclusive_scan<u64, kScanBlock>(vs, s_scan, &ts);
    u64 et = carry_t + dev::block_exclusive_scan<u64, kScanBlock>(vt, s_scan, &tt);
    if (whole) {
#pragma unroll
      for (int k = 0; k < kScanItems; k += 2) {
        ulonglong2 ws, wt;
        ws.x = es;
        wt.x = et;
        ws.y = es + ns[k];
        wt.y = et + tl[k];
        *reinterpret_cast<ulonglong2*>(span_off + first + k) = ws;
        *reinterpret_cast<ulonglong2*>(text_off + first + k) = wt;
        es = ws.y + ns[k + 1];
        et = wt.y + tl[k + 1];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kScanItems; ++k)
        if (first + k < E) {
          span_off[first + k] = es;
          text_off[first + k] = et;
          es += ns[k];
          et += tl[k];
        }
    }
    carry_s += ts;
    carry_t += tt;
  }
  if (threadIdx.x == 0) {
    span_off[E] = carry_s;
    text_off[E] = carry_t;
    ctr->spans = carry_s;
    ctr->text = carry_t;
  }
}

template <class Take>
void entry_layout(u64 entries, Take&& take) {
  take(sizeof(ShowCounters));  // ctr
  take(entries * 4);           // n_spans
  take(entries * 4);           // t_len
  take((entries + 1) * 8);     // span_off
  take((entries + 1) * 8);     // text_off
}

ShowJob make_job(const SearchIndex& ix, const SearchBatch& b, u32 queries, const u32* lines,
                 const u64* offsets, u64 entries, u32 show, const ShowBuffers& sb, u32* blocks) {
  LOCUST_CHECK_ARG(ix.text && ix.nl_pos && ix.lctr && ix.emits_per_line > 0 &&
                       ix.max_key_len > 0 && ix.max_key_len <= kKeyBytes && ix.bytes >= 1 &&
                       ix.bytes < (1ull << 32),
                   "show: the stage needs the index's text view, of less than 2^32 bytes");
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && entries >= 1 &&
                       entries <= sb.cap_entries && show >= 1 && show <= kShowMaxBytes,
                   "show: " + std::to_string(entries) + " entries of " + std::to_string(queries) +
                       " queries, N = " + std::to_string(show) + ", exceed the workspace (" +
                       std::to_string(sb.cap_entries) + " entries)");
  ShowJob j{};
  j.text = ix.text;
  j.bytes = ix.bytes;
  j.nl_pos = ix.nl_pos;
  j.lctr = ix.lctr;
  j.dm = ix.dm;
  j.emits_per_line = ix.emits_per_line;
  j.max_key_len = ix.max_key_len;
  // one entry per wave while they are few, up to 64 per wave and round (as the verify kernels)
  j.group = (u32)std::min<u64>(div_up(entries, (u64)kShowMaxBlocks), 64);
  *blocks = (u32)std::min<u64>(div_up(div_up(entries, (u64)j.group), (u64)kShowWaves),
                               (u64)kShowMaxBlocks);
  j.Q = queries;
  j.first_line = ix.first_line;
  j.show = show;
  j.q_meta = b.q_meta;
  j.keys = b.keys;
  j.pq = b.pat;
  j.lines = lines;
  j.offsets = offsets;
  j.E = entries;
  j.ctr = sb.ctr;
  j.n_spans = sb.n_spans;
  j.t_len = sb.t_len;
  j.span_off = sb.span_off;
  j.text_off = sb.text_off;
  j.spans = sb.spans;
  j.out = sb.text;
  return j;
}

}  // namespace

u64 show_entry_bytes(u64 entries) {
  u64 b = 0;
  entry_layout(entries, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void show_entry_carve(char* base, u64 entries, ShowBuffers* sb) {
  char* part[5];
  int k = 0;
  u64 b = 0;
  entry_layout(entries, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  sb->ctr = reinterpret_cast<ShowCounters*>(part[0]);
  sb->n_spans = reinterpret_cast<u32*>(part[1]);
  sb->t_len = reinterpret_cast<u32*>(part[2]);
  sb->span_off = reinterpret_cast<u64*>(part[3]);
  sb->text_off = reinterpret_cast<u64*>(part[4]);
  sb->cap_entries = entries;
}

void launch_show_measure(const SearchIndex& ix, const SearchBatch& b, u32 queries,
                         const u32* lines, const u64* offsets, u64 entries, u32 show,
                         const ShowBuffers& sb, hipStream_t s) {
  u32 blocks = 0;
  const ShowJob j = make_job(ix, b, queries, lines, offsets, entries, show, sb, &blocks);
  LOCUST_HIP_CHECK(hipMemsetAsync(sb.ctr, 0, sizeof(ShowCounters), s));
  if (b.pat)  // (a batch that has a pattern term: the sibling with the matcher)
    show_globmeasure_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  else
    show_measure_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  LOCUST_HIP_LAUNCH_CHECK();
  show_scan_kernel<<<dim3(1), dim3(kScanBlock), 0, s>>>(sb.n_spans, sb.t_len, entries, sb.span_off,
                                                        sb.text_off, sb.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_show_write(const SearchIndex& ix, const SearchBatch& b, u32 queries, const u32* lines,
                       const u64* offsets, u64 entries, const ShowBuffers& sb, hipStream_t s) {
  u32 blocks = 0;
  // (N = 1: write takes every length from text_off)
  const ShowJob j = make_job(ix, b, queries, lines, offsets, entries, 1, sb, &blocks);
  LOCUST_CHECK_ARG(sb.text && sb.spans, "show: the payload buffers are missing");
  if (b.pat)
    show_globwrite_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  else
    show_write_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_show() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&show_measure_kernel));
}

}  // namespace locust
