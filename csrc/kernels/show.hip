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
// A batch with a pattern term runs the siblings compiled with the matcher; one with a fuzzy term
// runs fuzzy.hip's (launch_fuzzy_show), one with a regex term regex.hip's (launch_regex_show).
#include <algorithm>

#include "locust/device/showwalk.hpp"
#include "locust/device/termmask.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;
constexpr int kScanBlock = 512;
constexpr int kScanItems = 8;  // consecutive entries per thread and tile

// The show kernels: the walk (device/showwalk.hpp), measuring or writing, without and with the
// matcher.
__global__ __launch_bounds__(kShowBlock) void show_measure_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  show_body<0, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, j);
}

__global__ __launch_bounds__(kShowBlock) void show_write_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  show_body<0, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, j);
}

// ... of a batch that has a pattern term (j.pq: its pattern flags and maps).
__global__ __launch_bounds__(kShowBlock) void show_globmeasure_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<1, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
}

__global__ __launch_bounds__(kShowBlock) void show_globwrite_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<1, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
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
  if (b.regex)  // (a batch that has a regex term: regex.hip's sibling)
    launch_regex_show(j, b.regex, blocks, false, s);
  else if (b.fuzzy)  // (a batch that has a fuzzy term: fuzzy.hip's sibling)
    launch_fuzzy_show(j, blocks, false, s);
  else if (b.pat)  // (a batch that has a pattern term: the sibling with the matcher)
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
  if (b.regex)
    launch_regex_show(j, b.regex, blocks, true, s);
  else if (b.fuzzy)
    launch_fuzzy_show(j, blocks, true, s);
  else if (b.pat)
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
