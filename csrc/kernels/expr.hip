// Boolean expression queries over the inverted index (kernels.hpp "expr.hip"; the semantics are
// engine.hpp "boolean expressions"): `( to AND be ) OR ( Ham* AND NOT Hamlet )`.
//
// A query has at most eight terms, so its expression is a 256-bit truth table the host made:
// no expression tree reaches the device.  The lookup (search.hip) resolves an `expr` query as
// `any` over all its terms; this file adds the two kernels that differ:
//  * expr_plan_kernel: one workgroup, one thread per query (four rounds for a full batch), and
//    the exclusive scan of the queries' bounds in the same pass: a batch with an `expr` query
//    costs one launch more in front of the hits.  Which earlier term has the same list (a wide
//    term that repeats an earlier term's words is never merged: its list is read through the
//    first), the greedy choice of the walked set S from the list lengths, and the query's bound:
//    the summed lengths of S's lists.  "Some mask inside U has its table bit set" needs no walk
//    over masks: a term outside U strikes out half the table, a fixed bit pattern inside every
//    word for the terms 0 .. 4 and whole words for the terms 5 .. 7, so the test is eight
//    masked words, the table in registers;
//  * expr_hit_kernel: search_hit_kernel's shape (gfx950, wave64): the flattened element space
//    [0, E) in tiles of kSearchTile, grid-stride, a binary search for the element's query, and
//    every step ends in commit_hits' wave-level ballots and atomics.  An element that is the
//    first of its line in its list, and whose line no earlier list of S holds, builds the line's
//    mask by binary searches in the other present terms' lists and reads one table bit.
// Data crosses between workgroups only at kernel boundaries; no polled word, no scratch; the only
// LDS is the plan's scan (five words).
#include <algorithm>

#include "locust/device/verify.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;
static_assert(kTerms == 8, "a 256-bit table: eight words, three bits of a term number");

// The table's words, in registers.
struct Table {
  u32 w0, w1, w2, w3, w4, w5, w6, w7;
};

// Does some mask m inside U (a subset of the terms in U) have its table bit set?
__device__ __forceinline__ bool any_inside(const Table& t, u32 U) {
  // the bits of one word whose masks hold none of the terms 0 .. 4 outside U
  u32 low = ~0u;
  low &= (U & 1u) ? ~0u : ~0xaaaaaaaau;
  low &= (U & 2u) ? ~0u : ~0xccccccccu;
  low &= (U & 4u) ? ~0u : ~0xf0f0f0f0u;
  low &= (U & 8u) ? ~0u : ~0xff00ff00u;
  low &= (U & 16u) ? ~0u : ~0xffff0000u;
  // word w holds the masks whose terms 5 .. 7 are w's bits
  const u32 out = ~(U >> 5) & 7u;
  u32 acc = 0;
  acc |= (0u & out) ? 0u : t.w0;
  acc |= (1u & out) ? 0u : t.w1;
  acc |= (2u & out) ? 0u : t.w2;
  acc |= (3u & out) ? 0u : t.w3;
  acc |= (4u & out) ? 0u : t.w4;
  acc |= (5u & out) ? 0u : t.w5;
  acc |= (6u & out) ? 0u : t.w6;
  acc |= (7u & out) ? 0u : t.w7;
  return (acc & low) != 0u;
}

// One `expr` query's plan: plan | src into the expression arrays, 0 into the shared bound; the
// elements it walks come back.
__device__ __forceinline__ u32 plan_query(u32 q, u32 meta, const u64* __restrict__ t_val,
                                          const u32* __restrict__ t_len, u32* __restrict__ ex,
                                          u32* __restrict__ q_bound,
                                          SearchCounters* __restrict__ ctr) {
  const u32 nterms = min(meta & 0xffu, (u32)kTerms);
  const u32 alias = ex[kExprAlias + q];
  const u32 pslots = alias >> 24;  // the query's pattern slots
  const u64* tv = t_val + (u64)q * kTerms;
  const u32* tl = t_len + (u64)q * kTerms;
  // the present terms, and per term the first term with its list
  u32 present = 0, src = 0;
  for (u32 t = 0; t < nterms; ++t) {
    const u32 len = tl[t];
    u32 s = t;
    if (len) {
      present |= 1u << t;
      if ((pslots >> t) & 1u) {
        // equal patterns, equal words: the host compared the patterns (a wide slot's t_val
        // says nothing before the expand stage)
        const u32 a = (alias >> (3u * t)) & 7u;
        s = a < t && tl[a] == len ? a : t;
      } else {
        // one CSR range: equal offsets and equal lengths are equal words
        const u64 v = tv[t];
        for (u32 i = 0; i < t; ++i)
          if (!((pslots >> i) & 1u) && tl[i] == len && tv[i] == v) {
            s = i;
            break;
          }
      }
    }
    src |= s << (3u * t);
  }
  const u32* tw = ex + kExprTruth + (u64)q * kTerms;
  Table tab;
  tab.w0 = tw[0] & ~1u;  // (truth[0] is clear: the host refuses every other expression)
  tab.w1 = tw[1];
  tab.w2 = tw[2];
  tab.w3 = tw[3];
  tab.w4 = tw[4];
  tab.w5 = tw[5];
  tab.w6 = tw[6];
  tab.w7 = tw[7];
  // S: from P, drop the longest lists first while the rest still covers -- while no mask of
  // present terms outside S has its bit set
  u32 S = 0;
  if (any_inside(tab, present)) {
    S = present;
    u32 todo = present;
    while (todo) {
      u32 best = 0, best_len = 0;
      for (u32 t = 0; t < nterms; ++t) {  // (of equal lengths the higher term number)
        if (!((todo >> t) & 1u)) continue;
        const u32 len = tl[t];
        if (len >= best_len) {
          best_len = len;
          best = t;
        }
      }
      todo &= ~(1u << best);
      const u32 rest = S & ~(1u << best);
      if (!any_inside(tab, present & ~rest)) S = rest;
    }
  }
  u64 sum = 0;
  for (u32 t = 0; t < nterms; ++t)
    if ((S >> t) & 1u) sum += tl[t];
  if (sum >> 32) {  // (pattern terms' lists may overlap; the host throws)
    atomicAdd(&ctr->anyover, 1u);
    sum = 0;
  }
  ex[kExprPlan + q] = S | (present << 8);
  ex[kExprSrc + q] = src;
  q_bound[q] = 0u;  // search_hit_kernel walks nothing for this query
  return (u32)sum;
}

// One workgroup: every query's plan (a query of another mode: bound 0) and, in the same pass,
// start[0 .. Q] = the exclusive scan of the bounds; the total, saturated, to ctr->ebound.
__global__ __launch_bounds__(kSearchBlock) void expr_plan_kernel(
    const u32* __restrict__ q_meta, u32 Q, const u64* __restrict__ t_val,
    const u32* __restrict__ t_len, u32* __restrict__ ex, u32* __restrict__ q_bound,
    SearchCounters* __restrict__ ctr) {
  __shared__ u64 s_scan[kSearchBlock / 64 + 1];
  u64* __restrict__ e_start = reinterpret_cast<u64*>(ex + kExprStart);
  u64 carry = 0;
  for (u32 base = 0; base < Q; base += kSearchBlock) {  // (workgroup-uniform)
    const u32 q = base + threadIdx.x;
    u32 bound = 0;
    if (q < Q) {
      const u32 meta = q_meta[q];
      if (meta & kSearchExpr) bound = plan_query(q, meta, t_val, t_len, ex, q_bound, ctr);
      ex[kExprBound + q] = bound;
    }
    u64 total;
    const u64 before = dev::block_exclusive_scan<u64, kSearchBlock>((u64)bound, s_scan, &total);
    if (q < Q) e_start[q] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    e_start[Q] = carry;
    ctr->ebound = carry < 0xffffffffull ? (u32)carry : 0xffffffffu;
  }
}

__global__ __launch_bounds__(kSearchBlock) void expr_hit_kernel(
    const u32* __restrict__ postings, const u32* __restrict__ merged, u32 first_line,
    const u32* __restrict__ ex, const u64* __restrict__ t_val, const u32* __restrict__ t_len,
    u32 Q, u64 E, u64* __restrict__ pairs, u64 pair_cap, u32* __restrict__ q_hits,
    SearchCounters* __restrict__ ctr) {
  const u64* __restrict__ e_start = search_expr_start(ex);
  for (u64 tile = blockIdx.x; tile * kSearchTile < E; tile += gridDim.x) {  // (uniform)
#pragma unroll 1
    for (int j = 0; j < kSearchItems; ++j) {
      const u64 e = tile * kSearchTile + (u64)j * kSearchBlock + threadIdx.x;
      bool hit = false;
      u32 q = 0, line = first_line;
      if (e < E) {
        // the query: e_start[q] <= e < e_start[q + 1] (e_start[0] = 0, e_start[Q] = E)
        u32 lo = 0, hi = Q;
        while (hi - lo > 1) {
          const u32 mid = lo + ((hi - lo) >> 1);
          if (e_start[mid] <= e)
            lo = mid;
          else
            hi = mid;
        }
        q = lo;
        u32 local = (u32)(e - e_start[q]);
        const u32 plan = ex[kExprPlan + q];
        const u32 S = plan & 0xffu, present = (plan >> 8) & 0xffu;
        const u32 src = ex[kExprSrc + q];
        const u64* tv = t_val + (u64)q * kTerms;
        const u32* tl = t_len + (u64)q * kTerms;
        // the lists of S one after the other
        u32 term = 0;
        bool found = false;
        for (u32 t = 0; t < (u32)kTerms && !found; ++t) {
          if (!((S >> t) & 1u)) continue;
          term = t;
          found = local < tl[t];
          if (!found) local -= tl[t];
        }
        const u32 st = (src >> (3u * term)) & 7u;  // the term that owns this list
        if (found && local < tl[st]) {  // (always, by the bound's construction)
          const u32* list = term_list(postings, merged, tv[st]);
          line = list[local];
          // duplicates are adjacent: an element counts once per line
          if (local == 0 || list[local - 1] != line) {
            u32 mask = 0;
            bool dropped = false;  // an earlier list of S holds the line: counted there
            for (u32 u = 0; u < (u32)kTerms && !dropped; ++u) {
              if (!((present >> u) & 1u)) continue;
              const u32 su = (src >> (3u * u)) & 7u;
              bool in;
              if (su == st)
                in = true;  // this list
              else if (su != u)
                in = ((mask >> su) & 1u) != 0u;  // an earlier term's list: searched already
              else
                in = list_has(term_list(postings, merged, tv[u]), tl[u], line);
              mask |= (in ? 1u : 0u) << u;
              dropped = in && u < term && ((S >> u) & 1u);
            }
            const u32 word = ex[kExprTruth + (u64)q * kTerms + (mask >> 5)];
            hit = !dropped && ((word >> (mask & 31u)) & 1u) != 0u;
          }
        }
      }
      // ---- the step's hits: the wave is converged here ----
      commit_hits(hit, q, line - first_line, pairs, pair_cap, q_hits, ctr);
    }
  }
}

}  // namespace

void launch_expr_plan(const SearchBatch& b, u32 queries, hipStream_t s) {
  LOCUST_CHECK_ARG(b.expr && queries >= 1 && queries <= kSearchMaxQueries,
                   "search: the expression plan needs the expression arrays");
  expr_plan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.q_meta, queries, b.t_val, b.t_len,
                                                           b.expr, b.q_bound, b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_expr_hits(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 ebound,
                      const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.expr && ebound < (1ull << 32) && ebound <= h.cap,
                   "search: " + std::to_string(ebound) + " list elements of expression queries "
                   "exceed the workspace (" + std::to_string(h.cap) + ")");
  if (!ebound) return;
  const u32 blocks = (u32)std::min<u64>(div_up(ebound, (u64)kSearchTile), (u64)kSearchMaxBlocks);
  expr_hit_kernel<<<dim3(blocks), dim3(kSearchBlock), 0, s>>>(
      ix.postings, b.merged, ix.first_line, b.expr, b.t_val, b.t_len, queries, ebound, h.pairs,
      h.cap, b.q_hits, b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_expr() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&expr_hit_kernel));
}

}  // namespace locust
