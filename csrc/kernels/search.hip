// Index search: all/any/phrase/near word queries over the inverted index in device memory
// (kernels.hpp "search.hip"; the semantics are engine.hpp "index search").
//
// launch_index has left the key-ordered records, the CSR offsets val[0 .. n] and the sorted
// postings in device memory.  A query's answer needs rank lookups and searches in sorted
// lists only, and is usually far smaller than the index: it is selected here and only the
// answers cross PCIe.
//
// Shape (gfx950, wave64):
//  * search_lookup_kernel: one thread per (query, term), 32 queries per workgroup.  The key
//    was packed on the host (kv.hpp); find_rank gives the rank, val[] and the record's count
//    the list.  The eight terms of a query meet in LDS: every term thread compares its rank
//    range with the others' (a repeated term has the range of an earlier one), and the
//    query's first thread combines the flags into the distinct terms and the score mask,
//    picks the driver and writes the bound on the query's hits = the elements the hit kernel
//    walks for it.
//    A prefix term (`ham*`, engine.hpp "prefix terms") finds the rank range of its words
//    instead (find_prefix_range): terms are told apart by their ranges, and the lengths of
//    the lists that cover two or more words add up to the batch's merge total X.
//    An exclusion term (engine.hpp "exclusion terms"; the host packs them behind the positive
//    terms) is resolved like any term, but stays out of the driver choice, the bound, the dead
//    flag and both masks: the present ones' lists go to the hit kernel as a mask of their own;
//  * search_match_kernel, only in a batch that has a pattern term (engine.hpp "pattern terms"):
//    a pattern term's words are a scattered set of ranks, so a grid walks the dictionary, one
//    record per thread with the key in registers, and tries every pattern slot of the batch on
//    it with the shared matcher (device/glob.hpp).  A pattern is wave-uniform (scalar loads);
//    one ballot per wave and pattern, and one lane of a wave with a match adds the matching
//    words and their summed counts to the slot's arrays.  The lookup then reads a pattern
//    slot's length and word count from there instead of searching a range; a slot of two or
//    more words is merged by the expand stage, where search_scatter_kernel -- the same walk
//    and match -- copies each matching word's postings, the whole wave per word, to a place a
//    wave prefix sum and one atomic on the slot's cursor reserve;
//  * search_scan_kernel: one workgroup, exclusive scan of u32 values into count + 1 u64
//    words (the bounds -> q_start, later the hit counts -> offsets, the merged lengths of
//    the Q * 8 slots -> x_start);
//  * expand, only when X > 0: search_gather_kernel writes the key slot << 32 | line of
//    every element of the lists to merge (tiles of kSearchTile over [0, X), the slot by a
//    binary search in x_start), radix_sort() orders them, search_strip_kernel writes
//    merged[e] and points the slots' t_val there.  From then on such a list is read like
//    any other (term_list);
//  * search_hit_kernel: the flattened element space [0, B) in tiles of kSearchTile, grid-
//    stride.  A thread finds its element's query by a binary search in q_start, then the
//    term and position, and decides the hit by binary searches confined to the other
//    terms' CSR ranges.  Every step ends in wave-level ballots: one atomic reserves the
//    step's slots, one atomic per distinct query of the wave adds to its hit count
//    (commit_hits).  A phrase of two or more terms is looked up and walked as `all`, but
//    what passes is a candidate: its pair word goes to `cands`.  Before that split, a line
//    found in one of the query's exclusion lists is dropped: it is no hit and no candidate;
//  * search_phrase_kernel: one wave per candidate line, up to 64 consecutive candidates per
//    wave and round.  The wave walks the line 64 bytes per step with index.hip's tokeniser
//    (device/linetok.hpp), compares each emitted token's key with the query's term keys
//    (staged in LDS) and runs a shift-and automaton over the tokens.  Lane i keeps candidate
//    i's verdict, and the round ends in commit_hits;
//  * search_near_kernel: the phrase kernel's skeleton and token masks (token_term_mask) over
//    the candidates of the `near` queries, which the hit kernel keeps apart (they fill
//    `cands` from its end).  Its state is, per term, the ordinal of the last matching token
//    (lane j < 8 keeps term j's); only tokens with a non-zero mask are walked, and behind
//    each a minimum over those lanes decides;
//  * order: the device-wide radix_sort() on the one-word key, as launch_index uses it;
//  * search_emit_kernel: lines[j] = first_line + low32(sorted[j]) and the misplaced check.
// A ranked batch (engine.hpp "ranked search") takes another way behind the seal:
//  * search_score_kernel: one thread per hit pair, tiles of kSearchTile, grid-stride.  The
//    line's tf in every distinct term's list is upper bound - lower bound, both confined to
//    the list's CSR range; the weight comes from the list's length and N = val[n].  The pair
//    becomes the rank key query << 54 | (kRankScoreMax - score) << 32 | rel_line, so the
//    same ascending one-word sort yields (query, score descending, line ascending);
//  * search_top_kernel: one thread per sorted key; position pos inside its query's segment
//    (the misplaced check as the emit kernel's), and when pos < K the line and its score go
//    to out_off[q] + pos: every output position is determined, no atomics, no compaction.
// Data crosses between workgroups only at kernel boundaries (the radix sort keeps its own
// look-back); this file adds no polled word.
#include <algorithm>

#include "locust/device/dictscan.hpp"
#include "locust/device/glob.hpp"
#include "locust/device/linetok.hpp"
#include "locust/device/rank.hpp"
#include "locust/device/termmask.hpp"
#include "locust/device/verify.hpp"
#include "locust/device/wave.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;
constexpr int kLookupQueries = kSearchBlock / kTerms;  // queries per lookup workgroup
static_assert(kTerms == 8 && kSearchBlock % kTerms == 0, "eight term threads per query");
static_assert(kSearchMaxQueries % kSearchBlock == 0, "the scan walks whole blocks");

// ---- pattern terms: the dictionary scan (the bodies: device/dictscan.hpp) ----
// words[slot] += the records the slot's pattern matches, len[slot] += their counts, rank[slot]
// = one of them (pw: words | len | rank, zeroed per batch).
__global__ __launch_bounds__(kSearchBlock) void search_match_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ keys,
    const u32* __restrict__ pq, u32 Q, u32* __restrict__ pw) {
  search_match_body<1>(recs, n, keys, pq, Q, pw);
}

__global__ __launch_bounds__(kSearchBlock) void search_lookup_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ val,
    const u64* __restrict__ keys, const u32* __restrict__ q_meta, u32 Q, u64* __restrict__ t_val,
    u32* __restrict__ t_len, u32* __restrict__ q_info, u32* __restrict__ q_bound,
    u32* __restrict__ x_len, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq,
    const u32* __restrict__ pw) {
  // a term's words: the rank range [lo, hi) -- one word, or a prefix term's; absent: n, n
  __shared__ u32 s_lo[kSearchBlock];
  __shared__ u32 s_hi[kSearchBlock];
  __shared__ u32 s_len[kSearchBlock];
  __shared__ u32 s_flag[kSearchBlock];  // 1: present | 2: dup | 4: inside | first << 4 (below)
  const u32 gid = blockIdx.x * kSearchBlock + threadIdx.x;
  const u32 q = gid / kTerms, t = gid % kTerms;
  const u32 meta = q < Q ? q_meta[q] : 0u;
  const u32 nterms = min(meta & 0xffu, (u32)kTerms);  // (the host checked: at most eight)
  // the positive terms stand first; terms npos .. nterms - 1 are exclusion terms
  const u32 npos = nterms - min((u32)__popc(meta >> kSearchExcludeShift), nterms);
  u32 lo = n, hi = n, len = 0;
  u64 at = 0;
  // a pattern slot (pq: the batch's pattern flags and maps, null in a batch without pattern
  // terms; pw: the match kernel's words | len | rank): its words are no range, so lo = hi = n
  // keeps it out of the range rules below, and pwords stands for hi - lo
  const u32 pfl = pq && q < Q ? pq[q] : 0u;
  const bool ispat = t < nterms && ((pfl >> t) & 1u);
  u32 pwords = 0;
  if (ispat) {
    pwords = pw[gid];
    const u32 rank = pw[2 * kSearchSlots + gid];
    if (pwords && rank < n) {
      len = pw[kSearchSlots + gid];
      if (pwords == 1) at = val[rank];  // the word's list in place
    } else {
      pwords = 0;
    }
  } else if (t < nterms) {
    const u64* k = keys + (u64)gid * kKeyWords;
    if ((meta >> (kSearchPrefixShift + t)) & 1u) {
      dev::find_prefix_range(recs, n, k[0], k[1], k[2], k[3], &lo, &hi);
      if (lo < hi) {
        at = val[lo];
        len = (u32)(val[hi] - at);  // (the index holds < 2^32 postings in all)
      } else {
        lo = hi = n;
      }
    } else {
      const u32 rank = dev::find_rank(recs, n, k[0], k[1], k[2], k[3]);
      if (rank < n) {
        lo = rank;
        hi = rank + 1;
        at = val[rank];
        len = (u32)recs[rank].count;  // (the index holds < 2^32 postings in all)
      }
    }
  }
  if (q < Q) {
    t_val[gid] = at;
    t_len[gid] = len;
  }
  s_lo[threadIdx.x] = lo;
  s_hi[threadIdx.x] = hi;
  s_len[threadIdx.x] = len;
  __syncthreads();
  // Ranges are nested or disjoint.  Every term thread looks at the query's other terms: dup,
  // an earlier term has the same words; inside, another present term's range holds this
  // one's (of equal ranges the first counts).  The eight threads of a query do this side by
  // side, so its first thread only has to combine eight flag words below.
  // `inside` is the positive terms' rule among themselves (an exclusion term's is not read);
  // first: the query's first term with this one's words, whose list stands for them all.
  bool dup = false, inside = false;
  u32 first = t;
  if (lo < hi) {
    const u32 base = threadIdx.x - t;
    for (u32 i = 0; i < nterms; ++i) {
      const u32 ilo = s_lo[base + i], ihi = s_hi[base + i];
      if (i == t || ilo >= ihi) continue;
      const bool same = ilo == lo && ihi == hi;
      dup |= same && i < t;
      first = same && i < first ? i : first;
      if (i < npos) inside |= same ? i < t : (ilo <= lo && hi <= ihi);
    }
  }
  if (pwords) {
    // pattern terms are the same term when their pattern words and maps are equal; the later
    // one repeats the earlier one (and counts as inside it: it scores once)
    const u64* k = keys + (u64)gid * kKeyWords;
    const u32 km = pq[kSearchPatMeta + gid];
    for (u32 i = 0; i < t; ++i) {
      if (!((pfl >> i) & 1u)) continue;
      const u64* o = keys + (u64)(gid - t + i) * kKeyWords;
      if (o[0] != k[0] || o[1] != k[1] || o[2] != k[2] || o[3] != k[3] ||
          pq[kSearchPatMeta + gid - t + i] != km)
        continue;
      dup = true;
      first = i < first ? i : first;
      inside |= i < npos;
    }
  }
  s_flag[threadIdx.x] = (lo < hi || pwords ? 1u : 0u) | (dup ? 2u : 0u) | (inside ? 4u : 0u) |
                        (first << 4);
  // a list of two or more words is merged (the expand stage), unless an earlier term of the
  // query has the same words.  Only a prefix term or a pattern term covers two words.
  const bool wide = (hi - lo >= 2u || pwords >= 2u) && !dup;
  if (q < Q) x_len[gid] = wide ? len : 0u;
  if (dev::ballot(wide)) {  // (wave-uniform; no batch without prefix terms gets here)
    const u64 x = dev::wave_reduce_sum<u64>(wide ? (u64)len : 0ull);
    if (dev::lane_id() == 0) atomicAdd((unsigned long long*)&ctr->merge, (unsigned long long)x);
  }
  __syncthreads();
  if (q < Q && t == 0) {
    const bool any = (meta & kSearchAny) != 0;  // (a phrase is looked up as `all`)
    const u32* fl = s_flag + threadIdx.x;
    const u32* ln = s_len + threadIdx.x;
    u32 mask = 0, smask = 0, xmask = 0, dead = 0, driver = 0, best = ~0u;
    u64 sum = 0;
    for (u32 j = 0; j < npos; ++j) {
      const u32 f = fl[j];
      if (!(f & 1u)) {  // absent
        dead |= any ? 0u : 1u;
        continue;
      }
      if (!(f & 4u)) smask |= 1u << j;
      // `any`: a list inside another adds no line to the union, and the lists left are
      // disjoint ranges of < 2^32 postings, so sum fits 32 bits -- but for pattern terms'
      // lists, which may overlap: anyover below
      if (f & (any ? 4u : 2u)) continue;
      mask |= 1u << j;
      sum += ln[j];
      if (ln[j] < best) {
        best = ln[j];
        driver = j;
      }
    }
    // the present exclusion terms' lists, each once: an absent one excludes nothing, and one
    // with an earlier term's words (a positive term's too) is that term's list -- the merged
    // one, when the words are two or more
    for (u32 j = npos; j < nterms; ++j)
      if (fl[j] & 1u) xmask |= 1u << (fl[j] >> 4);
    if (any && (sum >> 32)) atomicAdd(&ctr->anyover, 1u);  // (the host throws)
    const u32 bound = any ? (u32)sum : (dead || !mask ? 0u : best);
    q_info[q] = driver | (dead << 3) | (xmask << 8) | (mask << 16) | (smask << 24);
    q_bound[q] = bound;
  }
}

// One workgroup: out[0 .. Q] = exclusive scan of min(in[0 .. Q), clip); the total also to
// *total.
__global__ __launch_bounds__(kSearchBlock) void search_scan_kernel(const u32* __restrict__ in,
                                                                   u32 Q, u32 clip,
                                                                   u64* __restrict__ out,
                                                                   u64* __restrict__ total) {
  __shared__ u64 s_scan[kSearchBlock / 64 + 1];
  u64 carry = 0;
  for (u32 base = 0; base < Q; base += kSearchBlock) {  // (workgroup-uniform)
    const u32 i = base + threadIdx.x;
    const u64 v = i < Q ? (in[i] < clip ? in[i] : clip) : 0;
    u64 tv;
    const u64 ev = dev::block_exclusive_scan<u64, kSearchBlock>(v, s_scan, &tv);
    if (i < Q) out[i] = carry + ev;
    carry += tv;
  }
  if (threadIdx.x == 0) {
    out[Q] = carry;
    if (total) *total = carry;
  }
}

// ---- expand: the merged lists of the prefix terms that cover two or more words ----
// Such a term's postings are one CSR range, but a concatenation of per-word sorted lists.
// x_start (the scan of x_len over the S = Q * 8 slots) lays the lists out one after the
// other in [0, X); element e becomes the key slot << 32 | (line - first_line), the one-word
// radix_sort() orders the keys by (slot, line), and what is left is to strip the slot.
__global__ __launch_bounds__(kSearchBlock) void search_gather_kernel(
    const u32* __restrict__ postings, u32 first_line, const u64* __restrict__ x_start,
    const u64* __restrict__ t_val, u32 S, u64 X, u64 cap, u64* __restrict__ keys,
    SearchCounters* __restrict__ ctr, const u32* __restrict__ pq) {
  if (x_start[S] != X || X > cap) return;  // (uniform; never: the host throws on merge_n)
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr->merge_n = (u32)X;  // the sort's length
  for (u64 tile = blockIdx.x; tile * kSearchTile < X; tile += gridDim.x) {  // (uniform)
#pragma unroll 1
    for (int j = 0; j < kSearchItems; ++j) {
      const u64 e = tile * kSearchTile + (u64)j * kSearchBlock + threadIdx.x;
      if (e >= X) continue;
      // the slot: x_start[slot] <= e < x_start[slot + 1] (x_start[0] = 0, x_start[S] = X)
      u32 lo = 0, hi = S;
      while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (x_start[mid] <= e)
          lo = mid;
        else
          hi = mid;
      }
      // a pattern slot's words are no CSR range: the scatter kernel fills its part
      if (pq && ((pq[lo / kTerms] >> (lo % kTerms)) & 1u)) continue;
      // (e - x_start[lo] < x_len[lo] = the slot's t_len: inside its CSR range)
      const u32 line = postings[t_val[lo] + (e - x_start[lo])];
      keys[e] = ((u64)lo << 32) | (u64)(line - first_line);
    }
  }
}

// The wide pattern slots' part of the keys (x_len != 0 and a pattern slot): the match kernel's
// walk and match, and the whole wave copies each matching word's postings
// (device/dictscan.hpp).
__global__ __launch_bounds__(kSearchBlock) void search_scatter_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ val,
    const u32* __restrict__ postings, u32 first_line, const u64* __restrict__ pkeys,
    const u32* __restrict__ pq, u32 Q, const u32* __restrict__ x_len,
    const u64* __restrict__ x_start, u64 X, u64 cap, u32* __restrict__ cursor,
    u64* __restrict__ keys) {
  search_scatter_body<1>(recs, n, val, postings, first_line, pkeys, pq, Q, x_len, x_start, X, cap,
                         cursor, keys);
}

// merged[e] = first_line + the key's line; a key outside its slot's x_start range counts as
// unmerged.  The merged slots' t_val now name their lists in `merged`.
__global__ __launch_bounds__(256) void search_strip_kernel(
    const u64* __restrict__ sorted, u64 X, const u64* __restrict__ x_start,
    const u32* __restrict__ x_len, u32 S, u32 first_line, u32* __restrict__ merged,
    u64* __restrict__ t_val, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq,
    const u32* __restrict__ cursor) {
  if (ctr->merge_n != (u32)X) return;  // nothing was sorted (workgroup-uniform)
  const u64 gid = (u64)blockIdx.x * 256 + threadIdx.x, stride = (u64)gridDim.x * 256;
  u32 bad = 0;
  for (u64 e = gid; e < X; e += stride) {
    const u64 w = sorted[e];
    const u32 slot = (u32)(w >> 32);
    merged[e] = first_line + (u32)w;
    if (slot >= S || e < x_start[slot] || e >= x_start[slot + 1]) ++bad;
  }
  for (u64 slot = gid; slot < S; slot += stride)
    if (x_len[slot]) {
      t_val[slot] = kSearchMerged | x_start[slot];
      // a pattern slot the scatter kernel did not fill exactly
      if (pq && ((pq[slot / kTerms] >> (slot % kTerms)) & 1u) && cursor[slot] != x_len[slot]) ++bad;
    }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->unmerged, bad);
  }
}

// (list_has and term_list, which expr.hip shares: device/verify.hpp)
// How often does `line` occur among the len sorted postings at p?  (Never reads outside
// [p, p + len).)
__device__ __forceinline__ u32 list_tf(const u32* __restrict__ p, u32 len, u32 line) {
  u32 lo = 0, hi = len;
  while (lo < hi) {  // lower bound
    const u32 mid = lo + ((hi - lo) >> 1);
    if (p[mid] < line)
      lo = mid + 1;
    else
      hi = mid;
  }
  const u32 first = lo;
  if (lo == len || p[lo] != line) return 0;  // (most terms of an `any` query, on most lines)
  // the upper bound: tf is small on most lines, so gallop from the lower bound (p[at] == line
  // throughout), then bisect the last stride
  u32 at = lo, step = 1;
  while (step < len - at && p[at + step] == line) {
    at += step;
    if (step < (1u << 31)) step <<= 1;
  }
  lo = at + 1;
  hi = step < len - at ? at + step : len;  // p[hi] > line, or the list's end
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (p[mid] <= line)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - first;
}


__global__ __launch_bounds__(kSearchBlock) void search_hit_kernel(
    const u32* __restrict__ postings, const u32* __restrict__ merged, u32 first_line,
    const u32* __restrict__ q_meta,
    const u32* __restrict__ q_info, const u64* __restrict__ q_start, const u64* __restrict__ t_val,
    const u32* __restrict__ t_len, u32 Q, u64 B, u64* __restrict__ pairs,
    u64* __restrict__ cands, u64 pair_cap, u32* __restrict__ q_hits,
    SearchCounters* __restrict__ ctr) {
  const int lane = dev::lane_id();
  for (u64 tile = blockIdx.x; tile * kSearchTile < B; tile += gridDim.x) {  // (uniform)
#pragma unroll 1
    for (int j = 0; j < kSearchItems; ++j) {
      const u64 e = tile * kSearchTile + (u64)j * kSearchBlock + threadIdx.x;
      bool hit = false, cand = false, near = false;
      u32 q = 0, line = first_line;
      if (e < B) {
        // the query: q_start[q] <= e < q_start[q + 1] (q_start[0] = 0, q_start[Q] = B)
        u32 lo = 0, hi = Q;
        while (hi - lo > 1) {
          const u32 mid = lo + ((hi - lo) >> 1);
          if (q_start[mid] <= e)
            lo = mid;
          else
            hi = mid;
        }
        q = lo;
        u32 local = (u32)(e - q_start[q]);
        const u32 info = q_info[q];
        const u32 meta = q_meta[q];
        const bool any = (meta & kSearchAny) != 0;
        // a phrase of two or more terms: what passes the `all` test is only a candidate
        // (of two or more positive terms: exclusion terms are not part of the phrase)
        const bool verify = (meta & kSearchPhrase) != 0 &&
                            (meta & 0xffu) >= 2u + (u32)__popc(meta >> kSearchExcludeShift);
        const u32 mask = (info >> 16) & 0xffu;
        const u32 xmask = (info >> 8) & 0xffu;  // the exclusion lists (0: none, most batches)
        // so does a `near` query to verify, of two or more distinct terms (one: `all`)
        near = (meta & kSearchNear) != 0 && (mask & (mask - 1u)) != 0u;
        const u64* tv = t_val + (u64)q * kTerms;
        const u32* tl = t_len + (u64)q * kTerms;
        u32 term = info & 7u;  // `all`: the driver
        if (any) {                // the distinct terms' lists one after the other
          term = 0;
          for (u32 t = 0; t < (u32)kTerms; ++t) {
            if (!((mask >> t) & 1u)) continue;
            term = t;
            if (local < tl[t]) break;
            local -= tl[t];
          }
        }
        if (local < tl[term]) {  // (always, by the bound's construction)
          const u32* list = term_list(postings, merged, tv[term]);
          line = list[local];
          // duplicates are adjacent: an element counts once per line
          if (local == 0 || list[local - 1] != line) {
            hit = true;
            if (any) {
              for (u32 t = 0; t < term; ++t)
                if (((mask >> t) & 1u) &&
                    list_has(term_list(postings, merged, tv[t]), tl[t], line))
                  hit = false;
            } else {
              for (u32 t = 0; t < (u32)kTerms && hit; ++t)
                if (((mask >> t) & 1u) && t != term)
                  hit = list_has(term_list(postings, merged, tv[t]), tl[t], line);
            }
            // an excluded line is neither hit nor candidate
            if (hit && xmask) {
              for (u32 t = 0; t < (u32)kTerms && hit; ++t)
                if ((xmask >> t) & 1u)
                  hit = !list_has(term_list(postings, merged, tv[t]), tl[t], line);
            }
            cand = hit && (verify || near);
            hit = hit && !cand;
          }
        }
      }
      // ---- the step's candidates and hits: the wave is converged here ----
      if (dev::ballot(cand)) {  // (wave-uniform)
        // a phrase's from cands[0] upwards, a near query's from cands[pair_cap - 1] downwards
        const u64 nm = dev::ballot(cand && near);
        const u64 cm = dev::ballot(cand && !near);
        if (cm) {  // (wave-uniform)
          const int first = __ffsll((unsigned long long)cm) - 1;
          u32 at = 0;
          if (lane == first) at = atomicAdd(&ctr->cands, (u32)__popcll(cm));
          at = (u32)__shfl((int)at, first, 64);
          if (cand && !near) {
            const u64 slot = (u64)at + dev::lanes_below(cm);
            if (slot < pair_cap) cands[slot] = ((u64)q << 32) | (u64)(line - first_line);
          }
        }
        if (nm) {  // (wave-uniform)
          const int first = __ffsll((unsigned long long)nm) - 1;
          u32 at = 0;
          if (lane == first) at = atomicAdd(&ctr->ncands, (u32)__popcll(nm));
          at = (u32)__shfl((int)at, first, 64);
          if (cand && near) {
            const u64 slot = (u64)at + dev::lanes_below(nm);
            if (slot < pair_cap)
              cands[pair_cap - 1 - slot] = ((u64)q << 32) | (u64)(line - first_line);
          }
        }
      }
      commit_hits(hit, q, line - first_line, pairs, pair_cap, q_hits, ctr);
    }
  }
}


// The verify kernels: the phrase and the near body (device/verify.hpp), without and with the
// pattern matcher.
__global__ __launch_bounds__(kPhraseBlock) void search_phrase_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  search_phrase_body<0>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, nullptr, text,
                        bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta, keys,
                        Q, cands, pairs, pair_cap, q_hits, ctr);
}

// ... of a batch that has a pattern term (pq: its pattern flags and maps).
__global__ __launch_bounds__(kPhraseBlock) void search_globphrase_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_phrase_body<1>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                       text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                       keys, Q, cands, pairs, pair_cap, q_hits, ctr);
}

__global__ __launch_bounds__(kPhraseBlock) void search_near_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  search_near_body<0>(s_row[dev::wave_id()], s_keys[dev::wave_id()], nullptr, nullptr, text,
                        bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta, keys,
                        Q, cands, pairs, pair_cap, q_hits, ctr);
}

// ... of a batch that has a pattern term (pq: its pattern flags and maps).
__global__ __launch_bounds__(kPhraseBlock) void search_globnear_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_near_body<1>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                       text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                       keys, Q, cands, pairs, pair_cap, q_hits, ctr);
}

// One thread, between the hits and the sort: the sort takes its length from device memory,
// and never more than the workspace holds.
__global__ void search_seal_kernel(SearchCounters* __restrict__ ctr, u64 cap) {
  ctr->sort_n = ctr->written <= cap ? ctr->written : 0u;
}

// lines[j] = first_line + the pair's line; a pair outside its query's offsets range counts
// as misplaced.
__global__ __launch_bounds__(256) void search_emit_kernel(const u64* __restrict__ sorted, u64 H,
                                                          const u64* __restrict__ offsets, u32 Q,
                                                          u32 first_line, u32* __restrict__ lines,
                                                          SearchCounters* __restrict__ ctr) {
  if (ctr->sort_n != (u32)H) return;  // nothing was sorted (workgroup-uniform)
  u32 bad = 0;
  for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < H; j += (u64)gridDim.x * 256) {
    const u64 w = sorted[j];
    const u32 q = (u32)(w >> 32);
    lines[j] = first_line + (u32)w;
    if (q >= Q || j < offsets[q] || j >= offsets[q + 1]) ++bad;
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->misplaced, bad);
  }
}

// ---- ranked search ----
constexpr int kRankLineBits = 32, kRankScoreBits = 22;
constexpr int kRankQueryShift = kRankLineBits + kRankScoreBits;
constexpr u64 kRankScoreMask = (1ull << kRankScoreBits) - 1;
static_assert(kRankScoreMax <= kRankScoreMask, "kRankScoreMax - score fits the score field");
static_assert(kSearchMaxQueries == 1u << (64 - kRankQueryShift),
              "the query fills the bits above the score field");

// keys[e] = the rank key of pairs[e], e < H.  A hit whose score is 0 or above max_score (or
// whose query is none of the batch) counts in ctr->unscored: the host throws.
__global__ __launch_bounds__(kSearchBlock) void search_score_kernel(
    const u32* __restrict__ postings, const u32* __restrict__ merged,
    const u64* __restrict__ val, u32 n, u32 first_line,
    const u32* __restrict__ q_info, const u64* __restrict__ t_val, const u32* __restrict__ t_len,
    u32 Q, u32 max_score, const u64* __restrict__ pairs, u64 H, u64* __restrict__ keys,
    SearchCounters* __restrict__ ctr) {
  if (ctr->sort_n != (u32)H) return;  // the pairs are not all there (workgroup-uniform)
  const u32 N = (u32)val[n];          // (the index holds < 2^32 postings in all)
  u32 bad = 0;
  for (u64 tile = blockIdx.x; tile * kSearchTile < H; tile += gridDim.x) {  // (uniform)
#pragma unroll 1
    for (int j = 0; j < kSearchItems; ++j) {
      const u64 e = tile * kSearchTile + (u64)j * kSearchBlock + threadIdx.x;
      if (e >= H) continue;
      const u64 w = pairs[e];
      const u32 q = (u32)(w >> 32), rel = (u32)w;
      u64 score = 0;
      if (q < Q) {
        const u32 mask = q_info[q] >> 24;  // the score mask: nested ranges count once
        const u64* tv = t_val + (u64)q * kTerms;
        const u32* tl = t_len + (u64)q * kTerms;
        for (u32 t = 0; t < (u32)kTerms; ++t) {
          if (!((mask >> t) & 1u) || tl[t] == 0) continue;
          const u32 weight = 32u - (u32)__clz((int)(N / tl[t]));  // bit_length(N / c_t)
          score += (u64)weight *
                   list_tf(term_list(postings, merged, tv[t]), tl[t], first_line + rel);
        }
      }
      if (score < 1 || score > max_score) {
        ++bad;
        score = score < 1 ? 0 : kRankScoreMax;  // (any key: the host throws)
      }
      keys[e] = ((u64)(q & (kSearchMaxQueries - 1)) << kRankQueryShift) |
                ((u64)(kRankScoreMax - (u32)score) << kRankLineBits) | (u64)rel;
    }
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->unscored, bad);
  }
}

// Sorted key j lies at position pos = j - offsets[q] of its query's segment (outside it:
// misplaced, as the emit kernel counts); the first K of a segment go to out_off[q] + pos.
__global__ __launch_bounds__(256) void search_top_kernel(
    const u64* __restrict__ sorted, u64 H, const u64* __restrict__ offsets,
    const u64* __restrict__ out_off, u32 Q, u32 K, u32 first_line, u32* __restrict__ lines,
    u32* __restrict__ scores, SearchCounters* __restrict__ ctr) {
  if (ctr->sort_n != (u32)H) return;  // nothing was sorted (workgroup-uniform)
  u32 bad = 0;
  for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < H; j += (u64)gridDim.x * 256) {
    const u64 w = sorted[j];
    const u32 q = (u32)(w >> kRankQueryShift);
    if (q >= Q || j < offsets[q] || j >= offsets[q + 1]) {
      ++bad;
      continue;
    }
    const u64 pos = j - offsets[q];
    if (pos < (u64)K) {  // (pos < min(hits of q, K): inside out_off[q .. q + 1])
      const u64 o = out_off[q] + pos;
      lines[o] = first_line + (u32)w;
      scores[o] = kRankScoreMax - (u32)((w >> kRankLineBits) & kRankScoreMask);
    }
  }
  const u64 bm = dev::ballot(bad != 0);
  if (bm) {
    bad = dev::wave_reduce_sum(bad);
    if (dev::lane_id() == 0) atomicAdd(&ctr->misplaced, bad);
  }
}

constexpr u64 kQ = kSearchMaxQueries;
constexpr u64 kQT = kQ * kSearchMaxTerms;

// The batch block's parts in order.
template <class Take>
void batch_layout(Take&& take) {
  take(search_upload_bytes((u32)kQ, true));    // upload: q_meta | keys | within
  take(64 + kQ * 4);                           // zero: ctr (64 B) | q_hits
  take(kQT * 8);                               // t_val
  take(kQT * 4);                               // t_len
  take(kQ * 4);                                // q_info
  take(kQ * 4);                                // q_bound
  take((kQ + 1) * 8);                          // q_start
  take((kQ + 1) * 8);                          // offsets
  take(kQT * 4);                               // x_len
  take((kQT + 1) * 8);                         // x_start
}
static_assert(sizeof(SearchCounters) <= 64, "zero block layout");

template <class Take>
void hits_layout(u64 cap, Take&& take) {
  take(cap * 8);                                               // pairs
  take(cap * 8);                                               // cands
  take(cap * 8);                                               // zeros
  take(cap * 8);                                               // sorted
  take(cap * 8);                                               // spare
  take(cap * 4);                                               // lines
  take(radix_zero_bytes(cap));                                 // rx counters + status
  take((u64)radix_hist_blocks(cap) * kNumPositions * 256 * 4);  // rx hist_part
  take(sizeof(SortPlan));                                      // rx plan
  take(cap * 8);                                               // rx keys[0]
  take(cap * 8);                                               // rx keys[1]
  take(cap * 4);                                               // rx vals[0]
  take(cap * 4);                                               // rx vals[1]
}

}  // namespace

u64 search_upload_bytes(u32 queries, bool within) {
  return kQ * 4 + (u64)queries * kSearchMaxTerms * kKeyWords * 8 + (within ? (u64)queries * 4 : 0);
}

u64 search_batch_bytes() {
  u64 b = 0;
  batch_layout([&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void search_batch_carve(char* base, SearchBatch* sb) {
  char* part[10];
  int k = 0;
  u64 b = 0;
  batch_layout([&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  sb->upload = part[0];
  sb->q_meta = reinterpret_cast<u32*>(part[0]);
  sb->keys = reinterpret_cast<u64*>(part[0] + kQ * 4);
  sb->zero = part[1];
  sb->zero_bytes = 64 + kQ * 4;
  sb->ctr = reinterpret_cast<SearchCounters*>(part[1]);
  sb->q_hits = reinterpret_cast<u32*>(part[1] + 64);
  sb->t_val = reinterpret_cast<u64*>(part[2]);
  sb->t_len = reinterpret_cast<u32*>(part[3]);
  sb->q_info = reinterpret_cast<u32*>(part[4]);
  sb->q_bound = reinterpret_cast<u32*>(part[5]);
  sb->q_start = reinterpret_cast<u64*>(part[6]);
  sb->out_off = sb->q_start;  // (ranked: the hit kernel has read q_start by then)
  sb->offsets = reinterpret_cast<u64*>(part[7]);
  sb->x_len = reinterpret_cast<u32*>(part[8]);
  sb->x_start = reinterpret_cast<u64*>(part[9]);
}

u64 search_hits_bytes(u64 cap) {
  u64 b = 0;
  hits_layout(cap, [&](u64 bytes) { b = align_up(b, 256) + bytes; });
  return align_up(b, 256);
}

void search_hits_carve(char* base, u64 cap, SearchHits* h) {
  char* part[13];
  int k = 0;
  u64 b = 0;
  hits_layout(cap, [&](u64 bytes) {
    b = align_up(b, 256);
    part[k++] = base + b;
    b += bytes;
  });
  h->pairs = reinterpret_cast<u64*>(part[0]);
  h->cands = reinterpret_cast<u64*>(part[1]);
  h->zeros = reinterpret_cast<u64*>(part[2]);
  h->sorted = reinterpret_cast<u64*>(part[3]);
  h->spare = reinterpret_cast<u64*>(part[4]);
  h->lines = reinterpret_cast<u32*>(part[5]);
  h->rx.tile_counters = reinterpret_cast<u32*>(part[6]);
  h->rx.status = h->rx.tile_counters + kNumPositions;
  h->rx.hist_part = reinterpret_cast<u32*>(part[7]);
  h->rx.plan = reinterpret_cast<SortPlan*>(part[8]);
  h->rx.keys[0] = reinterpret_cast<u64*>(part[9]);
  h->rx.keys[1] = reinterpret_cast<u64*>(part[10]);
  h->rx.vals[0] = reinterpret_cast<u32*>(part[11]);
  h->rx.vals[1] = reinterpret_cast<u32*>(part[12]);
  h->rx.cap = cap;
  h->cap = cap;
}


void launch_search_lookup(const SearchIndex& ix, const SearchBatch& b, u32 queries,
                          hipStream_t s) {
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries,
                   "search: a batch holds 1 to " + std::to_string(kSearchMaxQueries) +
                       " queries, not " + std::to_string(queries));
  LOCUST_HIP_CHECK(hipMemsetAsync(b.zero, 0, b.zero_bytes, s));
  if (b.pat) {  // match: the pattern slots' words, lengths and cursors start from zero
    LOCUST_HIP_CHECK(hipMemsetAsync(b.pat + kSearchPatWords, 0,
                                    (kSearchPatEnd - kSearchPatWords) * sizeof(u32), s));
    if (ix.n && b.regex) {  // (a batch that has a regex term: regex.hip's scan)
      launch_regex_match(ix, b, queries, s);
    } else if (ix.n && b.fuzzy) {  // (a batch that has a fuzzy term: fuzzy.hip's scan)
      launch_fuzzy_match(ix, b, queries, s);
    } else if (ix.n) {
      search_match_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
          ix.recs, ix.n, b.keys, b.pat, queries, b.pat + kSearchPatWords);
      LOCUST_HIP_LAUNCH_CHECK();
    }
  }
  const u32 blocks = (u32)div_up((u64)queries, (u64)kLookupQueries);
  search_lookup_kernel<<<dim3(blocks), dim3(kSearchBlock), 0, s>>>(
      ix.recs, ix.n, ix.val, b.keys, b.q_meta, queries, b.t_val, b.t_len, b.q_info, b.q_bound,
      b.x_len, b.ctr, b.pat, b.pat ? b.pat + kSearchPatWords : nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  // (a batch that has an `expr` query: their walked sets and bounds; they leave q_bound)
  if (b.expr) launch_expr_plan(b, queries, s);
  search_scan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.q_bound, queries, ~0u, b.q_start,
                                                            &b.ctr->bound);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_search_expand(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          SearchHits& h, SortPlan* h_plan, hipStream_t s) {
  LOCUST_CHECK_ARG(queries >= 1 && queries <= kSearchMaxQueries && x >= 1 && x < (1ull << 32) &&
                       x <= h.cap && b.merged && x <= b.merged_cap,
                   "search: " + std::to_string(x) + " list elements to merge exceed the "
                   "workspace (" + std::to_string(h.cap) + ", " + std::to_string(b.merged_cap) +
                       ")");
  const u32 slots = queries * kSearchMaxTerms;
  search_scan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.x_len, slots, ~0u, b.x_start,
                                                            nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  const u32 gblocks = (u32)std::min<u64>(div_up(x, (u64)kSearchTile), (u64)kSearchMaxBlocks);
  search_gather_kernel<<<dim3(gblocks), dim3(kSearchBlock), 0, s>>>(
      ix.postings, ix.first_line, b.x_start, b.t_val, slots, x, h.cap, h.pairs, b.ctr, b.pat);
  LOCUST_HIP_LAUNCH_CHECK();
  if (b.pat && ix.n && b.regex) {
    launch_regex_scatter(ix, b, queries, x, h, s);
  } else if (b.pat && ix.n && b.fuzzy) {
    launch_fuzzy_scatter(ix, b, queries, x, h, s);
  } else if (b.pat && ix.n) {  // the wide pattern slots' part of the keys
    search_scatter_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
        ix.recs, ix.n, ix.val, ix.postings, ix.first_line, b.keys, b.pat, queries, b.x_len,
        b.x_start, x, h.cap, b.pat + kSearchPatCursor, h.pairs);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  ConstKeysSoA keys;
  KeysSoA sorted;
  keys.w[0] = h.pairs;
  sorted.w[0] = h.sorted;
  for (int j = 1; j < kKeyWords; ++j) {
    keys.w[j] = h.zeros;
    sorted.w[j] = h.spare;  // the gather's copies of the zero words
  }
  radix_sort(keys, &b.ctr->merge_n, x, h.rx, nullptr, sorted, nullptr, nullptr, h_plan, s);
  const u32 sblocks = (u32)std::min<u64>(div_up(std::max<u64>(x, slots), 256), 4096);
  search_strip_kernel<<<dim3(sblocks), dim3(256), 0, s>>>(h.sorted, x, b.x_start, b.x_len, slots,
                                                          ix.first_line, b.merged, b.t_val, b.ctr,
                                                          b.pat,
                                                          b.pat ? b.pat + kSearchPatCursor : nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_search_hits(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                        bool verify, bool near, const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(bound < (1ull << 32) && bound <= h.cap,
                   "search: " + std::to_string(bound) + " list elements exceed the workspace (" +
                       std::to_string(h.cap) + ")");
  if (bound) {
    const u32 blocks =
        (u32)std::min<u64>(div_up(bound, (u64)kSearchTile), (u64)kSearchMaxBlocks);
    search_hit_kernel<<<dim3(blocks), dim3(kSearchBlock), 0, s>>>(
        ix.postings, b.merged, ix.first_line, b.q_meta, b.q_info, b.q_start, b.t_val, b.t_len,
        queries, bound, h.pairs, h.cands, h.cap, b.q_hits, b.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  if (bound && verify && ix.bytes) {
    LOCUST_CHECK_ARG(ix.text && ix.nl_pos && ix.lctr && ix.emits_per_line > 0 &&
                         ix.max_key_len > 0 && ix.max_key_len <= kKeyBytes,
                     "search: a phrase needs the index's text view");
    // at most `bound` candidates: one per wave while they are few, up to 64 per wave and
    // round when every wave of a full grid has many to walk anyway (as launch_index)
    const u32 group = (u32)std::min<u64>(div_up(bound, (u64)kPhraseMaxBlocks), 64);
    const u32 blocks = (u32)std::min<u64>(div_up(div_up(bound, (u64)group), (u64)kPhraseWaves),
                                          (u64)kPhraseMaxBlocks);
    if (b.regex)  // (a batch that has a regex term: regex.hip's sibling)
      launch_regex_phrase(ix, b, queries, bound, h, s);
    else if (b.fuzzy)  // (a batch that has a fuzzy term: fuzzy.hip's sibling)
      launch_fuzzy_phrase(ix, b, queries, bound, h, s);
    else if (b.pat)  // (a batch that has a pattern term: the sibling with the matcher)
      search_globphrase_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
          ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
          b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat);
    else
      search_phrase_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
          ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
          b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  if (bound && near && ix.bytes) {
    LOCUST_CHECK_ARG(ix.text && ix.nl_pos && ix.lctr && ix.emits_per_line > 0 &&
                         ix.max_key_len > 0 && ix.max_key_len <= kKeyBytes,
                     "search: a near query needs the index's text view");
    // the phrase kernel's grid: at most `bound` candidates
    const u32 group = (u32)std::min<u64>(div_up(bound, (u64)kPhraseMaxBlocks), 64);
    const u32 blocks = (u32)std::min<u64>(div_up(div_up(bound, (u64)group), (u64)kPhraseWaves),
                                          (u64)kPhraseMaxBlocks);
    if (b.regex)
      launch_regex_near(ix, b, queries, bound, h, s);
    else if (b.fuzzy)
      launch_fuzzy_near(ix, b, queries, bound, h, s);
    else if (b.pat)
      search_globnear_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
          ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
          b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat);
    else
      search_near_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
          ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
          b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr);
    LOCUST_HIP_LAUNCH_CHECK();
  }
  search_seal_kernel<<<dim3(1), dim3(1), 0, s>>>(b.ctr, h.cap);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_search_order(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 hits,
                         SearchHits& h, SortPlan* h_plan, hipStream_t s) {
  LOCUST_CHECK_ARG(hits <= h.cap, "search: " + std::to_string(hits) +
                                      " hits exceed the workspace (" + std::to_string(h.cap) + ")");
  search_scan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.q_hits, queries, ~0u, b.offsets,
                                                            nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  if (hits == 0) return;
  ConstKeysSoA keys;
  KeysSoA sorted;
  keys.w[0] = h.pairs;
  sorted.w[0] = h.sorted;
  for (int j = 1; j < kKeyWords; ++j) {
    keys.w[j] = h.zeros;
    sorted.w[j] = h.spare;  // the gather's copies of the zero words
  }
  radix_sort(keys, &b.ctr->sort_n, hits, h.rx, nullptr, sorted, nullptr, nullptr, h_plan, s);
  const u32 eblocks = (u32)std::min<u64>(div_up(hits, 256), 4096);
  search_emit_kernel<<<dim3(eblocks), dim3(256), 0, s>>>(h.sorted, hits, b.offsets, queries,
                                                         ix.first_line, h.lines, b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_search_rank(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 hits,
                        u32 k, SearchHits& h, SortPlan* h_plan, hipStream_t s) {
  LOCUST_CHECK_ARG(hits <= h.cap, "search: " + std::to_string(hits) +
                                      " hits exceed the workspace (" + std::to_string(h.cap) + ")");
  // (pattern terms' lists may overlap: a token may count for each of a query's eight terms)
  const u32 per_token = b.pat ? 32u * kSearchMaxTerms : 32u;
  LOCUST_CHECK_ARG(k >= 1 && ix.emits_per_line > 0 &&
                       (u64)ix.emits_per_line * per_token <= (u64)kRankScoreMax,
                   "search: a ranked batch takes K >= 1 and emits_per_line <= kRankMaxEmits (a "
                   "batch with a pattern term: an eighth of it)");
  // the segments of the sorted keys, and where each query's first min(hits, K) go
  search_scan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.q_hits, queries, ~0u, b.offsets,
                                                            nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  search_scan_kernel<<<dim3(1), dim3(kSearchBlock), 0, s>>>(b.q_hits, queries, k, b.out_off,
                                                            nullptr);
  LOCUST_HIP_LAUNCH_CHECK();
  if (hits == 0) return;
  // the phrase and near kernels are done with `cands`: the rank keys go there
  const u32 sblocks = (u32)std::min<u64>(div_up(hits, (u64)kSearchTile), (u64)kSearchMaxBlocks);
  search_score_kernel<<<dim3(sblocks), dim3(kSearchBlock), 0, s>>>(
      ix.postings, b.merged, ix.val, ix.n, ix.first_line, b.q_info, b.t_val, b.t_len, queries,
      per_token * (u32)ix.emits_per_line, h.pairs, hits, h.cands, b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
  ConstKeysSoA keys;
  KeysSoA sorted;
  keys.w[0] = h.cands;
  sorted.w[0] = h.sorted;
  for (int j = 1; j < kKeyWords; ++j) {
    keys.w[j] = h.zeros;
    sorted.w[j] = h.spare;  // the gather's copies of the zero words
  }
  radix_sort(keys, &b.ctr->sort_n, hits, h.rx, nullptr, sorted, nullptr, nullptr, h_plan, s);
  const u32 tblocks = (u32)std::min<u64>(div_up(hits, 256), 4096);
  search_top_kernel<<<dim3(tblocks), dim3(256), 0, s>>>(h.sorted, hits, b.offsets, b.out_off,
                                                        queries, k, ix.first_line, h.lines,
                                                        search_rank_scores(h), b.ctr);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_search() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&search_hit_kernel));
}

}  // namespace locust
