// The kernels of a search batch that has a fuzzy term (kernels.hpp "fuzzy.hip"; the semantics
// are engine.hpp "fuzzy terms"): `word~1`, `word~2` -- the index keys within a bounded edit
// distance of a word.
//
// A fuzzy term's words are a scattered set of dictionary ranks, as a pattern term's are, and
// everything behind the matcher is the pattern terms' machinery: the dictionary scan finds the
// words, the lookup reads their number and summed counts, the gather / radix-sort / strip stage
// merges the lists of two or more words, and the verify and show kernels match tokens with the
// same rule.  So this file holds no kernel body of its own.  It instantiates the bodies that
// search.hip and show.hip instantiate (device/dictscan.hpp, device/verify.hpp,
// device/showwalk.hpp) at matcher level 2: the pattern matcher (device/glob.hpp) and the fuzzy
// matcher (device/fuzzy.hpp) side by side, chosen per term by a wave-uniform flag bit -- a
// fuzzy batch may hold pattern terms and the fold as well.
//
// Shape (gfx950, wave64): the siblings' shape.  The matcher is a banded Levenshtein row update:
// five cells and five key bytes in registers, len(w) rows on a scalar counter (the word is
// wave-uniform: scalar loads in the scan, one LDS address in the walks), after a length filter.
// Nothing is indexed, nothing lands in scratch, and no per-lane loop mask stays alive.
// A batch without a fuzzy term launches nothing of this file.
#include "locust/device/dictscan.hpp"
#include "locust/device/showwalk.hpp"
#include "locust/device/verify.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;

// ---- the dictionary scan ----
__global__ __launch_bounds__(kSearchBlock) void fuzzy_match_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ keys,
    const u32* __restrict__ pq, u32 Q, u32* __restrict__ pw) {
  search_match_body<2>(recs, n, keys, pq, Q, pw);
}

__global__ __launch_bounds__(kSearchBlock) void fuzzy_scatter_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ val,
    const u32* __restrict__ postings, u32 first_line, const u64* __restrict__ pkeys,
    const u32* __restrict__ pq, u32 Q, const u32* __restrict__ x_len,
    const u64* __restrict__ x_start, u64 X, u64 cap, u32* __restrict__ cursor,
    u64* __restrict__ keys) {
  search_scatter_body<2>(recs, n, val, postings, first_line, pkeys, pq, Q, x_len, x_start, X, cap,
                         cursor, keys);
}

// ---- verify ----
__global__ __launch_bounds__(kPhraseBlock) void fuzzy_phrase_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_phrase_body<2>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                        text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                        keys, Q, cands, pairs, pair_cap, q_hits, ctr);
}

__global__ __launch_bounds__(kPhraseBlock) void fuzzy_near_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_near_body<2>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                      text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                      keys, Q, cands, pairs, pair_cap, q_hits, ctr);
}

// ---- show ----
__global__ __launch_bounds__(kShowBlock) void fuzzy_showmeasure_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<2, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
}

__global__ __launch_bounds__(kShowBlock) void fuzzy_showwrite_kernel(ShowJob j) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<2, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j);
}

}  // namespace

// (every launch below stands where a sibling of search.hip or show.hip would: that launch
// function has checked the batch, the index view and the workspace)
void launch_fuzzy_match(const SearchIndex& ix, const SearchBatch& b, u32 queries, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.fuzzy && ix.n, "search: the fuzzy scan needs the pattern arrays");
  fuzzy_match_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
      ix.recs, ix.n, b.keys, b.pat, queries, b.pat + kSearchPatWords);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_fuzzy_scatter(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.fuzzy && ix.n, "search: the fuzzy scan needs the pattern arrays");
  fuzzy_scatter_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
      ix.recs, ix.n, ix.val, ix.postings, ix.first_line, b.keys, b.pat, queries, b.x_len,
      b.x_start, x, h.cap, b.pat + kSearchPatCursor, h.pairs);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_fuzzy_phrase(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                         const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.fuzzy && bound, "search: the fuzzy verify needs the pattern arrays");
  u32 group = 0;
  const u32 blocks = verify_grid(bound, &group);
  fuzzy_phrase_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
      ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
      b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_fuzzy_near(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                       const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.fuzzy && bound, "search: the fuzzy verify needs the pattern arrays");
  u32 group = 0;
  const u32 blocks = verify_grid(bound, &group);
  fuzzy_near_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
      ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
      b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_fuzzy_show(const ShowJob& j, u32 blocks, bool write, hipStream_t s) {
  LOCUST_CHECK_ARG(j.pq && blocks, "show: the fuzzy walk needs the pattern arrays");
  if (write)
    fuzzy_showwrite_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  else
    fuzzy_showmeasure_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_fuzzy() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&fuzzy_match_kernel));
}

}  // namespace locust
