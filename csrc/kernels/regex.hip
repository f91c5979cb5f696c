// The kernels of a search batch that has a regex term (kernels.hpp "regex.hip"; the semantics
// are engine.hpp "regex terms"): `/(king|queen)[!?]?/`, `/[A-Z][A-Z]+/` -- the index keys a
// regular expression matches as a whole.
//
// A regex term's words are a scattered set of dictionary ranks, as a pattern term's are, and
// everything behind the matcher is the pattern terms' machinery: the dictionary scan finds the
// words, the lookup reads their number and summed counts, the gather / radix-sort / strip stage
// merges the lists of two or more words, and the verify and show kernels match tokens with the
// same rule.  So this file holds no kernel body of its own.  It instantiates the bodies that
// search.hip, show.hip and fuzzy.hip instantiate (device/dictscan.hpp, device/verify.hpp,
// device/showwalk.hpp) at matcher level 3: the pattern matcher (device/glob.hpp), the fuzzy
// matcher (device/fuzzy.hpp) and the regex matcher (device/regex.hpp) side by side, chosen per
// term by wave-uniform flag bits -- a regex batch may hold pattern and fuzzy terms and the fold
// as well.
//
// Shape (gfx950, wave64): the siblings' shape, one key (the scan) or one token (the walks) per
// lane.  The matcher is the bit-parallel step of a Glushkov position automaton of at most 32
// positions: the state is one u32 per lane; the program (device/regex.hpp, 292 words, compiled
// on the host with the batch's fold) is wave-uniform, so first, last, the position count and
// follow[] come by scalar loads and the OR over follow[] runs on a scalar counter; only B[] is
// indexed per lane, by the lane's own key byte, through the vector cache.  The program is not
// staged in LDS: its 1168 bytes are read by every wave of the launch and stay cached, a lane's
// B[] read is one dword of eight 128-byte lines at the most, and a staged table would need a
// workgroup barrier pair per (tile, slot) in the scan and up to eight tables per wave in the
// walks.  Nothing is indexed in registers, nothing lands in scratch.
// A batch without a regex term launches nothing of this file.
#include "locust/device/dictscan.hpp"
#include "locust/device/showwalk.hpp"
#include "locust/device/verify.hpp"
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace {

constexpr int kTerms = (int)kSearchMaxTerms;

// ---- the dictionary scan ----
__global__ __launch_bounds__(kSearchBlock) void regex_match_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ keys,
    const u32* __restrict__ pq, u32 Q, u32* __restrict__ pw, const u32* __restrict__ rx) {
  search_match_body<3>(recs, n, keys, pq, Q, pw, rx);
}

__global__ __launch_bounds__(kSearchBlock) void regex_scatter_kernel(
    const OutRecord* __restrict__ recs, u32 n, const u64* __restrict__ val,
    const u32* __restrict__ postings, u32 first_line, const u64* __restrict__ pkeys,
    const u32* __restrict__ pq, u32 Q, const u32* __restrict__ x_len,
    const u64* __restrict__ x_start, u64 X, u64 cap, u32* __restrict__ cursor,
    u64* __restrict__ keys, const u32* __restrict__ rx) {
  search_scatter_body<3>(recs, n, val, postings, first_line, pkeys, pq, Q, x_len, x_start, X, cap,
                         cursor, keys, rx);
}

// ---- verify ----
__global__ __launch_bounds__(kPhraseBlock) void regex_phrase_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq,
    const u32* __restrict__ rx) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_phrase_body<3>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                        text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                        keys, Q, cands, pairs, pair_cap, q_hits, ctr, rx);
}

__global__ __launch_bounds__(kPhraseBlock) void regex_near_kernel(
    const char* __restrict__ text, u64 bytes, const u64* __restrict__ nl_pos,
    const MapCounters* __restrict__ lctr, DelimMask dm, int emits_per_line, int max_key_len,
    u32 group, const u32* __restrict__ q_meta, const u64* __restrict__ keys, u32 Q,
    const u64* __restrict__ cands, u64* __restrict__ pairs, u64 pair_cap,
    u32* __restrict__ q_hits, SearchCounters* __restrict__ ctr, const u32* __restrict__ pq,
    const u32* __restrict__ rx) {
  __shared__ unsigned char s_row[kPhraseWaves][dev::kLineRow];
  __shared__ u64 s_keys[kPhraseWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kPhraseWaves][kTerms];
  search_near_body<3>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], pq,
                      text, bytes, nl_pos, lctr, dm, emits_per_line, max_key_len, group, q_meta,
                      keys, Q, cands, pairs, pair_cap, q_hits, ctr, rx);
}

// ---- show ----
__global__ __launch_bounds__(kShowBlock) void regex_showmeasure_kernel(
    ShowJob j, const u32* __restrict__ rx) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<3, false>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j,
                      rx);
}

__global__ __launch_bounds__(kShowBlock) void regex_showwrite_kernel(
    ShowJob j, const u32* __restrict__ rx) {
  __shared__ unsigned char s_row[kShowWaves][dev::kLineRow];
  __shared__ u64 s_keys[kShowWaves][kTerms * kKeyWords];
  __shared__ u32 s_meta[kShowWaves][kTerms];
  show_body<3, true>(s_row[dev::wave_id()], s_keys[dev::wave_id()], s_meta[dev::wave_id()], j, rx);
}

}  // namespace

// (every launch below stands where a sibling of search.hip or show.hip would: that launch
// function has checked the batch, the index view and the workspace)
void launch_regex_match(const SearchIndex& ix, const SearchBatch& b, u32 queries, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.regex && ix.n, "search: the regex scan needs the pattern arrays");
  regex_match_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
      ix.recs, ix.n, b.keys, b.pat, queries, b.pat + kSearchPatWords, b.regex);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_regex_scatter(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 x,
                          const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.regex && ix.n, "search: the regex scan needs the pattern arrays");
  regex_scatter_kernel<<<match_grid(ix.n, queries), dim3(kSearchBlock), 0, s>>>(
      ix.recs, ix.n, ix.val, ix.postings, ix.first_line, b.keys, b.pat, queries, b.x_len,
      b.x_start, x, h.cap, b.pat + kSearchPatCursor, h.pairs, b.regex);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_regex_phrase(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                         const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.regex && bound, "search: the regex verify needs the pattern arrays");
  u32 group = 0;
  const u32 blocks = verify_grid(bound, &group);
  regex_phrase_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
      ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
      b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat, b.regex);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_regex_near(const SearchIndex& ix, const SearchBatch& b, u32 queries, u64 bound,
                       const SearchHits& h, hipStream_t s) {
  LOCUST_CHECK_ARG(b.pat && b.regex && bound, "search: the regex verify needs the pattern arrays");
  u32 group = 0;
  const u32 blocks = verify_grid(bound, &group);
  regex_near_kernel<<<dim3(blocks), dim3(kPhraseBlock), 0, s>>>(
      ix.text, ix.bytes, ix.nl_pos, ix.lctr, ix.dm, ix.emits_per_line, ix.max_key_len, group,
      b.q_meta, b.keys, queries, h.cands, h.pairs, h.cap, b.q_hits, b.ctr, b.pat, b.regex);
  LOCUST_HIP_LAUNCH_CHECK();
}

void launch_regex_show(const ShowJob& j, const u32* rx, u32 blocks, bool write, hipStream_t s) {
  LOCUST_CHECK_ARG(j.pq && rx && blocks, "show: the regex walk needs the pattern arrays");
  if (write)
    regex_showwrite_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j, rx);
  else
    regex_showmeasure_kernel<<<dim3(blocks), dim3(kShowBlock), 0, s>>>(j, rx);
  LOCUST_HIP_LAUNCH_CHECK();
}

void warm_module_regex() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&regex_match_kernel));
}

}  // namespace locust
