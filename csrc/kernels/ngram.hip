// Word n-gram map (Map stage, fast path): one record per n-gram of a line.
//
// The tile is the word map's (map_tile.hpp, tokenize.hip) with kGram > 1: the same staging,
// delimiter masks, line ordinals, slices, partition grouping, per-tile combining and
// counters, so everything downstream reads its output as it reads the word map's.  Two
// things differ:
//
//  * Which token starts emit.  The n-gram g_i = t_i ' ' ... ' ' t_(i+N-1) is emitted at the
//    start of t_i, so a live token start emits iff its in-line ordinal is below the emit cap
//    and N - 1 further words follow it in its line (no '\n', no NUL and no end of text in
//    between).  Most starts decide that from the ballot masks of their own step and the next
//    64 bytes (gram_follows); a word or a delimiter run that reaches past that window is
//    walked byte by byte through TileText::at, which reads LDS inside the staged range and
//    the text (with its bounds) outside it.  A delimiter run has no upper bound, so
//    correctness never depends on the staged size; the tile stages a 128-byte overhang
//    (kPostGram) so that nearly every walk stays in LDS.
//  * The key.  The words of an n-gram start at arbitrary offsets and its separators are
//    not the text's delimiters, so the key is assembled byte by byte (walk_gram) into four
//    u64 registers with static indices: the first max_key_len bytes of the joined words.
//    The full joined length feeds `truncated`.  The large tiles' token list keeps offsets
//    only; both sweeps walk the n-gram again.
//
// N-grams never cross a line: a line is the map's record, as in the reference's per-line
// map().
#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"
#include "map_tile.hpp"

namespace locust {
namespace {

using namespace maptile;

template <int kGram, int kSteps, int kBlock>
__global__ __launch_bounds__(kBlock) void map_ngram_kernel(
    const char* __restrict__ text, u64 bytes, Delims d, int E, int max_key, KeysSoA out,
    u8* __restrict__ parts, u64 out_cap, MapCounters* __restrict__ ctr, u64* __restrict__ trace,
    u32* __restrict__ part_off, PartMap pm, u64* __restrict__ counts, u32* __restrict__ part_occ,
    u32* __restrict__ plan_flag) {
  __shared__ MapTileLds<kSteps, kBlock, kPostGram> lds;
  const u32 tile = xcd_tile(blockIdx.x, gridDim.x);
  map_tile<kSteps, kBlock, kGram, kPostGram>(lds, tile, text, bytes, d, E, max_key, out, parts,
                                             out_cap, ctr, trace, part_off, pm, counts, part_occ,
                                             plan_flag);
}

template <int kGram>
void launch_gram(const char* text, u64 bytes, const Delims& d, int emits_per_line, int max_key_len,
                 KeysSoA out, u8* parts, u64 out_cap, MapCounters* ctr, hipStream_t s, u64* trace,
                 u32* part_off, PartMap pm, bool large_tiles, u64* counts, u32* part_occ,
                 u32* plan_flag) {
  // the word map's two tile shapes and their argument rules (launch_map_fast)
  if (bytes < kMapLargeInput && !large_tiles) {
    const u64 tiles = div_up(bytes, (u64)kMapTileBytesMin);
    constexpr int kBlock = kMapTileBytesMin;
    map_ngram_kernel<kGram, 1, kBlock><<<dim3((u32)tiles), dim3(kBlock), 0, s>>>(
        text, bytes, d, emits_per_line, max_key_len, out, parts, out_cap, ctr, trace, part_off, pm,
        nullptr, part_off ? part_occ : nullptr, part_off && part_occ ? plan_flag : nullptr);
  } else {
    constexpr int kTile = (kMapBlock / 64) * kMapSegStepsLarge * 64;
    const u64 tiles = div_up(bytes, (u64)kTile);
    map_ngram_kernel<kGram, kMapSegStepsLarge, kMapBlock>
        <<<dim3((u32)tiles), dim3(kMapBlock), 0, s>>>(text, bytes, d, emits_per_line, max_key_len,
                                                      out, parts, out_cap, ctr, trace, part_off, pm,
                                                      part_off ? counts : nullptr, nullptr, nullptr);
  }
  LOCUST_HIP_LAUNCH_CHECK();
}

}  // namespace

void launch_map_ngram(int ngram, const char* text, u64 bytes, const DelimMask& dm,
                      int emits_per_line, int max_key_len, KeysSoA out, u8* parts, u64 out_cap,
                      MapCounters* ctr, hipStream_t s, u64* trace, u32* part_off, PartMap pm,
                      bool large_tiles, u64* counts, u32* part_occ, u32* plan_flag) {
  LOCUST_CHECK_ARG(ngram >= 2 && ngram <= kMaxNgram,
                   "n-gram map: ngram must be in [2, " + std::to_string(kMaxNgram) + "]");
  static_assert(kMaxNgram == 3, "one instantiation per n-gram length");
  if (bytes == 0) return;
  const Delims d{dm.m[0] | 1ull | (1ull << '\n'), dm.m[1], dm.m[2], dm.m[3]};
  if (ngram == 2)
    launch_gram<2>(text, bytes, d, emits_per_line, max_key_len, out, parts, out_cap, ctr, s, trace,
                   part_off, pm, large_tiles, counts, part_occ, plan_flag);
  else
    launch_gram<3>(text, bytes, d, emits_per_line, max_key_len, out, parts, out_cap, ctr, s, trace,
                   part_off, pm, large_tiles, counts, part_occ, plan_flag);
}

// Loads this file's code object (one module per file) now rather than at its first launch.
void warm_module_ngram() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&map_ngram_kernel<2, 1, 1024>));
}

}  // namespace locust
