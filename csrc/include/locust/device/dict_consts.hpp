// Sizes of the dictionary kernels (dict.hip) and of the in-job partition plan
// (partplan.hip) that their stage tests build inputs from: table and window sizes, probe
// limits, the plan's sample count and weights.  Host and device; the bindings expose them
// (dict_constants), so the tests hold no copies.
#pragma once

#include "locust/common.hpp"

namespace locust {

// Words 1..3 of a table slot are stored XOR kWordMagic: a packed key word can never equal
// kWordMagic (bytes 00 00 FF FF 00 00 FF FF: a NUL followed by non-NUL bytes), so a stored 0
// means "not written yet" and a zero-initialised table needs no sentinel fill.
constexpr u64 kWordMagic = 0x0000FFFF0000FFFFull;
constexpr u32 kIdFull = 0xFFFFFFFFu;  // slot id of a key that did not fit the dense arrays

// dict_insert_kernel: the workgroup's LDS cache in front of the HBM table
constexpr int kInsBlock = 256;
constexpr int kLdsSlots = 1024;
constexpr int kLdsProbes = 8;

// dict_part_build_kernel and the ordered kernels: one LDS table per workgroup
constexpr int kPartBlock = 1024;       // 16 waves: latency hiding for the gathers
constexpr int kPartSlots = 2048;       // 80 KB of LDS
constexpr int kPartWindow = kPartBlock * 16;  // partition bytes scanned per round
// A key not placed within kPartProbes slots reports the table full (the caller falls back):
// probing a nearly full table to the end made an overflowing pass quadratic.  (512: a
// planned range holds up to ~1,500 of the 2,048 slots; linear probing at 75 % load runs
// clusters past 128.)
constexpr int kPartProbes = 512;

// rank_sort_kernel: rank[i] += #{ j in tile : key[j] < key[i] } over (i-tile, j-tile) pairs
constexpr int kRankI = 256;
constexpr int kRankJ = 256;

// scan_pack_kernel
constexpr int kPackItems = 8;
constexpr int kPackTile = 256 * kPackItems;

// part_plan_kernel.  Sizing, from an offline replay of the plan on the generator's 1M-line
// text (fullest range of the whole pass, in distinct keys; the mean is 792): 2,048 samples
// of a 512 KiB prefix 3,100 (sampling noise, ~8 samples per range); 8,192 1,800; 8,192 of a
// 1 MiB prefix, singletons weighted 9x, 1,768 -- the setting here; 16,384 of 1.5 MiB 1,477,
// but the larger sample and sort cost ~0.4 ms of compute in front of the first piece's map.
constexpr u32 kPlanSamples = 8192;
// A key the prefix saw once (a hapax) stands for the rare keys of the whole pass the prefix
// has not seen yet (Good-Turing): it weighs kSingletonWeight, a repeated key 1.
constexpr u32 kSingletonWeight = 9;

}  // namespace locust
