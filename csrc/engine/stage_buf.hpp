// Plain device buffers of the stage entry points (exch_stage.hip, dict_stage.hip): one
// hipMalloc per buffer, synchronous copies, freed with the object.  Nothing here goes
// through the engines' allocators or streams.
#pragma once

#include <algorithm>
#include <vector>

#include "locust/hip_check.hpp"
#include "locust/kernels.hpp"

namespace locust {
namespace stage {

constexpr u64 kStageMaxBytes = 1ull << 30;  // largest single buffer of a stage call

template <class T>
struct DevBuf {  // a plain device allocation of max(n, 1) elements
  T* p = nullptr;
  u64 n;
  explicit DevBuf(u64 count) : n(std::max<u64>(count, 1)) {
    LOCUST_CHECK_ARG(n * sizeof(T) <= kStageMaxBytes, "stage: buffer too large");
    LOCUST_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
  }
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void upload(const T* src, u64 count) {
    if (count) LOCUST_HIP_CHECK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void download(T* dst, u64 count) const {
    if (count) LOCUST_HIP_CHECK(hipMemcpy(dst, p, count * sizeof(T), hipMemcpyDeviceToHost));
  }
  std::vector<T> download_all() const {
    std::vector<T> v(n);
    download(v.data(), n);
    return v;
  }
  void fill(unsigned char byte) { fill(byte, n); }
  void fill(unsigned char byte, u64 count) {  // the first `count` elements
    if (count) LOCUST_HIP_CHECK(hipMemset(p, byte, count * sizeof(T)));
  }
};

struct DevKeys {  // packed keys, structure-of-arrays
  DevBuf<u64> w0, w1, w2, w3;
  explicit DevKeys(u64 n) : w0(n), w1(n), w2(n), w3(n) {}
  DevBuf<u64>& buf(int j) { return j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : w3; }
  u64* word(int j) { return buf(j).p; }
  KeysSoA soa() {
    KeysSoA k;
    for (int j = 0; j < kKeyWords; ++j) k.w[j] = word(j);
    return k;
  }
  void fill(unsigned char byte) {
    for (int j = 0; j < kKeyWords; ++j) buf(j).fill(byte);
  }
  template <class Rec>  // PackedKey or KeyCount: anything with w[kKeyWords]
  void upload(const Rec* recs, u64 n) {
    std::vector<u64> col(n);
    for (int j = 0; j < kKeyWords; ++j) {
      for (u64 i = 0; i < n; ++i) col[i] = recs[i].w[j];
      buf(j).upload(col.data(), n);
    }
  }
  void download(PackedKey* out, u64 n) {
    std::vector<u64> col(n);
    for (int j = 0; j < kKeyWords; ++j) {
      buf(j).download(col.data(), n);
      for (u64 i = 0; i < n; ++i) out[i].w[j] = col[i];
    }
  }
  std::vector<PackedKey> download_all() {
    std::vector<PackedKey> out(w0.n);
    download(out.data(), out.size());
    return out;
  }
};
static_assert(kKeyWords == 4, "DevKeys holds four word arrays");

inline void sync() { LOCUST_HIP_CHECK(hipStreamSynchronize(nullptr)); }

}  // namespace stage
}  // namespace locust
