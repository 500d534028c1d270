// A test-only stand-in for <hip/hip_runtime.h>: just enough for
// csrc/m521_device.hpp and csrc/chacha_device.hpp to compile for the host
// (tests/host/opcheck_host.cpp).  One "lane" runs at a time.  Whether these
// stand-ins mean what the hardware does is what tests/test_gpu_device_ops.py
// settles: the same cases run on the device against the same references.
#pragma once

#include <cstdint>
#include <cstring>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))

namespace dn_shim {
inline uint64_t oob_count = 0;     // buffer accesses outside their descriptor
inline bool ballot_other = false;  // "another lane of my wave votes true"
}  // namespace dn_shim

inline uint64_t __umul64hi(uint64_t a, uint64_t b) {
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
}
inline uint32_t __umulhi(uint32_t a, uint32_t b) {
  return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32);
}
inline uint64_t __ballot(int pred) { return ((pred || dn_shim::ballot_other) ? 1ull : 0ull); }

// v_alignbit_b32: the low 32 bits of {hi, lo} >> (s & 31)
inline uint32_t __builtin_amdgcn_alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
  return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (s & 31u));
}

// A raw buffer descriptor: base and byte count.  An access that does not lie
// wholly inside is counted and dropped (a load gives 0), as the hardware's
// range check drops it.
struct dn_shim_rsrc {
  uint8_t* base;
  uint32_t bytes;
};
#define __amdgpu_buffer_rsrc_t dn_shim_rsrc

inline dn_shim_rsrc __builtin_amdgcn_make_buffer_rsrc(void* base, short /*stride*/, int num_records, int /*flags*/) {
  return dn_shim_rsrc{static_cast<uint8_t*>(base), static_cast<uint32_t>(num_records)};
}
template <typename T>
inline T dn_shim_buffer_load(dn_shim_rsrc r, uint32_t voff, int soff) {
  const uint64_t o = static_cast<uint64_t>(voff) + static_cast<uint32_t>(soff);
  T v{};
  if (o + sizeof(T) > r.bytes) ++dn_shim::oob_count;
  else std::memcpy(&v, r.base + o, sizeof(T));
  return v;
}
template <typename T>
inline void dn_shim_buffer_store(T v, dn_shim_rsrc r, uint32_t voff, int soff) {
  const uint64_t o = static_cast<uint64_t>(voff) + static_cast<uint32_t>(soff);
  if (o + sizeof(T) > r.bytes) ++dn_shim::oob_count;
  else std::memcpy(r.base + o, &v, sizeof(T));
}
inline uint32_t __builtin_amdgcn_raw_buffer_load_b32(dn_shim_rsrc r, uint32_t voff, int soff, int /*aux*/) {
  return dn_shim_buffer_load<uint32_t>(r, voff, soff);
}
inline uint16_t __builtin_amdgcn_raw_buffer_load_b16(dn_shim_rsrc r, uint32_t voff, int soff, int /*aux*/) {
  return dn_shim_buffer_load<uint16_t>(r, voff, soff);
}
inline void __builtin_amdgcn_raw_buffer_store_b32(uint32_t v, dn_shim_rsrc r, uint32_t voff, int soff, int /*aux*/) {
  dn_shim_buffer_store<uint32_t>(v, r, voff, soff);
}
inline void __builtin_amdgcn_raw_buffer_store_b16(uint16_t v, dn_shim_rsrc r, uint32_t voff, int soff, int /*aux*/) {
  dn_shim_buffer_store<uint16_t>(v, r, voff, soff);
}
