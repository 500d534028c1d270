// wire_geom.hpp — the numbers every kernel that reads or writes share wire
// records agrees on: the record size, the LDS window a wave stages 64 records
// in, and the shape of the one-workgroup scan of block totals.
//
// A record is [len(xb)][xb][yb] (shamir.py:28-33): one length byte, x's minimal
// big-endian bytes (at most 8) and y's (at most 66 from the encoder; the
// decoder accepts leading zero bytes).  64 consecutive records are one
// contiguous byte window; the receiving kernels (wire_parse.hpp) stage it in
// LDS when it fits kWinLimit and parse byte-serially from global memory when
// it does not, the sending kernels (wire_emit.hpp) assemble it in LDS and flush
// it as aligned chunks.  Defined here once: the kernels, frame_plan.hpp and a
// host program (tests/host/wire_geom_check.cpp) read the same values.  Plain
// C++, no HIP header (lds_order alone is for the device compiler).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_WIRE_HD __host__ __device__ constexpr
#else
#define DN_WIRE_HD constexpr
#endif

namespace dn {

constexpr int kMaxRecord = 1 + 8 + 66;  // [len][x up to 8 bytes][y up to 66 bytes]
static_assert(kMaxRecord <= 255, "a u8 holds every record length");

// the receiving side: one wave's window of 64 records
constexpr int kWinPad = 16;  // LDS bytes before / after each wave's window
constexpr int kDecWindow = 64 * kMaxRecord + 8;
constexpr int kWinLimit = kDecWindow + 12;  // Bend - A4 at most this on the LDS path
constexpr int kDecRowWords = ((kDecWindow + 16 + 2 * kWinPad) / 4 + 3) & ~3;  // 16-B aligned rows
// loads per lane that cover the largest LDS-path window
constexpr int kStageQ = (kWinLimit / 16 + 63) / 64;  // 16-B loads (wide path)
constexpr int kStageW = (kWinLimit / 4 + 63) / 64;   // 4-B loads (narrow path)
constexpr int kStageRegs = 4 * kStageQ > kStageW ? 4 * kStageQ : kStageW;

// the sending side: 64 records of the encoder's and the up to 15 bytes
// between the 16-B boundary and the window's start
constexpr int kEncRowWords = ((64 * kMaxRecord + 8 + 16) / 4 + 2 + 3) & ~3;  // 16-B aligned rows

// The exclusive scan of block totals in one workgroup (wire_emit.hpp
// scan_block_totals): a pass stages kScanStage totals in LDS as 32-bit words,
// thread t scans the run kScanRun * t .. kScanRun * t + kScanRun - 1 of them,
// and every run is followed by one pad word (no bank conflicts).
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanRun = 8;                            // totals per thread and pass
constexpr uint32_t kScanStage = kScanThreads * kScanRun;    // totals per pass (8192)
constexpr uint32_t kScanLdsWords = kScanStage + kScanStage / kScanRun;  // runs and their pad words: 36 KB
// pass p takes the totals [p * kScanStage, ...), scan_count of them
DN_WIRE_HD uint64_t scan_passes(uint64_t nb) { return (nb + kScanStage - 1u) / kScanStage; }
DN_WIRE_HD uint32_t scan_count(uint64_t nb, uint64_t p) {
  const uint64_t left = nb - p * kScanStage;
  return left < kScanStage ? static_cast<uint32_t>(left) : kScanStage;
}

#if defined(__HIPCC__)
// A wave's window slice belongs to that wave alone: its LDS stores are made
// visible to its own later LDS loads (and the reverse) without a workgroup barrier.
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

}  // namespace dn
