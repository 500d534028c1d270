// frame_plan.hpp — the layout of a share wire frame and which thread touches
// which byte of it in the frame kernels (csrc/codec_frame.hip).
//
// A frame (version 1, little-endian) is one wire — the records of
// dn_m521_encode_shares and their lengths — in one buffer:
//     bytes  0.. 7   magic "DNSHREC1"
//     bytes  8..15   n              u64   records in the frame
//     bytes 16..23   x              u64   the wire's abscissa
//     bytes 24..31   records_bytes  u64   = offsets[n]
//     bytes 32..     lens           u8[n], zero-padded to a multiple of 16
//     bytes R(n)..   the records, R(n) = 32 + 16 * ceil(n / 16)
// The lengths come first, so every position depends on n alone.
//
// dn_m521_frame_finish is one launch: offsets[n + 1] -> lens[n], the pad, the
// header.  dn_m521_frame_open is three: per-block totals of the lengths, one
// scan of the block totals per frame, and the expansion into int64 offsets.
// A workgroup of kFrameBlock threads owns kFrameElems consecutive elements in
// all of them; a thread's 16 lengths are one 16-byte word of the frame, and
// the int64 side is accessed interleaved (local element t + 256 j), the two
// orders meeting in LDS.  This header holds that index arithmetic — shared by
// the kernels and by a host program that replays the four launches on a model
// of memory (tests/host/frame_plan_check.cpp): it is the one place where a
// mistake reads or writes outside a frame or an offsets array.  Plain C++: no
// HIP header.
#pragma once

#include <stdint.h>

#include "wire_geom.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_FRAME_HD __host__ __device__ constexpr
#else
#define DN_FRAME_HD constexpr
#endif

namespace dn {

constexpr uint64_t kFrameMagic = 0x3143455248534E44ull;  // "DNSHREC1" read as a little-endian u64
constexpr uint32_t kFrameHeader = 32;                    // bytes before the lengths
// (a u8 holds every record length: wire_geom.hpp kMaxRecord)

constexpr uint32_t kFrameBlock = 256;                        // threads per workgroup
constexpr uint32_t kFrameWord = 16;                          // lengths per thread: one 16-byte word
constexpr uint32_t kFrameElems = kFrameBlock * kFrameWord;   // B: elements per workgroup (4096)
// a block's total (<= 4096 * 255) and every in-block prefix fit 32 bits
static_assert(static_cast<uint64_t>(kFrameElems) * 255u < (1ull << 32), "in-block sums are 32-bit");
// The scan of the block totals is wire_geom.hpp's.  Its shape under the frame
// names, for the host replay and for the frame tests, which build their edge
// lists from the two literals below as they read them in this file.
constexpr uint32_t kFrameScanThreads = 1024;
constexpr uint32_t kFrameScanRun = 8;  // totals per thread and pass
constexpr uint32_t kFrameScanStage = kScanStage;
static_assert(kFrameScanThreads == kScanThreads && kFrameScanRun == kScanRun, "the frame names follow the scan");

DN_FRAME_HD uint64_t frame_pad16(uint64_t n) { return (n + 15u) & ~15ull; }
// R(n): where the records start
DN_FRAME_HD uint64_t frame_records_offset(uint64_t n) { return kFrameHeader + frame_pad16(n); }

// Workgroups per frame.  Finish: one per B lengths of the padded length area,
// and one for a header-only frame.  Open: the offsets have n + 1 entries, so
// element n (whose "length" is zero) has a workgroup too.
DN_FRAME_HD uint64_t frame_finish_blocks(uint64_t n) {
  const uint64_t b = (frame_pad16(n) + kFrameElems - 1u) / kFrameElems;
  return b ? b : 1u;
}
DN_FRAME_HD uint64_t frame_open_blocks(uint64_t n) { return n / kFrameElems + 1u; }

// LDS word of a workgroup's local element i (0 .. B): one pad word per 16, so
// that both access orders — 16 consecutive elements per thread, and element
// t + 256 j — are free of bank conflicts.
DN_FRAME_HD uint32_t frame_slot(uint32_t i) { return i + (i >> 4); }
constexpr uint32_t kFrameLdsWords = kFrameElems + kFrameElems / 16 + 1;  // frame_slot(B) + 1

// Finish, load phase: local element i (0 .. B, B included: the end of the last
// length) of workgroup b is offsets[frame_finish_src(...)] — clamped to n, so
// that every length past n comes out as zero (the pad).  n > 0.
DN_FRAME_HD uint64_t frame_finish_src(uint64_t n, uint64_t b, uint32_t i) {
  const uint64_t e = b * kFrameElems + i;
  return e < n ? e : n;
}
// Finish, store phase: thread t of workgroup b stores the lengths of local
// elements 16 t .. 16 t + 15 as one 16-byte word at byte *pos of the length
// area (frame + 32 + *pos), if it lies inside the padded area.
DN_FRAME_HD bool frame_finish_store(uint64_t n, uint64_t b, uint32_t t, uint64_t* pos) {
  *pos = b * kFrameElems + static_cast<uint64_t>(t) * kFrameWord;
  return *pos < frame_pad16(n);
}

// Open, launches 1 and 3: thread t of workgroup b loads the 16-byte word at
// byte *pos of the length area if any of its elements is below n; *live of its
// bytes (1 .. 16) are lengths, the rest is pad and is not trusted to be zero.
DN_FRAME_HD bool frame_open_load(uint64_t n, uint64_t b, uint32_t t, uint64_t* pos, uint32_t* live) {
  *pos = b * kFrameElems + static_cast<uint64_t>(t) * kFrameWord;
  if (*pos >= n) return false;
  const uint64_t left = n - *pos;
  *live = left < kFrameWord ? static_cast<uint32_t>(left) : kFrameWord;
  return true;
}
// The interleaved order of the int64 side (finish's loads, open's stores): in
// step j (0 .. 15) thread t takes local element t + 256 j, so that a wave
// covers 512 contiguous bytes of offsets.
DN_FRAME_HD uint32_t frame_local(uint32_t t, uint32_t j) { return t + kFrameBlock * j; }
// Open, launch 3, store phase: thread t of workgroup b stores offsets[*e] of
// that element in step j, if *e <= n.
DN_FRAME_HD bool frame_open_store(uint64_t n, uint64_t b, uint32_t t, uint32_t j, uint64_t* e) {
  *e = b * kFrameElems + frame_local(t, j);
  return *e <= n;
}

// Open, launch 2: pass p takes the block totals [p * kFrameScanStage, ...) of
// a frame, frame_scan_count of them; thread t scans totals kFrameScanRun * t + j
// of the pass (wire_geom.hpp's arithmetic, which the kernel uses).
DN_FRAME_HD uint64_t frame_scan_passes(uint64_t nb) { return scan_passes(nb); }
DN_FRAME_HD uint32_t frame_scan_count(uint64_t nb, uint64_t p) { return scan_count(nb, p); }

}  // namespace dn
