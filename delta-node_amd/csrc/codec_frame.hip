// codec_frame.hip — share wire frames: one wire (the records of
// dn_m521_encode_shares, reference shamir.py:28-45) and its record lengths in
// one self-describing buffer that the envelope can seal as it stands.
//
// The record calls speak (packed, offsets[n + 1]); records are not
// self-delimiting ([len(xb)][xb][yb] carries no length for yb), so the offsets
// have to travel.  A frame carries them as u8 lengths in front of the records
// (layout and index arithmetic: frame_plan.hpp).  The encoder writes its
// records at frame + R(n) itself — nothing is copied:
//
//   dn_m521_frame_finish   one launch for all wires of a call: offsets ->
//       lengths (one 16-byte store per thread), the zero pad and the header,
//       records_bytes = offsets[n] included, all on the device.
//   dn_m521_frame_open     three launches for all frames of a call: per-block
//       totals of the lengths (a thread's 16 lengths are one 16-byte load,
//       summed by four v_sad_u8), one scan of the block totals per frame
//       (wire_emit.hpp, the encoders' scan), and the expansion into int64
//       offsets, which meets the element-interleaved store order in LDS so
//       that every wave-level store covers 512 contiguous bytes.  No workgroup
//       waits on another.
//
// The frame is the second grid dimension; the per-frame descriptors travel in
// the kernel arguments (up to DN_M521_FRAME_GROUP frames a launch; the entry
// points chain longer lists), read by scalar loads: no device table, nothing
// that synchronises.  Frames come off the wire: whatever their bytes say, every
// offset written is min(prefix, frame_bytes - R(n)) — monotone and inside the
// `packed` view — and the faults are counted in a device flag.
#include <hip/hip_runtime.h>

#include "dn_internal.hpp"
#include "frame_plan.hpp"
#include "wire_emit.hpp"

namespace dn {
namespace fr {

constexpr int kGroup = DN_M521_FRAME_GROUP;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct FinWire {
  const uint64_t* offsets;  // uint64[n + 1]
  uint8_t* frame;
  uint64_t x;
};
struct FinArgs {
  FinWire w[kGroup];
  uint64_t n;
};
static_assert(sizeof(FinArgs) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

struct OpenWire {
  const uint8_t* frame;
  uint64_t rec_bytes;  // frame_bytes - R(n): the size of the `packed` view (host-known)
  uint64_t x;
  uint64_t* offsets;  // uint64[n + 1], written
};
struct OpenArgs {
  OpenWire w[kGroup];
  uint64_t n;
  uint64_t nb;    // frame_open_blocks(n)
  uint64_t* tot;  // [frames of this launch][nb] block totals, then their exclusive scan
  uint32_t* bad;  // [0] frames with a wrong header, [1] frames whose lengths do not sum to rec_bytes
};
static_assert(sizeof(OpenArgs) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

// offsets[n + 1] -> lens[n], pad, header.  The low dwords of a workgroup's
// B + 1 offsets are staged in LDS by coalesced loads (a length is the
// difference of two neighbours mod 256); thread t then packs the lengths of
// local elements 16 t .. 16 t + 15 into one 16-byte store.  Elements past n
// read offsets[n], so the pad is written as zero by the same stores.
__global__ void __launch_bounds__(kFrameBlock) frame_finish_kernel(const FinArgs a) {
  __shared__ uint32_t s[kFrameLdsWords];
  const uint32_t t = threadIdx.x;
  const uint64_t b = blockIdx.x, n = a.n;
  const FinWire& w = a.w[blockIdx.y];
  if (n) {
    const uint32_t* lo = reinterpret_cast<const uint32_t*>(w.offsets);  // little-endian: dword 2 i of entry i
#pragma unroll
    for (uint32_t j = 0; j < kFrameWord; ++j) {
      const uint32_t i = frame_local(t, j);
      s[frame_slot(i)] = lo[2u * frame_finish_src(n, b, i)];
    }
    if (t == 0) s[frame_slot(kFrameElems)] = lo[2u * frame_finish_src(n, b, kFrameElems)];
    __syncthreads();
    uint64_t pos;
    if (frame_finish_store(n, b, t, &pos)) {
      uint32_t v[kFrameWord + 1];
#pragma unroll
      for (uint32_t j = 0; j <= kFrameWord; ++j) v[j] = s[frame_slot(kFrameWord * t + j)];
      uint32_t q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        q[k] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[k] |= ((v[4 * k + i + 1] - v[4 * k + i]) & 0xFFu) << (8 * i);
      }
      u32x4 o;
      o.x = q[0];
      o.y = q[1];
      o.z = q[2];
      o.w = q[3];
      *reinterpret_cast<u32x4*>(w.frame + kFrameHeader + pos) = o;
    }
  }
  if (b == 0 && t == 0) {
    uint64_t* h = reinterpret_cast<uint64_t*>(w.frame);
    h[0] = kFrameMagic;
    h[1] = n;
    h[2] = w.x;
    h[3] = n ? w.offsets[n] : 0u;
  }
}

// A thread's 16 lengths: one 16-byte load, the bytes at and past element n
// (pad, not trusted to be zero) cleared.  Zero where the thread has none.
__device__ __forceinline__ u32x4 load_lens(const uint8_t* frame, uint64_t n, uint64_t b, uint32_t t) {
  u32x4 q = {0u, 0u, 0u, 0u};
  uint64_t pos;
  uint32_t live;
  if (frame_open_load(n, b, t, &pos, &live)) {
    q = *reinterpret_cast<const u32x4*>(frame + kFrameHeader + pos);
    if (live < kFrameWord) {
      uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int keep = static_cast<int>(live) - 4 * k;  // bytes of dword k that are lengths
        d[k] = keep >= 4 ? d[k] : (keep <= 0 ? 0u : (d[k] & ((1u << (8 * keep)) - 1u)));
      }
      q.x = d[0];
      q.y = d[1];
      q.z = d[2];
      q.w = d[3];
    }
  }
  return q;
}

// the sum of 16 bytes: four byte-sum instructions (v_sad_u8 against zero)
__device__ __forceinline__ uint32_t sum16(u32x4 q) {
  uint32_t s = __builtin_amdgcn_sad_u8(q.x, 0u, 0u);
  s = __builtin_amdgcn_sad_u8(q.y, 0u, s);
  s = __builtin_amdgcn_sad_u8(q.z, 0u, s);
  return __builtin_amdgcn_sad_u8(q.w, 0u, s);
}

// Open, launch 1: tot[frame][b] = the sum of workgroup b's lengths; workgroup
// 0 of a frame also checks the header against what the caller expects.
__global__ void __launch_bounds__(kFrameBlock) frame_totals_kernel(const OpenArgs a) {
  __shared__ uint32_t s_w[kFrameBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint64_t b = blockIdx.x;
  const OpenWire& w = a.w[blockIdx.y];
  uint32_t sum = sum16(load_lens(w.frame, a.n, b, t));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d);
  if (lane == 0) s_w[wv] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t tot = 0;
#pragma unroll
    for (int i = 0; i < static_cast<int>(kFrameBlock / 64); ++i) tot += s_w[i];
    a.tot[blockIdx.y * a.nb + b] = tot;
    if (b == 0) {
      const uint64_t* h = reinterpret_cast<const uint64_t*>(w.frame);
      if (h[0] != kFrameMagic || h[1] != a.n || h[2] != w.x || h[3] != w.rec_bytes) atomicAdd(a.bad, 1u);
    }
  }
}

// Open, launch 2: exclusive scan of a frame's block totals in one workgroup
// (the frame is blockIdx.y).  The grand total is compared with the size of
// the `packed` view.
__global__ void __launch_bounds__(kScanThreads) frame_scan_kernel(const OpenArgs a) {
  const uint64_t total = scan_block_totals(a.tot + blockIdx.y * a.nb, a.nb);
  if (threadIdx.x == 0 && total != a.w[blockIdx.y].rec_bytes) atomicAdd(a.bad + 1, 1u);
}

// Open, launch 3: the lengths again, their exclusive prefix inside the
// workgroup (16 per thread, then across lanes by shuffles, then across the 4
// waves), transposed through LDS to the interleaved order, plus the block base,
// clamped, stored as int64 — 512 contiguous bytes per wave-level store.
__global__ void __launch_bounds__(kFrameBlock) frame_expand_kernel(const OpenArgs a) {
  __shared__ uint32_t s[kFrameLdsWords];
  __shared__ uint32_t s_w[kFrameBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint64_t b = blockIdx.x, n = a.n;
  const OpenWire& w = a.w[blockIdx.y];
  const u32x4 q = load_lens(w.frame, n, b, t);
  const uint32_t sum = sum16(q);
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t run = inc - sum;  // exclusive prefix of this thread's 16 lengths
#pragma unroll
  for (int i = 0; i < static_cast<int>(kFrameBlock / 64); ++i) run += (i < static_cast<int>(wv)) ? s_w[i] : 0u;
  const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      s[frame_slot(kFrameWord * t + 4u * k + i)] = run;
      run += (d[k] >> (8u * i)) & 0xFFu;
    }
  }
  __syncthreads();
  const uint64_t base = a.tot[blockIdx.y * a.nb + b], cap = w.rec_bytes;
#pragma unroll
  for (uint32_t j = 0; j < kFrameWord; ++j) {
    uint64_t e;
    if (frame_open_store(n, b, t, j, &e)) {
      const uint64_t v = base + s[frame_slot(frame_local(t, j))];
      w.offsets[e] = v < cap ? v : cap;
    }
  }
}

}  // namespace fr
}  // namespace dn

using namespace dn;

// the tile limit of the other record calls: ceil(n / 256) workgroups below 2^31
static bool too_many_tiles(uint64_t n) { return (n + 255u) / 256u >= (1ull << 31); }

extern "C" uint64_t dn_m521_frame_records_offset(uint64_t n_elem) { return frame_records_offset(n_elem); }

extern "C" uint64_t dn_m521_frame_capacity(uint64_t n_elem, uint64_t x) {
  return frame_records_offset(n_elem) + dn_m521_encoded_capacity(n_elem, x);
}

extern "C" uint64_t dn_m521_frame_scratch_bytes(uint64_t n_elem, uint64_t m) {
  return m * frame_open_blocks(n_elem) * 8u;
}

extern "C" int dn_m521_frame_finish(const uint64_t* const* offsets, uint8_t* const* frames, const uint64_t* xs,
                                    uint64_t m, uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_frame_finish";
  if (m == 0) return set_error(DN_ERR_ARG, "%s: no wire", name);
  if (!offsets || !frames || !xs) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (too_many_tiles(n_elem))
    return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name, (unsigned long long)n_elem);
  for (uint64_t i = 0; i < m; ++i) {
    if (!offsets[i] || !frames[i]) return set_error(DN_ERR_ARG, "%s: null wire %llu", name, (unsigned long long)i);
    // the lengths go out as 16-byte words at frame + 32 + (a multiple of 16)
    if (reinterpret_cast<uintptr_t>(frames[i]) & 15u)
      return set_error(DN_ERR_ARG, "%s: frame of wire %llu must be 16-byte aligned", name, (unsigned long long)i);
    if (reinterpret_cast<uintptr_t>(offsets[i]) & 7u)
      return set_error(DN_ERR_ARG, "%s: offsets of wire %llu must be 8-byte aligned", name, (unsigned long long)i);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t gx = static_cast<uint32_t>(frame_finish_blocks(n_elem));
  for (uint64_t first = 0; first < m; first += fr::kGroup) {
    fr::FinArgs a{};
    const uint32_t k = static_cast<uint32_t>(m - first < fr::kGroup ? m - first : fr::kGroup);
    for (uint32_t i = 0; i < k; ++i) {
      a.w[i].offsets = offsets[first + i];
      a.w[i].frame = frames[first + i];
      a.w[i].x = xs[first + i];
    }
    a.n = n_elem;
    hipLaunchKernelGGL(fr::frame_finish_kernel, dim3(gx, k), dim3(kFrameBlock), 0, s, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  }
  return DN_OK;
}

extern "C" int dn_m521_frame_open(const uint8_t* const* frames, const uint64_t* frame_bytes, const uint64_t* xs,
                                  uint64_t m, uint64_t n_elem, uint64_t* const* offsets_out, uint32_t* bad_counts,
                                  void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* name = "dn_m521_frame_open";
  if (m == 0) return set_error(DN_ERR_ARG, "%s: no frame", name);
  if (!frames || !frame_bytes || !xs || !offsets_out || !bad_counts || !scratch)
    return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (too_many_tiles(n_elem))
    return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name, (unsigned long long)n_elem);
  const uint64_t R = frame_records_offset(n_elem);
  for (uint64_t i = 0; i < m; ++i) {
    if (!frames[i] || !offsets_out[i]) return set_error(DN_ERR_ARG, "%s: null frame %llu", name, (unsigned long long)i);
    // the lengths are loaded as 16-byte words from frame + 32 + (a multiple of 16)
    if (reinterpret_cast<uintptr_t>(frames[i]) & 15u)
      return set_error(DN_ERR_ARG, "%s: frame %llu must be 16-byte aligned", name, (unsigned long long)i);
    if (reinterpret_cast<uintptr_t>(offsets_out[i]) & 7u)
      return set_error(DN_ERR_ARG, "%s: offsets of frame %llu must be 8-byte aligned", name, (unsigned long long)i);
    if (frame_bytes[i] < R)
      return set_error(DN_ERR_ARG, "%s: frame %llu has %llu bytes, fewer than the %llu before its records", name,
                       (unsigned long long)i, (unsigned long long)frame_bytes[i], (unsigned long long)R);
  }
  if (reinterpret_cast<uintptr_t>(scratch) & 7u) return set_error(DN_ERR_ARG, "%s: scratch must be 8-byte aligned", name);
  if (scratch_bytes < dn_m521_frame_scratch_bytes(n_elem, m)) return set_error(DN_ERR_ARG, "%s: scratch too small", name);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t nb = frame_open_blocks(n_elem);
  const uint32_t gx = static_cast<uint32_t>(nb);
  for (uint64_t first = 0; first < m; first += fr::kGroup) {
    fr::OpenArgs a{};
    const uint32_t k = static_cast<uint32_t>(m - first < fr::kGroup ? m - first : fr::kGroup);
    for (uint32_t i = 0; i < k; ++i) {
      a.w[i].frame = frames[first + i];
      a.w[i].rec_bytes = frame_bytes[first + i] - R;
      a.w[i].x = xs[first + i];
      a.w[i].offsets = offsets_out[first + i];
    }
    a.n = n_elem;
    a.nb = nb;
    a.tot = static_cast<uint64_t*>(scratch) + first * nb;  // every frame of the call has its own totals
    a.bad = bad_counts;
    hipLaunchKernelGGL(fr::frame_totals_kernel, dim3(gx, k), dim3(kFrameBlock), 0, s, a);
    hipLaunchKernelGGL(fr::frame_scan_kernel, dim3(1, k), dim3(kScanThreads), 0, s, a);
    hipLaunchKernelGGL(fr::frame_expand_kernel, dim3(gx, k), dim3(kFrameBlock), 0, s, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  }
  return DN_OK;
}
