// commit_sha256.hip — SHA-256 share commitments over wire records
// (dn_sha256_commit_records, dn_sha256_verify_records): digest e is
// utils.calc_commitment(packed[offsets[e]:offsets[e + 1]])
// (utils/commitment.py:5-12), the commitment the reference's runner computes
// per share before it seals it (runner/horizontal/agg.py:160-162) and that
// the receiver and the coordinator check before they use the share
// (runner/horizontal/agg.py:257-272, coord/horizontal/agg.py:309-318, 342-348).
//
// One record per lane; one wave = 64 consecutive records = one contiguous
// byte window, staged in LDS by the record-reading kernels' own functions
// (wire_parse.hpp: win_of, stage_direct; wire_geom.hpp: the geometry).  Word j
// of a lane's block b is the big-endian dword at record byte 64 b + 4 j: bswap
// of one v_alignbyte of two LDS dwords, as parse_lds builds limbs, then the
// padding of sha256_core.hpp's pad_word (bytes past the record masked off,
// 0x80 at byte len, the bit length in words 14-15 of the last block), without
// a branch.  The block loop runs to the wave's largest block count with the
// finished lanes switched off; share records (at most 75 bytes) take two
// blocks.  A window beyond kWinLimit (records padded with leading zero bytes)
// is hashed byte-serially, every lane reading its own record from global
// memory, through the same loop: records of any length.
//
// There is no arithmetic here: rounds, schedule and padding are
// sha256_core.hpp's, which a host program rehearses against hashlib
// (tests/host/sha256_check.cpp).  No multiply, no MFMA: the bound is VALU
// issue.  One launch, no scratch, no device table, nothing
// that synchronises.
#include <hip/hip_runtime.h>

#include "dn_commit.h"
#include "dn_internal.hpp"
#include "sha256_core.hpp"
#include "wire_parse.hpp"

namespace dn {
namespace commit {

constexpr int kBlock = 256;

struct Args {
  const uint8_t* in;  // packed records
  uint64_t in_bytes;
  const uint64_t* offsets;  // uint64[n + 1]
  uint64_t n;
  uint8_t* digests;       // commit: [n][32] written
  const uint8_t* expect;  // verify: [n][32] read
  uint8_t* ok;            // verify: [n] written, or null
  uint32_t* bad;          // [0] unhashable records, [1] mismatches (verify)
  bool w16;               // the wire is 16-B aligned (the wide staging path)
  bool d16;               // digests / expect is 16-B aligned (16-byte stores / loads)
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The big-endian dword at window byte q of the staged window (S[k] = dword at
// window byte 4 k); a q at or past `end`, the record's end, is held to the
// dword pair at `end` (what it returns there is masked off by the caller).
__device__ __forceinline__ uint32_t be_dword_lds(const uint32_t* S, uint32_t q, uint32_t end) {
  const uint32_t k = q < end ? q >> 2 : end >> 2;
  return __builtin_bswap32(__builtin_amdgcn_alignbyte(S[k + 1], S[k], q & 3u));
}

// The same from global memory, byte by byte: bytes at or past `end` read as zero.
__device__ __forceinline__ uint32_t be_dword_global(const uint8_t* __restrict__ in, uint64_t q, uint64_t end) {
  uint32_t v = 0;
#pragma unroll
  for (uint64_t i = 0; i < 4; ++i) v = (v << 8) | (q + i < end ? in[q + i] : 0u);
  return v;
}

template <bool VERIFY>
__global__ void __launch_bounds__(kBlock) sha_records_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kBlock / 64][kDecRowWords];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * kBlock + 64u * wv;
  if (e0 >= a.n) return;  // wave-uniform
  const uint64_t e = e0 + lane;
  const bool valid = e < a.n;
  const uint64_t eN = e0 + 64 < a.n ? e0 + 64 : a.n;
  const uint8_t* __restrict__ in = a.in;
  const Win w = win_of((OffTab)a.offsets, a.in_bytes, a.w16, e0, eN);
  // untrusted offsets: a window is usable inside the wire, a record hashable inside its window
  const bool usable = w.Bend >= w.A && w.Bend <= a.in_bytes;
  uint64_t oe = 0, ee = 0;
  if (valid) {
    oe = a.offsets[e];
    ee = a.offsets[e + 1];
  }
  const bool hashable = valid && usable && oe >= w.A && ee >= oe && ee <= w.Bend;
  const uint64_t len = hashable ? ee - oe : 0u;
  const uint64_t nb = hashable ? sha::blocks_of(len) : 0u;

  const uint32_t* S = s_win[wv] + kWinPad / 4;  // S[k] = dword at window byte 4k
  if (w.lds) {
    stage_direct(s_win[wv] + kWinPad / 4, in, w, a.w16, lane);
    lds_order();
  }
  // (on the LDS path the window, and so every record position, is below kWinLimit + 16)
  const uint32_t o32 = static_cast<uint32_t>(oe - w.A4), end32 = static_cast<uint32_t>(ee - w.A4);

  uint32_t h[8];
  sha::init(h);
  // to the wave's largest block count; a lane is off once its own blocks are done
  for (uint64_t b = 0; __any(b < nb); ++b) {
    if (b < nb) {
      uint32_t m[16];
      if (w.lds) {
        sha::load_block(m, [&](uint64_t p) { return be_dword_lds(S, o32 + static_cast<uint32_t>(p), end32); }, len, b,
                        b + 1 == nb);
      } else {
        sha::load_block(m, [&](uint64_t p) { return be_dword_global(in, oe + p, ee); }, len, b, b + 1 == nb);
      }
      sha::compress(h, m);
    }
  }

  bool mismatch = false;
  if (valid) {
    if constexpr (VERIFY) {
      const uint8_t* x = a.expect + 32 * e;
      uint32_t diff = 0;
      if (a.d16) {
        const u32x4 lo = reinterpret_cast<const u32x4*>(x)[0], hi = reinterpret_cast<const u32x4*>(x)[1];
        diff = (lo.x ^ __builtin_bswap32(h[0])) | (lo.y ^ __builtin_bswap32(h[1])) |
               (lo.z ^ __builtin_bswap32(h[2])) | (lo.w ^ __builtin_bswap32(h[3])) |
               (hi.x ^ __builtin_bswap32(h[4])) | (hi.y ^ __builtin_bswap32(h[5])) |
               (hi.z ^ __builtin_bswap32(h[6])) | (hi.w ^ __builtin_bswap32(h[7]));
      } else {
        const uint32_t* xw = reinterpret_cast<const uint32_t*>(x);
#pragma unroll
        for (int i = 0; i < 8; ++i) diff |= xw[i] ^ __builtin_bswap32(h[i]);
      }
      mismatch = hashable && diff != 0u;
      if (a.ok) a.ok[e] = hashable && !mismatch ? 1 : 0;
    } else {
      // digest byte 4 i is the top byte of word i; an unhashable record's digest is 32 zero bytes
      uint32_t d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] = hashable ? __builtin_bswap32(h[i]) : 0u;
      uint8_t* y = a.digests + 32 * e;
      if (a.d16) {
        u32x4 lo, hi;
        lo.x = d[0], lo.y = d[1], lo.z = d[2], lo.w = d[3];
        hi.x = d[4], hi.y = d[5], hi.z = d[6], hi.w = d[7];
        reinterpret_cast<u32x4*>(y)[0] = lo;
        reinterpret_cast<u32x4*>(y)[1] = hi;
      } else {
        uint32_t* yw = reinterpret_cast<uint32_t*>(y);
#pragma unroll
        for (int i = 0; i < 8; ++i) yw[i] = d[i];
      }
    }
  }
  const uint32_t nbad = static_cast<uint32_t>(__popcll(__ballot(valid && !hashable)));
  const uint32_t nmis = static_cast<uint32_t>(__popcll(__ballot(mismatch)));
  if (lane == 0) {
    if (nbad) atomicAdd(a.bad, nbad);
    if (VERIFY && nmis) atomicAdd(a.bad + 1, nmis);
  }
}

// [p, p + pn) and [q, q + qn) share a byte
static bool overlap(const void* p, uint64_t pn, const void* q, uint64_t qn) {
  const uint64_t p0 = reinterpret_cast<uint64_t>(p), q0 = reinterpret_cast<uint64_t>(q);
  return pn && qn && p0 < q0 + qn && q0 < p0 + pn;
}

static int run(const char* name, bool verify, const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets,
               uint64_t n, uint8_t* digests, const uint8_t* expect, uint8_t* ok, uint32_t* bad_counts, void* stream) {
  if (n == 0) return DN_OK;
  const void* words = verify ? static_cast<const void*>(expect) : static_cast<const void*>(digests);
  if (!in || !offsets || !words || !bad_counts) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  // the narrow path loads dwords from in + (an offset that is a multiple of 4)
  if (reinterpret_cast<uintptr_t>(in) & 3u) return set_error(DN_ERR_ARG, "%s: in must be 4-byte aligned", name);
  if (reinterpret_cast<uintptr_t>(offsets) & 7u)
    return set_error(DN_ERR_ARG, "%s: offsets must be 8-byte aligned", name);
  if (reinterpret_cast<uintptr_t>(words) & 3u)
    return set_error(DN_ERR_ARG, "%s: %s must be 4-byte aligned", name, verify ? "expect" : "digests");
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks >= (1ull << 31))
    return set_error(DN_ERR_ARG, "%s: n %llu needs 2^31 workgroups or more", name, (unsigned long long)n);
  if (!verify && overlap(digests, 32 * n, in, in_bytes)) return set_error(DN_ERR_ARG, "%s: digests overlaps in", name);
  if (verify && ok && overlap(ok, n, in, in_bytes)) return set_error(DN_ERR_ARG, "%s: ok overlaps in", name);
  Args a{};
  a.in = in;
  a.in_bytes = in_bytes;
  a.offsets = offsets;
  a.n = n;
  a.digests = digests;
  a.expect = expect;
  a.ok = ok;
  a.bad = bad_counts;
  a.w16 = (reinterpret_cast<uintptr_t>(in) & 15u) == 0;
  a.d16 = (reinterpret_cast<uintptr_t>(words) & 15u) == 0;
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (verify)
    hipLaunchKernelGGL(sha_records_kernel<true>, g, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(sha_records_kernel<false>, g, dim3(kBlock), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  return DN_OK;
}

}  // namespace commit
}  // namespace dn

using namespace dn;

extern "C" int dn_sha256_commit_records(const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets, uint64_t n,
                                        uint8_t* digests, uint32_t* bad_counts, void* stream) {
  return commit::run("dn_sha256_commit_records", false, in, in_bytes, offsets, n, digests, nullptr, nullptr,
                     bad_counts, stream);
}

extern "C" int dn_sha256_verify_records(const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets, uint64_t n,
                                        const uint8_t* expect, uint8_t* ok, uint32_t* bad_counts, void* stream) {
  return commit::run("dn_sha256_verify_records", true, in, in_bytes, offsets, n, nullptr, expect, ok, bad_counts,
                     stream);
}
