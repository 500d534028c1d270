// codec_m521.hip — the share wire codec over whole vectors.
//
// Reference (delta_node/crypto/shamir/shamir.py:28-45, serialize/hex.py:44-50):
//   _share_to_bytes((x, y)) = bytes([len(xb)]) + xb + yb,
//   xb / yb = minimal big-endian bytes (0 -> b"").
// The vector form encodes share x of every element into one packed byte
// stream (records back to back) plus int64 offsets[n + 1]; record e is
// exactly the reference's bytes for (x, y_e).  Decoding parses records back
// into a tiled vector (and each record's x).
//
// Encode = three launches: (1) per 1024-element block: record lengths and
// their in-block exclusive scan, block total; (2) scan of the block totals;
// (3) per wave: records assembled in LDS at their final byte positions
// (mod 4 aligned like the destination), then written out as aligned dwords
// plus a few head/tail bytes, so global writes stay contiguous and wide.
#include <hip/hip_runtime.h>

#include <cstring>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "wire_emit.hpp"
#include "wire_parse.hpp"

namespace dn {

constexpr int kCodecBlock = 256;
constexpr int kScanElems = 1024;       // elements per scan block (4 per thread)

struct XBytes {
  uint32_t len;
  uint8_t b[8];  // big-endian minimal bytes of x
};

// y length of element w of a tile from limbs 15 .. 0 (the top limb was zero)
__device__ __noinline__ uint32_t y_len_low(const uint8_t* tb, uint32_t w) {
  for (int i = 15; i >= 0; --i) {
    const uint32_t l = reinterpret_cast<const uint32_t*>(tb)[i * kTile + w];
    if (l) return 4u * i + limb_bytes(l);
  }
  return 0u;
}

// Per 1024-element block: record lengths of 4 consecutive elements per thread
// (one 8-B load of their top-limb u16s: the only read unless a top limb is
// zero, odds 2^-9), their in-block exclusive prefix (wave scans by shuffles,
// then across the 4 waves) as one 16-B store per thread, and the block total.
__global__ void __launch_bounds__(kCodecBlock) lengths_scan_kernel(const uint8_t* __restrict__ vec, uint64_t n,
                                                                    uint32_t xlen, uint32_t* __restrict__ local,
                                                                    uint64_t* __restrict__ block_tot) {
  __shared__ uint32_t s_w[kCodecBlock / 64];
  const uint64_t b = blockIdx.x;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint64_t e0 = b * kScanElems + t * 4;  // 4 consecutive elements, one tile (256 % 4 == 0)
  uint32_t len[4] = {0u, 0u, 0u, 0u};
  if (e0 < n) {
    const uint8_t* tb = tile_base(vec, static_cast<uint32_t>(e0 / kTile));
    const uint32_t w0 = static_cast<uint32_t>(e0 % kTile);
    uint16_t top[4];
    if (e0 + 4 <= n) {
      const uint64_t q = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(tb + kHiOffset) + w0 / 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) top[j] = static_cast<uint16_t>(q >> (16 * j));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) top[j] = e0 + j < n ? reinterpret_cast<const uint16_t*>(tb + kHiOffset)[w0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e0 + j < n) {
        const uint32_t tp = top[j] & kTopMask;
        len[j] = 1u + xlen + (tp ? 64u + limb_bytes(tp) : y_len_low(tb, w0 + j));
      }
    }
  }
  const uint32_t sum = len[0] + len[1] + len[2] + len[3];
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t wbase = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kCodecBlock / 64; ++w) {
    wbase += (w < static_cast<int>(wv)) ? s_w[w] : 0u;
    tot += s_w[w];
  }
  uint32_t run = wbase + inc - sum;  // exclusive prefix of this thread's 4 elements
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 o;
  o.x = run;
  o.y = run + len[0];
  o.z = run + len[0] + len[1];
  o.w = run + len[0] + len[1] + len[2];
  if (e0 + 4 <= n) {
    __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(local + e0));
  } else {
    const uint32_t ov[4] = {o.x, o.y, o.z, o.w};
    for (int j = 0; j < 4; ++j)
      if (e0 + j < n) local[e0 + j] = ov[j];
  }
  if (t == 0) block_tot[b] = tot;
}

// Exclusive scan of the block totals in one workgroup, and their grand total.
__global__ void __launch_bounds__(kScanThreads) scan_blocks_kernel(uint64_t* __restrict__ tot, uint64_t nb,
                                                                   uint64_t* __restrict__ total_out) {
  const uint64_t total = scan_block_totals(tot, nb);
  if (threadIdx.x == 0) *total_out = total;
}

// One wave = 64 consecutive elements = one contiguous run of records.  Each
// lane lays its record into the wave's LDS window at its final byte position:
// the 1 + xlen header bytes one by one, then y (lay_y); the window is then
// written to HBM as aligned chunks (flush_window).  W16: `out` is 16-B aligned,
// so the window is laid out from the 16-B boundary at or below its start and
// the body goes out as 16-B stores (else 4-B ones).
template <bool W16>
__global__ void __launch_bounds__(kCodecBlock) encode_kernel(const uint8_t* __restrict__ vec, uint64_t n, XBytes xb,
                                                             const uint32_t* __restrict__ local,
                                                             const uint64_t* __restrict__ block_pre,
                                                             uint64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t s_buf[kCodecBlock / 64][kEncRowWords];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t e = (static_cast<uint64_t>(blockIdx.x) * kCodecBlock) + threadIdx.x;
  const bool valid = e < n;
  const uint64_t vmask = __ballot(valid);
  if (!vmask) return;  // wave-uniform: the whole wave is past the end
  uint32_t v[kLimbs];
  uint64_t off = 0;
  uint32_t ylen = 0;
  if (valid) {
    load_fe(tile_base(vec, static_cast<uint32_t>(e / kTile)), static_cast<uint32_t>(e % kTile), v);
    ylen = y_len(v);
    off = block_pre[e / kScanElems] + local[e];
    offsets[e] = off;
    if (e == n - 1) offsets[n] = off + 1 + xb.len + ylen;
  }
  // the wave's byte range [A, B)
  const uint64_t A = __shfl(off, 0);
  const uint32_t last = static_cast<uint32_t>(63 - __builtin_clzll(vmask));
  const uint64_t endl = off + (valid ? 1 + xb.len + ylen : 0);
  const uint64_t B = __shfl(endl, last);
  const uint64_t A4 = W16 ? (A & ~15ull) : (A & ~3ull);  // LDS byte 0 of the window
  uint8_t* sb = reinterpret_cast<uint8_t*>(s_buf[wv]);
  if (valid) {
    const int32_t p = static_cast<int32_t>(off - A4);
    sb[p] = static_cast<uint8_t>(xb.len);
    for (uint32_t i = 0; i < xb.len; ++i) sb[p + 1 + i] = xb.b[i];
    if (ylen) lay_y(s_buf[wv], p + 1 + static_cast<int32_t>(xb.len), static_cast<int32_t>(ylen), v);
  }
  flush_window(s_buf[wv], out, A, B, A4, W16, lane);
}

// Decode record e -> element e of a tiled vector (+ its x).  y is reduced
// mod p (resolve_shares reduces ys the same way, shamir.py:86-88).  Records
// whose y has more than 68 significant bytes, or whose x is longer than
// 8 bytes, are counted in *bad and stored as 0 (the caller re-decodes them).
//
// One wave = 64 consecutive records = one contiguous byte window, staged in LDS
// and parsed by wire_parse.hpp.  W16: the input is 16-B aligned, so the window
// is staged with 16-B loads and LDS stores from the 16-B boundary at or below
// its start (else 4-B ones).
template <bool W16>
__global__ void __launch_bounds__(kCodecBlock) decode_kernel(const uint8_t* __restrict__ in, uint64_t in_bytes,
                                                             const uint64_t* __restrict__ offsets, uint64_t n,
                                                             uint8_t* __restrict__ vec, uint64_t* __restrict__ xs,
                                                             uint32_t* __restrict__ bad) {
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kCodecBlock / 64][kDecRowWords];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t e0 = (static_cast<uint64_t>(blockIdx.x) * kCodecBlock) + (threadIdx.x & ~63u);
  if (e0 >= n) return;  // wave-uniform
  const uint64_t e = e0 + lane;
  const bool valid = e < n;
  const uint64_t eN = e0 + 64 < n ? e0 + 64 : n;
  const Win w = win_of(offsets, in_bytes, W16, e0, eN);
  uint64_t x = 0;
  uint32_t v[kLimbs];
  bool ok = false;
  if (w.lds) {
    uint32_t* S = s_win[wv] + kWinPad / 4;  // S[k] = dword at window byte 4k
    stage_direct(S, in, w, W16, lane);
    lds_order();
    if (valid) ok = parse_lds(S, w, offsets[e], offsets[e + 1], x, v);
  } else if (valid) {
    const uint64_t oe = offsets[e], ee = offsets[e + 1];
    ok = oe < ee && ee <= in_bytes && parse_global(in, oe, ee, x, v);
  }
  if (!valid) return;
  if (ok) {
    reduce(v);
  } else {
#pragma unroll
    for (int i = 0; i < kLimbs; ++i) v[i] = 0u;
    atomicAdd(bad, 1u);
  }
  store_fe(tile_base(vec, static_cast<uint32_t>(e / kTile)), static_cast<uint32_t>(e % kTile), v);
  if (xs) xs[e] = x;
}

}  // namespace dn

using namespace dn;

extern "C" uint64_t dn_m521_codec_scratch_bytes(uint64_t n_elem) {
  const uint64_t nb = (n_elem + kScanElems - 1) / kScanElems;
  return n_elem * 4 + nb * 8 + 8 + 256;
}

extern "C" uint64_t dn_m521_encoded_capacity(uint64_t n_elem, uint64_t x) {
  uint32_t xl = 0;
  while (xl < 8 && (x >> (8 * xl))) ++xl;
  return n_elem * (1 + xl + 66);
}

extern "C" int dn_m521_encode_shares(const void* vec, uint64_t n_elem, uint64_t x, uint64_t* offsets, uint8_t* out,
                                     uint64_t capacity, void* scratch, uint64_t scratch_bytes, void* stream) {
  if (n_elem == 0) return DN_OK;
  if (!vec || !offsets || !out || !scratch) return set_error(DN_ERR_ARG, "dn_m521_encode_shares: null pointer");
  // the narrow path stores dwords at out + (an offset that is a multiple of 4)
  if (reinterpret_cast<uintptr_t>(out) & 3u)
    return set_error(DN_ERR_ARG, "dn_m521_encode_shares: out must be 4-byte aligned");
  if (capacity < dn_m521_encoded_capacity(n_elem, x))
    return set_error(DN_ERR_ARG, "dn_m521_encode_shares: capacity %llu < %llu", (unsigned long long)capacity,
                     (unsigned long long)dn_m521_encoded_capacity(n_elem, x));
  if (scratch_bytes < dn_m521_codec_scratch_bytes(n_elem))
    return set_error(DN_ERR_ARG, "dn_m521_encode_shares: scratch too small");
  XBytes xb;
  std::memset(&xb, 0, sizeof(xb));
  while (xb.len < 8 && (x >> (8 * xb.len))) ++xb.len;
  for (uint32_t i = 0; i < xb.len; ++i) xb.b[i] = static_cast<uint8_t>(x >> (8 * (xb.len - 1 - i)));
  const uint64_t nb = (n_elem + kScanElems - 1) / kScanElems;
  uint32_t* local = static_cast<uint32_t*>(scratch);
  uint64_t* tot = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(scratch) + ((n_elem * 4 + 15) & ~15ull));
  uint64_t* total = tot + nb;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* v = static_cast<const uint8_t*>(vec);
  hipLaunchKernelGGL(lengths_scan_kernel, dim3(static_cast<uint32_t>(nb)), dim3(kCodecBlock), 0, s, v, n_elem,
                     xb.len, local, tot);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, tot, nb, total);
  const uint64_t blocks = (n_elem + kCodecBlock - 1) / kCodecBlock;
  bool w16 = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
#ifdef DN_TUNING
  if (tune_env("DN_ENCODE_W4") && tune_env("DN_ENCODE_W4")[0] == '1') w16 = false;  // A/B: 4-B stores
#endif
  if (w16)
    hipLaunchKernelGGL(encode_kernel<true>, dim3(static_cast<uint32_t>(blocks)), dim3(kCodecBlock), 0, s, v, n_elem,
                       xb, local, tot, offsets, out);
  else
    hipLaunchKernelGGL(encode_kernel<false>, dim3(static_cast<uint32_t>(blocks)), dim3(kCodecBlock), 0, s, v, n_elem,
                       xb, local, tot, offsets, out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_m521_encode_shares: %s", hipGetErrorString(err));
  return DN_OK;
}

extern "C" int dn_m521_decode_shares(const uint8_t* in, uint64_t in_bytes, const uint64_t* offsets, uint64_t n_elem,
                                     void* vec, uint64_t* xs, uint32_t* bad_count, void* stream) {
  if (n_elem == 0) return DN_OK;
  if (!in || !offsets || !vec || !bad_count) return set_error(DN_ERR_ARG, "dn_m521_decode_shares: null pointer");
  // the narrow path loads dwords from in + (an offset that is a multiple of 4)
  if (reinterpret_cast<uintptr_t>(in) & 3u)
    return set_error(DN_ERR_ARG, "dn_m521_decode_shares: in must be 4-byte aligned");
  const uint64_t blocks = (n_elem + kCodecBlock - 1) / kCodecBlock;
  bool w16 = (reinterpret_cast<uintptr_t>(in) & 15u) == 0;
#ifdef DN_TUNING
  if (tune_env("DN_DECODE_W4") && tune_env("DN_DECODE_W4")[0] == '1') w16 = false;  // A/B: 4-B staging
#endif
  if (w16)
    hipLaunchKernelGGL(decode_kernel<true>, dim3(static_cast<uint32_t>(blocks)), dim3(kCodecBlock), 0,
                       static_cast<hipStream_t>(stream), in, in_bytes, offsets, n_elem, static_cast<uint8_t*>(vec), xs,
                       bad_count);
  else
    hipLaunchKernelGGL(decode_kernel<false>, dim3(static_cast<uint32_t>(blocks)), dim3(kCodecBlock), 0,
                       static_cast<hipStream_t>(stream), in, in_bytes, offsets, n_elem, static_cast<uint8_t*>(vec), xs,
                       bad_count);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_m521_decode_shares: %s", hipGetErrorString(err));
  return DN_OK;
}
