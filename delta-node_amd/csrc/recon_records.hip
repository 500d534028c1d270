// recon_records.hip — reconstruct straight from wire records
// (dn_m521_reconstruct_records): the k packed `_share_to_bytes` streams of
// shamir.py:28-33 in, the secrets of `resolve_shares` (shamir.py:68-90) out, in
// one launch and without the k intermediate tiled vectors.
//
// Per element e and wire i the kernel parses record e of wire i with the
// functions decode_kernel (codec_m521.hip) parses with (wire_parse.hpp: the
// window staged in LDS, the byte-serial path for a window beyond the LDS
// slice, the treatment of untrusted offsets), reduces y, negates it where the
// weight is negative, accumulates |a_i| * y (mac_wide) and, after the last
// wire, finishes as recon_finish (shamir_m521.hip) does.  The finish is a copy
// of that one with a different INV = 1 product.  There is no
// arithmetic of its own here: every primitive is m521_device.hpp's.
//
// One wave = 64 consecutive elements (decode_kernel's unit), one workgroup =
// one 256-element output tile, one LDS slice per wave, reused wire after wire
// (the wire loop below).  A wire's whole window is loaded into registers (at most 5
// 16-byte or 19 4-byte loads per lane, all issued before the first LDS store)
// and then stored to LDS: kSerial.  Loading wire i + 1 under wire i's
// arithmetic (kAhead) was no faster at k = 3 and k = 5, and decode_kernel's
// staging loop (kDirect) 20-30 % slower; both are A/B only.
#include <hip/hip_runtime.h>

#include <cstring>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "wire_parse.hpp"

namespace dn {
namespace rr {

constexpr int kBlock = 256;

struct Wire {
  const uint8_t* in;        // packed records
  uint64_t in_bytes;
  const uint64_t* offsets;  // uint64[n_elem + 1]
  uint64_t x;               // the abscissa every record should carry
};

struct Args {
  Wire wire[DN_MAX_RESOLVE];
  uint8_t* out_fe;
  int64_t* out_u64;
  uint32_t* overflow;
  uint32_t* bad;  // [0] unrepresentable records, [1] records whose x is not the wire's
  uint64_t n_elem;
  int32_t k;
  uint32_t neg;
  uint32_t shift;
  uint32_t w16;  // bit i: wire i is 16-B aligned (the wide staging path)
  uint32_t a[DN_MAX_RESOLVE][kLimbs];
  uint32_t inv[kLimbs];
  uint32_t d, d_inv32, p_inv_d, pad;
  uint64_t d_recip;
  uint32_t w[kLimbs];
};
static_assert(sizeof(Args) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

// recon_finish (shamir_m521.hip) for element w of output tile `tile`: S
// reduced, divided by d and 2^shift, stored; returns whether it is >= 2^64.
template <int A, int INV>
__device__ __forceinline__ bool finish(const Args& a, uint32_t tile, uint32_t w, uint32_t (&S)[A + kLimbs]) {
  constexpr int N = A + kLimbs;
  constexpr int VB = (A == kLimbs) ? 1046 : (521 + 32 * A + 4);
  uint32_t r[kLimbs];
  reduce_wide<N, VB>(S, r);
  if constexpr (INV == 1) {
    // mulmod's two steps with the carry-rippling mac_wide: its FRESH form
    // leaves a 16-byte stack slot per lane in this kernel (in reconstruct_kernel
    // the same slot is promoted to LDS); the product is the same integer.
    uint32_t P[2 * kLimbs];
#pragma unroll
    for (int l = 0; l < 2 * kLimbs; ++l) P[l] = 0u;
    mac_wide<2 * kLimbs, kLimbs>(P, a.inv, r);
    reduce_wide<2 * kLimbs, 1042>(P, r);
  } else if constexpr (INV == 2) {
    exact_div_small(r, a.d, a.d_inv32, a.p_inv_d, a.d_recip, a.w);
  }
  if (a.shift != 0u) rotr521(r, a.shift);
  if (a.out_fe) store_fe(tile_base(a.out_fe, tile), w, r);
  if (a.out_u64) {
    const uint64_t lo = static_cast<uint64_t>(r[0]) | (static_cast<uint64_t>(r[1]) << 32);
    __builtin_nontemporal_store(static_cast<int64_t>(lo), a.out_u64 + static_cast<uint64_t>(tile) * kTile + w);
  }
  uint32_t hi_or = 0u;
#pragma unroll
  for (int l = 2; l < kLimbs; ++l) hi_or |= r[l];
  return hi_or != 0u;
}

// Wire i of one lane: its record parsed from the staged window (or from
// global memory where the window did not fit), y reduced, negated where the
// weight is, |a_i| * y added to acc; the wave's two counts.
template <int A>
__device__ __forceinline__ void wire_step(const Args& a, int32_t i, const uint32_t* S, const Win& cw, uint64_t oe,
                                          uint64_t ee, bool valid, uint32_t (&acc)[A + kLimbs], uint32_t& nbad,
                                          uint32_t& nmis) {
  bool ok = false;
  uint64_t x = 0;
  if (valid) {
    uint32_t v[kLimbs];
    if (cw.lds) {
      ok = parse_lds(S, cw, oe, ee, x, v);
    } else {
      ok = oe < ee && ee <= a.wire[i].in_bytes && parse_global(a.wire[i].in, oe, ee, x, v);
    }
    if (ok) {
      reduce(v);
    } else {  // counted below; contributes y = 0, as the decoded vector would
#pragma unroll
      for (int l = 0; l < kLimbs; ++l) v[l] = 0u;
    }
    if ((a.neg >> i) & 1u) {  // -y == p - y == ~y within 521 bits
#pragma unroll
      for (int l = 0; l < 16; ++l) v[l] = ~v[l];
      v[16] = (~v[16]) & kTopMask;
    }
    mac_wide<A + kLimbs, A>(acc, a.a[i], v);
  }
  nbad += static_cast<uint32_t>(__popcll(__ballot(valid && !ok)));
  nmis += static_cast<uint32_t>(__popcll(__ballot(valid && ok && x != a.wire[i].x)));
}

// The end of a wave's work: the element finished and stored, the counters.
template <int A, int INV>
__device__ __forceinline__ void wave_end(const Args& a, uint32_t tile, uint32_t lane, bool valid,
                                         uint32_t (&acc)[A + kLimbs], uint32_t nbad, uint32_t nmis) {
  bool over = false;
  if (valid) over = finish<A, INV>(a, tile, threadIdx.x, acc);
  if (a.overflow) {
    const uint64_t m = __ballot(over);
    if (lane == 0 && m) atomicAdd(a.overflow, static_cast<uint32_t>(__popcll(m)));
  }
  if (lane == 0) {
    if (nbad) atomicAdd(a.bad, nbad);
    if (nmis) atomicAdd(a.bad + 1, nmis);
  }
}

// A, INV as reconstruct_kernel's; K > 0: compile-time wire count (the wire
// loop unrolled), K == 0: runtime count.
template <int A, int INV, int K, int PF>
__device__ __forceinline__ void records_body(const Args& a, uint32_t (*s_win)[kDecRowWords]) {
  constexpr int N = A + kLimbs;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = blockIdx.x;  // one workgroup per 256-element output tile
  const uint64_t e0 = static_cast<uint64_t>(tile) * kTile + 64u * wv;
  if (e0 >= a.n_elem) return;  // wave-uniform
  const uint64_t e = e0 + lane;
  const bool valid = e < a.n_elem;
  const uint64_t eN = e0 + 64 < a.n_elem ? e0 + 64 : a.n_elem;
  uint32_t* S = s_win[wv] + kWinPad / 4;  // S[j] = dword at window byte 4j
  const int32_t k = K > 0 ? K : a.k;

  uint32_t acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0u;
  uint32_t nbad = 0u, nmis = 0u;  // wave-uniform counts
  constexpr int kUnroll = K > 0 ? K : 1;

  if constexpr (PF == kDirect) {
#pragma unroll kUnroll
    for (int32_t i = 0; i < k; ++i) {
      const bool w16 = (a.w16 >> i) & 1u;
      const Win cw = win_of((OffTab)a.wire[i].offsets, a.wire[i].in_bytes, w16, e0, eN);
      uint64_t oe = 0, ee = 0;
      if (valid) {
        oe = a.wire[i].offsets[e];
        ee = a.wire[i].offsets[e + 1];
      }
      if (cw.lds) stage_direct(S, a.wire[i].in, cw, w16, lane);
      lds_order();
      wire_step<A>(a, i, S, cw, oe, ee, valid, acc, nbad, nmis);
      lds_order();  // the slice is free for the next window
    }
  } else {
    Stage st;
    Win nw = win_of((OffTab)a.wire[0].offsets, a.wire[0].in_bytes, a.w16 & 1u, e0, eN);
    uint64_t noe = 0, nee = 0;
    if (nw.lds) stage_load(st, a.wire[0].in, nw, a.w16 & 1u, lane);
    if (valid) {
      noe = a.wire[0].offsets[e];
      nee = a.wire[0].offsets[e + 1];
    }
#pragma unroll kUnroll
    for (int32_t i = 0; i < k; ++i) {
      const Win cw = nw;
      const uint64_t oe = noe, ee = nee;
      if (cw.lds) stage_store(st, S, cw, (a.w16 >> i) & 1u, lane);
      lds_order();
      if (PF == kAhead && i + 1 < k) {  // wire i + 1's loads go out before wire i's arithmetic
        const bool w16n = (a.w16 >> (i + 1)) & 1u;
        nw = win_of((OffTab)a.wire[i + 1].offsets, a.wire[i + 1].in_bytes, w16n, e0, eN);
        if (nw.lds) stage_load(st, a.wire[i + 1].in, nw, w16n, lane);
        if (valid) {
          noe = a.wire[i + 1].offsets[e];
          nee = a.wire[i + 1].offsets[e + 1];
        }
      }
      wire_step<A>(a, i, S, cw, oe, ee, valid, acc, nbad, nmis);
      lds_order();  // the slice is free for the next window
      if (PF == kSerial && i + 1 < k) {
        const bool w16n = (a.w16 >> (i + 1)) & 1u;
        nw = win_of((OffTab)a.wire[i + 1].offsets, a.wire[i + 1].in_bytes, w16n, e0, eN);
        if (nw.lds) stage_load(st, a.wire[i + 1].in, nw, w16n, lane);
        if (valid) {
          noe = a.wire[i + 1].offsets[e];
          nee = a.wire[i + 1].offsets[e + 1];
        }
      }
    }
  }
  wave_end<A, INV>(a, tile, lane, valid, acc, nbad, nmis);
}

template <int A, int INV, int K, int PF>
__global__ void __launch_bounds__(kBlock) recon_records_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kBlock / 64][kDecRowWords];
  records_body<A, INV, K, PF>(a, s_win);
}

// A/B hooks of the tuning build: DN_RR_UNROLL=0 selects the runtime-k kernel,
// DN_RR_STAGE=0/1/2 one staging mode for every k.
static bool rr_unroll() {
  const char* e = tune_env("DN_RR_UNROLL");
  return !(e && e[0] == '0');
}

template <int A, int INV, int K, int PF>
static void launch_one(dim3 g, hipStream_t s, const Args& a) {
  hipLaunchKernelGGL((recon_records_kernel<A, INV, K, PF>), g, dim3(kBlock), 0, s, a);
}

template <int A, int INV, int K, int PF>
static void launch_mode(dim3 g, hipStream_t s, const Args& a) {
#ifdef DN_TUNING
  if (const char* e = tune_env("DN_RR_STAGE")) {
    if (e[0] == '0') launch_one<A, INV, K, kSerial>(g, s, a);
    else if (e[0] == '1') launch_one<A, INV, K, kAhead>(g, s, a);
    else launch_one<A, INV, K, kDirect>(g, s, a);
    return;
  }
#endif
  launch_one<A, INV, K, PF>(g, s, a);
}

template <int A, int INV>
static void launch(int k, dim3 g, hipStream_t s, const Args& a) {
  if constexpr (A == 1) {  // as reconstruct_kernel: unrolled counts for one-limb weights only, where they pay
    if (rr_unroll()) {
      switch (k) {
        case 2: launch_mode<A, INV, 2, kSerial>(g, s, a); return;
        case 3: launch_mode<A, INV, 3, kSerial>(g, s, a); return;
        default: break;  // at k = 5 the unrolled form was no faster than the runtime one
      }
    }
  }
  launch_mode<A, INV, 0, kSerial>(g, s, a);
}

}  // namespace rr
}  // namespace dn

using namespace dn;

extern "C" int dn_m521_reconstruct_records(const uint8_t* const* in, const uint64_t* in_bytes,
                                           const uint64_t* const* offsets, const uint64_t* xs,
                                           const dn_m521_lagrange_t* w, void* out_fe, int64_t* out_u64,
                                           uint32_t* overflow_count, uint32_t* bad_counts, uint64_t n_elem,
                                           void* stream) {
  const char* name = "dn_m521_reconstruct_records";
  if (n_elem == 0) return DN_OK;
  if (!in || !in_bytes || !offsets || !xs || !w || !bad_counts)
    return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (w->k < 2 || w->k > DN_MAX_RESOLVE)
    return set_error(DN_ERR_ARG, "%s: k=%d outside 2..%d", name, w->k, DN_MAX_RESOLVE);
  if (!(w->a_limbs == 1 || w->a_limbs == 2 || w->a_limbs == 17) || w->shift < 0 || w->shift > 31)
    return set_error(DN_ERR_ARG, "%s: malformed weights", name);
  const int inv = w->has_inv;
  if (inv < 0 || inv > 2 || (inv == 2 && (w->d < 3 || w->d >= 65536 || !(w->d & 1))))
    return set_error(DN_ERR_ARG, "%s: malformed divisor", name);
  if (!out_fe && !out_u64) return set_error(DN_ERR_ARG, "%s: no output", name);
  const uint64_t blocks = (n_elem + kTile - 1) / kTile;
  if (blocks >= (1ull << 31)) return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name,
                                               (unsigned long long)n_elem);
  rr::Args a{};
  for (int i = 0; i < w->k; ++i) {
    if (!in[i] || !offsets[i]) return set_error(DN_ERR_ARG, "%s: null wire %d", name, i);
    // the narrow path loads dwords from in + (an offset that is a multiple of 4)
    if (reinterpret_cast<uintptr_t>(in[i]) & 3u)
      return set_error(DN_ERR_ARG, "%s: wire %d must be 4-byte aligned", name, i);
    if (reinterpret_cast<uintptr_t>(offsets[i]) & 7u)
      return set_error(DN_ERR_ARG, "%s: offsets of wire %d must be 8-byte aligned", name, i);
    a.wire[i].in = in[i];
    a.wire[i].in_bytes = in_bytes[i];
    a.wire[i].offsets = offsets[i];
    a.wire[i].x = xs[i];
    if ((reinterpret_cast<uintptr_t>(in[i]) & 15u) == 0) a.w16 |= 1u << i;
  }
#ifdef DN_TUNING
  if (tune_env("DN_DECODE_W4") && tune_env("DN_DECODE_W4")[0] == '1') a.w16 = 0u;  // A/B: 4-B staging
#endif
  a.out_fe = static_cast<uint8_t*>(out_fe);
  a.out_u64 = out_u64;
  a.overflow = overflow_count;
  a.bad = bad_counts;
  a.n_elem = n_elem;
  a.k = w->k;
  a.neg = w->neg;
  a.shift = static_cast<uint32_t>(w->shift);
  std::memcpy(a.a, w->a, sizeof(a.a));
  std::memcpy(a.inv, w->inv, sizeof(a.inv));
  a.d = w->d;
  a.d_inv32 = w->d_inv32;
  a.p_inv_d = w->p_inv_d;
  a.d_recip = w->d_recip;
  std::memcpy(a.w, w->w, sizeof(a.w));
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (w->a_limbs * 4 + inv) {
    case 1 * 4 + 0: rr::launch<1, 0>(w->k, g, s, a); break;
    case 1 * 4 + 1: rr::launch<1, 1>(w->k, g, s, a); break;
    case 1 * 4 + 2: rr::launch<1, 2>(w->k, g, s, a); break;
    case 2 * 4 + 0: rr::launch<2, 0>(w->k, g, s, a); break;
    case 2 * 4 + 1: rr::launch<2, 1>(w->k, g, s, a); break;
    case 2 * 4 + 2: rr::launch<2, 2>(w->k, g, s, a); break;
    case 17 * 4 + 0: rr::launch<17, 0>(w->k, g, s, a); break;
    case 17 * 4 + 1: rr::launch<17, 1>(w->k, g, s, a); break;
    default: rr::launch<17, 2>(w->k, g, s, a); break;
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  return DN_OK;
}
