// robust_records.hip — the robust reconstruct straight from wire records
// (dn_m521_reconstruct_records_robust): the k >= t + 2 packed
// `_share_to_bytes` streams of shamir.py:28-33 in, f(0) per element out past one
// bad wire per element, with the counts and culprit bytes of
// dn_m521_reconstruct_robust and the record counts of
// dn_m521_reconstruct_records, in one launch and without the k intermediate
// tiled vectors.  A record the decoder cannot represent contributes y = 0 and is
// counted; its wire is then located like any other damaged share and the secret
// comes from the other wires.
//
// Three existing parts are joined; there is no arithmetic of its own here.
//   wire side     check_records.hip's: one wave = 64 consecutive elements, one
//                 256-thread workgroup = one tile, one workgroup per 256
//                 elements, no grid stride.  Each wave owns one LDS slice
//                 (kDecRowWords words) and reuses it wire after wire, so no
//                 workgroup barrier is needed.  A wire's whole window is loaded
//                 into registers, stored to LDS and parsed (wire_parse.hpp);
//                 wire i + 1's loads and its two offsets are issued after wire
//                 i's arithmetic; the 16- or 4-byte staging path is chosen per
//                 wire (w16); a window beyond the LDS slice is parsed from global
//                 memory; untrusted offsets are treated exactly as there.
//   accumulation  check_mac<R + 1> (check_core.hpp): the R syndromes and, chain
//                 R, T' weighted by |A_i|, unreduced, 18 limbs each — what
//                 robust_kernel (share_robust.hip) feeds rows_accumulate<R + 1>.
//   finish        robust_kernel's (robust_core.hpp): check_verdict on the first
//                 R chains, robust_plain for an element without a located wire,
//                 the wave-uniform candidate loop with robust_located under the
//                 lane's bit of the ballot.
//
// Stores: a wave's 64 elements are quarter `wave` of tile blockIdx.x, so the
// field form writes the tiled vector through the tile's buffer descriptor with
// no transpose; the int64 form is one non-temporal 8-byte store per live lane.
//
// Registers: the wire loop keeps R + 1 accumulators of 18 limbs, the staged
// window (20 registers), y and the parse temporaries live together.  The
// accumulators are the only state carried from wire to wire; the finish starts
// after the last wire's staging registers are dead.
//
// The two-error form (TWO) adds robust_pair.hpp's
// wave-cooperative pair search after the verdict, in the wave's LDS slice,
// which is free once the last wire is parsed.
//
// Everything a launch needs travels in its arguments (about 2.8 KB): no device
// table, no staging buffer, nothing to synchronise.  Lanes at or past n_elem
// read and write nothing, the padding lanes of a field output's last tile
// included.
#include <hip/hip_runtime.h>

#include "dn_internal.hpp"
#include "robust_core.hpp"
#include "robust_pair.hpp"
#include "robust_plan.hpp"
#include "share_rows.hpp"
#include "wire_parse.hpp"

namespace dn {
namespace rr {

constexpr int kBlock = 256;
static_assert(kBlock == kTile, "one workgroup per tile: wave q writes quarter q");
static_assert(kChkLimbs == kLimbs, "a parsed y is a syndrome term");

struct Args {
  Wire wire[DN_MAX_RESOLVE];
  CheckWeights wt;
  uint32_t a[DN_MAX_RESOLVE];                   // |A_i|
  dn_m521_div_small_t div[DN_MAX_RESOLVE + 1];  // [i]: |w_i| D_all; [kRobustAll]: D_all
  uint8_t* out_fe;
  int64_t* out_u64;
  uint32_t* counts;  // [0] inconsistent elements, [1] the corrected ones
  uint8_t* culprit;
  uint32_t* bad;     // [0] unrepresentable records, [1] records whose x is not the wire's
  uint64_t n_elem;
  uint32_t negate;
  uint32_t w16;  // bit i: wire i is 16-B aligned (the wide staging path)
};
static_assert(sizeof(Args) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

enum Out { kField, kInt64 };

// (wire_fetch and the parse of wire_step repeat check_records.hip's: DESIGN.md §4.30 notes the
// "written once" clean-up)

// Wire i's window geometry, its staging loads and the lane's two offsets.
__device__ __forceinline__ void wire_fetch(const Args& a, uint32_t i, uint64_t e0, uint64_t eN, uint64_t e, bool valid,
                                           uint32_t lane, Win& w, Stage& st, uint64_t& oe, uint64_t& ee) {
  const bool w16 = (a.w16 >> i) & 1u;
  w = win_of((OffTab)a.wire[i].offsets, a.wire[i].in_bytes, w16, e0, eN);
  if (w.lds) stage_load(st, a.wire[i].in, w, w16, lane);
  if (valid) {
    oe = a.wire[i].offsets[e];
    ee = a.wire[i].offsets[e + 1];
  }
}

// Wire i of one lane: its record parsed from the staged window (or from global
// memory where the window did not fit), y reduced, +-c[j][i] y added to the R
// syndromes and +-|A_i| y to chain R; the wave's two record counts.
template <int R>
__device__ __forceinline__ void wire_step(const Args& a, uint32_t i, const uint32_t* W, const Win& cw, uint64_t oe,
                                          uint64_t ee, bool valid, uint32_t (&S)[R + 1][kChkAcc], uint32_t& nbad,
                                          uint32_t& nmis) {
  bool ok = false;
  uint64_t x = 0;
  if (valid) {
    uint32_t v[kLimbs];
    if (cw.lds) {
      ok = parse_lds(W, cw, oe, ee, x, v);
    } else {
      ok = oe < ee && ee <= a.wire[i].in_bytes && parse_global(a.wire[i].in, oe, ee, x, v);
    }
    if (ok) {
      reduce(v);
    } else {  // counted below; contributes y = 0 (p under a negative weight), as the decoded vector would
#pragma unroll
      for (int l = 0; l < kLimbs; ++l) v[l] = 0u;
    }
    uint32_t c[R + 1];
    c[R] = a.a[i];
    const uint32_t sign = syndrome_weights<R>(a.wt, i, c);
    check_mac<R + 1>(S, v, c, sign);
  }
  nbad += static_cast<uint32_t>(__popcll(__ballot(valid && !ok)));
  nmis += static_cast<uint32_t>(__popcll(__ballot(valid && ok && x != a.wire[i].x)));
}

// R = 2 (3-of-5 with all five wires) is held to the registers of three waves per SIMD: 177 -> 168
// VGPRs, still without scratch; R = 3 and 4 need 196 and 214 and stay at two.
template <int R, int OUT, bool TWO = false>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(R == 2 ? 3 : 2)))
robust_records_kernel(const Args a) {
  static_assert(!TWO || R == 4, "two errors are located from four syndromes");
  static_assert(kPairWords <= kDecRowWords, "the pair search reuses the wave's window slice");
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kBlock / 64][kDecRowWords];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * kBlock + 64u * wv;
  if (e0 >= a.n_elem) return;  // wave-uniform
  const uint64_t e = e0 + lane;
  const bool valid = e < a.n_elem;  // a dead lane reads and writes nothing
  const uint64_t eN = e0 + 64 < a.n_elem ? e0 + 64 : a.n_elem;
  uint32_t* W = s_win[wv] + kWinPad / 4;  // W[j] = dword at window byte 4j
  const uint32_t k = a.wt.k;              // >= 3

  // the R syndromes and, chain R, T' weighted by |A_i|
  uint32_t S[R + 1][kChkAcc];
#pragma unroll
  for (int j = 0; j < R + 1; ++j)
#pragma unroll
    for (int l = 0; l < kChkAcc; ++l) S[j][l] = 0u;
  uint32_t nbad = 0u, nmis = 0u;  // wave-uniform counts

  {
    Stage st;
    Win nw;
    uint64_t noe = 0, nee = 0;
    wire_fetch(a, 0u, e0, eN, e, valid, lane, nw, st, noe, nee);
#pragma unroll 1
    for (uint32_t i = 0; i < k; ++i) {
      const Win cw = nw;
      const uint64_t oe = noe, ee = nee;
      if (cw.lds) stage_store(st, W, cw, (a.w16 >> i) & 1u, lane);
      lds_order();
      wire_step<R>(a, i, W, cw, oe, ee, valid, S, nbad, nmis);
      lds_order();  // the slice is free for the next window
      if (i + 1 < k) wire_fetch(a, i + 1u, e0, eN, e, valid, lane, nw, st, noe, nee);
    }
  }
  if (lane == 0) {
    if (nbad) atomicAdd(a.bad, nbad);
    if (nmis) atomicAdd(a.bad + 1, nmis);
  }

  // the finish: robust_kernel's (a dead lane votes "consistent" and stores nothing)
  uint8_t verdict = kChkConsistent;
  uint32_t f[kChkLimbs];
  if (valid) {
    verdict =
        check_verdict<R>(robust_syndromes<R>(S), static_cast<int>(k), [&a](int j, int s) { return a.wt.xp[j][s]; });
    if (verdict >= kChkUnexplained) robust_plain(S[R], a.div[kRobustAll], a.negate, f);
  }
  if constexpr (TWO) robust_pair_wave(a, s_win[wv], S, verdict, f);
  // the correction, wave-uniform: candidate i's constants in SGPRs, a candidate without lanes skipped
  if (__ballot(verdict < kChkUnexplained) != 0ull) {
#pragma unroll 1
    for (uint32_t i = 0; i < k; ++i) {
      const uint64_t mine = __ballot(verdict == i);
      if (mine == 0ull) continue;
      // (a lane's bit of the ballot, not `verdict == i`: under that branch the compiler replaces i by
      // the lane's verdict, and the constants come by vector loads)
      if ((mine >> lane) & 1ull) robust_located(S[0], S[R], a.wt.c[0][i], a.a[i], a.div[i], a.negate, f);
    }
  }
  if (valid) {
    if constexpr (OUT == kField) {
      store_fe_b(tile_rsrc(tile_base(a.out_fe, blockIdx.x)), 64u * wv + lane, f);
    } else {
      __builtin_nontemporal_store(static_cast<int64_t>(f[0] | (static_cast<uint64_t>(f[1]) << 32)), a.out_u64 + e);
    }
    if (a.culprit) a.culprit[e] = verdict;
  }
  verdict_count<true>(a.counts, verdict);
}

template <int OUT>
static void launch(int r, dim3 g, hipStream_t s, const Args& a) {
  switch (r) {
    case 2: hipLaunchKernelGGL((robust_records_kernel<2, OUT>), g, dim3(kBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((robust_records_kernel<3, OUT>), g, dim3(kBlock), 0, s, a); break;
    case 4: hipLaunchKernelGGL((robust_records_kernel<4, OUT>), g, dim3(kBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((robust_records_kernel<4, OUT, true>), g, dim3(kBlock), 0, s, a); break;  // two errors
  }
}

}  // namespace rr
}  // namespace dn

using namespace dn;

extern "C" int dn_m521_reconstruct_records_robust(const uint8_t* const* in, const uint64_t* in_bytes,
                                                  const uint64_t* const* offsets, const uint64_t* xs,
                                                  const dn_m521_robust_plan_t* plan, void* out_fe, int64_t* out_u64,
                                                  uint32_t* counts, uint8_t* culprit, uint32_t* bad_counts,
                                                  uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_reconstruct_records_robust";
  if (n_elem == 0) return DN_OK;
  if (!in || !in_bytes || !offsets || !xs || !plan || !counts || !bad_counts)
    return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if ((out_fe != nullptr) == (out_u64 != nullptr))
    return set_error(DN_ERR_ARG, "%s: exactly one of out_fe and out_u64", name);
  if (!robust_plan_wellformed(*plan)) return set_error(DN_ERR_ARG, "%s: malformed plan", name);
  const uint64_t blocks = (n_elem + rr::kBlock - 1) / rr::kBlock;
  if (blocks >= (1ull << 31)) return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name,
                                               (unsigned long long)n_elem);
  const dn_m521_check_plan_t& chk = plan->check;
  rr::Args a{};
  if (const int rc = fill_wires(name, in, in_bytes, offsets, xs, chk.k, a.wire, &a.w16)) return rc;
  weights_fill(a.wt, chk);
  for (int i = 0; i < chk.k; ++i) {
    a.a[i] = plan->a[i];
    a.div[i] = plan->div[i];
  }
  a.div[kRobustAll] = plan->div[kRobustAll];
  a.out_fe = static_cast<uint8_t*>(out_fe);
  a.out_u64 = out_u64;
  a.counts = counts;
  a.culprit = culprit;
  a.bad = bad_counts;
  a.n_elem = n_elem;
  a.negate = plan->negate;
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int form = plan->max_errors == 2u ? 5 : chk.r;  // (wellformed: two errors only with r == 4)
  if (out_fe) rr::launch<rr::kField>(form, g, s, a);
  else rr::launch<rr::kInt64>(form, g, s, a);
  return launch_status(name);
}
