// check_records.hip — the share consistency check straight from wire records
// (dn_m521_check_records): the k packed `_share_to_bytes`
// streams of shamir.py:28-33 in, the counts and culprit bytes of
// dn_m521_check_shares out, in one launch and without the k intermediate
// tiled vectors.  It is the check a receiver runs before it trusts
// dn_m521_reconstruct_records, on the wires that call reads.
//
// Per element e and wire i the kernel parses record e of wire i with the
// functions decode_kernel (codec_m521.hip) and recon_records.hip parse with
// (wire_parse.hpp: the window staged in LDS, the byte-serial path for a window
// beyond the LDS slice, the treatment of untrusted offsets), reduces y, and
// adds +-c[j][i] y to the R = k - t unreduced syndromes (check_core.hpp
// check_mac, which negates within 521 bits where the weight is negative: an
// unrepresentable record's y = 0 becomes p there, as on the decoded vector).
// After the last wire the syndromes are tested as check_kernel
// (share_check.hip) tests them.  There is no arithmetic of its own here.
//
// Work split: one wave = 64 consecutive elements (the parser's unit), one
// 256-thread workgroup = 256 elements, one workgroup per 256 elements, no grid
// stride.  Each wave owns one LDS slice (kDecRowWords words: 19456 B per
// workgroup) and reuses it wire after wire, so no workgroup barrier is needed.
// Staging is the serial form of recon_records.hip: a wire's whole window is
// loaded into registers (at most 5 16-byte or 19 4-byte loads per lane, all
// issued before the first LDS store), stored to LDS, and parsed; wire i + 1's
// loads and its two offsets are issued after wire i's arithmetic (loading ahead
// and decode_kernel's staging loop were slower there: DESIGN.md §4.15).  The
// 16-byte or 4-byte path is chosen per wire by its alignment (w16).
//
// Registers per lane: 18 R accumulator limbs, one 17-limb y, the staging
// registers.  Wire descriptors, weights, signs and powers are kernel arguments
// indexed by the wave-uniform wire counter: scalar loads.  k is a run-time
// count: eight instantiations (R x culprit or not), none per k.
#include <hip/hip_runtime.h>

#include "check_plan.hpp"
#include "dn_internal.hpp"
#include "share_rows.hpp"
#include "wire_parse.hpp"

namespace dn {
namespace cr {

constexpr int kBlock = 256;
static_assert(kBlock == kTile, "one workgroup per 256 elements");
static_assert(kChkLimbs == kLimbs, "a parsed y is a syndrome term");

struct Args {
  Wire wire[DN_MAX_RESOLVE];
  CheckWeights wt;
  uint32_t* counts;  // [0] inconsistent elements, [1] those with a located culprit
  uint8_t* culprit;
  uint32_t* bad;     // [0] unrepresentable records, [1] records whose x is not the wire's
  uint64_t n_elem;
  uint32_t w16;  // bit i: wire i is 16-B aligned (the wide staging path)
};
static_assert(sizeof(Args) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

// Wire i of one lane: its record parsed from the staged window (or from
// global memory where the window did not fit), y reduced, +-c[j][i] y added to
// the syndromes; the wave's two record counts.
template <int R>
__device__ __forceinline__ void wire_step(const Args& a, uint32_t i, const uint32_t* W, const Win& cw, uint64_t oe,
                                          uint64_t ee, bool valid, uint32_t (&S)[R][kChkAcc], uint32_t& nbad,
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
    } else {  // counted below; contributes y = 0, as the decoded vector would
#pragma unroll
      for (int l = 0; l < kLimbs; ++l) v[l] = 0u;
    }
    uint32_t c[R];
    const uint32_t sign = syndrome_weights<R>(a.wt, i, c);
    check_mac<R>(S, v, c, sign);
  }
  nbad += static_cast<uint32_t>(__popcll(__ballot(valid && !ok)));
  nmis += static_cast<uint32_t>(__popcll(__ballot(valid && ok && x != a.wire[i].x)));
}

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

template <int R, bool CULPRIT>
__global__ void __launch_bounds__(kBlock) check_records_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kBlock / 64][kDecRowWords];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t e0 = static_cast<uint64_t>(blockIdx.x) * kBlock + 64u * wv;
  if (e0 >= a.n_elem) return;  // wave-uniform
  const uint64_t e = e0 + lane;
  const bool valid = e < a.n_elem;  // a dead lane reads and writes nothing
  const uint64_t eN = e0 + 64 < a.n_elem ? e0 + 64 : a.n_elem;
  uint32_t* W = s_win[wv] + kWinPad / 4;  // W[j] = dword at window byte 4j
  const uint32_t k = a.wt.k;              // >= 2

  uint32_t S[R][kChkAcc];
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int l = 0; l < kChkAcc; ++l) S[j][l] = 0u;
  uint32_t nbad = 0u, nmis = 0u;  // wave-uniform counts

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

  uint8_t verdict = kChkConsistent;
  if (valid) {
    if constexpr (CULPRIT) {
      verdict = check_verdict<R>(S, static_cast<int>(k), [&a](int j, int s) { return a.wt.xp[j][s]; });
      a.culprit[e] = verdict;
    } else {
      verdict = check_consistent<R>(S) ? kChkConsistent : kChkUnexplained;
    }
  }
  verdict_count<CULPRIT>(a.counts, verdict);
  if (lane == 0) {
    if (nbad) atomicAdd(a.bad, nbad);
    if (nmis) atomicAdd(a.bad + 1, nmis);
  }
}

template <bool CULPRIT>
static void launch(int r, dim3 g, hipStream_t s, const Args& a) {
  switch (r) {
    case 1: hipLaunchKernelGGL((check_records_kernel<1, CULPRIT>), g, dim3(kBlock), 0, s, a); break;
    case 2: hipLaunchKernelGGL((check_records_kernel<2, CULPRIT>), g, dim3(kBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((check_records_kernel<3, CULPRIT>), g, dim3(kBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((check_records_kernel<4, CULPRIT>), g, dim3(kBlock), 0, s, a); break;
  }
}

}  // namespace cr
}  // namespace dn

using namespace dn;

extern "C" int dn_m521_check_records(const uint8_t* const* in, const uint64_t* in_bytes,
                                     const uint64_t* const* offsets, const uint64_t* xs,
                                     const dn_m521_check_plan_t* plan, uint32_t* counts, uint8_t* culprit,
                                     uint32_t* bad_counts, uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_check_records";
  if (n_elem == 0) return DN_OK;
  if (!in || !in_bytes || !offsets || !xs || !plan || !counts || !bad_counts)
    return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (!check_plan_wellformed(*plan)) return set_error(DN_ERR_ARG, "%s: malformed plan", name);
  const uint64_t blocks = (n_elem + cr::kBlock - 1) / cr::kBlock;
  if (blocks >= (1ull << 31)) return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name,
                                               (unsigned long long)n_elem);
  cr::Args a{};
  if (const int rc = fill_wires(name, in, in_bytes, offsets, xs, plan->k, a.wire, &a.w16)) return rc;
  weights_fill(a.wt, *plan);
  a.counts = counts;
  a.culprit = culprit;
  a.bad = bad_counts;
  a.n_elem = n_elem;
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (culprit) cr::launch<true>(plan->r, g, s, a);
  else cr::launch<false>(plan->r, g, s, a);
  return launch_status(name);
}
