// share_sum.hip — the share-domain sum (dn_m521_sum_vecs):
//   out_e = (sum_i +-y_{i,e}) mod p, canonical, for every lane of every tile
// of m tiled M521 vectors or blocks of one byte length.  Shamir is additively
// homomorphic: party x adds share x of every member's tensor, and any t
// parties' sums reconstruct the sum of the tensors.
//
// The sum is tile-local — no n_elem, no rows — so the unit of work is a part
// of one 16896-byte tile (64 lanes x DN_SUM_PER consecutive elements) and a
// launch covers a vector, a block of vectors or the flat buffer behind a list
// alike.  Every element lives in one lane, 17 u32 limbs in VGPRs.  Inputs are
// 521-bit values (the top plane masked to 9 bits, p itself legal); the lazy
// 17-limb form holds any value below 2^544, so a launch's up to
// DN_M521_SUM_GROUP additions need no fold in between: add, add, ..., one
// reduce().  A negated term is p - y = ~y within 521 bits.
//
// HBM-bound ((m + 1) * 66 B per element, 17 add-with-carry per input), so the
// work is in the loads: a ring of DN_SUM_DEPTH units of input (8.4 KB per
// wave each at two elements per lane) is filled before the first add and
// every slot is refilled with the input DEPTH further on as soon as it has
// been added.  The loads are raw — the top plane is masked where the slot is
// consumed, not where it is loaded, so nothing waits on a load before its
// slot's turn.  A lane's elements are independent carry chains, interleaved
// limb by limb (a lone v_addc chain pays wait states on the carry:
// m521_device.hpp fd_step).
//
// The input addresses and sign bits are kernel arguments, indexed by the
// wave-uniform input counter: scalar loads from the argument segment, every
// base in SGPRs — no device table, no staging buffer, no scratch, nothing
// that synchronises (the call can be captured into a graph).
#include <hip/hip_runtime.h>

#include <vector>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "sum_plan.hpp"

namespace dn {

struct ShareSumArgs {
  const uint8_t* in[DN_M521_SUM_GROUP];
  uint32_t neg[DN_M521_SUM_GROUP / 32];  // bit i of word i / 32: subtract input i
  uint8_t* out;
  uint64_t ntiles;
  uint32_t m;       // inputs of this launch, 1 .. DN_M521_SUM_GROUP
};
static_assert(sizeof(ShareSumArgs) <= 4096, "the kernel argument segment holds 4 KiB");
static_assert(DN_M521_SUM_GROUP % 32 == 0 && DN_M521_SUM_GROUP < (1 << 23), "sign words; lazy-form bound");

// DN_SUM_PER: consecutive elements per lane (1, 2 or 4) — a wave's load of a
// limb plane is then one 256-, 512- or 1024-byte instruction and a unit of
// work 64 * PER elements, a quarter, half or whole tile.  DN_SUM_DEPTH: units
// of input loaded ahead per wave (a slot is 16 * PER + 1 VGPRs next to the
// 17 * PER accumulator limbs).  Measured at m = 3 / 10 x 2^24 and 40 x 2^22
// (DESIGN.md §4.12): PER 1, DEPTH 4 0.81 / 2.29 / 2.07 ms; PER 2, DEPTH 2
// (default: 152 VGPRs, 3 waves per SIMD) 0.72 / 2.19 / 1.89; PER 2, DEPTH 3
// 0.73 / 2.21 / 1.89; PER 4, DEPTH 1 0.78 / 2.22 / 1.91; PER 4, DEPTH 2
// 0.76 / 2.13 / 1.86 but 256 VGPRs and 26 AGPR copies, one wave per SIMD.
#ifndef DN_SUM_PER
#define DN_SUM_PER 2
#endif
#ifndef DN_SUM_DEPTH
#define DN_SUM_DEPTH 2
#endif

constexpr int kSumBlock = 256;
constexpr int kSumWaves = kSumBlock / 64;
constexpr int kSumPer = DN_SUM_PER;
constexpr uint32_t kSumUnitsPerTile = 4 / kSumPer;
static_assert(kSumPer == 1 || kSumPer == 2 || kSumPer == 4, "1, 2 or 4 elements per lane");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// One input's unit as a wave holds it: limb l of the lane's element j in
// lo[l][j], the elements' 16-bit top words packed in hi as they lie in memory.
// Raw: the top words are masked where the slot is consumed (sum_add), not
// where it is loaded, so nothing waits on a load before its slot's turn.
struct SumSlot {
  uint32_t lo[16][kSumPer];
  uint32_t hi[(kSumPer + 1) / 2];
};

// Lane's first element within the tile for unit `sub` (< kSumUnitsPerTile) of it.
__device__ __forceinline__ uint32_t sum_first(uint32_t sub, uint32_t lane) {
  return (sub * 64u + lane) * kSumPer;
}

__device__ __forceinline__ void sum_load(const ShareSumArgs& a, uint32_t i, uint32_t tile, uint32_t e0, SumSlot& y) {
  const rsrc_t r = tile_rsrc(tile_base(a.in[i], tile));
  const uint32_t o4 = e0 * 4u, o2 = e0 * 2u;
#pragma unroll
  for (int l = 0; l < 16; ++l) {
    if constexpr (kSumPer == 4) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, o4, l * 4 * kTile, kNt);
      y.lo[l][0] = v[0], y.lo[l][1] = v[1], y.lo[l][2] = v[2], y.lo[l][3] = v[3];
    } else if constexpr (kSumPer == 2) {
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, o4, l * 4 * kTile, kNt);
      y.lo[l][0] = v[0], y.lo[l][1] = v[1];
    } else {
      y.lo[l][0] = __builtin_amdgcn_raw_buffer_load_b32(r, o4, l * 4 * kTile, kNt);
    }
  }
  if constexpr (kSumPer == 4) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, o2, static_cast<int>(kHiOffset), kNt);
    y.hi[0] = v[0], y.hi[1] = v[1];
  } else if constexpr (kSumPer == 2) {
    y.hi[0] = __builtin_amdgcn_raw_buffer_load_b32(r, o2, static_cast<int>(kHiOffset), kNt);
  } else {
    y.hi[0] = static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b16(r, o2, static_cast<int>(kHiOffset), kNt));
  }
}

// All-ones when input i is subtracted, else 0 (wave-uniform).
__device__ __forceinline__ uint32_t sum_sign(const ShareSumArgs& a, uint32_t i) {
  return 0u - ((a.neg[i >> 5] >> (i & 31u)) & 1u);
}

// acc[j] += the slot's element j as its 521-bit term — y, or ~y within 521
// bits (sign all-ones) — for the lane's elements: independent carry chains,
// interleaved limb by limb (a lone v_addc chain pays wait states on the
// carry: m521_device.hpp fd_step).
__device__ __forceinline__ void sum_add(uint32_t acc[kSumPer][kLimbs], const SumSlot& y, uint32_t sign) {
  unsigned c[kSumPer];
#pragma unroll
  for (int j = 0; j < kSumPer; ++j) c[j] = 0u;
#pragma unroll
  for (int l = 0; l < 16; ++l) {
#pragma unroll
    for (int j = 0; j < kSumPer; ++j) acc[j][l] = __builtin_addc(acc[j][l], y.lo[l][j] ^ sign, c[j], &c[j]);
  }
#pragma unroll
  for (int j = 0; j < kSumPer; ++j) {
    const uint32_t top = ((y.hi[j >> 1] >> (16 * (j & 1))) ^ sign) & kTopMask;
    acc[j][16] = __builtin_addc(acc[j][16], top, c[j], &c[j]);
  }
}

__device__ __forceinline__ void sum_store(uint8_t* tb, uint32_t e0, const uint32_t acc[kSumPer][kLimbs]) {
  const rsrc_t r = tile_rsrc(tb);
  const uint32_t o4 = e0 * 4u, o2 = e0 * 2u;
#pragma unroll
  for (int l = 0; l < 16; ++l) {
    if constexpr (kSumPer == 4)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{acc[0][l], acc[1][l], acc[2][l], acc[3][l]}, r, o4, l * 4 * kTile,
                                             kNt);
    else if constexpr (kSumPer == 2)
      __builtin_amdgcn_raw_buffer_store_b64(u32x2{acc[0][l], acc[1][l]}, r, o4, l * 4 * kTile, kNt);
    else
      __builtin_amdgcn_raw_buffer_store_b32(acc[0][l], r, o4, l * 4 * kTile, kNt);
  }
  if constexpr (kSumPer == 4)
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{acc[0][16] | (acc[1][16] << 16), acc[2][16] | (acc[3][16] << 16)}, r,
                                          o2, static_cast<int>(kHiOffset), kNt);
  else if constexpr (kSumPer == 2)
    __builtin_amdgcn_raw_buffer_store_b32(acc[0][16] | (acc[1][16] << 16), r, o2, static_cast<int>(kHiOffset), kNt);
  else
    __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(acc[0][16]), r, o2, static_cast<int>(kHiOffset), kNt);
}

__global__ void __launch_bounds__(kSumBlock) share_sum_kernel(const ShareSumArgs a) {
  constexpr int D = DN_SUM_DEPTH;
  static_assert(D >= 1, "at least one slot");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kSumWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kSumWaves;
  const uint32_t m = a.m;
  const uint64_t nunits = a.ntiles * kSumUnitsPerTile;
  for (uint64_t u = wave; u < nunits; u += nwaves) {
    const uint32_t tile = static_cast<uint32_t>(u / kSumUnitsPerTile);
    const uint32_t e0 = sum_first(static_cast<uint32_t>(u % kSumUnitsPerTile), lane);
    SumSlot y[D];
    uint32_t acc[kSumPer][kLimbs];
#pragma unroll
    for (int j = 0; j < kSumPer; ++j)
#pragma unroll
      for (int l = 0; l < kLimbs; ++l) acc[j][l] = 0u;
    uint32_t i = 0;
    if (m >= static_cast<uint32_t>(D)) {
      // The ring filled without a branch (a fill under `s < m` leaves the first wait behind it counting only
      // the loads every path has issued: it then waits for the whole ring) ...
#pragma unroll
      for (int s = 0; s < D; ++s) sum_load(a, s, tile, e0, y[s]);
      // ... rounds in which every slot holds an input and has one to be refilled with ...
      for (; i + 2 * D <= m; i += D) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
          sum_add(acc, y[s], sum_sign(a, i + s));
          sum_load(a, i + s + D, tile, e0, y[s]);
          // the scheduler otherwise gathers all D slots' adds in front of all D loads (one wait for the whole
          // ring per round, nothing in flight behind it): each slot waits for its own loads only
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ... and the round that refills the first m - i - D < D slots only.
#pragma unroll
      for (int s = 0; s < D; ++s) {
        sum_add(acc, y[s], sum_sign(a, i + s));
        if (i + s + D < m) sum_load(a, i + s + D, tile, e0, y[s]);
      }
      i += D;
    } else {
#pragma unroll
      for (int s = 0; s < D; ++s)
        if (static_cast<uint32_t>(s) < m) sum_load(a, s, tile, e0, y[s]);
    }
    // the last m - i < D inputs: the ring runs dry
#pragma unroll
    for (int s = 0; s < D - 1; ++s) {
      if (i + s < m) sum_add(acc, y[s], sum_sign(a, i + s));
    }
    // every accumulator < 2^521 * m < 2^544: one reduce each
#pragma unroll
    for (int j = 0; j < kSumPer; ++j) reduce(acc[j]);
    sum_store(tile_base(a.out, tile), e0, acc);
  }
}

// Workgroups per launch: one wave per unit, each 4-wave workgroup striding
// over the units, at most 16384 (as shamir_m521.hip grid_for; DN_GRID_CAP
// overrides it in the tuning build).
static uint32_t sum_grid(uint64_t ntiles) {
  const char* s = tune_env("DN_GRID_CAP");
  const int v = s ? std::atoi(s) : 0;
  const uint64_t cap = v > 0 ? static_cast<uint64_t>(v) : 16384u;
  const uint64_t blocks = (ntiles * kSumUnitsPerTile + kSumWaves - 1) / kSumWaves;
  return static_cast<uint32_t>(blocks < cap ? blocks : cap);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_m521_sum_vecs(const void* const* vecs, const uint8_t* negate, uint64_t m, void* out,
                                uint64_t n_tiles, void* stream) {
  const char* name = "dn_m521_sum_vecs";
  if (n_tiles == 0) return DN_OK;
  if (m == 0) return set_error(DN_ERR_ARG, "%s: no input", name);
  if (!vecs || !out) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (n_tiles >= (1ull << 32)) return set_error(DN_ERR_ARG, "%s: more than 2^32 tiles", name);
  std::vector<uint64_t> addr(m), order(m);
  for (uint64_t i = 0; i < m; ++i) {
    if (!vecs[i]) return set_error(DN_ERR_ARG, "%s: null input %llu", name, static_cast<unsigned long long>(i));
    addr[i] = reinterpret_cast<uint64_t>(vecs[i]);
  }
  const uint64_t o = reinterpret_cast<uint64_t>(out);
  switch (sum_plan_order(addr.data(), m, o, n_tiles * kTileBytes, order.data())) {
    case kSumPlanOverlap:
      return set_error(DN_ERR_ARG, "%s: an input overlaps out without being equal to it", name);
    case kSumPlanAliases:
      return set_error(DN_ERR_ARG, "%s: more than %d inputs equal to out", name, DN_M521_SUM_GROUP);
    default: break;
  }
  ShareSumArgs a{};
  a.out = static_cast<uint8_t*>(out);
  a.ntiles = n_tiles;
  const dim3 g(sum_grid(n_tiles));
  const uint64_t launches = sum_plan_launches(m);
  for (uint64_t j = 0; j < launches; ++j) {
    uint64_t ptrs[DN_M521_SUM_GROUP];
    a.m = sum_plan_fill(addr.data(), negate, order.data(), m, o, j, ptrs, a.neg);
    for (uint32_t i = 0; i < a.m; ++i) a.in[i] = reinterpret_cast<const uint8_t*>(ptrs[i]);
    hipLaunchKernelGGL(share_sum_kernel, g, dim3(kSumBlock), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: launch failed: %s", name, hipGetErrorString(err));
  }
  return DN_OK;
}
