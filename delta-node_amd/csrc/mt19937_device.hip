// mt19937_device.hip — CPython's MT19937 coefficient draw on the GPU, bit-exact.
//
// Reference: SecretShare.make_shares draws its t-1 coefficients per element
// with self.random.randint(1, p-1) (delta_node/crypto/shamir/shamir.py:59-61):
// 1 + getrandbits(521), redrawn while >= p-1; getrandbits(521) is 17 MT19937
// words, little-endian, the last >> 23.  dn_mt19937_draw_coeffs (host_m521.cpp)
// restates that stream sequentially; this file produces the same values on the
// device by cutting the word stream into S substreams of L = 17 * 2^k words
// (2^k whole draws each; k = 14 from 2^24 coefficients, 12 from 2^21, else
// 10), all on the GPU:
//
//  * jump kernel: the MT window at the start of every substream by
//    jump-ahead, g(f)(W) with g = x^J mod P (P the characteristic polynomial
//    of the one-word transition f; tools/gen_mt_jump.py), evaluated by Horner
//    over 64-bit chunks of g: r <- f^64(r) ^ sum of table rows, the table E the
//    64 combinations of six consecutive shifts of W, in LDS.  A wave holds r
//    (624 words + 80 free slots) in 11 VGPRs; f^64 appends 64 words (three
//    ds_bpermute + the twist per lane).  Windows are at most three jumps
//    (radix-64 digits of s - 1, mt19937_jump.inc) from the caller's window:
//    one launch per level, every jump of a level independent;
//  * generation kernel: one wave per substream keeps its window in the same
//    register ring, appends 64 words at a time, tempers them into an LDS ring
//    and turns every 17-word group into one coefficient (+1, rejection test):
//    stored in the tiled layout (T = 0) or consumed at once by the split of
//    the element it belongs to (T = t, the fused draw + split); one extra
//    wave steps the last window before CPython's final array to it, so
//    self.random continues exactly as after n sequential make_shares calls.
//    The fused form also takes a LIST of tensors (dn_mt19937_split_many_device):
//    the draw of their concatenation, each tensor's shares stored into its own
//    block (the SEG kernels, emit_split_seg; seg_plan.hpp).
// A rejected draw (probability ~2^-520 per coefficient) shifts every later
// word; the device flags it and the caller redoes the draw on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "mt_plan.hpp"
#include "seg_plan.hpp"

namespace dn {
namespace {

// The jump tables on the device, indexed by the job poly indices of
// mt_plan.hpp: the A / C / B rows of the three table lengths, then (from
// kMtDirectBase) the direct rows of the four lengths.
__device__ const uint64_t kMtPolysDev[kMtTabLens][kMtJumpRows][kMtPolyWords] = {
    DN_MT_JUMP_POLYS_L10, DN_MT_JUMP_POLYS_L12, DN_MT_JUMP_POLYS};
__device__ const uint64_t kMtDirectDev[kMtLens][kMtDirectRows][kMtPolyWords] = {
    DN_MT_JUMP_DIRECT_L10, DN_MT_JUMP_DIRECT_L12, DN_MT_JUMP_DIRECT_L14, DN_MT_JUMP_DIRECT_L8};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kMtM = 397;
constexpr uint32_t kMtA = 0x9908b0dfu, kMtUp = 0x80000000u, kMtLo = 0x7fffffffu;

__host__ __device__ inline uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

__host__ __device__ inline uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t m) {
  const uint32_t y = (a & kMtUp) | (b & kMtLo);
  return m ^ (y >> 1) ^ ((0u - (y & 1u)) & kMtA);
}

// A workgroup's waves work independently; LDS traffic between the lanes of
// one wave needs ordering, not a hardware barrier (a wavefront-scope fence
// keeps the compiler from moving LDS accesses across it; the LDS executes a
// wave's accesses in order).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The producer / consumer handoff: the ring half one wave wrote (ds_write)
// or read (ds_read) in this step is complete before the other wave touches it
// in the next, so a step ends with the LDS counter drained and s_barrier —
// not __syncthreads(), whose workgroup-scope release also drains the global
// stores: the consumer's 85 share stores per group would have to land before
// every barrier (emission alone 1.18 vs 1.04 ms at 2^24, profiles/r04/s/).
__device__ __forceinline__ void pc_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ------------------------------------------------------------------ jumps
struct JumpArgs {
  uint32_t* wins;  // window s at row s (row 0 the caller's array), the caller's window advanced idx words at row -1
  const JumpJob* jobs;
  uint32_t njobs;
  uint32_t probe;  // tuning build only (DN_MT_JUMP_PROBE): 1 = no Horner steps, 2 = no stream stepping (timing only)
  const uint64_t* rt;  // runtime direct rows on the device (poly >= kMtRtBase), or null
};

// Jump and generation waves keep a 624-word MT window in registers: Q[11] a
// 704-slot ring (slot 64 r + lane), the window's word i at slot 16 + i of the
// current frame.  One append = the next 64 words of the stream
// (mix(word l, word l + 1, word l + 397), operands by ds_bpermute), written
// to the frame's free register; the frame then moves by one register.
// APPEND<K> is append number K mod 11 of an unrolled run: logical register r
// is Q[(r + K) % 11], so no register moves.
struct Lanes {
  int pa, pb, pm;  // ds_bpermute byte addresses of lanes l + 16, l + 17, l + 29 (mod 64)
  bool la, lb, lm;  // lane < 16, < 17, < 29
};

template <int K>
__device__ __forceinline__ uint32_t append64(uint32_t (&Q)[11], const Lanes& L) {
  const uint32_t xa = static_cast<uint32_t>(
      __builtin_amdgcn_ds_bpermute(L.pa, static_cast<int>(L.la ? Q[(1 + K) % 11] : Q[K % 11])));
  const uint32_t xb = static_cast<uint32_t>(
      __builtin_amdgcn_ds_bpermute(L.pb, static_cast<int>(L.lb ? Q[(1 + K) % 11] : Q[K % 11])));
  const uint32_t xm = static_cast<uint32_t>(
      __builtin_amdgcn_ds_bpermute(L.pm, static_cast<int>(L.lm ? Q[(7 + K) % 11] : Q[(6 + K) % 11])));
  Q[(10 + K) % 11] = mt_mix(xa, xb, xm);
  return Q[(10 + K) % 11];
}

// Jump table of one source window W, E[v] = words 0..683 of the stream of
// T[v] = sum over bits j of v of f^j(W), laid out for ds_read_b64.  The ten
// words a lane XORs into its window registers for one chunk are E[v][64 k +
// m - 16] for k = 0..9 (main half) or k = 1..10 (wrap half, lanes whose row
// index wraps); they are stored as five 8-B pairs, pair i of (v, m) at
//   half * kEWrap + i * kEPair + (64 v + m) * 2
// so one chunk is five ds_read_b64 at immediate offsets from one address.
// Banking (64 x 4-B banks, a b64 lane group = 32 lanes = 64 banks): a lane
// group reads 32 consecutive rows m (mod 64) of one pair plane -> 32
// distinct bank pairs, and kEWrap is a multiple of 64 words, so wrapped lanes
// keep their pairs: conflict-free (SQ_LDS_BANK_CONFLICT ~0), 160 LDS cycles
// per 16 chunks.  kEPair is 8 B off a multiple of 512 B so the compiler cannot
// fuse the five reads into ds_read2(st64)_b64 (half-rate, banks mod 32).
// A/B at 2^24 (profiles/r02/mt_jump_layout.md): the earlier 28-word rows
// (two b128 + one b64, wrap copy at +12 words) took 252 cycles by the bank
// model, SQ_LDS_BANK_CONFLICT +54 % of the array cycles, and the level of
// 2016 jumps 0.37-0.41 ms; this layout 0.29-0.31 ms; 12-word rows read as
// three b128 (conflict-free by the model, 192 cycles) 0.34-0.37 ms.
constexpr int kEVWords = 64 * 2;                      // words per chunk value v in one pair plane
constexpr int kEPair = 16 * kEVWords + 2;              // 2050 words
constexpr int kEWrap = ((5 * kEPair + 63) / 64) * 64;  // 10304 words
constexpr int kEWords = kEWrap + 5 * kEPair;           // 82 KB

// a ^ b ^ c in one VALU instruction (gfx950 v_bitop3_b32, truth table 0x96;
// hipcc keeps two v_xor_b32 otherwise).  Inline asm on purpose in the jump
// kernel's Horner step: with the compiler builtin the scheduler hoists the
// table reads further and the kernel spills ~1,300 scratch accesses (the
// generation kernels' bitop3 below are builtins: no spill there, fewer s_nop).
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// the ten table words of chunk t (value c) for this lane: off = the lane's row offset for t
__device__ __forceinline__ void table_words(const uint32_t* E, uint32_t off, uint32_t c, uint32_t (&x)[10]) {
  const uint32_t* p = E + c * kEVWords + off;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const u32x2_t d = *reinterpret_cast<const u32x2_t*>(p + i * kEPair);
    x[2 * i] = d.x, x[2 * i + 1] = d.y;
  }
}

// One Horner step over the 64-bit word gw of g in frame K (logical register
// r is Q[(r + K) % 11]): f^64 into the frame's free register, then the 16
// table windows XORed (two per instruction) into the 624 window words, which
// now sit at slots 80 .. 703 of the frame (registers 1 .. 10).
template <int K>
__device__ __forceinline__ void jump_mega(uint32_t (&Q)[11], const Lanes& L, const uint32_t* E,
                                          const uint32_t (&off)[16], uint64_t gw) {
  // the table reads of chunk pair p + 1 are issued before the XORs of pair p
  // (f^64's ds_bpermute first: LDS results return in issue order)
  uint32_t x[2][2][10];
  append64<K>(Q, L);
  table_words(E, off[0], static_cast<uint32_t>(gw >> 60) & 15u, x[0][0]);
  table_words(E, off[1], static_cast<uint32_t>(gw >> 56) & 15u, x[0][1]);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    if (p < 7) {
      table_words(E, off[2 * p + 2], static_cast<uint32_t>(gw >> (52 - 8 * p)) & 15u, x[(p + 1) & 1][0]);
      table_words(E, off[2 * p + 3], static_cast<uint32_t>(gw >> (48 - 8 * p)) & 15u, x[(p + 1) & 1][1]);
    }
#pragma unroll
    for (int r = 1; r < 11; ++r)
      Q[(r + K) % 11] = xor3(Q[(r + K) % 11], x[p & 1][0][r - 1], x[p & 1][1][r - 1]);
  }
}

// A run's 11 words of g are read up front by scalar loads (g is read-only
// for the kernel's lifetime: the constant address space) — one wait per run,
// the chunk values extracted on the scalar unit (~70 fewer VALU per step) —
// instead of a vector load per step whose vmcnt(0) opened every step: the
// 2^24 level 171.6 vs 180.0 us on average, make_shares_vec 2^20 -2 %
// (profiles/r05/y/).
typedef __attribute__((address_space(4))) const uint64_t const_u64_t;

template <int... ks>
__device__ __forceinline__ void jump_run(uint32_t (&Q)[11], const Lanes& L, const uint32_t* E,
                                         const uint32_t (&off)[16], const uint64_t* g, int wi, int top,
                                         std::integer_sequence<int, ks...>) {
  const_u64_t* gc = (const_u64_t*)(g);
  const int tu = __builtin_amdgcn_readfirstlane(top);
  uint64_t gws[sizeof...(ks)];
  ((void)(gws[ks] = gc[__builtin_amdgcn_readfirstlane(wi - ks <= tu ? wi - ks : tu)]), ...);  // in range
  ((void)(gws[ks] = (wi - ks) <= tu ? gws[ks] : 0ull), ...);
  ((void)jump_mega<ks>(Q, L, E, off, gws[ks]), ...);
}

// One workgroup = up to W jumps (or parts of jumps, words [lo, hi) of g)
// from the same source window W and the same lo (the host groups them;
// padding jobs have dst < 0).  Horner over 4-bit chunks of g,
// 16 chunks (one 64-bit word of g) per step: r <- f^64(r) ^ sum_t
// f^(4 (15 - t))(T[c_t]); f^m(T[v]) is the window at offset m of T[v]'s own
// stream, which the workgroup tables once (E, 82 KB of LDS), so a step is
//   * f^64(r): 64 new words mix(r[l], r[l+1], r[l+397]), l = 0..63 — one
//     register, its operands gathered by 3 ds_bpermute;
//   * the XOR of 16 table windows into the 624 window words (10 registers;
//     80 ds_read_b64 and 80 v_bitop3 per lane).
template <int W>  // waves per workgroup (8 or 16)
__global__ void __launch_bounds__(64 * W) mt_jump_kernel(const JumpArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t E[kEWords];
  __shared__ uint32_t ext[kMtN + 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint32_t j0 = blockIdx.x * W;
  const JumpJob* jp = a.jobs + __builtin_amdgcn_readfirstlane(j0 + wid < a.njobs ? j0 + wid : j0);
  const int32_t poly = __builtin_amdgcn_readfirstlane(jp->poly), dsti = __builtin_amdgcn_readfirstlane(jp->dst);
  // the workgroup's jobs share the source and lo (one table; job j0 is never padding)
  const int32_t lo = __builtin_amdgcn_readfirstlane(a.jobs[j0].span) & 0xffff;
  const int32_t hi = __builtin_amdgcn_readfirstlane(jp->span) >> 16;
  const uint32_t* src = a.wins + static_cast<int64_t>(__builtin_amdgcn_readfirstlane(a.jobs[j0].src)) * kMtN;
  if (lo == 0) {
    // the source stream: words 0..623 of W, then 63 more (each from words <= 459 of W)
    for (uint32_t i = tid; i < kMtN; i += 64u * W) ext[i] = src[i];
    __syncthreads();
    if (tid < 63u) ext[kMtN + tid] = mt_mix(ext[tid], ext[tid + 1], ext[tid + kMtM]);
    __syncthreads();
  } else {
    // words 64 lo .. 64 lo + 686 of W's stream: step the stream in a 1024-word
    // LDS ring (the table's space, not yet built), 227 words per step (word
    // 624 + i needs words i, i + 1, i + 397).  A step writes ring slots
    // 624..850 past its base and reads 0..623, so one barrier per step.
    uint32_t* ring = E;
    for (uint32_t i = tid; i < kMtN; i += 64u * W) ring[i] = src[i];
    __syncthreads();
    const uint32_t need = a.probe == 2u ? 687u : 64u * static_cast<uint32_t>(lo) + 687u;
    for (uint32_t base = 0; base + kMtN < need; base += kMtN - kMtM) {
      if (tid < static_cast<uint32_t>(kMtN - kMtM)) {
        const uint32_t i = base + tid;
        ring[(i + kMtN) & 1023u] = mt_mix(ring[i & 1023u], ring[(i + 1u) & 1023u], ring[(i + kMtM) & 1023u]);
      }
      __syncthreads();
    }
    for (uint32_t i = tid; i < 687u; i += 64u * W) ext[i] = ring[(64u * static_cast<uint32_t>(lo) + i) & 1023u];
    __syncthreads();
  }
  // One thread per stream position q = 64 k + m (row k = 0..10 of the frame,
  // m = 0..63; T-stream word j = q - 16, zero outside 0..683): the 16
  // combinations of words j..j+3 from four LDS reads, stored to the main half
  // (row k = 2 i + parity, k <= 9) and the wrap half (k = 2 i + parity + 1,
  // k >= 1) of pair plane i.  The gap before the wrap half and the planes'
  // pad words are never read.
  for (uint32_t q = tid; q < 704u; q += 64u * W) {
    const int j = static_cast<int>(q) - 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (j >= 0 && j < 684) {
#pragma unroll
      for (int b = 0; b < 4; ++b) w[b] = ext[j + b];
    }
    const uint32_t k = q >> 6, m = q & 63u;
    uint32_t* em = k <= 9u ? E + (k >> 1) * kEPair + 2u * m + (k & 1u) : nullptr;
    uint32_t* ew = k >= 1u ? E + kEWrap + ((k - 1u) >> 1) * kEPair + 2u * m + ((k - 1u) & 1u) : nullptr;
    uint32_t c[16];
    c[0] = 0u;
#pragma unroll
    for (int v = 1; v < 16; ++v) c[v] = c[v & (v - 1)] ^ w[__builtin_ctz(v)];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      if (em) em[v * kEVWords] = c[v];
      if (ew) ew[v * kEVWords] = c[v];
    }
  }
  __syncthreads();
  if (j0 + wid >= a.njobs || dsti < 0) return;

  // poly = table * rows + row, kMtDirectBase + length * 64 + s - 1, or
  // kMtRtBase + s - 1 (wave-uniform)
  const uint64_t* g = poly < kMtDirectBase ? &kMtPolysDev[0][0][0] + static_cast<uint64_t>(poly) * kMtPolyWords
                      : poly < kMtRtBase
                          ? &kMtDirectDev[0][0][0] + static_cast<uint64_t>(poly - kMtDirectBase) * kMtPolyWords
                          : a.rt + static_cast<uint64_t>(poly - kMtRtBase) * kMtPolyWords;
  uint32_t Q[11];
#pragma unroll
  for (int r = 0; r < 11; ++r) Q[r] = 0u;
  Lanes L;
  L.pa = static_cast<int>(((lane + 16u) & 63u) * 4u);
  L.pb = static_cast<int>(((lane + 17u) & 63u) * 4u);
  L.pm = static_cast<int>(((lane + 29u) & 63u) * 4u);
  L.la = lane < 16u, L.lb = lane < 17u, L.lm = lane < 29u;
  // chunk t's words for register r (1..10): table index 64 (r - 1) + lane + 60 - 4 t
  uint32_t off[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint32_t u = lane + 60u - 4u * t;
    off[t] = (u & 63u) * 2u + (u >> 6) * static_cast<uint32_t>(kEWrap);
  }
  int top = hi - 1;
  while (top > lo && g[top] == 0ull) --top;  // steps above it leave r = 0
  top = __builtin_amdgcn_readfirstlane(top);
  // runs of 11 steps (the frame returns to Q[0] after 11) ending at word lo;
  // r = 0 before the first nonzero word, so a run starts with zero words above it
  if (a.probe != 1u)
    for (int wi = lo + 11 * ((top - lo) / 11) + 10; wi >= lo + 10; wi -= 11)
      jump_run(Q, L, E, off, g, wi, top, std::make_integer_sequence<int, 11>{});
  uint32_t* dst = a.wins + static_cast<uint64_t>(dsti) * kMtN;
#pragma unroll
  for (int r = 0; r < 11; ++r) {
    const int i = 64 * r + static_cast<int>(lane) - 16;
    if (i >= 0 && i < kMtN) dst[i] = Q[r];
  }
}

// ---- jumps with a contiguous table: the two-bit kernel that sits beside the
// generation, and a four-bit variant
// mt_jump_kernel's Horner over CB-bit chunks of g (64 / CB per word of g)
// with the table T[v] = sum over bits j of v of f^j(W), v < 2^CB, stored as
// the 704 consecutive stream positions q = 64 k + m of each value (T-stream
// word q - 16; zero outside the used range): chunk t of a step reads, for
// window register r = 1..10, position 64 (r - 1) + lane + 64 - CB - CB t of
// T[c_t] — ten ds_read_b32 from one address (immediate offsets 256 B apart,
// 64 consecutive words per instruction: conflict-free, no wrapped copy), two
// chunks XORed per v_bitop3 as in mt_jump_kernel.
//  * CB = 2, W = 4 (mt_jumpc_kernel<4, 2>): 4 values, 11 KB — a workgroup fits
//    on a CU beside the generation's eight 17.7 KB rings (160 KB), at twice
//    the table bytes and XORs per word of g; the speculated levels that run
//    beside the generation (DN_MT_SPEC_BESIDE).
//  * CB = 4 (DN_MT_JUMP4B, tuning build): 16 values, 45 KB instead of
//    mt_jump_kernel's 83 (no wrapped copy), so two 16-wave workgroups share
//    a CU (<= 64 VGPRs): twice the waves per CU at twice the LDS
//    instructions (b32, same bytes) — an A/B of the direct level.
constexpr int kE2Val = 704;  // words per table value
// CB = 3: 21 three-bit chunks and bit 0 alone (22 per word of g, offsets 61 - 3 t
// and 0); T[0] = 0 is not stored (7 values, 19.3 KB: it still fits beside the
// rings) — a zero chunk's read goes to T[1] and its XOR is skipped (the chunk
// values are wave-uniform: a scalar branch per pair)
template <int CB>
constexpr int kNVal = CB == 3 ? 7 : (1 << CB);
template <int CB>
constexpr int kECWords = kNVal<CB> * kE2Val;  // 11 KB at CB = 2, 19.3 KB at 3, 45 KB at 4
template <int CB>
constexpr int kNChunks = CB == 3 ? 22 : 64 / CB;
static_assert(kECWords<2> >= 1024 + kMtN + 63, "the stepping ring and the source stream fit in the table's space");

template <int CB>
__device__ __forceinline__ uint32_t chunk_val(uint64_t gw, int t) {
  if constexpr (CB == 3) return t < 21 ? static_cast<uint32_t>(gw >> (61 - 3 * t)) & 7u : static_cast<uint32_t>(gw) & 1u;
  else return static_cast<uint32_t>(gw >> (64 - CB * (t + 1))) & ((1u << CB) - 1u);
}
template <int CB>
constexpr int chunk_off(int t) { return CB == 3 ? (t < 21 ? 61 - 3 * t : 0) : 64 - CB - CB * t; }
template <int CB>
__device__ __forceinline__ uint32_t chunk_row(uint32_t c) { return CB == 3 ? (c ? c - 1u : 0u) : c; }

template <int CB>
__device__ __forceinline__ void table_words_c(const uint32_t* E, uint32_t c, int t, uint32_t lane, uint32_t (&x)[10]) {
  const uint32_t* p = E + chunk_row<CB>(c) * static_cast<uint32_t>(kE2Val) + lane + static_cast<uint32_t>(chunk_off<CB>(t));
#pragma unroll
  for (int i = 0; i < 10; ++i) x[i] = p[64 * i];
}

template <int CB, int K>
__device__ __forceinline__ void jump_mega_c(uint32_t (&Q)[11], const Lanes& L, const uint32_t* E, uint32_t lane,
                                            uint64_t gw) {
  constexpr int NC = kNChunks<CB>;
  uint32_t x[2][2][10];
  append64<K>(Q, L);
  table_words_c<CB>(E, chunk_val<CB>(gw, 0), 0, lane, x[0][0]);
  table_words_c<CB>(E, chunk_val<CB>(gw, 1), 1, lane, x[0][1]);
#pragma unroll
  for (int p = 0; p < NC / 2; ++p) {
    if (p < NC / 2 - 1) {
      table_words_c<CB>(E, chunk_val<CB>(gw, 2 * p + 2), 2 * p + 2, lane, x[(p + 1) & 1][0]);
      table_words_c<CB>(E, chunk_val<CB>(gw, 2 * p + 3), 2 * p + 3, lane, x[(p + 1) & 1][1]);
    }
    if constexpr (CB == 3) {
      const bool n0 = chunk_val<CB>(gw, 2 * p) != 0u, n1 = chunk_val<CB>(gw, 2 * p + 1) != 0u;
      if (n0 && n1) {
#pragma unroll
        for (int r = 1; r < 11; ++r)
          Q[(r + K) % 11] = xor3(Q[(r + K) % 11], x[p & 1][0][r - 1], x[p & 1][1][r - 1]);
      } else if (n0 || n1) {
#pragma unroll
        for (int r = 1; r < 11; ++r) Q[(r + K) % 11] ^= n0 ? x[p & 1][0][r - 1] : x[p & 1][1][r - 1];
      }
    } else {
#pragma unroll
      for (int r = 1; r < 11; ++r)
        Q[(r + K) % 11] = xor3(Q[(r + K) % 11], x[p & 1][0][r - 1], x[p & 1][1][r - 1]);
    }
  }
}

template <int CB, int... ks>
__device__ __forceinline__ void jump_run_c(uint32_t (&Q)[11], const Lanes& L, const uint32_t* E, uint32_t lane,
                                           const uint64_t* g, int wi, int top, std::integer_sequence<int, ks...>) {
  const_u64_t* gc = (const_u64_t*)(g);
  const int tu = __builtin_amdgcn_readfirstlane(top);
  uint64_t gws[sizeof...(ks)];
  ((void)(gws[ks] = gc[__builtin_amdgcn_readfirstlane(wi - ks <= tu ? wi - ks : tu)]), ...);  // in range
  ((void)(gws[ks] = (wi - ks) <= tu ? gws[ks] : 0ull), ...);
  ((void)jump_mega_c<CB, ks>(Q, L, E, lane, gws[ks]), ...);
}

// Jobs as mt_jump_kernel's (W jumps or parts of one source and lo per
// workgroup); the source stream is staged in the table's space and read into
// registers before the table overwrites it.
template <int W, int CB>
__global__ void __launch_bounds__(64 * W, CB == 4 ? 8 : 1) mt_jumpc_kernel(const JumpArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t E[kECWords<CB>];
  uint32_t* ext = E + 1024;  // words 0 .. 686 of the source stream, until the table is built
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint32_t j0 = blockIdx.x * W;
  const JumpJob* jp = a.jobs + __builtin_amdgcn_readfirstlane(j0 + wid < a.njobs ? j0 + wid : j0);
  const int32_t poly = __builtin_amdgcn_readfirstlane(jp->poly), dsti = __builtin_amdgcn_readfirstlane(jp->dst);
  const int32_t lo = __builtin_amdgcn_readfirstlane(a.jobs[j0].span) & 0xffff;
  const int32_t hi = __builtin_amdgcn_readfirstlane(jp->span) >> 16;
  const uint32_t* src = a.wins + static_cast<int64_t>(__builtin_amdgcn_readfirstlane(a.jobs[j0].src)) * kMtN;
  if (lo == 0) {
    for (uint32_t i = tid; i < kMtN; i += 64u * W) ext[i] = src[i];
    __syncthreads();
    if (tid < 63u) ext[kMtN + tid] = mt_mix(ext[tid], ext[tid + 1], ext[tid + kMtM]);
    __syncthreads();
  } else {
    // words 64 lo .. 64 lo + 686 of the stream, stepped in a 1024-word ring (E[0, 1024))
    uint32_t* ring = E;
    for (uint32_t i = tid; i < kMtN; i += 64u * W) ring[i] = src[i];
    __syncthreads();
    const uint32_t need = 64u * static_cast<uint32_t>(lo) + 687u;
    for (uint32_t base = 0; base + kMtN < need; base += kMtN - kMtM) {
      for (uint32_t tt = tid; tt < static_cast<uint32_t>(kMtN - kMtM); tt += 64u * W) {
        const uint32_t i = base + tt;
        ring[(i + kMtN) & 1023u] = mt_mix(ring[i & 1023u], ring[(i + 1u) & 1023u], ring[(i + kMtM) & 1023u]);
      }
      __syncthreads();
    }
    for (uint32_t i = tid; i < 687u; i += 64u * W) ext[i] = ring[(64u * static_cast<uint32_t>(lo) + i) & 1023u];
    __syncthreads();
  }
  // the table: position q holds T[v] word j = q - 16 = XOR of s_{j+b} over bits b of v
  constexpr int kQ = (kE2Val + 64 * W - 1) / (64 * W);
  constexpr int kJEnd = 687 - (CB - 1);  // j + CB - 1 <= 686
  uint32_t w[kQ][CB];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int q = static_cast<int>(tid) + 64 * W * k, j = q - 16;
    const bool in = q < kE2Val && j >= 0 && j < kJEnd;
#pragma unroll
    for (int b = 0; b < CB; ++b) w[k][b] = in ? ext[j + b] : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int q = static_cast<int>(tid) + 64 * W * k;
    if (q < kE2Val) {
      uint32_t c[1 << CB];
      c[0] = 0u;
#pragma unroll
      for (int v = 1; v < (1 << CB); ++v) c[v] = c[v & (v - 1)] ^ w[k][__builtin_ctz(v)];
#pragma unroll
      for (int v = CB == 3 ? 1 : 0; v < (1 << CB); ++v) E[(CB == 3 ? v - 1 : v) * kE2Val + q] = c[v];
    }
  }
  __syncthreads();
  if (j0 + wid >= a.njobs || dsti < 0) return;

  const uint64_t* g = poly < kMtDirectBase ? &kMtPolysDev[0][0][0] + static_cast<uint64_t>(poly) * kMtPolyWords
                      : poly < kMtRtBase
                          ? &kMtDirectDev[0][0][0] + static_cast<uint64_t>(poly - kMtDirectBase) * kMtPolyWords
                          : a.rt + static_cast<uint64_t>(poly - kMtRtBase) * kMtPolyWords;
  uint32_t Q[11];
#pragma unroll
  for (int r = 0; r < 11; ++r) Q[r] = 0u;
  Lanes L;
  L.pa = static_cast<int>(((lane + 16u) & 63u) * 4u);
  L.pb = static_cast<int>(((lane + 17u) & 63u) * 4u);
  L.pm = static_cast<int>(((lane + 29u) & 63u) * 4u);
  L.la = lane < 16u, L.lb = lane < 17u, L.lm = lane < 29u;
  int top = hi - 1;
  while (top > lo && g[top] == 0ull) --top;
  top = __builtin_amdgcn_readfirstlane(top);
  if (a.probe != 1u)
    for (int wi = lo + 11 * ((top - lo) / 11) + 10; wi >= lo + 10; wi -= 11)
      jump_run_c<CB>(Q, L, E, lane, g, wi, top, std::make_integer_sequence<int, 11>{});
  uint32_t* dst = a.wins + static_cast<int64_t>(dsti) * kMtN;
#pragma unroll
  for (int r = 0; r < 11; ++r) {
    const int i = 64 * r + static_cast<int>(lane) - 16;
    if (i >= 0 && i < kMtN) dst[i] = Q[r];
  }
}

// cb: the chunk width of the kernel beside the generation, 2 or 3 (MtKnobs::beside_cb)
void launch_jumpc4(dim3 grid, hipStream_t s, const JumpArgs& ja, int cb) {
  if (cb == 2) hipLaunchKernelGGL((mt_jumpc_kernel<4, 2>), grid, dim3(256), 0, s, ja);
  else hipLaunchKernelGGL((mt_jumpc_kernel<4, 3>), grid, dim3(256), 0, s, ja);
}

// The parts of a split level XORed into their jumps' windows: one thread per
// window word, the (at most 16) part loads issued together.
__global__ void __launch_bounds__(640) mt_combine_kernel(uint32_t* wins, const CombineJob* cj) {
  const CombineJob c = cj[blockIdx.x];
  const uint32_t i = threadIdx.x;
  if (i >= static_cast<uint32_t>(kMtN)) return;
  const uint32_t* p = wins + static_cast<uint64_t>(c.first) * kMtN + i;
  uint32_t x = 0u;
#pragma unroll
  for (int32_t j = 0; j < kMaxParts; ++j)
    if (j < c.parts) x ^= p[static_cast<uint64_t>(j) * kMtN];
  wins[static_cast<int64_t>(c.dst) * kMtN + i] = x;  // (dst -1: the W_idx row)
}

// ------------------------------------------------------------------ generation
struct GenArgs {
  const uint32_t* wins;  // [S + 1][624]
  uint8_t* coeffs;       // tm1 tiled vectors
  uint32_t* flag;        // != 0: a draw was rejected
  uint32_t* fin;         // CPython's final array (the final-state wave)
  uint64_t ncoef;
  union {
    uint64_t vb;
    uint64_t nseg;  // SEG kernels: entries of `segs` before its sentinel
  };
  uint64_t sub_draws;    // draws per substream (2^k)
  uint64_t tm1_magic;    // ceil(2^32 / tm1): x / tm1 = (x * magic) >> 32 for x < 2^16
  uint32_t S;            // substreams
  uint32_t idx;          // CPython index: stream words 0..623-idx are temper(window0[idx..])
  int32_t tm1;
  int32_t final_sig;     // window the final-state wave starts from (-1: no such wave)
  uint64_t final_pos;    // position of that window's first word (0: the caller's array)
  uint64_t final_tf;     // position of CPython's final array
  // fused split (mt_gen_kernel<T>, T > 0): int64 secrets in, n share vectors out
  // SEG kernels (dn_mt19937_split_many_device): `secrets` is the concatenation
  // of a list of tensors, n_elem their total, and in place of one share block
  // and its pitch the kernel gets the tensors' blocks (seg_plan.hpp) — in a
  // union, so the argument block of the other kernels is what it was
  const int64_t* secrets;
  union {
    uint8_t* shares;
    const SegEnt* segs;
  };
  uint64_t n_elem;
  int32_t n_shares;
  uint32_t ring;         // ring slots of one wave (2 emission groups; GenRing)
  uint32_t back;         // even substreams 2 .. S-2 run backward from the next window
  uint32_t probe;        // tuning build only (DN_MT_PROBE): 1 skip emissions, 2 skip generation
  uint32_t sub_lo;       // substream of workgroup 0 (a launch over substreams sub_lo ..: DN_MT_SPLIT2)
  uint32_t sub_n;        // workgroups of the launch (0: S + 1, every substream and the final-state wave)
  uint32_t* next_win;    // the next call's W_idx (null: not wanted), written with the final state
  uint64_t next_pos;     // its position idx + 17 ncoef (final-state wave)
  // tail_fin: the last substream writes the final state (and next_win) itself
  // after its generation, at positions fin_lo / next_lo of its own frame
  // (position 0 its first output); no final-state wave is launched
  uint32_t tail_fin;
  int32_t fin_lo, next_lo;  // (fin_lo < 0: words of the substream's window, still in the ring)
};

// DN_MT_PROBE (tuning build): time the generation and the emission apart.
#ifdef DN_TUNING
#define DN_PROBE_SKIP(a, bit) if (!((a).probe & (bit)))
#else
#define DN_PROBE_SKIP(a, bit)
#endif

// Raw (untempered) words of a substream pass through an LDS ring of M words
// (M = two emission groups): stream word p sits at slot (p + delta) mod M,
// physical word o + slot, and physical words [o + M, o + M + 64) mirror slots
// [0, 64).
//  * An append writes the 64 words p0 .. p0 + 63 (p0 + delta a multiple of
//    64, so its slots never wrap), word p = mix(word p - 624, word p - 623,
//    word p - 227): one address plus immediates, except in the first 688
//    slots of the ring, where the three operands' slots wrap per lane (a
//    wave-uniform branch, 11 of 68 appends at t = 3).
//  * An emission group [g G, (g + 1) G) reads physical o + delta + (g % 2) G
//    onwards, below o + M + 64: the mirror holds the slots past M.
// delta is 0 except in substream 0, whose stream starts with the caller's
// 624 - idx words; o = delta & 1 keeps every group's first word 8-byte aligned
// (the emission's b64 reads).  Tempering happens when a group is emitted.
// Per 64 words an append is one address add, three ds_read_b32, the mix
// (5 VALU) and one ds_write — against three ds_bpermute, their operand
// selects, the mix, the temper and the ring address arithmetic of a
// register-resident window.
struct GenRing {
  uint32_t M, delta, o;
};

__device__ __forceinline__ uint32_t ring_wrap(uint32_t s, uint32_t M) { return s >= M ? s - M : s; }

// mt_mix in five VALU: y = bfi(UP, a, b); m ^ (y >> 1) ^ (-(b & 1) & A), the
// last two terms by v_bitop3 ((S0 & S1) ^ S2, table 0x6a; S0 the index MSB).
__device__ __forceinline__ uint32_t mt_mix5(uint32_t a, uint32_t b, uint32_t m) {
  const uint32_t y = (kMtUp & a) | (~kMtUp & b);  // v_bfi_b32
  const uint32_t u = (y >> 1) ^ m;
  const uint32_t mk = static_cast<uint32_t>(static_cast<int32_t>(b << 31) >> 31);
  return __builtin_amdgcn_bitop3_b32(mk, kMtA, u, 0x6a);  // (mk & A) ^ u
}

// B appends (B <= 3: the appends of a batch read no word another one of the
// batch writes: word p + 64 i - 227 < p for i < 3), reads first, one wait.
// WRAP: some operand slots of the batch lie below 0 (the batch starts in the
// ring's first 688 slots, or the batch itself wraps) and are wrapped per lane.
// vals: the raw words (the final-state wave keeps them).
template <int B, bool WRAP>
__device__ __forceinline__ void ring_appends(uint32_t* Rg, const GenRing& g, uint32_t slot, uint32_t lane,
                                             uint32_t (&vals)[3]) {
  uint32_t s[B], xa[B], xb[B], xm[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    if constexpr (WRAP) {
      s[i] = ring_wrap(slot + 64u * i, g.M);
      const uint32_t q = s[i] + lane;
      const uint32_t qa = q < 624u ? q + g.M - 624u : q - 624u;
      const uint32_t qb = qa + 1u == g.M ? 0u : qa + 1u;
      const uint32_t qm = q < 227u ? q + g.M - 227u : q - 227u;
      xa[i] = Rg[g.o + qa];
      xb[i] = Rg[g.o + qb];
      xm[i] = Rg[g.o + qm];
    } else {
      s[i] = slot + 64u * i;
      const uint32_t* p = Rg + (g.o + s[i] - 624u) + lane;
      xa[i] = p[0];
      xb[i] = p[1];
      xm[i] = p[kMtM];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // every read of the batch issued before the first mix waits
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const uint32_t v = mt_mix5(xa[i], xb[i], xm[i]);
    vals[i] = v;
    Rg[g.o + s[i] + lane] = v;
    if (WRAP && s[i] == 0u) Rg[g.o + g.M + lane] = v;  // mirror of slots 0 .. 63
  }
}

template <int B>
__device__ __forceinline__ void ring_batch(uint32_t* Rg, const GenRing& g, uint32_t& slot, uint32_t lane,
                                           uint32_t (&vals)[3]) {
  const uint32_t s0 = __builtin_amdgcn_readfirstlane(slot);
  if (s0 >= 688u && s0 + 64u * B <= g.M) ring_appends<B, false>(Rg, g, s0, lane, vals);
  else ring_appends<B, true>(Rg, g, s0, lane, vals);
  slot = __builtin_amdgcn_readfirstlane(ring_wrap(s0 + 64u * B, g.M));
}

// NA appends as batches of three (one of one or two last).
// The final-state wave: CPython's final array (stream positions tf .. tf +
// 623) into a.fin, from the window at position P = a.final_pos (its word 0)
// onwards, and — when the call speculates on its successor (a.next_win,
// DN_MT_SPEC) — the window at position a.next_pos (>= tf): the next call's
// W_idx, the source of its jump levels.
__device__ __forceinline__ void final_state_wave(uint32_t* R, const GenRing& g, uint32_t slot, uint32_t lane,
                                                 const uint32_t* win, const GenArgs& a) {
  const uint64_t P = a.final_pos, tf = a.final_tf, nx = a.next_pos;
  uint32_t* nw = a.next_win;
  const uint64_t end = nw ? nx + kMtN : tf + kMtN;
  for (uint32_t i = lane; i < static_cast<uint32_t>(kMtN); i += 64u) {
    const uint64_t x = P + i;
    if (x >= tf && x < tf + kMtN) a.fin[x - tf] = win[i];
    if (nw && x >= nx && x < nx + kMtN) nw[x - nx] = win[i];
  }
  uint64_t np = P + kMtN;  // position of the next append's word 0
  while (np < end) {
    uint32_t v[3];
    ring_batch<3>(R, g, slot, lane, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint64_t x = np + 64u * k + lane;
      if (x >= tf && x < tf + kMtN) a.fin[x - tf] = v[k];
      if (nw && x >= nx && x < nx + kMtN) nw[x - nx] = v[k];
    }
    np += 192u;
  }
}

// The last substream's tail (tail_fin): CPython's final array (positions
// fin_lo .. fin_lo + 623 of the substream's frame) and, when the call
// speculates, the next call's W_idx (next_lo .., next_lo >= fin_lo), from the
// ring — which holds the substream's last M words, `end` being the position
// of the next append — and at most ten more appends.  The draw ends at
// next_lo, at most 624 words past fin_lo and at most a group before `end`, so
// every word needed is either still in the ring or appended here.
__device__ __forceinline__ void last_sub_tail(uint32_t* R, const GenRing& g, uint32_t slot, uint32_t lane, uint32_t end,
                                              const GenArgs& a) {
  const int32_t f0 = a.fin_lo, n0 = a.next_lo, e = static_cast<int32_t>(end);
  const int32_t off = static_cast<int32_t>(g.delta + g.M);  // slot of position x: (x + off) % M, x >= -624
  uint32_t* nw = a.next_win;
  for (int32_t i = static_cast<int32_t>(lane); i < kMtN; i += 64) {
    const int32_t x = f0 + i, y = n0 + i;
    if (x < e) a.fin[i] = R[g.o + static_cast<uint32_t>(x + off) % g.M];
    if (nw && y < e) nw[i] = R[g.o + static_cast<uint32_t>(y + off) % g.M];
  }
  const int32_t stop = (nw ? n0 : f0) + kMtN;
  for (int32_t p = e; p < stop; p += 64) {
    uint32_t v[3];
    ring_batch<1>(R, g, slot, lane, v);
    const int32_t x = p + static_cast<int32_t>(lane);
    if (x >= f0 && x < f0 + kMtN) a.fin[x - f0] = v[0];
    if (nw && x >= n0 && x < n0 + kMtN) nw[x - n0] = v[0];
  }
}

template <int NA>
__device__ __forceinline__ void ring_run(uint32_t* Rg, const GenRing& g, uint32_t& slot, uint32_t lane) {
  uint32_t v[3];
#pragma unroll
  for (int k = 0; k + 3 <= NA; k += 3) ring_batch<3>(Rg, g, slot, lane, v);
  if constexpr (NA % 3) ring_batch<NA % 3>(Rg, g, slot, lane, v);
}

// n appends, n known at run time (batches of three, then one or two).
__device__ __forceinline__ void ring_run_rt(uint32_t* Rg, const GenRing& g, uint32_t& slot, uint32_t lane,
                                            uint32_t n) {
  uint32_t v[3];
  uint32_t k = 0;
  for (; k + 3u <= n; k += 3u) ring_batch<3>(Rg, g, slot, lane, v);
  if (n - k == 2u) ring_batch<2>(Rg, g, slot, lane, v);
  else if (n - k == 1u) ring_batch<1>(Rg, g, slot, lane, v);
}

// The window (624 raw words at stream positions [p_start - 624, p_start))
// into the ring, with the mirror.
__device__ __forceinline__ void ring_init(uint32_t* Rg, const GenRing& g, const uint32_t* win, uint32_t p_start,
                                          uint32_t lane) {
  for (uint32_t i = lane; i < static_cast<uint32_t>(kMtN); i += 64u) {
    // slot of position p_start - 624 + i, in [0, M)
    const uint32_t s = (p_start + g.delta + g.M - static_cast<uint32_t>(kMtN) + i) % g.M;
    const uint32_t v = win[i];
    Rg[g.o + s] = v;
    if (s < 64u) Rg[g.o + g.M + s] = v;
  }
}

// ---- backward generation ----------------------------------------------------
// The word transition is invertible, so one jump window serves two
// substreams: substream s + 1 forward from W(s + 1) and substream s backward
// from it (W(s + 1) is the last 624 raw words of substream s).  Only windows
// of odd s (and of the last substream) are jumped to — half of level B.
// From word p + 624 = mix(x_p, x_{p+1}, x_{p+397}) with t_p = x_{p+624} ^
// x_{p+397} = (y >> 1) ^ (y odd ? A : 0), y = (x_p & UP) | (x_{p+1} & LO):
// A's top bit is set and y >> 1's is clear, so y's low bit is t_p's top bit and
// y = ((t_p ^ (that bit ? A : 0)) << 1) | bit.  x_p takes its top bit from y_p
// (bit 30 of t_p, A's bit 30 being clear) and its low 31 bits from y_{p-1}:
//   x_p = alignbit(bfi(2^30, t_p, t_{p-1} ^ (A & -(t_{p-1} >> 31))), t_{p-1}, 31)
// — six VALU over words p + 396, p + 397, p + 623 and p + 624.  A word needs
// none of the 395 words below it, so six 64-word blocks are independent.
__device__ __forceinline__ uint32_t mt_unmix(uint32_t x396, uint32_t x397, uint32_t x623, uint32_t x624) {
  const uint32_t t1 = x624 ^ x397, t0 = x623 ^ x396;
  const uint32_t m0 = static_cast<uint32_t>(static_cast<int32_t>(t0) >> 31);
  const uint32_t u0 = __builtin_amdgcn_bitop3_b32(m0, kMtA, t0, 0x6a);  // (m0 & A) ^ t0
  const uint32_t up = (0x40000000u & t1) | (~0x40000000u & u0);        // v_bfi_b32
  return __builtin_amdgcn_alignbit(up, t0, 31);
}

// B blocks below ring slot `top` (block i: slots [top - 64 (i + 1), top - 64 i),
// lane = word), reads first.  Backward substreams use delta = 0 (slot =
// position mod M).  WRAP: operand slots at or past M wrap (top > M - 624).
// PART: only slots below `lim` are written (the first block under the window).
template <int B, bool WRAP, bool PART>
__device__ __forceinline__ void back_blocks(uint32_t* Rg, uint32_t M, uint32_t top, uint32_t lane, uint32_t lim) {
  uint32_t q[B], x396[B], x397[B], x623[B], x624[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    q[i] = top - 64u * (i + 1) + lane;
    if constexpr (WRAP) {
      auto w = [&](uint32_t s) { return Rg[s >= M ? s - M : s]; };
      x396[i] = w(q[i] + 396u);
      x397[i] = w(q[i] + 397u);
      x623[i] = w(q[i] + 623u);
      x624[i] = w(q[i] + 624u);
    } else {
      const uint32_t* p = Rg + q[i] + 396u;
      x396[i] = p[0];
      x397[i] = p[1];
      x623[i] = p[227];
      x624[i] = p[228];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // every read issued before the first unmix waits
#pragma unroll
  for (int i = 0; i < B; ++i) {
    const uint32_t v = mt_unmix(x396[i], x397[i], x623[i], x624[i]);
    if (!PART || q[i] < lim) Rg[q[i]] = v;
  }
}

template <int B>
__device__ __forceinline__ void back_batch(uint32_t* Rg, uint32_t M, uint32_t& top, uint32_t lane) {
  const uint32_t t0 = __builtin_amdgcn_readfirstlane(top);
  if (t0 + 624u <= M) back_blocks<B, false, false>(Rg, M, t0, lane, 0u);
  else back_blocks<B, true, false>(Rg, M, t0, lane, 0u);
  top = t0 - 64u * B;
}

// NB blocks down from `top`, as batches of six (one shorter last); a run that
// ended at slot 0 continues from slot M.
template <int NB>
__device__ __forceinline__ void back_run(uint32_t* Rg, uint32_t M, uint32_t& top, uint32_t lane) {
  if (top == 0u) top = M;
#pragma unroll
  for (int k = 0; k + 6 <= NB; k += 6) back_batch<6>(Rg, M, top, lane);
  if constexpr (NB % 6) back_batch<NB % 6>(Rg, M, top, lane);
}

// A rejected draw: every writer stores the same nonzero word, so a plain
// store serves (no atomic: the flag may live in pinned host memory, where a
// device atomic would be a PCIe atomic).
__device__ __forceinline__ void mt_flag(const GenArgs& a) { __hip_atomic_store(a.flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// 64 draws of one group (lane = draw c of this substream, raw words 17 c ..
// 17 c + 16 of the group at `rb`): temper, +1, rejection test, tiled store.
__device__ __forceinline__ void emit_group(const GenArgs& a, const uint32_t* rb, uint64_t qb, uint32_t rbm,
                                          uint32_t c, uint32_t nloc, uint32_t lane, bool mid = false) {
  if (c >= nloc) return;
  uint32_t v[kLimbs];  // (the group's ring slice is 64 draws of 17 words)
  const uint32_t* w = rb + 17u * lane;
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = w[i];
  if (mid) pc_barrier();  // mt_gen_pc_kernel: the producer may now overwrite this group's slots
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = mt_temper(v[i]);
  v[16] >>= 23;
  uint32_t all = v[1];
#pragma unroll
  for (int i = 2; i < 16; ++i) all &= v[i];
  if (v[16] == 0x1FFu && v[0] >= 0xFFFFFFFEu && all == 0xFFFFFFFFu) mt_flag(a);  // >= p - 1: rejected
  uint32_t cy = 1u;  // + 1 (randint's lower bound); v < p - 1: no carry out of limb 16
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = __builtin_addc(v[i], 0u, cy, &cy);
  // draw number of the whole stream = S0 + c with S0 = qb tm1 + rbm: element, row
  const uint32_t x = rbm + c;
  const uint32_t ex = static_cast<uint32_t>((static_cast<uint64_t>(x) * a.tm1_magic) >> 32);
  const uint32_t j = x - ex * static_cast<uint32_t>(a.tm1);
  const uint64_t e = qb + ex;
  uint8_t* tb = a.coeffs + j * a.vb + (e >> 8) * kTileBytes;
  const uint32_t wl = static_cast<uint32_t>(e & 255u);
#pragma unroll
  for (int i = 0; i < 16; ++i) __builtin_nontemporal_store(v[i], reinterpret_cast<uint32_t*>(tb) + i * kTile + wl);
  __builtin_nontemporal_store(static_cast<uint16_t>(v[16]), reinterpret_cast<uint16_t*>(tb + kHiOffset) + wl);
}

// Fused split (T = t): the 64 elements of one group (lane = element, 64 (t-1)
// consecutive draws of this substream, element-major as make_shares draws
// them: raw words 17 ((t-1) lane + j - 1) .. + 16 of the group for
// coefficient j), their int64 secrets, and the split of split_kernel<T,
// false, false>: the forward-difference table stored share by share.
// The group's coefficients (ring words of this lane's element, tempered, +1,
// rejection flagged) and secret s into the difference table c (fd_init).
template <int T>
__device__ __forceinline__ void emit_prepare(const GenArgs& a, const uint32_t* rb, uint32_t lane, uint64_t s,
                                             uint32_t (&c)[T][kLimbs], bool mid) {
  constexpr int TM1 = T - 1;
  const uint32_t* w = rb + 17u * TM1 * lane;
  if constexpr (TM1 % 2 == 0) {
    // an element's 17 (t-1) words start at an even word: 8-B reads, and with
    // a lane stride of 34 words (t = 3) the 32 lanes of a b64 group hit 32
    // distinct bank pairs (b32 reads at that stride are 2-way conflicted)
    uint32_t ww[17 * TM1];
#pragma unroll
    for (int k = 0; k < 17 * TM1 / 2; ++k) {
      const u32x2_t d = *reinterpret_cast<const u32x2_t*>(w + 2 * k);
      ww[2 * k] = d.x, ww[2 * k + 1] = d.y;
    }
    if (mid) pc_barrier();  // mt_gen_pc_kernel: the producer may now overwrite this group's slots
#pragma unroll
    for (int j = 1; j < T; ++j)
#pragma unroll
      for (int i = 0; i < kLimbs; ++i) c[j][i] = mt_temper(ww[17 * (j - 1) + i]);
  } else {
#pragma unroll
    for (int j = 1; j < T; ++j)
#pragma unroll
      for (int i = 0; i < kLimbs; ++i) c[j][i] = w[17 * (j - 1) + i];
    if (mid) pc_barrier();
#pragma unroll
    for (int j = 1; j < T; ++j)
#pragma unroll
      for (int i = 0; i < kLimbs; ++i) c[j][i] = mt_temper(c[j][i]);
  }
#pragma unroll
  for (int j = 1; j < T; ++j) {
    c[j][16] >>= 23;
    uint32_t all = c[j][1];
#pragma unroll
    for (int i = 2; i < 16; ++i) all &= c[j][i];
    if (c[j][16] == 0x1FFu && c[j][0] >= 0xFFFFFFFEu && all == 0xFFFFFFFFu) mt_flag(a);
    uint32_t cy = 1u;  // randint(1, p-1) = 1 + getrandbits(521)
#pragma unroll
    for (int i = 0; i < kLimbs; ++i) c[j][i] = __builtin_addc(c[j][i], 0u, cy, &cy);
  }
  c[0][0] = static_cast<uint32_t>(s);
  c[0][1] = static_cast<uint32_t>(s >> 32);
#pragma unroll
  for (int i = 2; i < kLimbs; ++i) c[0][i] = 0u;
  fd_init<T>(c);
}

// The segment table of a SEG kernel, as a pointer into the constant address
// space: the host wrote it before the launch and no kernel writes it, so its
// entries come by scalar loads (a uniform index, SGPR results: wave-uniform
// descriptors without a waterfall loop, and no vector load queued behind the
// share stores in flight).
typedef const __attribute__((address_space(4))) SegEnt* SegTab;
__device__ __forceinline__ SegTab seg_table(const GenArgs& a) { return (SegTab)a.segs; }

__device__ __forceinline__ uint64_t uniform64(uint64_t x) {  // a wave-uniform value, into SGPRs
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
  return static_cast<uint64_t>(hi) << 32 | lo;
}

// A group that is not one tile of one share block (SEG only): per share, one
// pass over the segments [k, ...) that intersect the group — a wave-uniform
// loop, one iteration per segment (64 for a group of one-element tensors) —
// each storing its lanes through one scalar descriptor per share row, based at
// the row's first touched tile and clamped to the row's end; a lane adds only
// its offset (one tile's bytes more once it has crossed into the next tile).
template <int T, int SAUX>
__device__ __forceinline__ void emit_pieces(const GenArgs& a, uint32_t k0, uint64_t ebase, uint32_t lane, int32_t ns,
                                            uint32_t (&c)[T][kLimbs]) {
  const uint64_t gend = a.n_elem - ebase < 64u ? a.n_elem : ebase + 64u;
  const SegTab tab = seg_table(a);
#pragma unroll 1
  for (int32_t xi = 0; xi < ns; ++xi) {
#pragma unroll 1
    for (uint32_t k = k0; tab[k].e_begin < gend; ++k) {  // (the sentinel's n_total >= gend ends it)
      const SegEnt sg{tab[k].e_begin, tab[k].shares, tab[k].row_bytes};
      const SegPiece p = seg_piece(sg.e_begin, tab[k + 1u].e_begin, sg.row_bytes, ebase, a.n_elem);
      const uint8_t* base = sg.shares + static_cast<uint64_t>(xi) * sg.row_bytes + p.tile0 * kTileBytes;
      const rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, static_cast<int>(p.range),
                                                         0x00020000);
      if (lane >= p.lane_lo && lane < p.lane_hi) {
        const uint32_t w = p.w0 + lane - p.lane_lo;
        store_reduced_at<SAUX>(r, seg_voff32(w), seg_voff16(w), c[0]);
      }
    }
    fd_step<T>(c);
  }
}

template <int T, int SAUX, int NS, bool WHOLE>
__device__ __forceinline__ void emit_split(const GenArgs& a, const uint32_t* rb, uint64_t ebase, uint32_t lane,
                                           uint64_t s, bool mid = false) {
  // ebase (the group's first element) is wave-uniform and a multiple of 64, so
  // the group's 64 elements share one tile: its index is a scalar and every
  // share store takes the tile's buffer descriptor from SGPRs (no per-lane
  // descriptor, no waterfall loop around the stores)
  const uint32_t tile = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(ebase >> 8));
  const uint64_t e = ebase + lane;
  if (!WHOLE && e >= a.n_elem) return;  // WHOLE: every element of the group is in the vector
  uint32_t c[T][kLimbs];
  emit_prepare<T>(a, rb, lane, s, c, mid);
  const uint32_t wl = static_cast<uint32_t>(e & 255u);
  if constexpr (NS > 0) {
#pragma unroll
    for (int xi = 1; xi <= NS; ++xi) {
      store_reduced<SAUX>(tile_rsrc(tile_base(a.shares + static_cast<uint64_t>(xi - 1) * a.vb, tile)), wl, c[0]);
      if (xi < NS) fd_step<T>(c);
    }
  } else {
#pragma unroll 1
    for (int32_t xi = 1; xi <= a.n_shares; ++xi) {
      store_reduced<SAUX>(tile_rsrc(tile_base(a.shares + static_cast<uint64_t>(xi - 1) * a.vb, tile)), wl, c[0]);
      fd_step<T>(c);
    }
  }
}

// emit_split where the elements are the concatenation of a list of tensors,
// each with a share block of its own (a.segs; SEG kernels).  `seg` is the
// wave's cursor into the table, moved here to the segment of the group's first
// element.  A group inside one segment that starts at a multiple of 64 is one
// tile of that segment's block: emit_split's stores from the segment's base
// and pitch.  Any other group goes segment by segment (emit_pieces).
template <int T, int SAUX, int NS, bool WHOLE>
__device__ __forceinline__ void emit_split_seg(const GenArgs& a, const uint32_t* rb, uint64_t ebase, uint32_t lane,
                                               uint64_t s, uint32_t& seg, bool mid = false) {
  const uint64_t e = ebase + lane;
  if (!WHOLE && e >= a.n_elem) return;
  // (the table's scalar loads before the ring reads and the tempering)
  const uint64_t eb = uniform64(ebase);
  const SegTab tab = seg_table(a);
  seg = __builtin_amdgcn_readfirstlane(seg_step(tab, seg, eb));
  const SegEnt sg{tab[seg].e_begin, tab[seg].shares, tab[seg].row_bytes};
  const uint64_t seg_next = tab[seg + 1u].e_begin;
  uint32_t c[T][kLimbs];
  emit_prepare<T>(a, rb, lane, s, c, mid);
  if (!seg_single_tile(sg.e_begin, seg_next, eb, a.n_elem)) {
    emit_pieces<T, SAUX>(a, seg, eb, lane, NS > 0 ? NS : a.n_shares, c);
    return;
  }
  const uint64_t l0 = eb - sg.e_begin;  // a multiple of 64: the lanes stay in its tile
  const uint32_t tile = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(l0 >> 8));
  const uint32_t wl = (static_cast<uint32_t>(l0) & 255u) + lane;
  if constexpr (NS > 0) {
#pragma unroll
    for (int xi = 1; xi <= NS; ++xi) {
      store_reduced<SAUX>(tile_rsrc(tile_base(sg.shares + static_cast<uint64_t>(xi - 1) * sg.row_bytes, tile)), wl,
                          c[0]);
      if (xi < NS) fd_step<T>(c);
    }
  } else {
#pragma unroll 1
    for (int32_t xi = 1; xi <= a.n_shares; ++xi) {
      store_reduced<SAUX>(tile_rsrc(tile_base(sg.shares + static_cast<uint64_t>(xi - 1) * sg.row_bytes, tile)), wl,
                          c[0]);
      fd_step<T>(c);
    }
  }
}

// One 64-thread workgroup per substream (one extra for CPython's final state):
// T == 0 stores the coefficients (groups of 64 draws), T > 0 splits the
// substream's elements (groups of 64 elements) with them as they are drawn.
// Dynamic LDS: 1 + ring + 64 words (GenRing).
template <int T, int SAUX = kNt, int NS = 0, bool SEG = false>
__global__ void __launch_bounds__(64) mt_gen_kernel(const GenArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t sub = blockIdx.x + a.sub_lo;
  if (sub > a.S || (sub == a.S && a.final_sig < 0)) return;
  const bool fin_wave = sub == a.S;
  const bool fwd = fin_wave || mt_sub_forward(sub, a.S, static_cast<int>(a.back));
  const uint32_t sub_words = 17u * static_cast<uint32_t>(a.sub_draws);
  const uint32_t wsel = fin_wave ? static_cast<uint32_t>(a.final_sig) : fwd ? sub : sub + 1u;
  const uint32_t* win = a.wins + static_cast<uint64_t>(wsel) * kMtN;
  // positions of this substream: word 0 is its first output; the window holds
  // [p_start - 624, p_start) (substream 0: the caller's array, whose words
  // idx .. 623 are outputs 0 .. 623 - idx; a backward substream: its last 624
  // words, slots M - 624 .. M - 1 since the substream is a whole number of
  // ring lengths)
  const uint32_t p_start = (sub == 0 && !fin_wave) ? kMtN - a.idx : fwd ? 0u : sub_words;
  GenRing g;
  g.M = a.ring;
  g.delta = (64u - (p_start & 63u)) & 63u;
  g.o = g.delta & 1u;
  uint32_t* R = s_ring;
  ring_init(R, g, win, p_start, lane);
  uint32_t slot = __builtin_amdgcn_readfirstlane((p_start + g.delta) % g.M);  // slot of the next append
  wave_sync();
  if (fin_wave) {
    final_state_wave(R, g, slot, lane, win, a);
    return;
  }
  const uint32_t group = a.ring / 2u;                            // words per emission group
  const uint64_t k0 = static_cast<uint64_t>(sub) * a.sub_draws;  // first draw of this substream
  const uint32_t nloc = static_cast<uint32_t>(a.ncoef - k0 < a.sub_draws ? a.ncoef - k0 : a.sub_draws);
  const uint32_t gdraws = T ? 64u * (T - 1) : 64u;  // draws per group
  const uint32_t ngroups = (nloc + gdraws - 1u) / gdraws;
  const uint64_t qb = k0 / static_cast<uint64_t>(a.tm1);
  const uint32_t rbm = static_cast<uint32_t>(k0 - qb * static_cast<uint64_t>(a.tm1));
  constexpr int kRun = 17 * (T ? T - 1 : 1);  // appends per run = one group's words / 64
  static_assert(kRun > 10, "a group holds the 640 words under the window");
  // SEG: the segment of the first group emitted (the substream's top group
  // when it runs backward); emit_split steps the cursor from there
  [[maybe_unused]] uint32_t seg = 0u;
  if constexpr (SEG && T > 0) {
    const uint64_t efirst = uniform64(fwd ? qb : qb + 64u * (ngroups - 1u));
    seg = __builtin_amdgcn_readfirstlane(seg_find(seg_table(a), static_cast<uint32_t>(a.nseg), efirst));
  }
  if (!fwd) {
    // Backward: whole groups, all inside the vector (never the last
    // substream), last group first; group gi sits in ring half gi % 2
    // (ngroups is even, so the window is the top of half 1).  First the 16
    // words under the window (one block, masked), then the group's other
    // kRun - 10 blocks, then per group: emit it, generate the one below.
    const uint32_t M = a.ring;
    back_blocks<1, true, true>(R, M, M - 576u, lane, M - 624u);
    uint32_t top = M - 640u;
    back_run<kRun - 10>(R, M, top, lane);
    wave_sync();
    if constexpr (T == 0) {
      for (uint32_t gi = ngroups - 1u;; --gi) {
        emit_group(a, R + (gi & 1u) * group, qb, rbm, 64u * gi + lane, nloc, lane);
        if (gi == 0u) break;
        wave_sync();
        back_run<kRun>(R, M, top, lane);
        wave_sync();
      }
    } else {
      // the next (lower) group's secrets loaded before this group's share
      // stores, into one of two registers by parity (as the forward loop)
      const uint64_t e0 = qb + lane;
      auto secret_of = [&](uint32_t gi) {
        return static_cast<uint64_t>(__builtin_nontemporal_load(a.secrets + e0 + 64u * gi));
      };
      auto bstep = [&](uint32_t gi, uint64_t cur, uint64_t& nxt) {
        DN_PROBE_SKIP(a, 2u) back_run<kRun>(R, M, top, lane);
        wave_sync();
        nxt = secret_of(gi ? gi - 1u : 0u);
        DN_PROBE_SKIP(a, 1u)
        if constexpr (SEG)
          emit_split_seg<T, SAUX, NS, true>(a, R + (gi & 1u) * group, qb + 64u * gi, lane, cur, seg);
        else
          emit_split<T, SAUX, NS, true>(a, R + (gi & 1u) * group, qb + 64u * gi, lane, cur);
        wave_sync();
      };
      uint64_t secA = secret_of(ngroups - 1u), secB = secret_of(ngroups - 2u);
      DN_PROBE_SKIP(a, 1u)
      if constexpr (SEG)
        emit_split_seg<T, SAUX, NS, true>(a, R + group, qb + 64u * (ngroups - 1u), lane, secA, seg);
      else
        emit_split<T, SAUX, NS, true>(a, R + group, qb + 64u * (ngroups - 1u), lane, secA);
      wave_sync();
      for (uint32_t gi = ngroups - 2u;; gi -= 2u) {
        bstep(gi, secB, secA);
        if (gi == 0u) break;
        bstep(gi - 1u, secA, secB);
        if (gi == 1u) break;
      }
      asm volatile("" : : "v"(secA ^ secB));  // no load left in flight at the end
    }
    return;
  }
  // Every run appends exactly one group's words (have = p_start + runs * group
  // with p_start < group), so each run is followed by exactly one emission.
  if constexpr (T == 0) {
    for (uint32_t done = 0; done < ngroups; ++done) {
      DN_PROBE_SKIP(a, 2u) ring_run<kRun>(R, g, slot, lane);
      wave_sync();
      DN_PROBE_SKIP(a, 1u)
      emit_group(a, R + g.o + g.delta + (done & 1u) * group, qb, rbm, 64u * done + lane, nloc, lane);
      wave_sync();
    }
    if (a.tail_fin && sub + 1u == a.S) last_sub_tail(R, g, slot, lane, p_start + ngroups * group, a);
  } else {
    // The int64 secret of this lane's element in the next group is loaded a
    // group ahead — before the current group's share stores, since loads and
    // stores retire in issue order and a load issued after them would wait for
    // them — into one of two registers by group parity (no copy of a pending
    // load), from an index clamped to the vector (the last prefetch is unused).
    // With the share count a template argument (NS) and only whole groups
    // (all 64 elements in the vector) in the loop, the share stores are
    // straight-line code on every path and the wait before a prefetched
    // secret's use leaves them in flight (vmcnt(63)); a runtime share loop or a
    // lane-masked emission gets vmcnt(<= 1).  A last partial group is emitted
    // after the loop, with a secret loaded at that point.
    const uint64_t e0 = qb + lane;  // k0 / (t-1) = the substream's first element
    const uint64_t elast = a.n_elem - 1u;
    auto secret_of = [&](uint32_t gi) {
      const uint64_t e = e0 + 64u * gi;
      return static_cast<uint64_t>(__builtin_nontemporal_load(a.secrets + (e < elast ? e : elast)));
    };
    const uint64_t rem = a.n_elem - qb;  // elements from this substream's first one to the vector's end
    const uint32_t nfull = rem >= 64ull * ngroups ? ngroups : static_cast<uint32_t>(rem / 64u);
    auto step = [&](uint32_t gi, uint64_t cur, uint64_t& nxt) {
      DN_PROBE_SKIP(a, 2u) ring_run<kRun>(R, g, slot, lane);
      wave_sync();
      nxt = secret_of(gi + 1u);
      DN_PROBE_SKIP(a, 1u)
      if constexpr (SEG)
        emit_split_seg<T, SAUX, NS, true>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, cur, seg);
      else
        emit_split<T, SAUX, NS, true>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, cur);
      wave_sync();
    };
    uint64_t secA = secret_of(0), secB = 0;
    uint32_t gi = 0;
    if (nfull > 0u) {
      step(0u, secA, secB);
      gi = 1u;
      for (; gi + 1u < nfull; gi += 2u) {
        step(gi, secB, secA);
        step(gi + 1u, secA, secB);
      }
      if (gi < nfull) {
        step(gi, secB, secA);
        ++gi;
      }
    }
    if (gi < ngroups) {  // the vector's last, partial group
      ring_run<kRun>(R, g, slot, lane);
      wave_sync();
      if constexpr (SEG)
        emit_split_seg<T, SAUX, NS, false>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane,
                                           secret_of(gi), seg);
      else
        emit_split<T, SAUX, NS, false>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, secret_of(gi));
    }
    asm volatile("" : : "v"(secA ^ secB));  // no load left in flight at the end
    if (a.tail_fin && sub + 1u == a.S) {
      wave_sync();
      last_sub_tail(R, g, slot, lane, p_start + ngroups * group, a);
    }
  }
}

// The fused draw + split with generation and emission on separate waves: a
// 128-thread workgroup per substream, wave 1 (producer) appends group i + 1
// to the LDS ring while wave 0 (consumer) emits group i (temper, split, the
// share stores), one workgroup barrier per group.  A group's words depend on
// the 624 words before it only (a group is 2176 words or more), so the
// producer writes the ring half the consumer emitted one step earlier while
// both read the other: the emission (at the share block's write rate) no
// longer waits for the generation, which in mt_gen_kernel's one wave per
// substream runs between two emissions (r04i: full 1.02 ms, emission alone
// 0.93, generation alone 0.50 at 2^24 3-of-5 on a share block).  Backward
// substreams the same way downwards.  Same output and final state as
// mt_gen_kernel<T> (T = 2, 3, 5; T = 0 the coefficient draw, whose consumer
// stores the tempered draws instead of splitting).
// Dynamic LDS as mt_gen_kernel; registers for 4 waves per SIMD (8 workgroups
// per CU, the most the rings' LDS allows at t <= 3), 2 at t = 5 (4 fit).
template <int T, int SAUX = kNt, int NS = 0, bool SEG = false>
__global__ void __launch_bounds__(128, T == 5 ? 2 : 4) mt_gen_pc_kernel(const GenArgs a) {
  static_assert(T == 0 || T >= 2, "coefficient draw or fused split");
  extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
  const uint32_t lane = threadIdx.x & 63u;
  // (roles alternating with the workgroup's parity: no faster, profiles/r04/l/)
  const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // 0 consumer, 1 producer
  const uint32_t sub = blockIdx.x + a.sub_lo;
  if (sub > a.S || (sub == a.S && a.final_sig < 0)) return;
  const bool fin_wave = sub == a.S;
  const bool fwd = fin_wave || mt_sub_forward(sub, a.S, static_cast<int>(a.back));
  const uint32_t sub_words = 17u * static_cast<uint32_t>(a.sub_draws);
  const uint32_t wsel = fin_wave ? static_cast<uint32_t>(a.final_sig) : fwd ? sub : sub + 1u;
  const uint32_t* win = a.wins + static_cast<uint64_t>(wsel) * kMtN;
  const uint32_t p_start = (sub == 0 && !fin_wave) ? kMtN - a.idx : fwd ? 0u : sub_words;
  GenRing g;
  g.M = a.ring;
  g.delta = (64u - (p_start & 63u)) & 63u;
  g.o = g.delta & 1u;
  uint32_t* R = s_ring;
  uint32_t slot = __builtin_amdgcn_readfirstlane((p_start + g.delta) % g.M);  // producer: slot of the next append
  if (fin_wave) {
    if (wid != 0u) return;  // one wave steps to CPython's final array (as mt_gen_kernel)
    ring_init(R, g, win, p_start, lane);
    wave_sync();
    final_state_wave(R, g, slot, lane, win, a);
    return;
  }
  const uint32_t group = a.ring / 2u;
  const uint64_t k0 = static_cast<uint64_t>(sub) * a.sub_draws;
  const uint32_t nloc = static_cast<uint32_t>(a.ncoef - k0 < a.sub_draws ? a.ncoef - k0 : a.sub_draws);
  constexpr uint32_t gdraws = T ? 64u * (T - 1) : 64u;
  const uint32_t ngroups = (nloc + gdraws - 1u) / gdraws;
  const uint64_t qb = k0 / static_cast<uint64_t>(a.tm1);
  const uint32_t rbm = static_cast<uint32_t>(k0 - qb * static_cast<uint64_t>(a.tm1));
  constexpr int kRun = 17 * (T ? T - 1 : 1);
  static_assert(kRun > 10, "a group holds the 640 words under the window");
  const bool prod = wid == 1u;
  [[maybe_unused]] uint32_t seg = 0u;  // SEG: the consumer's segment cursor (as mt_gen_kernel)
  if constexpr (SEG && T > 0) {
    const uint64_t efirst = uniform64(fwd ? qb : qb + 64u * (ngroups - 1u));
    if (!prod) seg = __builtin_amdgcn_readfirstlane(seg_find(seg_table(a), static_cast<uint32_t>(a.nseg), efirst));
  }
  // The two waves run separate loops with the same number of barriers (one
  // per step, ngroups + 1 steps), so the consumer's secrets stay in two
  // registers by group parity as in mt_gen_kernel: no copy of a pending load
  // (a copy waits vmcnt(0), i.e. for every share store in flight).
  if (!fwd) {
    // backward (whole groups, ngroups even; group gi in ring half gi % 2):
    // the producer fills the top group under the window, then per step
    // generates group gi - 1 while the consumer emits group gi
    const uint32_t M = a.ring;
    if (prod) {
      uint32_t top = M - 640u;
      ring_init(R, g, win, p_start, lane);
      wave_sync();
      back_blocks<1, true, true>(R, M, M - 576u, lane, M - 624u);
      back_run<kRun - 10>(R, M, top, lane);
      pc_barrier();
      for (uint32_t gi = ngroups - 1u; gi > 0u; --gi) {
        DN_PROBE_SKIP(a, 2u) back_run<kRun>(R, M, top, lane);
        pc_barrier();
      }
      pc_barrier();
      return;
    }
    if constexpr (T == 0) {
      pc_barrier();  // the top group is in the ring
      for (uint32_t gi = ngroups - 1u;; --gi) {
        DN_PROBE_SKIP(a, 1u) emit_group(a, R + (gi & 1u) * group, qb, rbm, 64u * gi + lane, nloc, lane);
        pc_barrier();
        if (gi == 0u) break;
      }
    } else {
    const uint64_t e0 = qb + lane;
    auto secret_of = [&](uint32_t gi) {
      return static_cast<uint64_t>(__builtin_nontemporal_load(a.secrets + e0 + 64u * gi));
    };
    auto bstep = [&](uint32_t gi, uint64_t cur, uint64_t& nxt) {
      nxt = secret_of(gi ? gi - 1u : 0u);
      DN_PROBE_SKIP(a, 1u)
      if constexpr (SEG)
        emit_split_seg<T, SAUX, NS, true>(a, R + (gi & 1u) * group, qb + 64u * gi, lane, cur, seg);
      else
        emit_split<T, SAUX, NS, true>(a, R + (gi & 1u) * group, qb + 64u * gi, lane, cur);
      pc_barrier();
    };
    uint64_t secA = secret_of(ngroups - 1u), secB = 0;
    pc_barrier();  // the top group is in the ring
    for (uint32_t gi = ngroups - 1u;; gi -= 2u) {
      bstep(gi, secA, secB);
      bstep(gi - 1u, secB, secA);
      if (gi == 1u) break;
    }
    asm volatile("" : : "v"(secA ^ secB));  // no load left in flight at the end
    }
    return;
  }
  // forward: step i generates group i (producer) and emits group i - 1 (consumer).
  // Substream 0 starting inside the caller's array (p_start > 0) is the one
  // place a run reaches past its group: run i ends with the first p_start
  // words of group i + 1, whose ring slots are group i - 1's, which the
  // consumer is emitting.  There each step has a second barrier: the consumer
  // passes it once group i - 1's words are in its registers, the producer
  // before the blocks from `kstar` on (the first one holding a word of group i
  // + 1).
  const bool mid = sub == 0u && p_start > 0u;
  const uint32_t kstar = mid ? (group - p_start) / 64u : static_cast<uint32_t>(kRun);
#ifdef DN_TUNING
  const bool skip_emit = (a.probe & 1u) != 0u, skip_gen = (a.probe & 2u) != 0u;
#else
  constexpr bool skip_emit = false, skip_gen = false;
#endif
  if (prod) {
    ring_init(R, g, win, p_start, lane);
    wave_sync();
    for (uint32_t i = 0; i < ngroups; ++i) {
      if (mid) {
        if (!skip_gen) ring_run_rt(R, g, slot, lane, kstar);
        pc_barrier();
        if (!skip_gen) ring_run_rt(R, g, slot, lane, static_cast<uint32_t>(kRun) - kstar);
      } else if (!skip_gen) {
        ring_run<kRun>(R, g, slot, lane);
      }
      pc_barrier();
    }
    if (mid) pc_barrier();
    pc_barrier();  // the consumer has read its last group: the ring is the producer's
    if (a.tail_fin && sub + 1u == a.S) last_sub_tail(R, g, slot, lane, p_start + ngroups * group, a);
    return;
  }
  if constexpr (T == 0) {
    if (mid) pc_barrier();
    pc_barrier();  // group 0 is in the ring
    for (uint32_t gi = 0; gi < ngroups; ++gi) {
      if (!skip_emit) emit_group(a, R + g.o + g.delta + (gi & 1u) * group, qb, rbm, 64u * gi + lane, nloc, lane, mid);
      else if (mid) pc_barrier();
      pc_barrier();
    }
  } else {
  const uint64_t e0 = qb + lane;
  const uint64_t elast = a.n_elem - 1u;
  auto secret_of = [&](uint32_t gi) {
    const uint64_t e = e0 + 64u * gi;
    return static_cast<uint64_t>(__builtin_nontemporal_load(a.secrets + (e < elast ? e : elast)));
  };
  const uint64_t rem = a.n_elem - qb;
  const uint32_t nfull = rem >= 64ull * ngroups ? ngroups : static_cast<uint32_t>(rem / 64u);
  auto cstep = [&](uint32_t gi, uint64_t cur, uint64_t& nxt) {
    nxt = secret_of(gi + 1u);
    if (!skip_emit) {
      if constexpr (SEG)
        emit_split_seg<T, SAUX, NS, true>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, cur, seg,
                                          mid);
      else
        emit_split<T, SAUX, NS, true>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, cur, mid);
    } else if (mid) {
      pc_barrier();
    }
    pc_barrier();
  };
  uint64_t secA = secret_of(0), secB = 0;
  if (mid) pc_barrier();
  pc_barrier();  // group 0 is in the ring
  uint32_t gi = 0;
  for (; gi + 1u < nfull; gi += 2u) {
    cstep(gi, secA, secB);
    cstep(gi + 1u, secB, secA);
  }
  if (gi < nfull) {
    cstep(gi, secA, secB);
    ++gi;
  }
  if (gi < ngroups) {  // the vector's last, partial group
    if constexpr (SEG)
      emit_split_seg<T, SAUX, NS, false>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, secret_of(gi),
                                         seg, mid);
    else
      emit_split<T, SAUX, NS, false>(a, R + g.o + g.delta + (gi & 1u) * group, qb + 64u * gi, lane, secret_of(gi),
                                     mid);
    pc_barrier();
  }
  asm volatile("" : : "v"(secA ^ secB));
  }
}

// Pinned staging buffers for a draw's small copies (from pageable memory HIP
// stages every copy through a buffer of its own and the host waits for it).
// A process-wide pool: a call leases one for its duration — every call
// synchronises its stream before it returns, so the buffer is idle again —
// and gives it back, so the pool holds as many buffers as calls ever ran at
// once, whatever number of threads made them.  The pool is never destroyed
// (the HIP runtime may be torn down before static destructors run).
struct PinPool {
  std::mutex m;
  std::vector<std::pair<uint32_t*, size_t>> idle;
};
PinPool& pin_pool() {
  static PinPool* pool = new PinPool;
  return *pool;
}

struct PinLease {
  uint32_t* p = nullptr;
  size_t words = 0;
  explicit PinLease(size_t need) {
    PinPool& pool = pin_pool();
    {
      std::lock_guard<std::mutex> g(pool.m);
      if (!pool.idle.empty()) {
        auto it = std::max_element(pool.idle.begin(), pool.idle.end(),
                                   [](const auto& a, const auto& b) { return a.second < b.second; });
        p = it->first;
        words = it->second;
        pool.idle.erase(it);
      }
    }
    if (words < need) {
      if (p) (void)hipHostFree(p);
      void* q = nullptr;
      p = hipHostMalloc(&q, need * 4, hipHostMallocDefault) == hipSuccess ? static_cast<uint32_t*>(q) : nullptr;
      words = p ? need : 0;
    }
  }
  ~PinLease() {
    if (!p) return;
    PinPool& pool = pin_pool();
    std::lock_guard<std::mutex> g(pool.m);
    pool.idle.push_back({p, words});
  }
  PinLease(const PinLease&) = delete;
  PinLease& operator=(const PinLease&) = delete;
};

// The levels' job tables on the device, one upload per (device, shape): they
// depend on (S, ki, back, parts) only, so a call copies just its own state
// (head, W_idx, row 0: ~7.8 KB — a blit, where the job tables of a large draw
// went by SDMA and the first jump waited ~11-14 us on its completion signal;
// profiles/r04/c/msv_timeline.json).  Library-owned, never freed (a few KB to
// ~100 KB per shape; the runtime may be torn down before static destructors).
struct DevJobs {
  int dev;
  uint64_t S;
  int ki, back, parts_b;
  bool rt, split2;
  void* p;
};

const void* device_jobs(const MtHost& H, int* err) {
  static std::mutex* m = new std::mutex;
  static auto* cache = new std::vector<DevJobs>;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    *err = 1;
    return nullptr;
  }
  std::lock_guard<std::mutex> g(*m);
  for (const DevJobs& d : *cache)
    if (d.dev == dev && d.S == H.S && d.ki == H.ki && d.back == H.back && d.parts_b == H.parts_b && d.rt == H.rt &&
        d.split2 == H.split2)
      return d.p;
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(H.jobs.size() * 4, 16);
  if (hipMalloc(&p, bytes) != hipSuccess ||
      (!H.jobs.empty() && hipMemcpy(p, H.jobs.data(), H.jobs.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
    if (p) (void)hipFree(p);
    *err = 1;
    return nullptr;
  }
  cache->push_back({dev, H.S, H.ki, H.back, H.parts_b, H.rt, H.split2, p});
  return p;
}

// The runtime direct rows on the device: one kMtRtRows-row buffer per device,
// rows copied when the host has computed rows the device copy lacks (rows are
// only ever added, never changed).  Library-owned, never freed (5.1 MB).
struct DevRt {
  int dev;
  uint64_t* p;
  uint64_t version, rows;
};

const uint64_t* device_rt(uint64_t S, int* err) {
  static std::mutex* m = new std::mutex;
  static auto* cache = new std::vector<DevRt>;
  uint64_t version = 0;
  const uint64_t* host = mt_direct_rows_l14(S, &version);
  int dev = 0;
  if (!host || hipGetDevice(&dev) != hipSuccess) {
    *err = 1;
    return nullptr;
  }
  std::lock_guard<std::mutex> g(*m);
  DevRt* d = nullptr;
  for (DevRt& c : *cache)
    if (c.dev == dev) d = &c;
  if (!d) {
    void* p = nullptr;
    if (hipMalloc(&p, kMtRtRows * kMtPolyWords * sizeof(uint64_t)) != hipSuccess) {
      *err = 1;
      return nullptr;
    }
    cache->push_back({dev, static_cast<uint64_t*>(p), 0, 0});
    d = &cache->back();
  }
  const uint64_t need = S - 1;
  if (d->version != version || d->rows < need) {
    const uint64_t n = std::max(d->rows, need);
    if (hipMemcpy(d->p, host, n * kMtPolyWords * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
      *err = 1;
      return nullptr;
    }
    d->version = version;
    d->rows = n;
  }
  return d->p;
}

// split2's side stream and its two events, per thread and device (created
// once, never destroyed: the runtime may be torn down first).
struct SideStream {
  int dev = -1;
  hipStream_t s = nullptr;
  hipEvent_t levels = nullptr, gen = nullptr;
};
SideStream* side_stream() {
  thread_local SideStream side[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  SideStream& x = side[dev];
  if (!x.s) {
    if (hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) != hipSuccess) return x.s = nullptr, nullptr;
    if (hipEventCreateWithFlags(&x.levels, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.gen, hipEventDisableTiming) != hipSuccess)
      return nullptr;
    x.dev = dev;
  }
  return &x;
}

// Every knob of a run, with the product's values as the defaults: the
// product build reads no environment variable (tune_env), the tuning build
// reads each DN_MT_* variable of that name once per call, here.  (The
// planner's own knobs — DN_MT_BACK, _RT, _SPLIT2, _PARTS_B — are mt_plan.hpp's.)
struct MtKnobs {
  // a call speculates on its successor (SpecState, below; DN_MT_SPEC=0 off)
  bool spec = true;
  // The final state by the last substream (last_sub_tail) rather than a
  // final-state wave (DN_MT_TAIL_FIN=0): that wave stepped the whole last
  // substream again, one wave alone, and finished ~100 us after the other
  // substreams at 2^24 (profiles/r06/g/timeline_spec.json: substreams
  // 0.88-0.91 ms, the wave 0.93-1.09 ms).
  bool tail_fin = true;
  // the speculated levels of a runtime-direct-level draw (2^24 scale) beside
  // the generation rather than after it (DN_MT_SPEC_BESIDE=0 off), by
  // mt_jumpc_kernel<4, beside_cb> (DN_MT_BESIDE_CB, 2 or 3)
  bool spec_beside = true;
  int beside_cb = 2;
  // draws of fewer coefficients than spec_min do not speculate after the
  // generation (DN_MT_SPEC_MIN), nor beside it below beside_min
  // (DN_MT_BESIDE_MIN: the levels of a small generation beside it, round 6)
  uint64_t spec_min = 1ull << 23, beside_min = 1ull << 16;
  // DN_MT_SPEC_PROBE=5: the call's own runtime direct level by
  // mt_jumpc_kernel<4, beside_cb> (its time alone, and the kernel's test); no
  // speculation.  (Values 1-4 were timing probes with wrong output, retired.)
  bool own_by_jumpc = false;
  uint32_t jump_probe = 0;  // DN_MT_JUMP_PROBE (JumpArgs::probe)
  bool jump4b = false;      // DN_MT_JUMP4B=1: 16-wave levels by mt_jumpc_kernel<16, 4>
  uint32_t gen_probe = 0;   // DN_MT_PROBE (GenArgs::probe)
  bool pc = true;           // DN_MT_PC_FORCE=0: the one-wave generation kernel (A/B)
  // DN_MT_GEN_SUBS (timing probe only: the output is partial and CPython's
  // final state is not computed): launch only the first K substream
  // workgroups — how the generation's time scales with the substreams in flight
  uint32_t gen_subs = 0;
  // DN_MT_FORCE_RETRY=1 takes the rejected-draw exit so the caller's host
  // fallback can be exercised
  bool force_retry = false;
};

MtKnobs mt_knobs() {
  MtKnobs k;
  auto on = [](const char* n, bool dflt) { const char* e = tune_env(n); return e ? e[0] != '0' : dflt; };
  auto is1 = [](const char* n) { const char* e = tune_env(n); return e && e[0] == '1'; };
  auto num = [](const char* n) { const char* e = tune_env(n); return e ? std::atoi(e) : 0; };
  k.spec = on("DN_MT_SPEC", k.spec);
  k.tail_fin = on("DN_MT_TAIL_FIN", k.tail_fin);
  k.spec_beside = on("DN_MT_SPEC_BESIDE", k.spec_beside);
  if (const char* e = tune_env("DN_MT_BESIDE_CB")) k.beside_cb = e[0] == '2' ? 2 : 3;
  if (const char* e = tune_env("DN_MT_SPEC_MIN")) k.spec_min = std::strtoull(e, nullptr, 10);
  if (const char* e = tune_env("DN_MT_BESIDE_MIN")) k.beside_min = std::strtoull(e, nullptr, 10);
  k.own_by_jumpc = num("DN_MT_SPEC_PROBE") == 5;
  k.jump_probe = static_cast<uint32_t>(num("DN_MT_JUMP_PROBE"));
  k.jump4b = is1("DN_MT_JUMP4B");
  k.gen_probe = static_cast<uint32_t>(num("DN_MT_PROBE"));
  k.pc = on("DN_MT_PC_FORCE", k.pc);
  if (tune_env("DN_MT_GEN_SUBS")) k.gen_subs = static_cast<uint32_t>(std::max(1, num("DN_MT_GEN_SUBS")));
  k.force_retry = is1("DN_MT_FORCE_RETRY");
  return k;
}

// Speculation (MtKnobs::spec): a call speculates
// that the next draw on this device has the same size and starts where this
// one ends — the loop `for x in batch: make_shares_vec(x)` — and computes the
// next call's windows while its own host side finishes: the generation's last
// substream also writes the next call's W_idx (the window at stream position
// idx + 17 ncoef) into a buffer of the device's speculation state, then the
// shape's jump levels from it run on a side stream into that buffer.  The
// next call uses the buffer in place of its jump levels when its draw size,
// CPython index and 624-word array equal the ones this call left (anything
// else — another size, random.Random touched in between, a rejected draw —
// is a miss: the call jumps itself).  A call speculates only when it
// continues the previous call (same size, starting where that one ended), so
// a lone call, or equal calls on fresh random.Random states, launch nothing
// extra.  Two buffers alternate (one the generation reads, one the side
// stream fills); the side stream's work is always awaited by the call stream
// before a buffer is reused.  One state per device, process-wide; a call that
// finds it busy (another thread's call) neither speculates nor hits.
struct SpecState {
  std::mutex m;
  hipStream_t side = nullptr, side2 = nullptr;
  hipEvent_t win = nullptr, done = nullptr;  // this call's windows in place (call stream), the side streams done
  hipEvent_t j0ev = nullptr, done2 = nullptr;
  bool widx2 = false;  // beside: buf[next ^ 1]'s row -1 holds the W_idx of the call after the armed one
  void* buf[2] = {nullptr, nullptr};
  uint64_t bytes = 0;  // of each buffer
  bool armed = false;  // buf[next] holds (at `done`) the windows of a call starting as below
  int next = 0;
  uint64_t ncoef = 0;
  int32_t idx = -1;
  uint32_t state[kMtN];
  bool have_end = false;  // ncoef, idx, state: where the previous call ended
  uint64_t hits = 0, misses = 0, launched = 0;
  uint64_t* xpow = nullptr;  // device: x^xpow_words mod P (the next call's W_idx from this one's)
  uint64_t xpow_words = 0;
  bool xpow_failed = false;  // no carry-less multiply here, or the upload failed: no beside levels
};

std::mutex& spec_table_mutex() {
  static std::mutex* m = new std::mutex;
  return *m;
}
SpecState* spec_slot(int dev) {  // created once per device, never destroyed (the runtime may go first)
  static SpecState* table[16] = {};
  if (dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> g(spec_table_mutex());
  if (!table[dev]) {
    auto* x = new SpecState;
    if (hipStreamCreateWithFlags(&x->side, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&x->side2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x->j0ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x->done2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x->win, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x->done, hipEventDisableTiming) != hipSuccess)
      return nullptr;  // (leaks the half-made state: a runtime that cannot make a stream has bigger problems)
    table[dev] = x;
  }
  return table[dev];
}

// x^words mod P on the device for the beside chain's first jump (computed on
// the host once per draw size: ~30 Barrett products, a few ms)
bool spec_xpow(SpecState& sp, uint64_t words) {
  if (sp.xpow_failed) return false;
  if (sp.xpow && sp.xpow_words == words) return true;
  std::vector<uint64_t> g(kMtPolyWords);
  if (!mt_xpow_mod(words, g.data()) ||
      (!sp.xpow && hipMalloc(reinterpret_cast<void**>(&sp.xpow), kMtPolyWords * sizeof(uint64_t)) != hipSuccess)) {
    sp.xpow_failed = true;
    return false;
  }
  (void)hipStreamSynchronize(sp.side);  // the previous size's polynomial may still be read
  (void)hipStreamSynchronize(sp.side2);
  if (hipMemcpy(sp.xpow, g.data(), kMtPolyWords * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
    sp.xpow_failed = true;
    return false;
  }
  sp.xpow_words = words;
  return true;
}

// both buffers at least `need` bytes (false: allocation failed; no speculation)
bool spec_buffers(SpecState& sp, uint64_t need) {
  if (sp.bytes >= need && sp.buf[0] && sp.buf[1]) return true;
  (void)hipStreamSynchronize(sp.side);  // nothing of ours uses them once the side streams are idle
  (void)hipStreamSynchronize(sp.side2);
  sp.armed = false;
  sp.widx2 = false;
  for (void*& b : sp.buf)
    if (b) (void)hipFree(b), b = nullptr;
  sp.bytes = 0;
  for (void*& b : sp.buf)
    if (hipMalloc(&b, need) != hipSuccess) {
      for (void*& c : sp.buf)
        if (c) (void)hipFree(c), c = nullptr;
      return false;
    }
  sp.bytes = need;
  return true;
}

constexpr uint64_t kCus = 256, kLdsPerCu = 160 * 1024;  // MI355X: CUs, LDS bytes per CU

// What a call decides about speculation: whether its own windows were
// speculated by the previous call, and whether and how it speculates on the
// next one.
struct SpecPlan {
  bool hit = false;        // this call's windows are in place, in sp->buf[sp->next]
  bool spec_next = false;  // the next call's windows go to sp->buf[dst] ...
  bool beside = false;     // ... beside this call's generation rather than after it
  bool widx2 = false;      // beside: the previous call left the next call's W_idx in place
  int dst = 0;
};

// sp: the device's speculation state, held by this call (null: none).
// beside (runtime direct level): the next call's W_idx by one jump from this
// call's, then its level, both by mt_jumpc_kernel<4, 2> on the side stream
// beside this call's generation.  Other shapes: the levels as they are
// (mt_jump_kernel, 83 KB workgroups) when the generation's rings leave a CU
// that much LDS (a generation of at most ~1000 3-of-5 substreams: 2^22
// coefficients and less), and when the generation outlasts them: substreams
// of 2^12 draws, or of 2^10 and at most 256 of them (loops of 2^20 / 2^16
// elements -15 / -10 %; 512 substreams of 2^10 draws, 2^18 elements, +2.5 %:
// profiles/r06/y/).
SpecPlan spec_decide(SpecState* sp, const MtKnobs& k, const MtHost& H, uint64_t ncoef, int ring_units, int32_t idx,
                     const uint32_t* mt_state) {
  SpecPlan p;
  if (!sp) return p;
  // this call continues the previous one (same size, starting where it
  // ended): a hit if that call speculated, and a reason to speculate again
  const bool cont = sp->have_end && sp->ncoef == ncoef && sp->idx == idx && !std::memcmp(sp->state, mt_state, kMtN * 4);
  p.hit = cont && sp->armed;
  if (sp->armed && !p.hit) ++sp->misses;
  p.widx2 = p.hit && sp->widx2;
  sp->armed = false;
  sp->widx2 = false;
  sp->have_end = false;
  p.spec_next = cont && spec_buffers(*sp, mt_scratch_bytes(ncoef));
  const uint64_t gen_lds = (1u + 2u * 17u * 64u * static_cast<uint32_t>(ring_units) + 64u) * 4u;
  const bool levels_fit = (H.S + kCus - 1) / kCus * gen_lds + (kEWords + kMtN + 64) * 4u <= kLdsPerCu;
  p.beside = p.spec_next && k.spec_beside && ncoef >= k.beside_min &&
             (H.rt ? !H.beside.jobs.empty() : levels_fit && (mt_sub_draws(H.ki) >= 4096 || H.S <= 256)) &&
             !H.j0.jobs.empty() && spec_xpow(*sp, 17 * ncoef);
  if (!p.beside && ncoef < k.spec_min) p.spec_next = false;  // (no speculation after the generation this small)
  p.dst = sp->next ^ 1;
  return p;
}

// Where the call ended; the next call, if it starts here, uses the
// speculated windows (spec_next) or speculates itself.
void spec_record_end(SpecState& sp, const SpecPlan& p, uint64_t ncoef, int32_t fidx, const uint32_t* mt_state) {
  sp.have_end = true;
  sp.ncoef = ncoef;
  sp.idx = fidx;
  std::memcpy(sp.state, mt_state, kMtN * 4);
  sp.armed = p.spec_next;
  sp.widx2 = p.beside;  // this call's buffer now holds the W_idx after the next call's
  if (p.spec_next) sp.next = p.dst;
}

// What the launches of one call share.
struct MtCall {
  const MtKnobs& k;
  const MtHost& H;  // the shape's levels (H.S substreams of length H.ki)
  hipStream_t s;    // the caller's stream
  // the buffer the generation reads its windows from (the caller's scratch or
  // a speculation buffer): head | W_idx (row -1) | rows 0..S | part rows
  uint8_t* sc;
  uint32_t* dwin;          // its row 0
  const void* jobs_dev;    // the shape's job tables on the device (MtHost::jobs)
  const uint64_t* rt_dev;  // the runtime direct rows on the device (H.rt)
  SpecState* sp;           // held by this call, or null
  SideStream* side;        // split2
};

// The shape's jump levels into the windows `wins` (row 0) on stream ls;
// after0: recorded once level 0 is complete.
hipError_t launch_levels(const MtCall& c, hipStream_t ls, uint32_t* wins, hipEvent_t after0 = nullptr) {
  const Level* lv = c.H.lv;
  const JumpJob* djobs = static_cast<const JumpJob*>(c.jobs_dev);
  const CombineJob* dcomb =
      reinterpret_cast<const CombineJob*>(djobs + lv[0].jobs.size() + lv[1].jobs.size() + lv[2].jobs.size());
  hipError_t err = hipSuccess;
  uint64_t off = 0, coff = 0;
  for (int k = 0; k < 3; ++k) {
    const Level& l = lv[k];
    if (!l.jobs.empty()) {
      const JumpArgs ja{wins, djobs + off, static_cast<uint32_t>(l.jobs.size()), c.k.jump_probe, c.rt_dev};
      const dim3 grid(static_cast<uint32_t>(l.jobs.size() / static_cast<size_t>(l.W)));
      if (l.W == 16 && c.k.jump4b) hipLaunchKernelGGL((mt_jumpc_kernel<16, 4>), grid, dim3(64 * 16), 0, ls, ja);
      else if (l.W == 16) hipLaunchKernelGGL(mt_jump_kernel<16>, grid, dim3(64 * 16), 0, ls, ja);
      else hipLaunchKernelGGL(mt_jump_kernel<8>, grid, dim3(64 * 8), 0, ls, ja);
    }
    if (!l.comb.empty())
      hipLaunchKernelGGL(mt_combine_kernel, dim3(static_cast<uint32_t>(l.comb.size())), dim3(640), 0, ls, wins,
                         dcomb + coff);
    off += l.jobs.size();
    coff += l.comb.size();
    if (after0 && k == 0) err = hipEventRecord(after0, ls);
  }
  return err;
}

// The runtime direct level by mt_jumpc_kernel<4, 2> (H.beside: whole jumps).
void launch_beside_level(const MtCall& c, hipStream_t ls, uint32_t* wins) {
  const Level& l = c.H.beside;
  if (l.jobs.empty()) return;
  const JumpJob* bj = reinterpret_cast<const JumpJob*>(static_cast<const uint32_t*>(c.jobs_dev) + c.H.beside_off);
  const JumpArgs ja{wins, bj, static_cast<uint32_t>(l.jobs.size()), 0u, c.rt_dev};
  launch_jumpc4(dim3(static_cast<uint32_t>(l.jobs.size() / 4)), ls, ja, c.k.beside_cb);
}

// Row S -> row -1 of the windows w by x^(17 ncoef) (H.j0: parts, then their combine).
void jump0(const MtCall& c, hipStream_t ls, uint32_t* w) {
  const uint32_t* hj = static_cast<const uint32_t*>(c.jobs_dev);
  const JumpArgs j0{w, reinterpret_cast<const JumpJob*>(hj + c.H.j0_off), static_cast<uint32_t>(c.H.j0.jobs.size()), 0u,
                    c.sp->xpow};
  launch_jumpc4(dim3(static_cast<uint32_t>(c.H.j0.jobs.size() / 4)), ls, j0, c.k.beside_cb);
  hipLaunchKernelGGL(mt_combine_kernel, dim3(static_cast<uint32_t>(c.H.j0.comb.size())), dim3(640), 0, ls, w,
                     reinterpret_cast<const CombineJob*>(hj + c.H.j0_comb_off));
}

// The four ways a call launches its generation (`gen(ga, stream)`, after its
// own levels).  err: the call's first error so far; a path goes on launching
// after an error (the caller drains the streams) but makes no further event
// or copy call, and returns the first error.
struct MtLaunched {
  hipError_t err;
  bool side_used;  // work of this call is on the speculation side streams
};

// split2: substreams [0, S/2) on the side stream once level 0 is done (beside
// level 1's jumps), then [S/2, S] and the final-state wave on the call's
// stream after level 1; the call's stream then waits for the side stream.
template <typename G>
MtLaunched run_split2(const MtCall& c, GenArgs& ga, G gen, hipError_t err) {
  const uint32_t half = static_cast<uint32_t>(mt_split_half(c.H.S)), nwg = ga.sub_n;
  if (err == hipSuccess) err = hipStreamWaitEvent(c.side->s, c.side->levels, 0);
  GenArgs g1 = ga;
  g1.sub_lo = 0u;
  g1.sub_n = half;
  gen(g1, c.side->s);
  if (err == hipSuccess) err = hipEventRecord(c.side->gen, c.side->s);
  ga.sub_lo = half;
  ga.sub_n = nwg - half;
  gen(ga, c.s);
  if (err == hipSuccess) err = hipStreamWaitEvent(c.s, c.side->gen, 0);
  return {err, false};
}

// Speculation beside the generation.  Once this call's windows are in place,
// in workgroups of 11 KB that fit on a CU beside the generation's rings: on
// the side stream the next call's level into the other buffer from its W_idx
// (row -1 there) — which the previous call computed (widx2) or, first, one
// jump by x^(17 ncoef) from this call's W_idx computes (copied to row S, 32
// parts + combine); on the second side stream the W_idx of the call after
// that, jumped from the next call's into this call's buffer (rows S, part rows
// and -1: none of them read by this call's generation).
template <typename G>
MtLaunched run_beside(const MtCall& c, const SpecPlan& p, GenArgs& ga, G gen) {
  SpecState* sp = c.sp;
  const uint64_t S = c.H.S;
  uint8_t* nb = static_cast<uint8_t*>(sp->buf[p.dst]);
  uint32_t* nw = reinterpret_cast<uint32_t*>(nb + kHead) + kMtN;  // the next call's row 0
  hipError_t err = hipEventRecord(sp->win, c.s);
  gen(ga, c.s);
  if (err == hipSuccess) err = hipStreamWaitEvent(sp->side, sp->win, 0);
  if (err == hipSuccess) err = hipStreamWaitEvent(sp->side2, sp->win, 0);
  if (!p.widx2) {
    if (err == hipSuccess)
      err = hipMemcpyAsync(nw + S * kMtN, c.dwin - kMtN, kMtN * 4, hipMemcpyDeviceToDevice, sp->side);
    jump0(c, sp->side, nw);
    if (err == hipSuccess) err = hipEventRecord(sp->j0ev, sp->side);
    if (err == hipSuccess) err = hipStreamWaitEvent(sp->side2, sp->j0ev, 0);
  }
  if (c.H.rt) launch_beside_level(c, sp->side, nw);
  else (void)launch_levels(c, sp->side, nw);
  if (err == hipSuccess) err = hipEventRecord(sp->done, sp->side);
  if (err == hipSuccess)
    err = hipMemcpyAsync(c.dwin + S * kMtN, nw - kMtN, kMtN * 4, hipMemcpyDeviceToDevice, sp->side2);
  jump0(c, sp->side2, c.dwin);
  if (err == hipSuccess) err = hipEventRecord(sp->done2, sp->side2);
  ++sp->launched;
  return {err, true};
}

// Speculation after the generation, whose last substream also writes the
// next call's W_idx into row -1 of the other buffer; then on the side stream
// the next call's jump levels from it, while this call's host side finishes
// and the next call's begins.
template <typename G>
MtLaunched run_spec_after(const MtCall& c, const SpecPlan& p, GenArgs& ga, G gen) {
  SpecState* sp = c.sp;
  uint8_t* nb = static_cast<uint8_t*>(sp->buf[p.dst]);
  ga.next_win = reinterpret_cast<uint32_t*>(nb + kHead);
  gen(ga, c.s);
  hipError_t err = hipEventRecord(sp->win, c.s);
  if (err == hipSuccess) err = hipStreamWaitEvent(sp->side, sp->win, 0);
  (void)launch_levels(c, sp->side, reinterpret_cast<uint32_t*>(nb + kHead) + kMtN);
  if (err == hipSuccess) err = hipEventRecord(sp->done, sp->side);
  ++sp->launched;
  return {err, true};
}

template <typename G>
MtLaunched run_plain(const MtCall& c, GenArgs& ga, G gen, hipError_t err) {
  gen(ga, c.s);
  return {err, false};
}

// The generation's arguments but for what the caller's launch_gen adds;
// head: the flag (word 0) and the final array (from word 64) as the device sees them.
GenArgs gen_args(const MtCall& c, const MtFinal& fin, bool tail_fin, int32_t idx, uint64_t n_elem, int tm1,
                 uint32_t* head) {
  GenArgs ga{};
  ga.wins = c.dwin;
  ga.flag = head;
  ga.fin = head + 64;
  ga.ncoef = n_elem * static_cast<uint64_t>(tm1);
  ga.sub_draws = mt_sub_draws(c.H.ki);
  ga.vb = dn_m521_vec_bytes(n_elem);
  ga.tm1_magic = ((1ull << 32) + static_cast<uint64_t>(tm1) - 1) / static_cast<uint64_t>(tm1);
  ga.S = static_cast<uint32_t>(c.H.S);
  ga.idx = static_cast<uint32_t>(idx);
  ga.tm1 = tm1;
  ga.final_sig = fin.sig;
  ga.final_pos = fin.pos;
  ga.final_tf = fin.tf;
  ga.n_elem = n_elem;
  ga.back = static_cast<uint32_t>(c.H.back);
  ga.probe = c.k.gen_probe;
  if (tail_fin) ga.tail_fin = 1u, ga.fin_lo = fin.fin_lo, ga.next_lo = fin.next_lo;
  ga.sub_n = ga.S + (tail_fin ? 0u : 1u);  // + the final-state wave
  return ga;
}

// The device's speculation state, held for the call through `hold` (null:
// none, or another thread's call holds it).
SpecState* spec_try_hold(std::unique_lock<std::mutex>& hold) {
  int dev = 0;
  SpecState* sp = hipGetDevice(&dev) == hipSuccess ? spec_slot(dev) : nullptr;
  if (sp) hold = std::unique_lock<std::mutex>(sp->m, std::try_to_lock);
  return sp && hold.owns_lock() ? sp : nullptr;
}

// The device draw of n_elem * tm1 coefficients from CPython state
// (mt_state, *mt_index): the plan (mt_plan.hpp), the call's state to the
// device, its jump levels unless the previous call speculated them, then
// `launch_gen(ga, stream, knobs)` (the generation kernel: coefficients or
// fused split) by one of the four paths above, then CPython's final state.
template <typename F>
int mt_device_run(const char* name, uint32_t* mt_state, int32_t* mt_index, uint64_t n_elem, int tm1, void* scratch,
                  uint64_t scratch_bytes, void* stream, int ring_units, F launch_gen) {
  if (!mt_state || !mt_index) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (tm1 < 0 || tm1 >= DN_MAX_THRESHOLD) return set_error(DN_ERR_ARG, "%s: t-1=%d", name, tm1);
  const int32_t idx = *mt_index;
  if (idx < 0 || idx > kMtN) return set_error(DN_ERR_ARG, "%s: bad MT index", name);
  const uint64_t ncoef = n_elem * static_cast<uint64_t>(tm1);
  if (ncoef == 0) return DN_OK;
  if (!scratch) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  const uint64_t S = mt_subs(ncoef);
  if (S > mt_jump_max_subs() - 1)
    return set_error(DN_ERR_UNSUPPORTED, "%s: %llu words exceed the jump table", name,
                     static_cast<unsigned long long>(17 * ncoef));
  if (scratch_bytes < mt_scratch_bytes(ncoef)) return set_error(DN_ERR_ARG, "%s: scratch too small", name);

  const MtKnobs k = mt_knobs();
  const int ki = mt_sub_len(ncoef);
  const MtFinal fin = mt_final_plan(idx, ncoef, S, ki);
  const bool tail_fin = fin.sig >= 0 && k.tail_fin;
  MtHost& H = mt_levels(S, ki);
  // The job tables are the device copy of this shape's (device_jobs).  What
  // the GPU needs from the host is the scratch prefix head .. row 0: ONE copy
  // from the pinned staging buffer, which holds that prefix and, in its tail,
  // the head the generation writes (flag, final array).
  int jerr = 0;
  const void* jobs_dev = device_jobs(H, &jerr);
  if (jerr) return set_error(DN_ERR_HIP, "%s: job tables on the device", name);
  const uint64_t* rt_dev = H.rt ? device_rt(S, &jerr) : nullptr;
  if (jerr) return set_error(DN_ERR_HIP, "%s: runtime jump rows on the device", name);
  const size_t wpre = kHead / 4 + 2 * kMtN, wh = 256 / 4 + kMtN;
  PinLease lease(wpre + wh);  // idle again once this call has synchronised its stream
  uint32_t* pin = lease.p;
  if (!pin) return set_error(DN_ERR_HIP, "%s: pinned staging buffer", name);
  uint32_t *stw = pin + kHead / 4, *head = pin + wpre;
  std::memset(pin, 0, 256);  // the flag (the final array is written by the device)
  mt_advance_window(mt_state, static_cast<uint64_t>(idx), stw);  // W_idx
  std::memcpy(stw + kMtN, mt_state, kMtN * 4);                    // row 0
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the speculation state: this call's draw may have been speculated (hit),
  // and it may speculate on the next one (spec_next)
  const bool spec_on = k.spec && !k.own_by_jumpc && !H.split2 && tail_fin && S >= 2 &&  // (S >= 2: there are levels)
                       ncoef >= std::min(k.spec_min, k.beside_min);
  std::unique_lock<std::mutex> spl;
  SpecState* sp = spec_on ? spec_try_hold(spl) : nullptr;
  const SpecPlan p = spec_decide(sp, k, H, ncoef, ring_units, idx, mt_state);
  // a hit generates from its speculated buffer; a beside call runs in the
  // other library buffer too (the side stream reads its W_idx from there)
  uint8_t* sc = p.hit || p.beside ? static_cast<uint8_t*>(sp->buf[sp->next]) : static_cast<uint8_t*>(scratch);
  // the side stream's last work (the speculated levels) is done before this
  // call writes a speculation buffer or reads one (a wait on the device only
  // if it is still running)
  hipError_t err = (p.spec_next || p.hit) && hipEventQuery(sp->done) != hipSuccess ? hipStreamWaitEvent(s, sp->done, 0)
                                                                                   : hipSuccess;
  if (err == hipSuccess && (p.spec_next || p.hit) && hipEventQuery(sp->done2) != hipSuccess)
    err = hipStreamWaitEvent(s, sp->done2, 0);
  if (err == hipSuccess) err = hipMemcpyAsync(sc, pin, wpre * 4, hipMemcpyHostToDevice, s);
  if (err != hipSuccess) {
    (void)hipStreamSynchronize(s);  // the staging buffer is reused by the next call
    return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  }
  SideStream* side = H.split2 ? side_stream() : nullptr;
  if (H.split2 && !side) {
    (void)hipStreamSynchronize(s);
    return set_error(DN_ERR_HIP, "%s: side stream", name);
  }
  const MtCall c{k, H, s, sc, reinterpret_cast<uint32_t*>(sc + kHead) + kMtN, jobs_dev, rt_dev, sp, side};
  if (k.own_by_jumpc) launch_beside_level(c, s, c.dwin);
  else if (!p.hit) err = launch_levels(c, s, c.dwin, H.split2 ? side->levels : nullptr);  // (a hit's windows are in place)

  // The generation writes the flag and CPython's final array straight into
  // the staging buffer's tail (mapped host memory, visible once the stream has
  // synchronised): no read-back copy (make_shares_vec 2^12 -1.5 us, profiles/r04/e/)
  head[0] = 0u;
  void* dhead = nullptr;
  if (hipHostGetDevicePointer(&dhead, head, 0) != hipSuccess || !dhead) {
    (void)hipStreamSynchronize(s);
    return set_error(DN_ERR_HIP, "%s: staging buffer not mapped", name);
  }
  GenArgs ga = gen_args(c, fin, tail_fin, idx, n_elem, tm1, static_cast<uint32_t*>(dhead));
  auto gen = [&](GenArgs& g, hipStream_t gs) { launch_gen(g, gs, k); };
  const MtLaunched r = H.split2      ? run_split2(c, ga, gen, err)
                       : p.beside    ? run_beside(c, p, ga, gen)
                       : p.spec_next ? run_spec_after(c, p, ga, gen)
                                     : run_plain(c, ga, gen, err);
  err = r.err;
  // an early exit waits for this call's side work too (it writes the staging buffer)
  auto drain_side = [&]() {
    if (r.side_used) (void)hipStreamSynchronize(sp->side), (void)hipStreamSynchronize(sp->side2);
  };
  if (err != hipSuccess) {
    (void)hipStreamSynchronize(s);
    drain_side();
    return set_error(DN_ERR_HIP, "%s: side stream: %s", name, hipGetErrorString(err));
  }
  err = hipGetLastError();
  if (err != hipSuccess) {
    (void)hipStreamSynchronize(s);
    drain_side();
    return set_error(DN_ERR_HIP, "%s: launch: %s", name, hipGetErrorString(err));
  }
  err = hipStreamSynchronize(s);
  if (err != hipSuccess) {
    drain_side();
    return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  }
  if (p.hit) ++sp->hits;
  if (head[0] || k.force_retry) return set_error(DN_ERR_RETRY, "%s: a draw was rejected; redo on the host", name);
  if (fin.sig >= 0) std::memcpy(mt_state, head + 256 / 4, kMtN * 4);
  *mt_index = fin.fidx;
  if (sp) spec_record_end(*sp, p, ncoef, fin.fidx, mt_state);
  return DN_OK;
}

// buffer-store cache policy of the 3-of-5 share stores: sc1 (16) rather than
// non-temporal: 2.2 % faster on two buffers of one process
// (profiles/r03/ab/mt_store_aux_ns5.json)
constexpr int kSc1 = 16;

// The generation kernel of a call.  The headline 3-of-5: straight-line share
// stores (see mt_gen_kernel).  Generation and emission on two waves per
// substream (mt_gen_pc_kernel): at 2^24 the kernel runs at its emission-only
// time (0.92 vs 1.01 ms for the one-wave kernel on a share block,
// profiles/r04/t/), at 2^20 / 2^16 / 2^12 make_shares_vec -12 / -8 / -3 %
// (profiles/r04/l/); the one-wave kernel (mt_gen_kernel) is the tuning
// build's A/B (MtKnobs::pc).
// SEG: the segmented emission (ga.segs; dn_mt19937_split_many_device)
template <int T, bool SEG = false>
void launch_gen(GenArgs& ga, hipStream_t s, const MtKnobs& k) {
  ga.ring = 2u * 17u * 64u * (T ? T - 1 : 1);
  const uint32_t lds_words = 1u + ga.ring + 64u;  // GenRing: alignment word, ring, mirror
  uint32_t grid = ga.sub_n ? ga.sub_n : ga.S + 1;
  if (k.pc) {
    if (k.gen_subs) grid = std::min(grid, k.gen_subs);
    if (T == 3 && ga.n_shares == 5)
      hipLaunchKernelGGL((mt_gen_pc_kernel<T, kSc1, T == 3 ? 5 : 0, SEG>), dim3(grid), dim3(128), lds_words * 4u, s, ga);
    else
      hipLaunchKernelGGL((mt_gen_pc_kernel<T, kNt, 0, SEG>), dim3(grid), dim3(128), lds_words * 4u, s, ga);
  } else if (T == 3 && ga.n_shares == 5) {
    hipLaunchKernelGGL((mt_gen_kernel<T, kSc1, T == 3 ? 5 : 0, SEG>), dim3(grid), dim3(64), lds_words * 4u, s, ga);
  } else {
    hipLaunchKernelGGL((mt_gen_kernel<T, kNt, 0, SEG>), dim3(grid), dim3(64), lds_words * 4u, s, ga);
  }
}

}  // namespace
}  // namespace dn

using namespace dn;

extern "C" uint64_t dn_mt19937_device_scratch_bytes(uint64_t n_elem, int tm1) {
  return mt_scratch_bytes(tm1 > 0 ? n_elem * static_cast<uint64_t>(tm1) : 0);
}

extern "C" int dn_mt19937_draw_coeffs_device(uint32_t* mt_state, int32_t* mt_index, uint64_t n_elem, int tm1,
                                             void* coeffs, void* scratch, uint64_t scratch_bytes, void* stream) {
  if (n_elem && tm1 > 0 && !coeffs) return set_error(DN_ERR_ARG, "dn_mt19937_draw_coeffs_device: null pointer");
  return mt_device_run("dn_mt19937_draw_coeffs_device", mt_state, mt_index, n_elem, tm1, scratch, scratch_bytes, stream, 1,
                       [&](GenArgs& ga, hipStream_t s, const MtKnobs& k) {
                         ga.coeffs = static_cast<uint8_t*>(coeffs);
                         launch_gen<0>(ga, s, k);
                       });
}

extern "C" int dn_mt19937_split_supported(uint64_t n_elem, int threshold, int n_shares) {
  if (!(threshold == 2 || threshold == 3 || threshold == 5) || threshold > n_shares || n_shares > DN_MAX_SHARES ||
      fd_needs_fold(threshold, n_shares))
    return 0;
  const uint64_t ncoef = n_elem * static_cast<uint64_t>(threshold - 1);
  return !ncoef || mt_subs(ncoef) <= mt_jump_max_subs() - 1;
}

extern "C" int dn_mt19937_split_device(uint32_t* mt_state, int32_t* mt_index, const int64_t* secrets, void* shares,
                                       uint64_t n_elem, int threshold, int n_shares, void* scratch,
                                       uint64_t scratch_bytes, void* stream) {
  const char* name = "dn_mt19937_split_device";
  if (threshold < 1 || threshold > DN_MAX_THRESHOLD)
    return set_error(DN_ERR_UNSUPPORTED, "%s: threshold %d outside 1..%d", name, threshold, DN_MAX_THRESHOLD);
  if (threshold > n_shares) return set_error(DN_ERR_THRESHOLD, "threshold should be little equal than shares");
  if (!(threshold == 2 || threshold == 3 || threshold == 5) || fd_needs_fold(threshold, n_shares) ||
      n_shares > DN_MAX_SHARES)
    return set_error(DN_ERR_UNSUPPORTED, "%s: fused form needs t in {2, 3, 5} and forward differences (t=%d, n=%d)",
                     name, threshold, n_shares);
  if (n_elem && (!secrets || !shares)) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  return mt_device_run(name, mt_state, mt_index, n_elem, threshold - 1, scratch, scratch_bytes, stream, threshold - 1,
                       [&](GenArgs& ga, hipStream_t s, const MtKnobs& k) {
                         ga.secrets = secrets;
                         ga.shares = static_cast<uint8_t*>(shares);
                         ga.n_shares = n_shares;
                         if (threshold == 2) launch_gen<2>(ga, s, k);
                         else if (threshold == 3) launch_gen<3>(ga, s, k);
                         else launch_gen<5>(ga, s, k);
                       });
}

// ---- one fused draw + split over a list of tensors ---------------------------
// make_shares draws every coefficient from one sequential stream
// (shamir.py:59-61), so splitting tensors A, B, C in turn draws the words one
// split of concat(A, B, C) draws: the draw runs as for one vector of n_total
// elements (same levels, substreams, speculation), and only the emission
// differs — each tensor's shares go to that tensor's own tiled block
// (emit_split_seg, seg_plan.hpp).  The segment table sits behind the draw's
// own scratch, uploaded from a pinned buffer on the caller's stream.
extern "C" uint64_t dn_mt19937_split_many_scratch_bytes(uint64_t n_total, int tm1, uint64_t n_segments) {
  return dn_mt19937_device_scratch_bytes(n_total, tm1) + (n_segments + 1) * sizeof(SegEnt);
}

extern "C" int dn_mt19937_split_many_supported(uint64_t n_total, int threshold, int n_shares, uint64_t n_segments) {
  return n_segments <= kMaxSegments && dn_mt19937_split_supported(n_total, threshold, n_shares);
}

extern "C" int dn_mt19937_split_many_device(uint32_t* mt_state, int32_t* mt_index, const int64_t* secrets,
                                            const dn_m521_segment_t* segments, uint64_t n_segments, int threshold,
                                            int n_shares, void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* name = "dn_mt19937_split_many_device";
  if (threshold < 1 || threshold > DN_MAX_THRESHOLD)
    return set_error(DN_ERR_UNSUPPORTED, "%s: threshold %d outside 1..%d", name, threshold, DN_MAX_THRESHOLD);
  if (threshold > n_shares) return set_error(DN_ERR_THRESHOLD, "threshold should be little equal than shares");
  if (!(threshold == 2 || threshold == 3 || threshold == 5) || fd_needs_fold(threshold, n_shares) ||
      n_shares > DN_MAX_SHARES)
    return set_error(DN_ERR_UNSUPPORTED, "%s: fused form needs t in {2, 3, 5} and forward differences (t=%d, n=%d)",
                     name, threshold, n_shares);
  if (n_segments > kMaxSegments)
    return set_error(DN_ERR_ARG, "%s: %llu segments (at most %llu)", name, static_cast<unsigned long long>(n_segments),
                     static_cast<unsigned long long>(kMaxSegments));
  if (n_segments && !segments) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  uint64_t n_total = 0, nseg = 0;
  for (uint64_t k = 0; k < n_segments; ++k) {
    if (!segments[k].n_elem) continue;  // an empty tensor consumes no draw
    if (!segments[k].shares) return set_error(DN_ERR_ARG, "%s: null pointer", name);
    n_total += segments[k].n_elem;
    ++nseg;
  }
  if (!mt_state || !mt_index) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (!n_total) return DN_OK;
  if (!secrets || !scratch) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  const int tm1 = threshold - 1;
  if (!dn_mt19937_split_supported(n_total, threshold, n_shares))
    return set_error(DN_ERR_UNSUPPORTED, "%s: %llu words exceed the jump table", name,
                     static_cast<unsigned long long>(17 * n_total * static_cast<uint64_t>(tm1)));
  const uint64_t draw_bytes = dn_mt19937_device_scratch_bytes(n_total, tm1);
  if (scratch_bytes < dn_mt19937_split_many_scratch_bytes(n_total, tm1, n_segments))
    return set_error(DN_ERR_ARG, "%s: scratch too small", name);
  const size_t tab_bytes = (nseg + 1) * sizeof(SegEnt);
  PinLease tab((tab_bytes + 3) / 4);  // idle again once the stream has been synchronised (below, on every path)
  if (!tab.p) return set_error(DN_ERR_HIP, "%s: pinned staging buffer", name);
  SegEnt* ent = reinterpret_cast<SegEnt*>(tab.p);
  uint64_t e = 0, j = 0;
  for (uint64_t k = 0; k < n_segments; ++k) {
    if (!segments[k].n_elem) continue;
    ent[j++] = SegEnt{e, static_cast<uint8_t*>(segments[k].shares), dn_m521_vec_bytes(segments[k].n_elem)};
    e += segments[k].n_elem;
  }
  ent[j] = SegEnt{n_total, nullptr, 0};
  SegEnt* dtab = reinterpret_cast<SegEnt*>(static_cast<uint8_t*>(scratch) + draw_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(dtab, ent, tab_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return set_error(DN_ERR_HIP, "%s: segment table upload", name);
  }
  const int rc = mt_device_run(name, mt_state, mt_index, n_total, tm1, scratch, draw_bytes, stream, tm1,
                               [&](GenArgs& ga, hipStream_t s, const MtKnobs& k) {
                                 ga.secrets = secrets;
                                 ga.n_shares = n_shares;
                                 ga.segs = dtab;
                                 ga.nseg = nseg;  // (after mt_device_run's ga.vb: the same storage)
                                 if (threshold == 2) launch_gen<2, true>(ga, s, k);
                                 else if (threshold == 3) launch_gen<3, true>(ga, s, k);
                                 else launch_gen<5, true>(ga, s, k);
                               });
  // the draw synchronises the stream before DN_OK and DN_ERR_RETRY; an
  // argument error may return before it, with the table's copy in flight
  if (rc != DN_OK && rc != DN_ERR_RETRY) (void)hipStreamSynchronize(st);
  return rc;
}

// The current device's speculation counters (DN_MT_SPEC): out[0] calls that
// used speculated windows, out[1] speculations a call did not match, out[2]
// speculations launched, out[3] 1 if one is armed now (the device's state is
// made here if no draw has made it yet: all zero).
extern "C" int dn_mt19937_spec_stats(uint64_t* out) {
  if (!out) return set_error(DN_ERR_ARG, "dn_mt19937_spec_stats: null pointer");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(DN_ERR_HIP, "dn_mt19937_spec_stats: no device");
  SpecState* sp = spec_slot(dev);
  if (!sp) return set_error(DN_ERR_HIP, "dn_mt19937_spec_stats: speculation state");
  std::lock_guard<std::mutex> g(sp->m);
  out[0] = sp->hits;
  out[1] = sp->misses;
  out[2] = sp->launched;
  out[3] = sp->armed ? 1u : 0u;
  return DN_OK;
}
