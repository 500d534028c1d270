// mimc7_bn254.hip — MiMC7 data / weight commitments on gfx950.
//
// Reference: delta_node/utils/mimc7.py:18-92 over the BN254 scalar field
// q = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
// (utils/constant.py:6-7) with 13 round constants (constant.py:14-30):
//   mimc7_hash(x, k)      = r_13 + k,  r_0 = x,  r_{i+1} = ((r_i + k + c_i) mod q)^7 mod q
//   mimc7_hash_arr(xs, k) = fold r <- (r + x + mimc7_hash(x, r)) mod q, r_0 = k
//   _float2mpz(v, p)      = min(a, q - a),  a = int(v * 10^p)
//   data commitment: rows -> field ints (features 10^8, label 10^21), zero
//   rows padded to a multiple of 128, hash_arr(row, 2) per row, then a
//   binary Merkle tree of hash_arr([left, right], 2) per 128-row block.
//
// Arithmetic: Montgomery over 9 x 29-bit limbs (R = 2^261, one element per
// lane), separated operand scanning: the 81 limb products of a b and the 81 of
// m q go into 64-bit column accumulators (29-bit limbs leave room for 18
// products per column), so every v_mad_u64_u32 takes its addend straight from
// the accumulator pair — no carry chain per product, no register moves to
// build zero-extended addends (the 8 x 32-bit CIOS form compiled to ~750 VALU
// per product, this one to ~250) and short dependency chains.  R > 170 q, so
// products of operands below 3 q still leave a result below 2 q: the round
// sums r + k + c are carry-normalized but not reduced.  Everything stays in
// Montgomery form between rounds (sums commute with the form);
// t^7 = t^4 t^3: 2 squares (45 limb products) and 2 products per round.  Field values cross memory as
// 8 x 32-bit plain limbs.  The row pass
// is one lane per row (rows are independent chains); the Merkle pass is one
// 64-lane workgroup per 128-leaf block, levels handed over through LDS.
// The weight commitment is one sequential chain by definition (each step
// keys the next hash): one lane, latency-bound.
//
// The field arithmetic itself (limb helpers, mont_mul, mont_sqr, hash_m,
// arr_step, float_to_field, make_consts) is in mimc7_field.hpp, which a plain
// C++ compiler can include: tests/host/mimc7_field_check.cpp rehearses it on
// the host.  This file holds the kernels and the entry points.
#include <hip/hip_runtime.h>

#include <cstring>

#include "dn_internal.hpp"
#include "dn_mimc7.h"
#include "mimc7_consts.hpp"
#include "mimc7_field.hpp"

namespace dn {
namespace mimc {

struct RowArgs {
  Consts k;
  const double* data;  // [rows][cols], row-major
  uint64_t rows, rows_pad;
  int32_t cols;
  double scale_feat, scale_label;
  uint32_t* out;  // [rows_pad][8] plain canonical hashes
  uint32_t* bad;
};

__global__ void __launch_bounds__(256) rows_kernel(const RowArgs a) {
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (row >= a.rows_pad) return;
  uint32_t r[N];
  {  // key 2 in Montgomery form
    const uint32_t two[L] = {2, 0, 0, 0, 0, 0, 0, 0};
    to_mont(r, two, a.k);
  }
  bool ok = true;
  for (int c = 0; c < a.cols; ++c) {
    uint32_t x[L], xm[N];
    if (row < a.rows) {
      const double v = a.data[row * a.cols + c];
      ok &= float_to_field(v, c == a.cols - 1 ? a.scale_label : a.scale_feat, x, a.k);
    } else {
      for (int i = 0; i < L; ++i) x[i] = 0;  // padding rows: [0] * cols
    }
    to_mont(xm, x, a.k);
    arr_step(r, xm, a.k);
  }
  uint32_t h[L];
  from_mont(h, r, a.k);
  for (int i = 0; i < L; ++i) a.out[row * L + i] = h[i];
  if (!ok) atomicAdd(a.bad, 1u);
}

struct MerkleArgs {
  Consts k;
  const uint32_t* leaves;  // [blocks * 128][8] plain
  uint32_t* roots;         // [blocks][8] plain
};

// BPW 128-leaf blocks per workgroup of 64 BPW lanes; level sizes 64, 32,
// ..., 1 nodes per block.  The nodes of a level are packed onto the first
// lanes (thread t -> block t / w, node t % w), so every active wave is full
// until a level has fewer than 64 nodes in the workgroup: 33 wave-levels per
// 16 blocks instead of 7 per block (many blocks); BPW = 1 when there are few
// blocks (each level is then one hash-pair latency per wave either way).
template <int BPW>
__global__ void __launch_bounds__(64 * BPW) merkle_kernel(const MerkleArgs a, uint64_t blocks) {
  __shared__ uint32_t s[64 * BPW][N];
  const uint32_t t = threadIdx.x;
  const uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * BPW;
  uint32_t key[N];
  {
    const uint32_t two[L] = {2, 0, 0, 0, 0, 0, 0, 0};
    to_mont(key, two, a.k);
  }
  if (b0 + t / 64 < blocks) {
    const uint32_t* lv = a.leaves + (b0 + t / 64) * 128 * L;
    const uint32_t j = t % 64;
    uint32_t l[L], r[L], lm[N], rm[N], acc[N];
    for (int i = 0; i < L; ++i) {
      l[i] = lv[(2 * j) * L + i];
      r[i] = lv[(2 * j + 1) * L + i];
    }
    to_mont(lm, l, a.k);
    to_mont(rm, r, a.k);
    for (int i = 0; i < N; ++i) acc[i] = key[i];
    arr_step(acc, lm, a.k);
    arr_step(acc, rm, a.k);
    for (int i = 0; i < N; ++i) s[t][i] = acc[i];  // Montgomery form from here on; block b at s[64 b ..]
  }
  __syncthreads();
  for (uint32_t width = 32; width >= 1; width >>= 1) {
    uint32_t nxt[N];
    const uint32_t b = t / width, j = t % width;
    const bool act = t < BPW * width && b0 + b < blocks;
    if (act) {
      for (int i = 0; i < N; ++i) nxt[i] = key[i];
      arr_step(nxt, s[64 * b + 2 * j], a.k);
      arr_step(nxt, s[64 * b + 2 * j + 1], a.k);
    }
    __syncthreads();
    if (act)
      for (int i = 0; i < N; ++i) s[64 * b + j][i] = nxt[i];
    __syncthreads();
  }
  if (t < BPW && b0 + t < blocks) {
    uint32_t out[L];
    from_mont(out, s[64 * t], a.k);
    for (int i = 0; i < L; ++i) a.roots[(b0 + t) * L + i] = out[i];
  }
}

struct ChainArgs {
  Consts k;
  const double* w;
  uint64_t n;
  double scale;
  uint32_t key[L];  // plain
  uint32_t* out;    // [8] plain
  uint32_t* bad;
};

__global__ void chain_kernel(const ChainArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t r[N];
  to_mont(r, a.key, a.k);
  // keep the chain on the VALU: every value here is wave-uniform, and the
  // compiler would otherwise run the products on the scalar unit (slower:
  // DESIGN.md 4.6); an asm-defined VGPR value counts as divergent
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(r[i]));
  bool ok = true;
  for (uint64_t i = 0; i < a.n; ++i) {
    uint32_t x[L], xm[N];
    ok &= float_to_field(a.w[i], a.scale, x, a.k);
    to_mont(xm, x, a.k);
    arr_step(r, xm, a.k);
  }
  uint32_t h[L];
  from_mont(h, r, a.k);
  for (int i = 0; i < L; ++i) a.out[i] = h[i];
  if (!ok) atomicAdd(a.bad, 1u);
}

struct HashArgs {
  Consts k;
  const uint32_t* x;    // [n][8] plain, < q
  const uint32_t* key;  // [n][8] plain, < q
  uint32_t* out;        // [n][9] plain unreduced r + k (< 2q < 2^255; 9th limb 0)
  uint64_t n;
};

__global__ void __launch_bounds__(256) hash_kernel(const HashArgs a) {
  const uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  uint32_t x[L], k[L], xm[N], km[N];
  for (int i = 0; i < L; ++i) {
    x[i] = a.x[e * L + i];
    k[i] = a.key[e * L + i];
  }
  to_mont(xm, x, a.k);
  to_mont(km, k, a.k);
  uint32_t r[N];
  for (int i = 0; i < N; ++i) r[i] = xm[i];
  for (int c = 0; c < kRounds; ++c) {
    uint32_t t[N];
    for (int i = 0; i < N; ++i) t[i] = r[i] + km[i] + a.k.cts[c][i];  // < 3 q
    norm29(t);
    uint32_t t2[N], t3[N], t6[N];
    mont_mul(t2, t, t, a.k);
    mont_mul(t3, t2, t, a.k);
    mont_mul(t6, t3, t3, a.k);
    mont_mul(r, t6, t, a.k);
  }
  uint32_t rp[L];
  from_mont(rp, r, a.k);
  const uint32_t carry = add_in(rp, k);  // r + k, unreduced (mimc7.py:26)
  for (int i = 0; i < L; ++i) a.out[e * 9 + i] = rp[i];
  a.out[e * 9 + 8] = carry;
}

}  // namespace mimc
}  // namespace dn

using namespace dn;
using namespace dn::mimc;

namespace {
void consts(Consts& k) {
  std::memset(&k, 0, sizeof(k));
  make_consts(k);
  for (int c = 0; c < kRounds; ++c) {
    uint32_t plain[L];
    dec_to_limbs(kCtsDec[c], plain);
    to_mont(k.cts[c], plain, k);
  }
}

}  // namespace

extern "C" int dn_mimc7_data_rows(const double* data, uint64_t rows, int cols, uint32_t* row_hashes,
                                  uint32_t* bad_count, void* stream) {
  if (cols < 1 || rows == 0) return set_error(DN_ERR_ARG, "dn_mimc7_data_rows: empty data");
  if (!data || !row_hashes || !bad_count) return set_error(DN_ERR_ARG, "dn_mimc7_data_rows: null pointer");
  RowArgs a;
  std::memset(&a, 0, sizeof(a));
  consts(a.k);
  a.data = data;
  a.rows = rows;
  a.rows_pad = (rows + 127) / 128 * 128;
  a.cols = cols;
  a.scale_feat = pow10d(8);
  a.scale_label = pow10d(21);
  a.out = row_hashes;
  a.bad = bad_count;
  hipLaunchKernelGGL(rows_kernel, dim3(static_cast<uint32_t>((a.rows_pad + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_mimc7_data_rows: %s", hipGetErrorString(err));
  return DN_OK;
}

extern "C" int dn_mimc7_merkle_blocks(const uint32_t* leaves, uint64_t blocks, uint32_t* roots, void* stream) {
  if (blocks == 0) return DN_OK;
  if (!leaves || !roots) return set_error(DN_ERR_ARG, "dn_mimc7_merkle_blocks: null pointer");
  MerkleArgs a;
  std::memset(&a, 0, sizeof(a));
  consts(a.k);
  a.leaves = leaves;
  a.roots = roots;
  // blocks per workgroup: pack levels across blocks once there are >= 512 workgroups' worth
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (blocks >= 16 * 512)
    hipLaunchKernelGGL(merkle_kernel<16>, dim3(static_cast<uint32_t>((blocks + 15) / 16)), dim3(64 * 16), 0, s, a, blocks);
  else if (blocks >= 4 * 512)
    hipLaunchKernelGGL(merkle_kernel<4>, dim3(static_cast<uint32_t>((blocks + 3) / 4)), dim3(64 * 4), 0, s, a, blocks);
  else
    hipLaunchKernelGGL(merkle_kernel<1>, dim3(static_cast<uint32_t>(blocks)), dim3(64), 0, s, a, blocks);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_mimc7_merkle_blocks: %s", hipGetErrorString(err));
  return DN_OK;
}

extern "C" int dn_mimc7_weight_chain(const double* w, uint64_t n, int precision, uint32_t* out, uint32_t* bad_count,
                                    void* stream) {
  if (!w || !out || !bad_count) return set_error(DN_ERR_ARG, "dn_mimc7_weight_chain: null pointer");
  if (precision < 0 || precision > 22) return set_error(DN_ERR_ARG, "dn_mimc7_weight_chain: precision 0..22");
  ChainArgs a;
  std::memset(&a, 0, sizeof(a));
  consts(a.k);
  a.w = w;
  a.n = n;
  a.scale = pow10d(precision);
  a.key[0] = 2;
  a.out = out;
  a.bad = bad_count;
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_mimc7_weight_chain: %s", hipGetErrorString(err));
  return DN_OK;
}

extern "C" int dn_mimc7_hash(const uint32_t* xs, const uint32_t* keys, uint64_t n, uint32_t* out, void* stream) {
  if (n == 0) return DN_OK;
  if (!xs || !keys || !out) return set_error(DN_ERR_ARG, "dn_mimc7_hash: null pointer");
  HashArgs a;
  std::memset(&a, 0, sizeof(a));
  consts(a.k);
  a.x = xs;
  a.key = keys;
  a.out = out;
  a.n = n;
  hipLaunchKernelGGL(hash_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "dn_mimc7_hash: %s", hipGetErrorString(err));
  return DN_OK;
}
