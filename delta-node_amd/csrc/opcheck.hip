// opcheck.hip — lib/libdn_opcheck.so: the device-header suite's kernel (test
// infrastructure; linked into neither libdn_shamir.so nor the tuning library).
// Lane i runs case i of one operation of csrc/opcheck_ops.hpp.
#include <hip/hip_runtime.h>

#include "opcheck_ops.hpp"

namespace {

__global__ __launch_bounds__(256) void opcheck_kernel(int32_t op, const uint32_t* __restrict__ in,
                                                      uint32_t* __restrict__ out, uint64_t n_cases, uint32_t iw,
                                                      uint32_t ow) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= n_cases) return;
  dn::opcheck::run_op(op, in + i * iw, out + i * ow);
}

}  // namespace

// in: n_cases * dn_opcheck_in_words(op) u32 words, out: n_cases *
// dn_opcheck_out_words(op), both device memory; out pre-filled by the caller.
// Returns 0, -1 for a bad argument, or the hipError_t of the launch.
extern "C" int dn_opcheck_in_words(int op) { return dn::opcheck::in_words(op); }
extern "C" int dn_opcheck_out_words(int op) { return dn::opcheck::out_words(op); }

extern "C" int dn_opcheck_run(int op, const void* in, void* out, uint64_t n_cases, void* stream) {
  const int iw = dn::opcheck::in_words(op), ow = dn::opcheck::out_words(op);
  if (iw == 0 || ow == 0 || !in || !out || n_cases > (1ull << 24)) return -1;
  if (n_cases == 0) return 0;
  const uint32_t blocks = static_cast<uint32_t>((n_cases + 255u) / 256u);
  hipLaunchKernelGGL(opcheck_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), op,
                     static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), n_cases,
                     static_cast<uint32_t>(iw), static_cast<uint32_t>(ow));
  return static_cast<int>(hipGetLastError());
}
