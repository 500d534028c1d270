// recon_low_check.cpp — the five-limb reconstruct's per-element arithmetic
// (delta-node_amd/csrc/recon_low.hpp, the function reconstruct_low_kernel
// calls) and its routing decision (recon_low_eligible / recon_low_covers,
// csrc/recon_plan.hpp) on the host: no GPU and no HIP needed.
// tests/test_recon_low_host.py feeds it limb vectors and compares the words
// with Python big integers.
//
// stdin, one query per line (numbers in hex):
//   C u64 fe ovf a_limbs has_inv k shift neg a_0 .. a_{k-1}
//       a call: which outputs it asks for, the descriptor's fields, the
//       weights' first limbs.  Prints "R <eligible> <covers> <a_sum>".
//   E y_0[0] y_0[1] y_0[2] y_0[15] hi_0  ...  (5 words per share row, k rows)
//       one element of the last call, which must be routed to the five-limb
//       path.  Prints "W <word>".
// Exit status 1 on a malformed query.
//
// build: c++ -O1 -std=c++17 -I../delta-node_amd/csrc recon_low_check.cpp
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "recon_low.hpp"
#include "recon_plan.hpp"

using namespace dn;

namespace {

struct Call {
  int k = 0;
  uint32_t shift = 0, neg = 0, a_sum = 0;
  uint32_t a[16] = {};
  bool low = false;
};

template <int K>
uint64_t word(const Call& c, const std::vector<uint32_t>& v) {
  uint32_t y[K][kLowPlanes], a[K];
  for (int i = 0; i < K; ++i) {
    a[i] = c.a[i];
    for (int l = 0; l < kLowPlanes; ++l) y[i][l] = v[static_cast<size_t>(i) * kLowPlanes + l];
  }
  return recon_low_word<K>(y, a, c.neg, c.shift, c.a_sum);
}

}  // namespace

int main() {
  Call c;
  char buf[4096];
  while (std::fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    in >> std::hex;
    std::string op;
    if (!(in >> op)) continue;
    if (op == "C") {
      uint32_t u64 = 0, fe = 0, ovf = 0, a_limbs = 0, has_inv = 0, k = 0;
      c = Call{};
      if (!(in >> u64 >> fe >> ovf >> a_limbs >> has_inv >> k >> c.shift >> c.neg) || k > 16 || c.shift > 31) return 1;
      c.k = static_cast<int>(k);
      for (int i = 0; i < c.k; ++i)
        if (!(in >> c.a[i])) return 1;
      const bool el = recon_low_eligible(u64 != 0, fe != 0, ovf != 0, static_cast<int>(a_limbs),
                                         static_cast<int>(has_inv), c.k, c.a, 1u, &c.a_sum);
      const bool cov = recon_low_covers(c.k);
      c.low = el && cov;
      std::printf("R %d %d %" PRIx32 "\n", el ? 1 : 0, cov ? 1 : 0, el ? c.a_sum : 0u);
    } else if (op == "E") {
      if (!c.low) return 1;
      std::vector<uint32_t> v(static_cast<size_t>(c.k) * kLowPlanes);
      for (uint32_t& x : v)
        if (!(in >> x)) return 1;
      uint64_t w = 0;
      switch (c.k) {
        case 2: w = word<2>(c, v); break;
        case 3: w = word<3>(c, v); break;
        case 4: w = word<4>(c, v); break;
        default: w = word<5>(c, v); break;
      }
      std::printf("W %" PRIx64 "\n", w);
    } else {
      return 1;
    }
  }
  return 0;
}
