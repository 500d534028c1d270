// check_core_check.cpp — csrc/check_plan.hpp and csrc/check_core.hpp on the CPU
// (the text the kernel runs), driven from stdin by tests/test_share_check_host.py:
// first line "<threshold> <k> <x_1> .. <x_k>", then per line the k shares of one
// element in hex (< 2^521)  ->  "<culprit byte> <byte of the form without culprit>".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "check_core.hpp"
#include "check_plan.hpp"

using namespace dn;

static void limbs_of(const std::string& hex, uint32_t (&y)[kChkLimbs]) {
  for (int l = 0; l < kChkLimbs; ++l) y[l] = 0u;
  int bit = 0;
  for (auto it = hex.rbegin(); it != hex.rend(); ++it, bit += 4) {
    if (bit >= 32 * kChkLimbs) std::abort();
    y[bit / 32] |= static_cast<uint32_t>(std::stoul(std::string(1, *it), nullptr, 16)) << (bit % 32);
  }
}

template <int R>
static void run_row(const dn_m521_check_plan_t& p, const std::vector<std::string>& ys) {
  uint32_t S[R][kChkAcc] = {};
  for (int i = 0; i < p.k; ++i) {
    uint32_t y[kChkLimbs], c[R];
    limbs_of(ys[i], y);
    y[16] |= 0xABCD0000u & ~kChkTop;  // what the 16-bit top plane may carry above bit 9 is ignored
    for (int j = 0; j < R; ++j) c[j] = static_cast<uint32_t>(p.c[j][i]);
    check_mac<R>(S, y, c, 0u - ((p.neg >> i) & 1u));
  }
  const bool consistent = check_consistent<R>(S);
  const unsigned verdict = check_verdict<R>(S, p.k, [&p](int j, int i) { return p.xp[j][i]; });
  std::printf("%u %u\n", verdict, consistent ? unsigned(kChkConsistent) : unsigned(kChkUnexplained));
}

int main() {
  dn_m521_check_plan_t plan{};
  int t = 0, k = 0;
  std::cin >> t >> k;
  std::vector<uint64_t> xs(k > 0 ? k : 0);
  for (auto& x : xs) std::cin >> x;
  char why[160] = "";
  if (check_plan_build(xs.data(), k, t, &plan, why, sizeof(why)) != DN_OK || !check_plan_wellformed(plan)) return 2;
  std::vector<std::string> ys(plan.k);
  while (std::cin >> ys[0]) {
    for (int i = 1; i < plan.k; ++i) std::cin >> ys[i];
    switch (plan.r) {
      case 1: run_row<1>(plan, ys); break;
      case 2: run_row<2>(plan, ys); break;
      case 3: run_row<3>(plan, ys); break;
      default: run_row<4>(plan, ys); break;
    }
  }
  return 0;
}
