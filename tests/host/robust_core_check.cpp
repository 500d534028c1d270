// robust_core_check.cpp — csrc/robust_plan.hpp and csrc/robust_core.hpp on the CPU
// (the text the kernel runs), driven from stdin by tests/test_resolve_robust_host.py:
// first line "<threshold> <k> <x_1> .. <x_k>"  ->  "error <code> <message>" and no
// more, or the plan: "plan <negate>", then k + 1 lines "<|A_i|> <d> <shift> <d_inv32>
// <p_inv_d> <d_recip> <w_0> .. <w_16>" (the last: D_all alone, |A| printed as 0);
// then per line the k shares of one element in hex (< 2^521)  ->  "<verdict> <f in hex>".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "robust_core.hpp"
#include "robust_plan.hpp"

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
static void run_row(const dn_m521_robust_plan_t& p, const std::vector<std::string>& ys) {
  const dn_m521_check_plan_t& chk = p.check;
  uint32_t S[R + 1][kChkAcc] = {};
  for (int i = 0; i < chk.k; ++i) {
    uint32_t y[kChkLimbs], c[R + 1];
    limbs_of(ys[i], y);
    y[16] |= 0xABCD0000u & ~kChkTop;  // what the 16-bit top plane may carry above bit 9 is ignored
    for (int j = 0; j < R; ++j) c[j] = static_cast<uint32_t>(chk.c[j][i]);
    c[R] = p.a[i];
    check_mac<R + 1>(S, y, c, 0u - ((chk.neg >> i) & 1u));
  }
  const unsigned v = check_verdict<R>(robust_syndromes<R>(S), chk.k, [&chk](int j, int i) { return chk.xp[j][i]; });
  uint32_t f[kChkLimbs];
  if (v >= kChkUnexplained) robust_plain(S[R], p.div[kRobustAll], p.negate, f);
  else robust_located(S[0], S[R], static_cast<uint32_t>(chk.c[0][v]), p.a[v], p.div[v], p.negate, f);
  std::printf("%u ", v);
  for (int l = kChkLimbs - 1; l >= 0; --l) std::printf("%08x", f[l]);
  std::printf("\n");
}

int main() {
  dn_m521_robust_plan_t plan{};
  int t = 0, k = 0;
  std::cin >> t >> k;
  std::vector<uint64_t> xs(k > 0 ? k : 0);
  for (auto& x : xs) std::cin >> x;
  char why[160] = "";
  const int rc = robust_plan_build(xs.data(), k, t, &plan, why, sizeof(why));
  if (rc != DN_OK) {
    std::printf("error %d %s\n", rc, why);
    return 0;
  }
  if (!robust_plan_wellformed(plan)) return 2;
  std::printf("plan %u\n", plan.negate);
  for (int i = 0; i <= plan.check.k; ++i) {
    const dn_m521_div_small_t& q = plan.div[i < plan.check.k ? i : kRobustAll];
    std::printf("%u %u %u %u %u %llu", i < plan.check.k ? plan.a[i] : 0u, q.d, q.shift, q.d_inv32, q.p_inv_d,
                static_cast<unsigned long long>(q.d_recip));
    for (int l = 0; l < kChkLimbs; ++l) std::printf(" %u", q.w[l]);
    std::printf("\n");
  }
  std::vector<std::string> ys(plan.check.k);
  while (std::cin >> ys[0]) {
    for (int i = 1; i < plan.check.k; ++i) std::cin >> ys[i];
    switch (plan.check.r) {
      case 2: run_row<2>(plan, ys); break;
      case 3: run_row<3>(plan, ys); break;
      default: run_row<4>(plan, ys); break;
    }
  }
  return 0;
}
