// robust_pair_check.cpp — csrc/robust_pair.hpp and robust_plan.hpp's robust_plan_build2 on the CPU
// (the text the kernel runs), driven from stdin by tests/test_resolve_robust2_host.py.  Per line:
//   "div <v>"                       ->  "<d> <shift> <d_inv32> <p_inv_d> <d_recip> <w_0> .. <w_16>" or "reject"
//   "plan <errors> <t> <k> <x> .."  ->  "error <code> <message>" or "ok <max_errors> <same>", same = 1 when the
//                                       plan is dn_m521_robust_plan's byte for byte outside max_errors
//   "bounds <k> <x> .."             ->  "error <code> <message>" or "ok": robust_pair_bounds alone
//   "fin <S_0> .. <S_3> <T'>"       ->  "<verdict> <passing pairs> <f in hex>" under the last plan: the five
//                                       chains in hex as check_mac leaves them (unreduced, < 2^576)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "robust_pair.hpp"
#include "robust_plan.hpp"

using namespace dn;

static void chain_of(const std::string& hex, uint32_t (&s)[kChkAcc]) {
  for (int l = 0; l < kChkAcc; ++l) s[l] = 0u;
  int bit = 0;
  for (auto it = hex.rbegin(); it != hex.rend(); ++it, bit += 4)
    s[bit / 32] |= static_cast<uint32_t>(std::stoul(std::string(1, *it), nullptr, 16)) << (bit % 32);
}

int main() {
  dn_m521_robust_plan_t plan{};
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "div") {
      uint32_t v;
      std::cin >> v;
      dn_m521_div_small_t q;
      if (!robust_div_consts(v, &q)) {
        std::printf("reject\n");
        continue;
      }
      std::printf("%u %u %u %u %llu", q.d, q.shift, q.d_inv32, q.p_inv_d, static_cast<unsigned long long>(q.d_recip));
      for (int l = 0; l < kChkLimbs; ++l) std::printf(" %u", q.w[l]);
      std::printf("\n");
    } else if (cmd == "plan") {
      int errors, t, k;
      std::cin >> errors >> t >> k;
      std::vector<uint64_t> xs(k);
      for (auto& x : xs) std::cin >> x;
      char why[160] = "", why1[160] = "";
      dn_m521_robust_plan_t one{};
      const int rc = robust_plan_build2(xs.data(), k, t, errors, &plan, why, sizeof(why));
      if (rc != DN_OK) {
        std::printf("error %d %s\n", rc, why);
        continue;
      }
      if (robust_plan_build(xs.data(), k, t, &one, why1, sizeof(why1)) != DN_OK || !robust_plan_wellformed(plan)) return 2;
      one.max_errors = plan.max_errors;
      std::printf("ok %u %d\n", plan.max_errors, std::memcmp(&one, &plan, sizeof(plan)) == 0 ? 1 : 0);
    } else if (cmd == "bounds") {
      int k;
      std::cin >> k;
      std::vector<uint64_t> xs(k);
      for (auto& x : xs) std::cin >> x;
      char why[160] = "";
      const int rc = robust_pair_bounds(xs.data(), k, why, sizeof(why));
      if (rc != DN_OK) std::printf("error %d %s\n", rc, why);
      else std::printf("ok\n");
    } else {  // fin: robust_kernel<4, .., true>'s finish, the wave's lanes one after another
      uint32_t S[5][kChkAcc], f[kChkLimbs], win[kPairWords];
      for (auto& s : S) {
        std::string hex;
        std::cin >> hex;
        chain_of(hex, s);
      }
      const dn_m521_check_plan_t& chk = plan.check;
      unsigned v = check_verdict<4>(robust_syndromes<4>(S), chk.k, [&chk](int j, int i) { return chk.xp[j][i]; });
      unsigned hits = 0;
      if (v >= kChkUnexplained) robust_plain(S[4], plan.div[kRobustAll], plan.negate, f);
      else robust_located(S[0], S[4], static_cast<uint32_t>(chk.c[0][v]), plan.a[v], plan.div[v], plan.negate, f);
      if (v == kChkUnexplained && plan.max_errors == 2u) {
        robust_pair_publish(S, win);
        uint32_t found = 0, i, j;
        for (uint32_t idx = 0; idx < static_cast<uint32_t>(chk.k * (chk.k - 1) / 2); ++idx) {
          robust_pair_of(idx, &i, &j);
          if (robust_pair_test(win, chk.xp[1][i], chk.xp[1][j]) && hits++ == 0) found = idx;
        }
        if (hits) {
          robust_pair_of(found, &i, &j);
          robust_pair_correct(win, chk.xp[1][i], chk.xp[1][j], plan.a[i], plan.a[j], plan.div[i], plan.div[j],
                              plan.negate, f);
          v = kPairBase + found;
        }
      }
      std::printf("%u %u ", v, hits);
      for (int l = kChkLimbs - 1; l >= 0; --l) std::printf("%08x", f[l]);
      std::printf("\n");
    }
  }
  return 0;
}
