// sum_plan_check.cpp — the share sum's launch plan (csrc/sum_plan.hpp)
// replayed on a model of memory, on the host.
//
// dn_m521_sum_vecs chains launches of up to GROUP inputs: launch 0 writes
// `out`, every later launch takes `out` as a positive input and adds the next
// GROUP - 1 inputs.  `out` may equal input addresses, addresses may repeat.
// For m = 1 .. 3 GROUP + 2 and `out` aliasing no input, input 0, an input of
// the middle group, the last input, and several inputs at once — with repeated
// addresses and seeded random signs — the program builds the plan as the entry
// point does (sum_plan_order, sum_plan_launches, sum_plan_fill) and runs the
// launches on a map address -> 64-bit value (every launch reads all of its
// inputs, then writes `out`).  Checked:
//   * every input is consumed exactly once, with its own sign;
//   * every input whose address is `out` is read by launch 0, and launches
//     1, 2, ... take `out` first, positive;
//   * no launch has more than GROUP inputs or fewer than one, and the launch
//     count is the least possible;
//   * the final `out` equals the signed sum of the inputs' ORIGINAL values
//     (no launch read an `out` that an earlier one had overwritten);
//   * partial overlaps with `out` are refused at both ends of the range, ranges
//     that only touch are accepted, more aliases than GROUP are refused.
// Exit status 0 and "ok" when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "sum_plan.hpp"

using namespace dn;

namespace {

int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (failures++ < 20) {                      \
        std::fprintf(stderr, "FAIL %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);        \
        std::fprintf(stderr, "\n");               \
      }                                           \
    }                                             \
  } while (0)

constexpr uint64_t kBytes = 5 * 16896;  // every range's length
constexpr uint64_t kBase = 0x7f0000000000ull;

// One call: addresses, signs, `out`; replays the plan and checks it.
void replay(const std::vector<uint64_t>& addr, const std::vector<uint8_t>& neg, uint64_t out, bool use_neg,
            std::mt19937_64& rng, const char* what) {
  const uint64_t m = addr.size(), G = kSumGroup;
  std::map<uint64_t, uint64_t> mem;  // address -> value (equal addresses: one value)
  for (uint64_t a : addr)
    if (!mem.count(a)) mem[a] = rng();
  if (!mem.count(out)) mem[out] = rng();  // garbage the call must not read
  uint64_t want = 0;
  for (uint64_t i = 0; i < m; ++i) want += (use_neg && neg[i]) ? 0u - mem[addr[i]] : mem[addr[i]];

  std::vector<uint64_t> order(m, ~0ull);
  const SumPlanStatus st = sum_plan_order(addr.data(), m, out, kBytes, order.data());
  CHECK(st == kSumPlanOk, "%s m=%llu: status %d", what, (unsigned long long)m, (int)st);
  if (st != kSumPlanOk) return;
  std::vector<int> seen(m, 0);
  for (uint64_t i = 0; i < m; ++i) {
    CHECK(order[i] < m, "%s m=%llu: order[%llu] out of range", what, (unsigned long long)m, (unsigned long long)i);
    if (order[i] < m) ++seen[order[i]];
  }
  for (uint64_t i = 0; i < m; ++i) CHECK(seen[i] == 1, "%s m=%llu: input %llu in the order %d times", what,
                                         (unsigned long long)m, (unsigned long long)i, seen[i]);

  const uint64_t launches = sum_plan_launches(m);
  const uint64_t least = m <= G ? 1 : 1 + (m - G + G - 2) / (G - 1);
  CHECK(launches == least, "%s m=%llu: %llu launches", what, (unsigned long long)m, (unsigned long long)launches);
  std::vector<int> used(m, 0);
  uint64_t consumed = 0;
  for (uint64_t j = 0; j < launches; ++j) {
    // guard words around the arrays the entry point passes (ASan has the stack ones; these are checked too)
    std::vector<uint64_t> ptrs(G + 2, 0xDEADull);
    std::vector<uint32_t> bits(G / 32 + 2, 0xDEADu);
    const uint32_t n = sum_plan_fill(addr.data(), use_neg ? neg.data() : nullptr, order.data(), m, out, j,
                                     ptrs.data() + 1, bits.data() + 1);
    CHECK(ptrs[0] == 0xDEADull && ptrs[G + 1] == 0xDEADull && bits[0] == 0xDEADu && bits[G / 32 + 1] == 0xDEADu,
          "%s m=%llu launch %llu wrote outside its arrays", what, (unsigned long long)m, (unsigned long long)j);
    CHECK(n >= 1 && n <= G, "%s m=%llu launch %llu has %u inputs", what, (unsigned long long)m,
          (unsigned long long)j, n);
    if (n < 1 || n > G) return;
    uint64_t begin, count;
    sum_plan_slice(m, j, &begin, &count);
    CHECK(begin == consumed && begin + count <= m && n == count + (j ? 1 : 0), "%s m=%llu launch %llu slice", what,
          (unsigned long long)m, (unsigned long long)j);
    if (begin + count > m) return;
    if (j > 0) {
      CHECK(ptrs[1] == out && !((bits[1] >> 0) & 1u), "%s m=%llu launch %llu does not take out first, positive", what,
            (unsigned long long)m, (unsigned long long)j);
      CHECK(n >= 2, "%s m=%llu launch %llu adds nothing", what, (unsigned long long)m, (unsigned long long)j);
    }
    uint64_t acc = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t p = ptrs[1 + i];
      const bool sub = (bits[1 + i / 32] >> (i % 32)) & 1u;
      if (!(j > 0 && i == 0)) {
        const uint64_t src = order[begin + i - (j ? 1 : 0)];
        ++used[src];
        CHECK(p == addr[src], "%s m=%llu launch %llu input %u address", what, (unsigned long long)m,
              (unsigned long long)j, i);
        CHECK(sub == (use_neg && neg[src] != 0), "%s m=%llu launch %llu input %u sign", what, (unsigned long long)m,
              (unsigned long long)j, i);
        CHECK(!(p == out && j > 0), "%s m=%llu: input %llu aliases out in launch %llu", what, (unsigned long long)m,
              (unsigned long long)src, (unsigned long long)j);
      }
      acc += sub ? 0u - mem[p] : mem[p];  // the launch reads ...
    }
    for (uint32_t w = n; w < G; ++w)
      CHECK(!((bits[1 + w / 32] >> (w % 32)) & 1u), "%s m=%llu launch %llu sign bit %u beyond its inputs", what,
            (unsigned long long)m, (unsigned long long)j, w);
    mem[out] = acc;  // ... then writes
    consumed += count;
  }
  CHECK(consumed == m, "%s m=%llu: %llu inputs consumed", what, (unsigned long long)m, (unsigned long long)consumed);
  for (uint64_t i = 0; i < m; ++i) CHECK(used[i] == 1, "%s m=%llu: input %llu used %d times", what,
                                         (unsigned long long)m, (unsigned long long)i, used[i]);
  CHECK(mem[out] == want, "%s m=%llu: wrong sum", what, (unsigned long long)m);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240521);
  const uint64_t G = kSumGroup;
  for (uint64_t m = 1; m <= 3 * G + 2; ++m) {
    std::vector<uint64_t> addr(m);
    std::vector<uint8_t> neg(m);
    for (uint64_t i = 0; i < m; ++i) {
      addr[i] = kBase + i * kBytes;  // back to back: ranges that touch, none that overlap
      neg[i] = static_cast<uint8_t>(rng() & 1u) * 7u;  // any non-zero flag
    }
    const uint64_t fresh = kBase + (m + 3) * kBytes;
    replay(addr, neg, fresh, false, rng, "no alias, no signs");
    replay(addr, neg, fresh, true, rng, "no alias");
    replay(addr, neg, kBase - kBytes, true, rng, "out just below the inputs");
    replay(addr, neg, kBase + m * kBytes, true, rng, "out just above the inputs");
    replay(addr, neg, addr[0], true, rng, "out is input 0");
    replay(addr, neg, addr[m - 1], true, rng, "out is the last input");
    replay(addr, neg, addr[m / 2], true, rng, "out is a middle input");
    if (m > G + 3) replay(addr, neg, addr[G + 3], true, rng, "out is input GROUP + 3");
    // repeated addresses: every third input is input 1's buffer, and out is that buffer
    if (m >= 2) {
      std::vector<uint64_t> rep(addr);
      for (uint64_t i = 1; i < m; i += 3) rep[i] = addr[1];
      replay(rep, neg, fresh, true, rng, "repeated addresses");
      if ((m + 1) / 3 <= G) replay(rep, neg, addr[1], true, rng, "out is the repeated address");
      // one buffer m times
      std::vector<uint64_t> same(m, addr[0]);
      replay(same, neg, fresh, true, rng, "one buffer m times");
      if (m <= G) replay(same, neg, addr[0], true, rng, "one buffer m times, in place");
    }
    // refusals: partial overlap from either side by one byte and by all but one
    std::vector<uint64_t> order(m);
    const uint64_t victim = addr[m / 2];
    for (uint64_t d : {uint64_t{1}, uint64_t{16896}, kBytes - 1}) {
      CHECK(sum_plan_order(addr.data(), m, victim + d, kBytes, order.data()) == kSumPlanOverlap,
            "m=%llu: out %llu bytes above an input accepted", (unsigned long long)m, (unsigned long long)d);
      CHECK(sum_plan_order(addr.data(), m, victim - d, kBytes, order.data()) == kSumPlanOverlap,
            "m=%llu: out %llu bytes below an input accepted", (unsigned long long)m, (unsigned long long)d);
    }
    // ... and an alias does not excuse another input's partial overlap
    if (m >= 2) {
      std::vector<uint64_t> mixed(addr);
      mixed[0] = addr[m - 1] + 16896;
      CHECK(sum_plan_order(mixed.data(), m, addr[m - 1], kBytes, order.data()) == kSumPlanOverlap,
            "m=%llu: overlap next to an alias accepted", (unsigned long long)m);
    }
    if (m > G) {
      std::vector<uint64_t> same(m, addr[0]);
      CHECK(sum_plan_order(same.data(), m, addr[0], kBytes, order.data()) == kSumPlanAliases,
            "m=%llu: more aliases than a launch holds accepted", (unsigned long long)m);
    }
  }
  // ranges at the top of the address space: the distance test must not wrap
  {
    const uint64_t hi = ~0ull - kBytes + 1;
    uint64_t a[1] = {hi}, order[1];
    CHECK(sum_plan_order(a, 1, 0x1000, kBytes, order) == kSumPlanOk, "far apart refused");
    CHECK(sum_plan_order(a, 1, hi - kBytes, kBytes, order) == kSumPlanOk, "touching refused");
    CHECK(sum_plan_order(a, 1, hi - kBytes + 1, kBytes, order) == kSumPlanOverlap, "overlap at the top accepted");
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
