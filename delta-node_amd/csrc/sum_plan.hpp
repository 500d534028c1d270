// sum_plan.hpp — which input goes into which launch of dn_m521_sum_vecs.
//
// One launch of the share-sum kernel (share_sum.hip) takes up to
// DN_M521_SUM_GROUP inputs; a longer list is chained: launch 0 writes `out`,
// every later launch takes `out` as its first (positive) input and adds the
// next GROUP - 1 inputs to it.  `out` may equal an input's address (in-place
// accumulation), any number of times.  A lane reads its element of every input
// of a launch before it writes that element of `out`, so an alias is safe
// within one launch — but launch 0 overwrites `out`, so every input equal to
// `out` must be read by launch 0.  The order built here puts those first (both
// parts otherwise in the caller's order); an input that overlaps `out` without
// being equal to it is refused, and so are more aliases than one launch holds.
// This header holds that logic — shared by the entry point and by a host
// program that replays the launches on a model of memory
// (tests/host/sum_plan_check.cpp).  Plain C++: no HIP header.
#pragma once

#include <stdint.h>

#include "dn_shamir.h"

namespace dn {

constexpr uint64_t kSumGroup = DN_M521_SUM_GROUP;

enum SumPlanStatus { kSumPlanOk = 0, kSumPlanOverlap = 1, kSumPlanAliases = 2 };

// order[0 .. m) = a permutation of 0 .. m-1: the inputs whose address is `out`,
// then the others.  `bytes`: the length of every input and of `out`.
inline SumPlanStatus sum_plan_order(const uint64_t* addr, uint64_t m, uint64_t out, uint64_t bytes, uint64_t* order,
                                    uint64_t group = kSumGroup) {
  uint64_t aliases = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const uint64_t a = addr[i];
    if (a == out) {
      ++aliases;
      continue;
    }
    const uint64_t dist = a > out ? a - out : out - a;
    if (dist < bytes) return kSumPlanOverlap;
  }
  if (aliases > group) return kSumPlanAliases;
  uint64_t head = 0, tail = aliases;
  for (uint64_t i = 0; i < m; ++i) order[addr[i] == out ? head++ : tail++] = i;
  return kSumPlanOk;
}

// Launches of a list of m inputs (m >= 1).
inline uint64_t sum_plan_launches(uint64_t m, uint64_t group = kSumGroup) {
  return m <= group ? 1u : 1u + (m - group + group - 2u) / (group - 1u);
}

// Launch j (< sum_plan_launches(m)) takes order[*begin .. *begin + *count);
// j > 0 takes `out` before them (*count <= group - 1 then).
inline void sum_plan_slice(uint64_t m, uint64_t j, uint64_t* begin, uint64_t* count, uint64_t group = kSumGroup) {
  if (j == 0) {
    *begin = 0;
    *count = m < group ? m : group;
    return;
  }
  *begin = group + (j - 1u) * (group - 1u);
  const uint64_t left = m - *begin;
  *count = left < group - 1u ? left : group - 1u;
}

// The kernel arguments of launch j: its input addresses into ptrs[0 .. n) and
// their signs into the bit set neg (bit i of word i / 32: subtract input i;
// group / 32 words, zeroed here); returns n (1 .. group).  negate: m flags, or null.
inline uint32_t sum_plan_fill(const uint64_t* addr, const uint8_t* negate, const uint64_t* order, uint64_t m,
                              uint64_t out, uint64_t j, uint64_t* ptrs, uint32_t* neg, uint64_t group = kSumGroup) {
  for (uint64_t w = 0; w < (group + 31u) / 32u; ++w) neg[w] = 0u;
  uint64_t begin, count;
  sum_plan_slice(m, j, &begin, &count, group);
  uint32_t n = 0;
  if (j > 0) ptrs[n++] = out;
  for (uint64_t i = begin; i < begin + count; ++i, ++n) {
    const uint64_t src = order[i];
    ptrs[n] = addr[src];
    if (negate && negate[src]) neg[n / 32u] |= 1u << (n % 32u);
  }
  return n;
}

}  // namespace dn
