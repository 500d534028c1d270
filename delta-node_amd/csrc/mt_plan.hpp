// mt_plan.hpp — what the host decides for an MT19937 device draw
// (mt19937_device.hip): the substream geometry, the jump levels' job tables,
// the scratch size and where CPython's final state comes from.  Plain C++17,
// no HIP header, so the planner builds and is checked with the host compiler
// alone (tools/mt_levels_check.cpp, tests/test_mt_levels_host.py); the two
// predicates the generation kernels also call are DN_MT_HD.
//
// Everything sits in an unnamed namespace, like the jump tables'
// constants it includes: the header is part of exactly one translation unit
// of the library, and of the host tool, and the per-thread planner state
// (tls_mt) is that unit's own.
//
// The planner's knobs (tuning build only, dn_internal.hpp tune_env):
// DN_MT_BACK, DN_MT_RT, DN_MT_SPLIT2 and DN_MT_PARTS_B, read in mt_levels /
// push_level; the product build reads none.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "dn_internal.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_MT_HD __host__ __device__ inline
#else
#define DN_MT_HD inline
#endif

namespace dn {
namespace {

#include "mt19937_jump.inc"
#include "mt19937_jump_short.inc"
#include "mt19937_jump_direct.inc"

// Substream lengths: L_k = 17 * 2^k words (2^k whole draws), k = 10, 12, 14,
// one jump table each (rows A, C, B as in mt19937_jump.inc).  A draw of ncoef
// coefficients uses one k for all its substreams (mt_sub_len): long
// substreams for big draws (fewer jumps), short ones for small draws (a
// substream's generation is one wave's sequential run: ~48 ns per draw, so
// 2^14 draws cost ~0.8 ms whatever the vector size).
// Index 3 (2^8 draws) serves only draws of at most 65 substreams, whose
// windows are all one jump from the caller's (direct rows D_s, below): it has
// no A / C / B rows.
constexpr int kMtLens = 4;
constexpr int kMtLenLog2[kMtLens] = {10, 12, 14, 8};
constexpr int kMtTabLens = 3;  // lengths with A / C / B rows
static_assert(kMtJumpL10 == 17ull << 10 && kMtJumpL12 == 17ull << 12 && kMtJumpL == 17ull << 14, "table lengths");
// Direct rows (tools/gen_mt_jump.py --direct): D_s = x^(L - 624 + (s - 1) L),
// W(s) = D_s(W_idx), s = 1..64, per length in kMtLenLog2's order.  A draw of
// S <= 65 substreams takes ONE jump level from the caller's window instead of
// A then B (one launch, one combine and one level's latency less).  Job poly
// indices from kMtDirectBase address that table.
static_assert(kMtJumpL8 == 17ull << 8, "table lengths");
constexpr int32_t kMtDirectBase = kMtTabLens * kMtJumpRows;
// Runtime direct rows (host_gf2poly.cpp, kMtRtRows of them for L = 17 * 2^14,
// uploaded once per device): job poly indices from kMtRtBase address them.
constexpr int32_t kMtRtBase = kMtDirectBase + kMtLens * kMtDirectRows;

constexpr int kMtN = 624;

// table index of the substream length of a draw of ncoef coefficients:
// 2^14 draws from 2^24 coefficients, 2^12 from 2^21, 2^10 down to 65 * 2^8
// + 1, else 2^8 (at least ~2048 substreams for the big draws; a few hundred
// jumps and a short generation run below; the smallest draws: at most 65
// substreams of 2^8 draws, one direct jump level and a ~4352-word run)
inline int mt_sub_len(uint64_t ncoef) {
  if (ncoef <= static_cast<uint64_t>(kMtDirectRows + 1) << 8) return 3;
  return ncoef >= (1ull << 24) ? 2 : ncoef >= (1ull << 21) ? 1 : 0;
}
inline uint64_t mt_sub_draws(int ki) { return 1ull << kMtLenLog2[ki]; }

uint64_t mt_subs(uint64_t ncoef) {
  const uint64_t d = mt_sub_draws(mt_sub_len(ncoef));
  return (ncoef + d - 1) / d;
}

// Substream s runs forward from W(s) unless backward generation is on
// (back = 1) and s is even, not 0 and not the last (then backward from
// W(s + 1)).  back = 2 (tuning build, DN_MT_BACK=2: a probe of the backward
// generation rate) runs every substream but the first and the last backward.
DN_MT_HD bool mt_sub_forward(uint32_t s, uint64_t S, int back) {
  if (back == 2) return s == 0u || s + 1u >= S;
  return !back || s == 0u || (s & 1u) || s + 1u >= S;
}

// W(s) is jumped to when substream s starts from it or substream s - 1 ends on it.
DN_MT_HD bool mt_window_needed(uint32_t s, uint64_t S, int back) {
  return mt_sub_forward(s, S, back) || !mt_sub_forward(s - 1u, S, back);
}

// ------------------------------------------------------------------ jump jobs
struct JumpJob {
  int32_t src, poly, dst;  // window indices (dst < 0: padding), jump-table row
  int32_t span;            // words [lo, hi) of g this job evaluates: lo | hi << 16
};

// A latency-bound level (few jobs: one Horner chain of ~312 steps per jump)
// splits every jump into P parts over word ranges [lo, hi) of g.  Since
// g(f) W = sum_k f^(64 k) g_k(f) W, part [lo, hi) evaluates
// sum_{k in [lo, hi)} f^(64 (k - lo)) g_k(f) (f^(64 lo) W) by Horner over its
// own words from the window 64 lo words further down W's stream, and the
// parts' windows XOR to the jump (mt_combine_kernel).
struct CombineJob {
  int32_t dst, first, parts, pad;  // dst = XOR of window rows first .. first + parts - 1
};

constexpr int kJumpWaves = 16;  // at most this many jumps (waves) per workgroup, all from one source and part
// 32: small levels (the direct level of a small draw, level A) split into
// parts of ~10 Horner steps (make_shares_vec 2^12 -1.5 us, level A 26.5 vs
// 29.1 us at 2^24; profiles/r04/e/)
constexpr int kMaxParts = 32;  // at most this many parts per jump

constexpr int32_t kFullSpan = kMtPolyWords << 16;  // words [0, 312)
constexpr uint64_t kPartRows = 4096;  // part windows of one split level (jumps x parts <= 4096)

// The jobs of one level: W waves per workgroup (one job each; padding jobs
// have dst -1), grouped by source window and part (one table per workgroup).
struct Level {
  int W = 8;
  std::vector<JumpJob> jobs;
  std::vector<CombineJob> comb;
};

void push_group(Level& L, int32_t src, const std::vector<std::pair<int32_t, int32_t>>& pd, int32_t span) {
  for (size_t i = 0; i < pd.size(); ++i) L.jobs.push_back({src, pd[i].first, pd[i].second, span});
  while (L.jobs.size() % static_cast<size_t>(L.W)) L.jobs.push_back({src, 0, -1, span});
}

// a source's jobs in groups of at most `per`
void push_groups(Level& L, int32_t src, const std::vector<std::pair<int32_t, int32_t>>& pd, size_t per,
                 int32_t span = kFullSpan) {
  for (size_t i = 0; i < pd.size(); i += per)
    push_group(L, src, std::vector<std::pair<int32_t, int32_t>>(pd.begin() + i, pd.begin() + std::min(pd.size(), i + per)),
               span);
}

// One level: (source, [(poly, dst)]) lists of n jumps in all.  A jump's
// Horner chain is ~312 dependent steps of LDS-table reads, so the level is
// latency-bound unless every CU holds many waves.  The level therefore splits
// each jump into P = min(16, 4096 / n) parts over word ranges of g (n P part
// jobs, each ~312 / P steps, written to part rows prow0 .. and XORed into the
// jump's window by mt_combine_kernel) and groups per = clamp(n P / 256, 2,
// 16) part jobs of one source and part per workgroup (one table): ~256
// workgroups, one per CU (82 KB of LDS each), 2..16 waves.  Large levels
// (n >= 4096) stay whole, 16 jumps per workgroup.
// Word ranges [cut[j], cut[j + 1]) of g for at most P parts.  A part costs
// its Horner steps — whole runs of 11 words (jump_run), the words above g's
// top included — plus the stepping of its source stream to word 64 lo, about
// r runs' worth per word of lo (r ~ 0.053 / 11 for 8-wave workgroups, ~0.014 / 11
// for 16-wave ones: profiles/r03/ab/jump_probe/).  Parts nearer the top of g
// start further down the stream, so they get fewer runs: the smallest cost
// bound T (in steps) the greedy split meets with at most P parts.
std::vector<int32_t> part_cuts(int P, int W) {
  const double r = W >= 16 ? 0.014 : 0.053;  // stepping cost per word of lo, in Horner steps
  const int runs_total = (kMtPolyWords + 10) / 11;
  for (int T = 11; ; T += 1) {
    std::vector<int32_t> cut{0};
    while (cut.back() < kMtPolyWords && static_cast<int>(cut.size()) <= P) {
      const int lo = cut.back();
      const int runs = static_cast<int>((T - r * lo) / 11.0);
      if (runs < 1) break;
      cut.push_back(std::min(kMtPolyWords, lo + 11 * runs));
    }
    if (cut.back() >= kMtPolyWords && static_cast<int>(cut.size()) - 1 <= P) return cut;
    if (T > 11 * runs_total + 1000) break;
  }
  std::vector<int32_t> cut;  // unreachable: one part of all the words
  for (int j = 0; j <= P; ++j) cut.push_back(kMtPolyWords * j / P);
  return cut;
}

void push_level(Level& L, const std::vector<std::pair<int32_t, std::vector<std::pair<int32_t, int32_t>>>>& srcs,
                int32_t prow0, int p_force = 0, int w_force = 0) {
  size_t n = 0, most = 0;  // jumps, and the most of one source
  for (auto& sp : srcs) n += sp.second.size(), most = std::max(most, sp.second.size());
  if (n == 0) return;
  int P = static_cast<int>(std::max<size_t>(1, std::min<size_t>(kMaxParts, kPartRows / n)));
  if (p_force > 0) P = std::min(p_force, kMaxParts);
  // DN_MT_PARTS_B (tuning build): the part count of levels of 256 jumps or more
  const char* pb = n >= 256 ? tune_env("DN_MT_PARTS_B") : nullptr;
  if (pb && std::atoi(pb) >= 1) P = std::min(kMaxParts, std::atoi(pb));
  size_t per = std::min<size_t>(kJumpWaves, std::max<size_t>(2, (n * P + 255) / 256));
  L.W = std::min(per, most) > 8 ? 16 : 8;
  if (w_force > 0) L.W = w_force, per = static_cast<size_t>(w_force);  // (mt_jumpc_kernel's workgroups)
  if (P == 1) {
    for (auto& sp : srcs) push_groups(L, sp.first, sp.second, per);
    return;
  }
  const std::vector<int32_t> cut = part_cuts(P, L.W);
  P = static_cast<int>(cut.size()) - 1;
  int32_t row = prow0;
  for (auto& sp : srcs)
    for (auto& pd : sp.second) {
      L.comb.push_back({pd.second, row, P, 0});
      row += P;
    }
  for (int j = 0; j < P; ++j) {
    const int32_t lo = cut[j], hi = cut[j + 1];
    row = prow0 + j;
    for (auto& sp : srcs) {
      std::vector<std::pair<int32_t, int32_t>> pd;
      for (auto& q : sp.second) {
        pd.push_back({q.first, row});
        row += P;
      }
      push_groups(L, sp.first, pd, per, lo | hi << 16);
    }
  }
}

// Levels for windows 1 .. S-1 (s - 1 = 4096 c + 64 a + b; row S holds W_idx;
// part rows from S + 1) with the jump table of substream length ki:
// A: W(1 + 64 a) = A_a(W_idx); C: W(1 + 4096 c + 64 a) = C_c(W(1 + 64 a));
// B: W(base + b) = B_b(W(base)).  back: only the windows a generation wave
// starts from (mt_sub_forward: odd s, the last one) — A and C windows are odd.
// rt: one direct level through the runtime rows (host_gf2poly.cpp) for the
// draws of up to kMtRtRows + 1 substreams of 2^14 draws that generate
// backward: the 1024 windows of a 2^24-element 3-of-5 draw in one level of
// ~150 us instead of level A (~28 us), its combine and level B (~148 us).
// The first substream of split2's second half: even, so the first half's
// last substream (odd) runs forward from a window of the first half, and every
// even substream runs backward from a window of its own half.
inline uint64_t mt_split_half(uint64_t S) { return (S / 2 + 1) & ~1ull; }

// split2 (DN_MT_SPLIT2): the runtime direct level as two levels, the windows
// of substreams [0, S/2) and of [S/2, S), at the whole level's part count, so
// the first half's generation can start while the second half's jumps run.
void build_levels(uint64_t S, int ki, int back, bool rt, Level lv[3], bool split2 = false) {
  const uint64_t R = kMtJumpRadix;
  if (S < 2) return;
  const uint64_t last = S - 2;  // largest s - 1
  const int32_t prow0 = static_cast<int32_t>(S + 1);
  if (rt && split2) {
    const uint64_t half = mt_split_half(S);
    std::vector<std::pair<int32_t, int32_t>> pd1, pd2;
    for (uint64_t s = 1; s < S; ++s)
      if (mt_window_needed(static_cast<uint32_t>(s), S, back))
        (s < half ? pd1 : pd2).push_back({kMtRtBase + static_cast<int32_t>(s - 1), static_cast<int32_t>(s)});
    const int P = static_cast<int>(std::max<size_t>(1, std::min<size_t>(kMaxParts, kPartRows / (pd1.size() + pd2.size()))));
    push_level(lv[0], {{-1, pd1}}, prow0, P);
    int32_t prow1 = prow0;
    for (auto& c : lv[0].comb) prow1 = std::max(prow1, c.first + c.parts);
    push_level(lv[1], {{-1, pd2}}, prow1, P);
    return;
  }
  if (rt) {
    std::vector<std::pair<int32_t, int32_t>> pd;
    for (uint64_t s = 1; s < S; ++s)
      if (mt_window_needed(static_cast<uint32_t>(s), S, back))
        pd.push_back({kMtRtBase + static_cast<int32_t>(s - 1), static_cast<int32_t>(s)});
    push_level(lv[0], {{-1, pd}}, prow0);
    return;
  }
  if (last < static_cast<uint64_t>(kMtDirectRows)) {
    // every window one jump from W_idx: W(s) = D_s(W_idx), one level
    std::vector<std::pair<int32_t, int32_t>> pd;
    for (uint64_t s = 1; s < S; ++s)
      if (mt_window_needed(static_cast<uint32_t>(s), S, back))
        pd.push_back({kMtDirectBase + ki * kMtDirectRows + static_cast<int32_t>(s - 1), static_cast<int32_t>(s)});
    push_level(lv[0], {{-1, pd}}, prow0);
    return;
  }
  const int32_t t0 = ki * kMtJumpRows;  // the table's first row
  {
    std::vector<std::pair<int32_t, int32_t>> pd;
    for (uint64_t a = 0; a <= last / R && a < R; ++a)
      pd.push_back({t0 + kMtRowA + static_cast<int32_t>(a), static_cast<int32_t>(1 + R * a)});
    push_level(lv[0], {{-1, pd}}, prow0);  // source: W_idx, the row before row 0
  }
  {
    std::vector<std::pair<int32_t, std::vector<std::pair<int32_t, int32_t>>>> srcs;
    for (uint64_t a = 0; a < R && R * a <= last; ++a) {  // C: per source W(1 + 64 a), its c digits
      std::vector<std::pair<int32_t, int32_t>> pd;
      for (uint64_t c = 1; c < R && R * R * c + R * a <= last; ++c)
        pd.push_back({t0 + kMtRowC + static_cast<int32_t>(c), static_cast<int32_t>(1 + R * R * c + R * a)});
      if (!pd.empty()) srcs.push_back({static_cast<int32_t>(1 + R * a), pd});
    }
    push_level(lv[1], srcs, prow0);
  }
  {
    std::vector<std::pair<int32_t, std::vector<std::pair<int32_t, int32_t>>>> srcs;
    for (uint64_t base = 0; base <= last; base += R) {  // B: per source W(1 + base)
      std::vector<std::pair<int32_t, int32_t>> pd;
      for (uint64_t b = 1; b < R && base + b <= last; ++b)
        if (mt_window_needed(static_cast<uint32_t>(1 + base + b), S, back))
          pd.push_back({t0 + kMtRowB + static_cast<int32_t>(b), static_cast<int32_t>(1 + base + b)});
      if (!pd.empty()) srcs.push_back({static_cast<int32_t>(1 + base), pd});
    }
    push_level(lv[2], srcs, prow0);
  }
}

// Per-thread host side of a draw: the job tables of the last substream count
// and length (they depend on S and ki only; plain host memory, freed with the
// thread).
struct MtHost {
  uint64_t S = ~0ull;
  int ki = -1;
  int back = 0;
  int parts_b = 0;  // tuning build: DN_MT_PARTS_B the levels were built with
  bool rt = false;  // one direct level through the runtime rows
  bool split2 = false;  // that level in two halves (DN_MT_SPLIT2)
  Level lv[3];
  Level beside;  // rt: the direct level for mt_jumpc_kernel<4, 2> (whole jumps, 4 per workgroup)
  Level j0;      // rt: one jump, row S -> row -1 by x^(17 ncoef) (the rt pointer), in parts, mt_jumpc_kernel<4, 2>
  std::vector<uint32_t> jobs;  // the levels' jobs, their combine jobs, beside's jobs, j0's jobs and combine job
  uint64_t beside_off = 0, j0_off = 0, j0_comb_off = 0;  // word offsets in `jobs`
  uint64_t part_rows = 0;      // part windows the largest split level writes (levels reuse them)
};
thread_local MtHost tls_mt;

// Backward generation of the even substreams (on; DN_MT_BACK=0 in the tuning
// build turns it off for A/B).
int mt_back() {
  const char* e = tune_env("DN_MT_BACK");
  return e ? (e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1) : 1;
}

// DN_MT_SPLIT2: the 2^24 draw's direct level in two halves; the first half's
// generation (substreams [0, S/2), on a side stream) runs while the second
// half's jumps do (their 85 KB tables beside the generation's rings), then the
// second half's generation (round 6).  Off; the tuning build's env knob of
// the same name A/Bs it.
constexpr bool kMtSplit2 = false;

MtHost& mt_levels(uint64_t S, int ki) {
  MtHost& H = tls_mt;
  // 2^8-draw substreams run forward only: at t = 5 one holds a single
  // emission group, and backward generation needs an even count (its window
  // is the top of ring half 1); their one direct level takes the extra jumps
  const int back = ki == 3 ? 0 : mt_back();
  const char* pb = tune_env("DN_MT_PARTS_B");
  const int parts_b = pb ? std::atoi(pb) : 0;
  // the runtime direct level: 2^14-draw substreams generating backward, more
  // than the tabulated direct rows cover, at most kMtRtRows + 1 of them, and
  // rows available on this host (DN_MT_RT=0, tuning build: off)
  const char* rte = tune_env("DN_MT_RT");
  const bool rt = !(rte && rte[0] == '0') && ki == 2 && back == 1 &&
                  S - 1 > static_cast<uint64_t>(kMtDirectRows) && S - 1 <= kMtRtRows &&
                  mt_direct_rows_l14(S, nullptr) != nullptr;
  const char* sp = tune_env("DN_MT_SPLIT2");
  const bool split2 = rt && (sp ? sp[0] == '1' : kMtSplit2) && S >= 4;
  if (H.S != S || H.ki != ki || H.back != back || H.parts_b != parts_b || H.rt != rt || H.split2 != split2) {
    for (auto& l : H.lv) l = Level();
    build_levels(S, ki, back, rt, H.lv, split2);
    H.beside = Level();
    H.j0 = Level();
    if (rt && !split2) {
      std::vector<std::pair<int32_t, int32_t>> pd;
      for (uint64_t s = 1; s < S; ++s)
        if (mt_window_needed(static_cast<uint32_t>(s), S, back))
          pd.push_back({kMtRtBase + static_cast<int32_t>(s - 1), static_cast<int32_t>(s)});
      push_level(H.beside, {{-1, pd}}, static_cast<int32_t>(S + 1), 1, 4);
    }
    // the next call's W_idx for a speculation beside the generation (any
    // shape with jump levels: the levels of a small generation run beside it
    // as they are, mt_device_run)
    if (!split2 && S >= 2)
      push_level(H.j0, {{static_cast<int32_t>(S), {{kMtRtBase, -1}}}}, static_cast<int32_t>(S + 1), kMaxParts, 4);
    uint64_t nj = 0, nc = 0;
    for (auto& l : H.lv) nj += l.jobs.size(), nc += l.comb.size();
    nj += H.beside.jobs.size() + H.j0.jobs.size();
    nc += H.j0.comb.size();
    H.part_rows = 0;
    for (auto& l : H.lv)
      for (auto& c : l.comb) H.part_rows = std::max<uint64_t>(H.part_rows, c.first + c.parts - (S + 1));
    for (auto& c : H.j0.comb) H.part_rows = std::max<uint64_t>(H.part_rows, c.first + c.parts - (S + 1));
    H.jobs.assign((nj * sizeof(JumpJob) + nc * sizeof(CombineJob)) / 4, 0u);
    uint64_t o = 0;
    auto put = [&](const void* p, size_t bytes) {  // (an empty table has no bytes and no pointer to copy from)
      if (bytes) std::memcpy(H.jobs.data() + o, p, bytes);
      o += bytes / 4;
    };
    for (auto& l : H.lv) put(l.jobs.data(), l.jobs.size() * sizeof(JumpJob));
    for (auto& l : H.lv) put(l.comb.data(), l.comb.size() * sizeof(CombineJob));
    H.beside_off = o;
    put(H.beside.jobs.data(), H.beside.jobs.size() * sizeof(JumpJob));
    H.j0_off = o;
    put(H.j0.jobs.data(), H.j0.jobs.size() * sizeof(JumpJob));
    H.j0_comb_off = o;
    put(H.j0.comb.data(), H.j0.comb.size() * sizeof(CombineJob));
    H.S = S;
    H.ki = ki;
    H.back = back;
    H.parts_b = parts_b;
    H.rt = rt;
    H.split2 = split2;
  }
  return H;
}

// ------------------------------------------------------------------ scratch
// head (flag at 0, final array at 256) | W_idx (the caller's array advanced
// idx words: window "-1", the level-A source) | windows 0..S (row 0 the
// caller's array; row S unused) | part rows (split levels)
constexpr uint64_t kHead = 2816;  // flag (4 B at 0), final array (2496 B at 256), pad to 256 B

inline uint64_t mt_scratch_bytes(uint64_t ncoef) {
  const uint64_t S = ncoef ? mt_subs(ncoef) : 0;
  if (!S) return kHead + kMtN * 4;
  const MtHost& H = mt_levels(S, mt_sub_len(ncoef));
  return kHead + (1 + S + 1 + H.part_rows) * kMtN * 4;
}

// ------------------------------------------------------------------ final state
// CPython's state after a draw of ncoef coefficients (17 ncoef words) from
// index idx, in S substreams of length ki.  While the draw ends inside the
// caller's array (words <= 624 - idx) only the index moves (sig = -1).
// Otherwise the final array is the one at stream position tf = 624 q (the
// first array boundary at or past the draw's last word), stepped from window
// `sig` (position pos < tf; 0: the caller's array), and the index fidx counts
// into it.  fin_lo / next_lo: the final array and the next call's W_idx
// (position idx + 17 ncoef) in the last substream's frame, whose position 0
// is stream position idx + (S - 1) L (the tail_fin form, last_sub_tail).
struct MtFinal {
  int32_t sig = -1, fidx = 0;
  uint64_t pos = 0, tf = 0;
  int32_t fin_lo = 0, next_lo = 0;
};

inline MtFinal mt_final_plan(int32_t idx, uint64_t ncoef, uint64_t S, int ki) {
  const uint64_t words = 17 * ncoef, h = static_cast<uint64_t>(kMtN - idx);
  MtFinal f;
  f.fidx = idx + static_cast<int32_t>(words <= h ? words : 0);
  if (words <= h) return f;
  const uint64_t m_end = words - h, q = (m_end + kMtN - 1) / kMtN, tf = kMtN * q;
  const uint64_t Lk = 17 * mt_sub_draws(ki);  // words per substream
  uint64_t sg = (tf + kMtN - 1 - static_cast<uint64_t>(idx)) / Lk;  // idx + sg L - 624 < tf
  if (sg > S - 1) sg = S - 1;
  f.sig = static_cast<int32_t>(sg);
  f.pos = sg ? static_cast<uint64_t>(idx) + sg * Lk - kMtN : 0;
  f.tf = tf;
  f.fidx = static_cast<int32_t>(m_end - kMtN * (q - 1));
  const uint64_t base = static_cast<uint64_t>(idx) + (S - 1) * Lk;
  f.fin_lo = static_cast<int32_t>(static_cast<int64_t>(tf) - static_cast<int64_t>(base));
  f.next_lo = static_cast<int32_t>(static_cast<int64_t>(idx + words) - static_cast<int64_t>(base));
  return f;
}

}  // namespace
}  // namespace dn
