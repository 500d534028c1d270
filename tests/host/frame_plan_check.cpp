// frame_plan_check.cpp — the wire-frame kernels' index arithmetic
// (csrc/frame_plan.hpp) replayed on a model of memory, on the host.
//
// For a record count n and lengths lens[n] the program replays the finish
// launch (offsets -> lens, pad) and the three open launches (block totals,
// scan of the totals, expansion) thread by thread with the header's functions,
// as csrc/codec_frame.hip's kernels use them, LDS included.  Checked:
//   * finish: every offsets index read is in [0, n]; every byte of the padded
//     length area [0, pad16(n)) is written exactly once and nothing beyond it
//     (so nothing at or past R(n)); lens come out as given, the pad as zero;
//     no LDS word is written twice or read unwritten;
//   * open: every 16-byte load lies inside the padded length area; the pad
//     (filled with 0xFF here) never reaches a sum; every scratch total and
//     every offsets entry in [0, n] is written exactly once and nothing
//     outside; every offset equals the naive clamped prefix
//     min(lens[0] + ... + lens[e - 1], cap), for a cap that is the sum, below
//     it and above it;
//   * the scan of the totals alone at the block counts where its load loop
//     and its passes turn over.
// Inputs: the edge list of tests/test_gpu_frames.py (the largest with all
// lengths 255 only) and 1000 seeded random (n, lens).  Exit status 0 and "ok"
// when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "frame_plan.hpp"

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

struct Lds {
  std::vector<uint32_t> w;
  std::vector<uint8_t> set;
  Lds() : w(kFrameLdsWords), set(kFrameLdsWords) {}
  void clear() { std::fill(set.begin(), set.end(), 0); }
  void put(uint32_t slot, uint32_t v) {
    CHECK(slot < kFrameLdsWords, "LDS slot %u", slot);
    if (slot >= kFrameLdsWords) return;
    CHECK(!set[slot], "LDS slot %u written twice", slot);
    set[slot] = 1;
    w[slot] = v;
  }
  uint32_t get(uint32_t slot) {
    CHECK(slot < kFrameLdsWords && set[slot], "LDS slot %u read unwritten", slot);
    return slot < kFrameLdsWords ? w[slot] : 0u;
  }
};

// frame_finish_kernel without its header store
void replay_finish(uint64_t n, const std::vector<uint64_t>& offsets, const std::vector<uint8_t>& lens) {
  const uint64_t pad = frame_pad16(n);
  CHECK(frame_records_offset(n) == kFrameHeader + pad && pad % 16 == 0 && pad >= n && pad < n + 16, "R(%llu)",
        (unsigned long long)n);
  if (!n) return;
  std::vector<uint8_t> area(pad, 0xEE), hits(pad, 0);
  Lds s;
  const uint64_t blocks = frame_finish_blocks(n);
  for (uint64_t b = 0; b < blocks; ++b) {
    s.clear();
    for (uint32_t t = 0; t < kFrameBlock; ++t) {
      for (uint32_t j = 0; j < kFrameWord; ++j) {
        const uint32_t i = frame_local(t, j);
        const uint64_t src = frame_finish_src(n, b, i);
        CHECK(src <= n, "finish reads offsets[%llu], n %llu", (unsigned long long)src, (unsigned long long)n);
        s.put(frame_slot(i), static_cast<uint32_t>(offsets[src <= n ? src : n]));
      }
      if (t == 0) {
        const uint64_t src = frame_finish_src(n, b, kFrameElems);
        CHECK(src <= n, "finish reads offsets[%llu], n %llu", (unsigned long long)src, (unsigned long long)n);
        s.put(frame_slot(kFrameElems), static_cast<uint32_t>(offsets[src <= n ? src : n]));
      }
    }
    for (uint32_t t = 0; t < kFrameBlock; ++t) {
      uint64_t pos;
      if (!frame_finish_store(n, b, t, &pos)) continue;
      CHECK(pos % 16 == 0 && pos + 16 <= pad, "finish stores at %llu, pad %llu", (unsigned long long)pos,
            (unsigned long long)pad);
      if (pos + 16 > pad) continue;
      for (uint32_t j = 0; j < kFrameWord; ++j) {
        const uint32_t v = s.get(frame_slot(kFrameWord * t + j + 1)) - s.get(frame_slot(kFrameWord * t + j));
        area[pos + j] = static_cast<uint8_t>(v);
        ++hits[pos + j];
      }
    }
  }
  for (uint64_t i = 0; i < pad; ++i) {
    CHECK(hits[i] == 1, "length byte %llu of n %llu written %d times", (unsigned long long)i, (unsigned long long)n,
          hits[i]);
    CHECK(area[i] == (i < n ? lens[i] : 0), "length byte %llu of n %llu is %u", (unsigned long long)i,
          (unsigned long long)n, area[i]);
  }
}

// load_lens: the thread's 16 lengths as bytes, pad bytes cleared
bool model_load(uint64_t n, uint64_t b, uint32_t t, const std::vector<uint8_t>& area, uint8_t out[16]) {
  for (int i = 0; i < 16; ++i) out[i] = 0;
  uint64_t pos;
  uint32_t live = 0;
  if (!frame_open_load(n, b, t, &pos, &live)) return false;
  CHECK(pos % 16 == 0 && pos + 16 <= area.size(), "open loads at %llu of %zu", (unsigned long long)pos, area.size());
  CHECK(live >= 1 && live <= 16 && pos + live <= n && (live == 16 || pos + live == n), "live %u at %llu, n %llu", live,
        (unsigned long long)pos, (unsigned long long)n);
  if (pos + 16 > area.size()) return false;
  for (uint32_t i = 0; i < live && i < 16; ++i) out[i] = area[pos + i];
  return true;
}

// frame_scan_kernel over one frame's totals, in place; returns the grand total
uint64_t replay_scan(std::vector<uint64_t>& tot) {
  const uint64_t nb = tot.size();
  std::vector<uint8_t> hits(nb, 0);
  uint64_t carry = 0, seen = 0;
  const uint64_t passes = frame_scan_passes(nb);
  for (uint64_t p = 0; p < passes; ++p) {
    const uint64_t base = p * kFrameScanStage;
    const uint32_t m = frame_scan_count(nb, p);
    CHECK(m >= 1 && m <= kFrameScanStage && base + m <= nb, "pass %llu takes %u of %llu", (unsigned long long)p, m,
          (unsigned long long)nb);
    seen += m;
    std::vector<uint32_t> staged(m);
    for (uint32_t t = 0; t < kFrameScanThreads; ++t)
      for (uint32_t i = t; i < m; i += kFrameScanThreads) staged[i] = static_cast<uint32_t>(tot[base + i]);
    uint64_t run = carry;  // threads in order: what the cross-thread scan hands thread t
    for (uint32_t t = 0; t < kFrameScanThreads; ++t) {
      for (uint32_t j = 0; j < kFrameScanRun; ++j) {
        const uint32_t i = kFrameScanRun * t + j;
        if (i < m) {
          ++hits[base + i];
          tot[base + i] = run;
          run += staged[i];
        }
      }
    }
    carry = run;
  }
  CHECK(seen == nb, "the passes take %llu of %llu totals", (unsigned long long)seen, (unsigned long long)nb);
  for (uint64_t i = 0; i < nb; ++i) CHECK(hits[i] == 1, "total %llu written %d times", (unsigned long long)i, hits[i]);
  return carry;
}

// the three open launches; cap = frame_bytes - R(n)
void replay_open(uint64_t n, const std::vector<uint8_t>& lens, uint64_t cap) {
  const uint64_t pad = frame_pad16(n);
  std::vector<uint8_t> area(pad, 0xFF);  // the pad is not trusted
  for (uint64_t i = 0; i < n; ++i) area[i] = lens[i];
  const uint64_t nb = frame_open_blocks(n);
  CHECK(nb * kFrameElems > n && (nb - 1) * kFrameElems <= n, "open blocks %llu for n %llu", (unsigned long long)nb,
        (unsigned long long)n);
  std::vector<uint64_t> tot(nb, ~0ull);
  for (uint64_t b = 0; b < nb; ++b) {
    uint64_t sum = 0;
    for (uint32_t t = 0; t < kFrameBlock; ++t) {
      uint8_t q[16];
      model_load(n, b, t, area, q);
      for (int i = 0; i < 16; ++i) sum += q[i];
    }
    CHECK(sum < (1ull << 32), "block total %llu", (unsigned long long)sum);
    tot[b] = sum;
  }
  uint64_t want_total = 0;
  for (uint64_t i = 0; i < n; ++i) want_total += lens[i];
  const uint64_t total = replay_scan(tot);
  CHECK(total == want_total, "scan total %llu, lengths sum to %llu", (unsigned long long)total,
        (unsigned long long)want_total);
  std::vector<uint64_t> off(n + 1, ~0ull);
  std::vector<uint8_t> hits(n + 1, 0);
  Lds s;
  for (uint64_t b = 0; b < nb; ++b) {
    s.clear();
    uint32_t run = 0;  // threads in order: what the in-block scan hands thread t
    for (uint32_t t = 0; t < kFrameBlock; ++t) {
      uint8_t q[16];
      model_load(n, b, t, area, q);
      for (uint32_t i = 0; i < kFrameWord; ++i) {
        s.put(frame_slot(kFrameWord * t + i), run);
        run += q[i];
      }
    }
    for (uint32_t t = 0; t < kFrameBlock; ++t) {
      for (uint32_t j = 0; j < kFrameWord; ++j) {
        uint64_t e;
        if (!frame_open_store(n, b, t, j, &e)) continue;
        CHECK(e <= n, "open stores offsets[%llu], n %llu", (unsigned long long)e, (unsigned long long)n);
        if (e > n) continue;
        const uint64_t v = tot[b] + s.get(frame_slot(frame_local(t, j)));
        off[e] = v < cap ? v : cap;
        ++hits[e];
      }
    }
  }
  uint64_t prefix = 0;
  for (uint64_t e = 0; e <= n; ++e) {
    CHECK(hits[e] == 1, "offsets[%llu] of n %llu written %d times", (unsigned long long)e, (unsigned long long)n,
          hits[e]);
    const uint64_t want = prefix < cap ? prefix : cap;
    CHECK(off[e] == want, "offsets[%llu] of n %llu is %llu, want %llu", (unsigned long long)e, (unsigned long long)n,
          (unsigned long long)off[e], (unsigned long long)want);
    if (e < n) prefix += lens[e];
  }
}

void run_case(uint64_t n, std::mt19937_64& rng, int mode) {
  std::vector<uint8_t> lens(n);
  for (auto& l : lens) {
    const uint64_t r = rng();
    l = mode == 1 ? 255 : (r % 16 == 0 ? 0 : (r % 16 == 1 ? 255 : static_cast<uint8_t>(r >> 8)));
  }
  std::vector<uint64_t> offsets(n + 1);
  // a base beyond 32 bits: the finish kernel reads low dwords only
  uint64_t o = mode == 2 ? 0xFFFFFFF0ull : 0;
  const uint64_t first = o;
  for (uint64_t e = 0; e < n; ++e) {
    offsets[e] = o;
    o += lens[e];
  }
  offsets[n] = o;
  const uint64_t total = o - first;
  replay_finish(n, offsets, lens);
  replay_open(n, lens, total);
  if (mode == 0) {
    replay_open(n, lens, total / 2);
    replay_open(n, lens, total + 7);
  }
}

}  // namespace

int main() {
  static_assert(kFrameElems == 4096 && kFrameLdsWords == frame_slot(kFrameElems) + 1, "geometry");
  std::mt19937_64 rng(20261020);
  const uint64_t B = kFrameElems;
  const uint64_t edges[] = {0,     1,     15,    16,        17,         63, 64, 65, 255, 256, 257, B - 1, B, B + 1,
                            2 * B, 3 * B, 3 * B + 17, static_cast<uint64_t>(kFrameScanThreads) * B - 1,
                            static_cast<uint64_t>(kFrameScanThreads) * B,
                            static_cast<uint64_t>(kFrameScanThreads) * B + 1};
  for (uint64_t n : edges)
    for (int mode = 0; mode < 3; ++mode) {
      if (n > 4 * B && mode == 2) continue;
      run_case(n, rng, mode);
    }
  // the scan's second pass: one block total more than a pass stages (all lengths 255, one open)
  run_case(static_cast<uint64_t>(kFrameScanStage) * B, rng, 1);
  for (int it = 0; it < 1000; ++it) run_case(rng() % (3 * B + 100), rng, 0);
  // the scan alone where its load loop and its passes turn over
  const uint64_t S = kFrameScanStage, T = kFrameScanThreads;
  const uint64_t counts[] = {1, 7, 8, 9, T - 1, T, T + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 5};
  for (uint64_t nb : counts) {
    std::vector<uint64_t> tot(nb), want(nb);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < nb; ++i) {
      tot[i] = rng() % (static_cast<uint64_t>(B) * 255 + 1);
      want[i] = sum;
      sum += tot[i];
    }
    const uint64_t got = replay_scan(tot);
    CHECK(got == sum, "scan of %llu totals", (unsigned long long)nb);
    for (uint64_t i = 0; i < nb; ++i)
      CHECK(tot[i] == want[i], "scanned total %llu of %llu", (unsigned long long)i, (unsigned long long)nb);
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
