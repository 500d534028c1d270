// enc_plan_check.cpp — the segmented share encode's plan (csrc/enc_plan.hpp)
// against a per-element map, and a CPU model of its three launches, on the host.
//
// For a list of tensor sizes the program builds the table as
// dn_m521_encode_shares_many builds it (empty tensors dropped, a sentinel at
// the total tile count and n_total), gives every element a record length
// (header + 0..66 bytes, seeded), and runs what the kernels of
// csrc/codec_many.hip do with (table, global tile):
//   launch 1  one wave per tile, lane j words 4 j .. 4 j + 3: the tile's bytes;
//   launch 2  exclusive scan of the tile totals;
//   launch 3  one workgroup per tile, thread = word: in-tile prefix (wave scan,
//             then across the 4 waves), offsets[] at the global element index,
//             each wave's byte range [A, B) written as head bytes, aligned
//             body and tail bytes — for 4-byte and for 16-byte bodies.
// Checked:
//   * the binary search equals the brute-force owner, and the cursor
//     (recon_seg_step over increasing tiles) equals the binary search;
//   * every global element is visited exactly once, at its own (segment, local
//     tile, word) and its own global index; the tile lies inside the row;
//   * no word at or past n_k is live (and enc_tile's live count says the same);
//   * offsets[] equals the running sum of the lengths, offsets[n_total] is
//     written once, by the list's last element, and equals the scan's total;
//   * the byte ranges assigned to the tiles' waves are disjoint and tile
//     [0, total) exactly: every byte written exactly once, none outside.
// Inputs: the ragged list of tests/test_gpu_encode_many.py and 1000 seeded
// random tables with sizes 0..700.  Exit status 0 and "ok" when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "enc_plan.hpp"

using namespace dn;

namespace {

uint64_t vec_bytes(uint64_t n) { return (n + kSegTile - 1) / kSegTile * kSegTileBytes; }

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

typedef unsigned long long ull;

struct Table {
  std::vector<EncSegEnt> ent;              // nseg entries and the sentinel
  std::vector<uint32_t> owner;             // global tile -> segment (brute force)
  std::vector<std::vector<uint32_t>> len;  // per segment, per element: record bytes
  std::vector<uint64_t> first;             // per segment: its first global element (brute force)
  uint32_t nseg = 0, ntiles = 0;
  uint64_t n_total = 0;
};

Table build(const std::vector<uint64_t>& sizes, std::mt19937& rng, uint32_t xlen) {
  Table t;
  for (uint64_t n : sizes) {
    if (!n) continue;
    t.ent.push_back(EncSegEnt{t.ntiles, 0u, t.n_total, n, nullptr, vec_bytes(n)});
    const uint32_t nt = static_cast<uint32_t>((n + kSegTile - 1) / kSegTile);
    for (uint32_t i = 0; i < nt; ++i) t.owner.push_back(t.nseg);
    std::vector<uint32_t> l(n);
    for (auto& v : l) {
      const uint32_t r = rng();
      // mostly 65 / 66 bytes (a random field element), some short and empty ones
      v = 1u + xlen + ((r & 7u) ? 66u - ((r >> 3) & 1u) : (r >> 4) % 67u);
    }
    t.len.push_back(l);
    t.first.push_back(t.n_total);
    t.ntiles += nt;
    t.n_total += n;
    ++t.nseg;
  }
  t.ent.push_back(EncSegEnt{t.ntiles, 0u, t.n_total, 0u, nullptr, 0u});
  return t;
}

void check_list(const std::vector<uint64_t>& sizes, std::mt19937& rng, uint32_t xlen, uint32_t row) {
  Table t = build(sizes, rng, xlen);
  if (!t.ntiles) return;
  const EncSegEnt* tab = t.ent.data();
  CHECK(enc_n_total(tab, t.nseg) == t.n_total, "n_total");

  // launch 1: tile totals (and the search / cursor checks)
  std::vector<uint64_t> tot(t.ntiles);
  uint32_t cur = 0;
  for (uint32_t g = 0; g < t.ntiles; ++g) {
    const uint32_t s = recon_seg_find(tab, t.nseg, g);
    cur = recon_seg_step(tab, cur, g);
    CHECK(s == t.owner[g] && cur == s, "tile %u: search %u, cursor %u, owner %u", g, s, cur, t.owner[g]);
    if (s != t.owner[g]) return;
    const EncTile tl = enc_tile(tab, t.nseg, s, g, row);
    const uint64_t n = tab[s].n_elem;
    CHECK(tl.row_byte >= row * tab[s].pitch && tl.row_byte + kSegTileBytes <= row * tab[s].pitch + vec_bytes(n),
          "tile %u: bytes from %llu outside row %u of segment %u", g, (ull)tl.row_byte, row, s);
    CHECK((tl.row_byte - row * tab[s].pitch) / kSegTileBytes == tl.lt, "tile %u: local tile %u", g, tl.lt);
    uint64_t sum = 0;
    uint32_t live = 0;
    for (uint32_t lane = 0; lane < 64u; ++lane)
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t w = 4u * lane + j;
        if (!recon_live(n, tl.lt, w)) continue;
        const uint64_t e = recon_elem(tl.lt, w);
        CHECK(e < n, "tile %u word %u: element %llu of %llu", g, w, (ull)e, (ull)n);
        if (e >= n) return;
        sum += t.len[s][e];
        ++live;
      }
    CHECK(live == tl.live && live >= 1u, "tile %u: %u live words, enc_tile says %u", g, live, tl.live);
    tot[g] = sum;
  }

  // launch 2: exclusive scan
  std::vector<uint64_t> pre(t.ntiles);
  uint64_t total = 0;
  for (uint32_t g = 0; g < t.ntiles; ++g) {
    pre[g] = total;
    total += tot[g];
  }

  // launch 3
  std::vector<uint32_t> visits(t.n_total, 0u);
  std::vector<uint64_t> offsets(t.n_total + 1, ~0ull);
  uint32_t end_writes = 0;
  std::vector<uint8_t> written4(total, 0u), written16(total, 0u);
  for (uint32_t g = 0; g < t.ntiles; ++g) {
    const uint32_t s = recon_seg_find(tab, t.nseg, g);
    const EncTile tl = enc_tile(tab, t.nseg, s, g, row);
    const uint64_t n = tab[s].n_elem;
    uint32_t len[256], inc[256], wsum[4] = {0u, 0u, 0u, 0u};
    bool valid[256];
    for (uint32_t th = 0; th < 256u; ++th) {
      valid[th] = recon_live(n, tl.lt, th);
      CHECK(valid[th] == (th < tl.live), "tile %u word %u: live %d, live count %u", g, th, (int)valid[th], tl.live);
      len[th] = valid[th] ? t.len[s][recon_elem(tl.lt, th)] : 0u;
    }
    for (uint32_t wv = 0; wv < 4u; ++wv) {  // the wave's inclusive scan; lane 63 holds the wave's sum
      uint32_t run = 0;
      for (uint32_t lane = 0; lane < 64u; ++lane) inc[64u * wv + lane] = run += len[64u * wv + lane];
      wsum[wv] = run;
    }
    for (uint32_t wv = 0; wv < 4u; ++wv) {
      uint32_t wbase = 0;
      for (uint32_t w = 0; w < wv; ++w) wbase += wsum[w];
      uint64_t A = 0, B = 0;
      bool any = false;
      for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t th = 64u * wv + lane;
        if (!valid[th]) continue;
        const uint64_t off = pre[g] + wbase + inc[th] - len[th];
        const uint64_t e = tl.e0 + th;  // the global element index
        CHECK(e == t.first[s] + recon_elem(tl.lt, th) && e < t.n_total, "tile %u word %u: global element %llu", g, th,
              (ull)e);
        if (e >= t.n_total) return;
        ++visits[e];
        offsets[e] = off;
        if (tl.ends_list && th + 1u == tl.live) {
          CHECK(e + 1u == t.n_total, "tile %u word %u ends the list at element %llu of %llu", g, th, (ull)e,
                (ull)t.n_total);
          offsets[e + 1u] = off + len[th];
          ++end_writes;
        }
        if (!any) {
          CHECK(lane == 0u, "tile %u wave %u: first live lane %u", g, wv, lane);
          A = off;
          any = true;
        }
        B = off + len[th];
      }
      if (!any) continue;  // the wave returns (behind the barrier)
      CHECK(A < B && B <= total, "tile %u wave %u: range [%llu, %llu) of %llu", g, wv, (ull)A, (ull)B, (ull)total);
      if (B > total) return;
      // head [A, a4), aligned body [a4, b4), tail [b4, B); or the byte path
      for (uint64_t al : {4ull, 16ull}) {
        std::vector<uint8_t>& wr = al == 4u ? written4 : written16;
        const uint64_t a4 = (A + al - 1) & ~(al - 1), b4 = B & ~(al - 1);
        if (a4 > b4) {
          for (uint64_t q = A; q < B; ++q) ++wr[q];
          continue;
        }
        CHECK(a4 - A < 64u && B - b4 < 64u, "tile %u wave %u: head / tail wider than a wave", g, wv);
        for (uint64_t q = A; q < a4; ++q) ++wr[q];
        for (uint64_t q = b4; q < B; ++q) ++wr[q];
        CHECK((b4 - a4) % al == 0u && a4 >= A && b4 <= B, "tile %u wave %u: body [%llu, %llu)", g, wv, (ull)a4, (ull)b4);
        for (uint64_t q = a4; q < b4; ++q) ++wr[q];
      }
    }
  }
  uint64_t run = 0;
  for (uint32_t s = 0; s < t.nseg; ++s)
    for (uint64_t e = 0; e < t.len[s].size(); ++e) {
      const uint64_t ge = t.first[s] + e;
      CHECK(visits[ge] == 1u, "element %llu of segment %u visited %u times", (ull)e, s, visits[ge]);
      CHECK(offsets[ge] == run, "element %llu of segment %u at byte %llu, not %llu", (ull)e, s, (ull)offsets[ge],
            (ull)run);
      run += t.len[s][e];
    }
  CHECK(run == total && end_writes == 1u && offsets[t.n_total] == total, "total %llu, scan %llu, %u writes of the end",
        (ull)run, (ull)total, end_writes);
  for (uint64_t q = 0; q < total; ++q)
    CHECK(written4[q] == 1u && written16[q] == 1u, "byte %llu written %u / %u times", (ull)q, written4[q], written16[q]);
}

}  // namespace

int main() {
  std::mt19937 rng(20240611u);
  const std::vector<uint64_t> list_a = {1, 63, 64, 65, 0, 127, 128, 1, 1, 1, 300, 257, 256, 1000, 4097, 2500};
  for (uint32_t xlen : {0u, 1u, 2u, 6u, 8u})
    for (uint32_t row : {0u, 4u, 16u}) check_list(list_a, rng, xlen, row);
  check_list({64, 192, 256, 320, 1024, 4096, 2048, 832}, rng, 1u, 2u);
  check_list({256, 512, 768, 256}, rng, 1u, 0u);
  check_list(std::vector<uint64_t>(200, 1), rng, 1u, 1u);
  for (int it = 0; it < 1000; ++it) {
    const uint32_t cnt = 1u + rng() % 40u;
    std::vector<uint64_t> sizes(cnt);
    for (auto& n : sizes) {
      const uint32_t r = rng();
      // sizes 0..700, with small ones and multiples of 256 over-represented
      n = (r >> 28) < 4u ? (r % 5u) : (r >> 28) < 8u ? 256u * (r % 3u) + (r >> 8) % 2u : r % 701u;
    }
    check_list(sizes, rng, rng() % 9u, rng() % 5u);
  }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
