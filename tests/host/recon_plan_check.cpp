// recon_plan_check.cpp — the segmented reconstruct's tile plan
// (csrc/recon_plan.hpp) against a per-element map, on the host.
//
// For a list of tensor sizes the program builds the table as
// dn_m521_reconstruct_many builds it (empty tensors dropped, a sentinel at the
// total tile count) and walks the global tile range the way
// reconstruct_many_kernel does, for every wave of several grids in each
// wave-sched mode (cyclic, blocked, and the coop mode's single quarters): one
// recon_seg_find for the wave's first tile, recon_seg_step after that, then per
// quarter either the load-ahead path (all four quarters of a full tile,
// unguarded) or the guarded one (recon_live, stopping at the first dead
// quarter).  Checked:
//   * the cursor equals a fresh binary search and the brute-force owner;
//   * every element of every tensor is visited exactly once, at its own
//     (segment, local tile, word): share-row / tiled-output byte offset inside
//     vec_bytes(n), int64 index == the element's own index;
//   * no lane at or past n is visited, and the unguarded path runs on full
//     tiles only.
// Inputs: the ragged list of tests/test_gpu_resolve_many.py and 1000 seeded
// random tables with sizes 0..700.  Exit status 0 and "ok" when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "recon_plan.hpp"

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

struct Table {
  std::vector<ReconSegEnt> ent;        // nseg entries and the sentinel
  std::vector<uint32_t> owner;         // global tile -> segment (brute force)
  std::vector<std::vector<uint32_t>> visits;  // per segment, per element
  uint32_t nseg = 0, ntiles = 0;
};

Table build(const std::vector<uint64_t>& sizes) {
  Table t;
  uint32_t tiles = 0;
  for (uint64_t n : sizes) {
    if (!n) continue;
    t.ent.push_back(ReconSegEnt{tiles, 0u, n, nullptr, nullptr, nullptr});
    const uint32_t nt = static_cast<uint32_t>((n + kSegTile - 1) / kSegTile);
    for (uint32_t i = 0; i < nt; ++i) t.owner.push_back(t.nseg);
    t.visits.emplace_back(n, 0u);
    tiles += nt;
    ++t.nseg;
  }
  t.ntiles = tiles;
  t.ent.push_back(ReconSegEnt{tiles, 0u, 0u, nullptr, nullptr, nullptr});
  return t;
}

// one lane's work on word w of local tile lt of segment s
void visit(Table& t, uint32_t s, uint32_t lt, uint32_t w) {
  const uint64_t n = t.ent[s].n_elem;
  const uint64_t e = recon_elem(lt, w);
  CHECK(w < kSegTile, "word %u", w);
  CHECK(e < n, "segment %u: lane at element %llu of %llu", s, static_cast<unsigned long long>(e),
        static_cast<unsigned long long>(n));
  if (e >= n) return;
  // limb i < 16 at tile offset + i * 4 * 256 + 4 w, the top limb at + 64 * 256 + 2 w
  const uint64_t off = recon_tile_offset(lt);
  CHECK(off % kSegTileBytes == 0 && off + kSegTileBytes <= vec_bytes(n), "segment %u: tile %u at byte %llu of %llu", s,
        lt, static_cast<unsigned long long>(off), static_cast<unsigned long long>(vec_bytes(n)));
  CHECK(off / kSegTileBytes == e / kSegTile && w == e % kSegTile, "segment %u: element %llu at tile %llu word %u", s,
        static_cast<unsigned long long>(e), static_cast<unsigned long long>(off / kSegTileBytes), w);
  ++t.visits[s][e];
}

// the tiles first, first + step, ... < end of one wave, quarters [q0, q1)
void walk_wave(Table& t, uint32_t first, uint32_t step, uint32_t end, uint32_t q0, uint32_t q1) {
  if (first >= end) return;
  uint32_t seg = recon_seg_find(t.ent.data(), t.nseg, first);
  for (uint32_t tile = first; tile < end; tile += step) {
    seg = recon_seg_step(t.ent.data(), seg, tile);
    const uint32_t found = recon_seg_find(t.ent.data(), t.nseg, tile);
    CHECK(seg == found && seg == t.owner[tile], "tile %u: cursor %u, search %u, owner %u", tile, seg, found,
          t.owner[tile]);
    if (seg != t.owner[tile]) return;
    const ReconSegEnt& e = t.ent[seg];
    CHECK(e.tile_begin <= tile && tile < t.ent[seg + 1].tile_begin, "tile %u outside segment %u", tile, seg);
    const uint32_t lt = tile - e.tile_begin;
    if (q0 == 0u && q1 == 4u && recon_tile_full(e.n_elem, lt)) {  // the load-ahead path: no guard
      CHECK(recon_elem(lt, kSegTile - 1u) < e.n_elem, "tile %u of segment %u called full", lt, seg);
      for (uint32_t q = 0; q < 4u; ++q)
        for (uint32_t lane = 0; lane < 64u; ++lane) visit(t, seg, lt, lane + 64u * q);
      continue;
    }
    for (uint32_t q = q0; q < q1; ++q) {
      bool any_dead = false;
      for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t w = lane + 64u * q;
        if (recon_live(e.n_elem, lt, w)) visit(t, seg, lt, w);
        else any_dead = true;
      }
      // (the kernel's lanes leave the quarter loop one by one; a dead lane's
      // later quarters are dead too, so stopping here visits the same set)
      if (any_dead) {
        for (uint32_t q2 = q + 1; q2 < 4u; ++q2)
          CHECK(!recon_live(e.n_elem, lt, 64u * q2), "tile %u of segment %u: live quarter %u after a dead lane", lt,
                seg, q2);
      }
    }
  }
}

void expect_each_once(Table& t, const char* what) {
  for (uint32_t s = 0; s < t.nseg; ++s)
    for (uint64_t e = 0; e < t.visits[s].size(); ++e) {
      CHECK(t.visits[s][e] == 1u, "%s: element %llu of segment %u visited %u times", what,
            static_cast<unsigned long long>(e), s, t.visits[s][e]);
      t.visits[s][e] = 0u;
    }
}

void check_list(const std::vector<uint64_t>& sizes) {
  Table t = build(sizes);
  if (!t.ntiles) return;
  // every global tile on its own: a fresh search, all four quarters
  for (uint32_t tile = 0; tile < t.ntiles; ++tile) walk_wave(t, tile, 1u, tile + 1u, 0u, 4u);
  expect_each_once(t, "tile by tile");
  for (uint32_t waves : {1u, 4u, 12u, 52u}) {
    // cyclic (modes 0 and 1 differ only in which wave takes which start)
    for (uint32_t w = 0; w < waves; ++w) walk_wave(t, w, waves, t.ntiles, 0u, 4u);
    expect_each_once(t, "cyclic");
    // blocked
    const uint32_t per = (t.ntiles + waves - 1u) / waves;
    for (uint32_t w = 0; w < waves; ++w) {
      const uint32_t first = w * per;
      walk_wave(t, first, 1u, first + per < t.ntiles ? first + per : t.ntiles, 0u, 4u);
    }
    expect_each_once(t, "blocked");
    // coop: workgroup b strides by the grid, its wave i takes quarter i
    for (uint32_t b = 0; b < waves; ++b)
      for (uint32_t q = 0; q < 4u; ++q) walk_wave(t, b, waves, t.ntiles, q, q + 1u);
    expect_each_once(t, "coop");
  }
}

}  // namespace

int main() {
  check_list({1, 63, 64, 65, 0, 127, 128, 255, 256, 257, 1, 1, 300, 512, 1000, 4097, 2500});
  check_list({256, 512, 768, 256});
  check_list(std::vector<uint64_t>(200, 1));
  std::mt19937 rng(20240608u);
  for (int it = 0; it < 1000; ++it) {
    const uint32_t cnt = 1u + rng() % 40u;
    std::vector<uint64_t> sizes(cnt);
    for (auto& n : sizes) {
      const uint32_t r = rng();
      // sizes 0..700, with small ones and multiples of 256 over-represented
      n = (r >> 28) < 4u ? (r % 5u) : (r >> 28) < 8u ? 256u * (r % 3u) + (r >> 8) % 2u : r % 701u;
    }
    check_list(sizes);
  }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
