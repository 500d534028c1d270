// many_plan_check.cpp — the segmented emission's store plan (csrc/seg_plan.hpp)
// against a per-element map, on the host.
//
// For a list of tensor sizes the program builds the segment table as
// dn_mt19937_split_many_device builds it (empty tensors dropped, a sentinel at
// n_total) and walks every emission group the way emit_split_seg does: the
// cursor found by seg_find or stepped by seg_step (upwards and downwards), the
// single-tile case where seg_single_tile says so, else one seg_piece per
// intersecting segment.  Every store a lane would make is checked:
//   * each element below n_total is stored exactly once per group walk;
//   * it lands in its own segment, at the tile and word of its local index;
//   * the lane ranges of a group's pieces are disjoint;
//   * every descriptor lies inside its row, every store inside its descriptor.
// Inputs: the ragged list of tests/test_gpu_many.py and 1000 seeded random
// tables with sizes 0..700.  Exit status 0 and "ok" when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "seg_plan.hpp"

using namespace dn;

namespace {

uint64_t vec_bytes(uint64_t n) { return (n + kSegTile - 1) / kSegTile * kSegTileBytes; }

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (failures++ < 20) {                   \
        std::fprintf(stderr, "FAIL %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);     \
        std::fprintf(stderr, "\n");            \
      }                                        \
    }                                          \
  } while (0)

struct Store {
  uint32_t count;  // stores seen for the element (the fields below: the last one)
  uint32_t seg;
  uint64_t off32, off16;  // byte offsets in the row of limb 0 and of the 16-bit top limb
};

// one lane's store through a descriptor at row offset `base`, `range` bytes long
void lane_store(std::vector<Store>& got, uint64_t e, uint32_t seg, uint64_t row_bytes, uint64_t base,
                uint32_t range, uint32_t o4, uint32_t o2) {
  CHECK(base + range <= row_bytes, "descriptor [%llu, +%u) past the row's %llu bytes",
        static_cast<unsigned long long>(base), range, static_cast<unsigned long long>(row_bytes));
  CHECK(o4 % 4u == 0 && o2 % 2u == 0, "misaligned offsets %u %u", o4, o2);
  // limb i < 16 at o4 + i * 4 * 256 (4 bytes), the top limb at o2 + 64 * 256 (2 bytes)
  CHECK(o4 + 15u * 4u * kSegTile + 4u <= range, "limb 15 of element %llu outside its descriptor",
        static_cast<unsigned long long>(e));
  CHECK(o2 + 64u * kSegTile + 2u <= range, "top limb of element %llu outside its descriptor",
        static_cast<unsigned long long>(e));
  got[e] = Store{got[e].count + 1u, seg, base + o4, base + o2 + 64u * kSegTile};
}

// the stores of group [ebase, ebase + 64) with the cursor already on ebase's segment
void emit_group(const std::vector<SegEnt>& t, uint32_t seg, uint64_t ebase, uint64_t n_total,
                std::vector<Store>& got) {
  const SegEnt& sg = t[seg];
  CHECK(sg.e_begin <= ebase && ebase < t[seg + 1].e_begin, "cursor %u does not hold element %llu", seg,
        static_cast<unsigned long long>(ebase));
  if (seg_single_tile(sg.e_begin, t[seg + 1].e_begin, ebase, n_total)) {
    const uint64_t l0 = ebase - sg.e_begin;
    const uint64_t tile = l0 >> 8;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      if (ebase + lane >= n_total) continue;
      const uint32_t wl = (static_cast<uint32_t>(l0) & 255u) + lane;
      CHECK(wl < kSegTile, "single-tile word %u", wl);
      const uint64_t left = sg.row_bytes - tile * kSegTileBytes;
      CHECK(left >= kSegTileBytes, "tile %llu past the row", static_cast<unsigned long long>(tile));
      lane_store(got, ebase + lane, seg, sg.row_bytes, tile * kSegTileBytes, kSegTileBytes, wl * 4u, wl * 2u);
    }
    return;
  }
  const uint64_t gend = n_total - ebase < 64u ? n_total : ebase + 64u;
  uint64_t lanes_seen = 0;
  for (uint32_t k = seg; t[k].e_begin < gend; ++k) {
    CHECK(k + 1 < t.size(), "piece loop ran past the sentinel");
    const SegPiece p = seg_piece(t[k].e_begin, t[k + 1].e_begin, t[k].row_bytes, ebase, n_total);
    CHECK(p.lane_lo < p.lane_hi && p.lane_hi <= 64u, "lanes [%u, %u)", p.lane_lo, p.lane_hi);
    CHECK(p.w0 < kSegTile, "w0 %u", p.w0);
    for (uint32_t lane = p.lane_lo; lane < p.lane_hi && lane < 64u; ++lane) {
      CHECK(!(lanes_seen >> lane & 1u), "lane %u in two pieces", lane);
      lanes_seen |= 1ull << lane;
      const uint32_t w = p.w0 + lane - p.lane_lo;
      lane_store(got, ebase + lane, k, t[k].row_bytes, p.tile0 * kSegTileBytes, p.range, seg_voff32(w), seg_voff16(w));
    }
  }
}

void check_list(const std::vector<uint64_t>& sizes) {
  std::vector<SegEnt> t;
  uint64_t e = 0;
  for (uint64_t n : sizes) {
    if (!n) continue;
    t.push_back(SegEnt{e, nullptr, vec_bytes(n)});
    e += n;
  }
  const uint64_t n_total = e;
  t.push_back(SegEnt{n_total, nullptr, 0});
  const uint32_t nseg = static_cast<uint32_t>(t.size() - 1);
  if (!n_total) return;
  // the brute-force map: element -> (segment, local index)
  std::vector<uint32_t> seg_of(n_total);
  for (uint32_t k = 0; k < nseg; ++k)
    for (uint64_t x = t[k].e_begin; x < t[k + 1].e_begin; ++x) seg_of[x] = k;
  const uint64_t ngroups = (n_total + 63) / 64;
  // three walks: a fresh search per group, the cursor stepped upwards, stepped downwards
  for (int walk = 0; walk < 3; ++walk) {
    std::vector<Store> got(n_total, Store{0u, 0u, 0u, 0u});
    uint32_t cur = walk == 2 ? seg_find(t.data(), nseg, 64 * (ngroups - 1)) : 0u;
    for (uint64_t i = 0; i < ngroups; ++i) {
      const uint64_t g = walk == 2 ? ngroups - 1 - i : i;
      const uint64_t ebase = 64 * g;
      const uint32_t found = seg_find(t.data(), nseg, ebase);
      CHECK(found == seg_of[ebase], "seg_find(%llu) = %u, not %u", static_cast<unsigned long long>(ebase), found,
            seg_of[ebase]);
      if (walk == 0) cur = found;
      else cur = seg_step(t.data(), cur, ebase);
      CHECK(cur == seg_of[ebase], "seg_step to %llu = %u, not %u", static_cast<unsigned long long>(ebase), cur,
            seg_of[ebase]);
      if (cur != seg_of[ebase]) return;
      emit_group(t, cur, ebase, n_total, got);
    }
    for (uint64_t x = 0; x < n_total; ++x) {
      CHECK(got[x].count == 1u, "element %llu stored %u times", static_cast<unsigned long long>(x), got[x].count);
      if (got[x].count != 1u) continue;
      const uint32_t k = seg_of[x];
      const uint64_t l = x - t[k].e_begin;
      const uint64_t tile = l / kSegTile, w = l % kSegTile;
      const Store& s = got[x];
      CHECK(s.seg == k, "element %llu in segment %u, not %u", static_cast<unsigned long long>(x), s.seg, k);
      CHECK(s.off32 == tile * kSegTileBytes + w * 4, "element %llu limb 0 at %llu", static_cast<unsigned long long>(x),
            static_cast<unsigned long long>(s.off32));
      CHECK(s.off16 == tile * kSegTileBytes + 64u * kSegTile + w * 2, "element %llu top limb at %llu",
            static_cast<unsigned long long>(x), static_cast<unsigned long long>(s.off16));
    }
  }
}

}  // namespace

int main() {
  const std::vector<uint64_t> list_a = {1, 63, 64, 65, 0, 127, 128, 1, 1, 1, 300, 257, 256, 1000, 4097, 2500};
  check_list(list_a);
  check_list({64, 192, 256, 320, 1024, 4096, 2048, 832});
  check_list(std::vector<uint64_t>(200, 1));  // groups of 64 one-element tensors
  std::mt19937 rng(20240607u);
  for (int it = 0; it < 1000; ++it) {
    const uint32_t cnt = 1u + rng() % 40u;
    std::vector<uint64_t> sizes(cnt);
    for (auto& n : sizes) {
      const uint32_t r = rng();
      // sizes 0..700, with small ones and multiples of 64 over-represented
      n = (r >> 28) < 4u ? (r % 5u) : (r >> 28) < 8u ? 64u * (r % 11u) : r % 701u;
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
