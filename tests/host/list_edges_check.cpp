// list_edges_check.cpp — the lists of tests/list_edges.py through the segmented
// emission's store plan (csrc/seg_plan.hpp), walked the way the generation
// kernels walk it: substream by substream, the cursor found once per substream
// with seg_find on the first group emitted (the TOP group of a backward
// substream) and moved with seg_step from group to group — upwards in forward
// substreams, downwards in backward ones.  Every store is checked as
// many_plan_check.cpp checks it (that file's emit_group and per-element map
// are used as they are): each element stored exactly once, in its own segment,
// tile and word, descriptors inside their rows.
//
// Input (argv[1]): one list per line,
//   E S B b_1 .. b_B N n_1 .. n_N
// E elements per substream, S substreams, the B backward ones, N tensor sizes.
// Output: per list "list <i> down <d> up <u>" (the largest cursor step of a
// backward / forward walk, in table entries), then "ok"; exit status 0.
#define main many_plan_check_main
#include "many_plan_check.cpp"
#undef main

#include <fstream>
#include <set>
#include <sstream>
#include <string>

namespace {

void check_substreams(int index, uint64_t E, uint64_t S, const std::set<uint64_t>& backward,
                      const std::vector<uint64_t>& sizes) {
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
  CHECK(n_total > 0 && (n_total + E - 1) / E == S, "list %d: %llu elements are not %llu substreams", index,
        static_cast<unsigned long long>(n_total), static_cast<unsigned long long>(S));
  if (!n_total || (n_total + E - 1) / E != S) return;
  std::vector<Store> got(n_total, Store{0u, 0u, 0u, 0u});
  uint32_t down = 0, up = 0;
  for (uint64_t s = 0; s < S; ++s) {
    const uint64_t qb = s * E;
    const uint64_t nel = n_total - qb < E ? n_total - qb : E;
    const uint64_t ngroups = (nel + 63) / 64;
    const bool back = backward.count(s) != 0;
    CHECK(!back || (nel == E && ngroups % 2 == 0), "backward substream %llu is not whole groups",
          static_cast<unsigned long long>(s));
    uint32_t cur = seg_find(t.data(), nseg, back ? qb + 64 * (ngroups - 1) : qb);
    for (uint64_t i = 0; i < ngroups; ++i) {
      const uint64_t ebase = qb + 64 * (back ? ngroups - 1 - i : i);
      const uint32_t next = seg_step(t.data(), cur, ebase);
      if (back && cur - next > down) down = cur - next;
      if (!back && next - cur > up) up = next - cur;
      CHECK(back ? next <= cur : next >= cur, "cursor moved against substream %llu's direction",
            static_cast<unsigned long long>(s));
      cur = next;
      emit_group(t, cur, ebase, n_total, got);
    }
  }
  for (uint64_t x = 0; x < n_total; ++x) {
    CHECK(got[x].count == 1u, "list %d: element %llu stored %u times", index, static_cast<unsigned long long>(x),
          got[x].count);
    if (got[x].count != 1u) continue;
    const uint32_t k = seg_find(t.data(), nseg, x);
    const uint64_t l = x - t[k].e_begin;
    const uint64_t tile = l / kSegTile, w = l % kSegTile;
    CHECK(got[x].seg == k, "list %d: element %llu in segment %u, not %u", index, static_cast<unsigned long long>(x),
          got[x].seg, k);
    CHECK(got[x].off32 == tile * kSegTileBytes + w * 4, "list %d: element %llu limb 0 at %llu", index,
          static_cast<unsigned long long>(x), static_cast<unsigned long long>(got[x].off32));
    CHECK(got[x].off16 == tile * kSegTileBytes + 64u * kSegTile + w * 2, "list %d: element %llu top limb at %llu",
          index, static_cast<unsigned long long>(x), static_cast<unsigned long long>(got[x].off16));
  }
  std::printf("list %d down %u up %u\n", index, down, up);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s LISTS\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  int index = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    uint64_t E = 0, S = 0, B = 0, N = 0;
    if (!(ls >> E >> S >> B)) continue;
    std::set<uint64_t> backward;
    for (uint64_t i = 0, b; i < B && ls >> b; ++i) backward.insert(b);
    ls >> N;
    std::vector<uint64_t> sizes(N);
    for (auto& n : sizes) ls >> n;
    CHECK(!ls.fail() && E > 0 && E % 64 == 0, "list %d: malformed line", index);
    if (ls.fail() || !E) return 2;
    check_substreams(index, E, S, backward, sizes);
    // and the whole-list walks of many_plan_check.cpp (fresh search, all up, all down)
    check_list(sizes);
    ++index;
  }
  if (!index) {
    std::fprintf(stderr, "no list read\n");
    return 2;
  }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
