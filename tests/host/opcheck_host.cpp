// opcheck_host — csrc/opcheck_ops.hpp's run_op on the host, one case at a
// time, over a binary file of cases (tests/test_device_ops_host.py builds it
// with AddressSanitizer and UndefinedBehaviorSanitizer; never loaded into
// Python).
//
//   opcheck_host CASES RESULTS
//
// CASES is a run of sections: 6 u32 words {magic, op, n_cases, in_words,
// out_words, flags} and then n_cases * in_words words.  flags bit 0 makes
// __ballot answer as if another lane of the wave were rare.  RESULTS gets
// every section's n_cases * out_words words in the same order; each out
// record starts as the byte pattern fill_byte(offset in the record).  Exits 3
// when any buffer access fell outside its descriptor.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "opcheck_ops.hpp"

static constexpr uint32_t kMagic = 0x504F4E44u;  // "DNOP"

static inline uint8_t fill_byte(size_t b) { return static_cast<uint8_t>(b * 37u + 11u); }

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
    return 2;
  }
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) {
    std::fprintf(stderr, "cannot open files\n");
    return 2;
  }
  uint32_t h[6];
  size_t sections = 0, cases = 0;
  while (std::fread(h, sizeof(uint32_t), 6, fi) == 6) {
    const int op = static_cast<int>(h[1]);
    const size_t n = h[2], iw = h[3], ow = h[4];
    if (h[0] != kMagic || op < 0 || op >= dn::opcheck::kOpCount || iw != static_cast<size_t>(dn::opcheck::in_words(op)) ||
        ow != static_cast<size_t>(dn::opcheck::out_words(op))) {
      std::fprintf(stderr, "section %zu: bad header (op %d, %zu in, %zu out)\n", sections, op, iw, ow);
      return 2;
    }
    std::vector<uint32_t> in(n * iw), out(n * ow);
    if (std::fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) {
      std::fprintf(stderr, "section %zu: short read\n", sections);
      return 2;
    }
    uint8_t* ob = reinterpret_cast<uint8_t*>(out.data());
    for (size_t i = 0; i < n; ++i)
      for (size_t b = 0; b < ow * 4; ++b) ob[i * ow * 4 + b] = fill_byte(b);
    dn_shim::ballot_other = (h[5] & 1u) != 0u;
    for (size_t i = 0; i < n; ++i) dn::opcheck::run_op(op, in.data() + i * iw, out.data() + i * ow);
    if (std::fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) {
      std::fprintf(stderr, "section %zu: short write\n", sections);
      return 2;
    }
    ++sections;
    cases += n;
  }
  std::fclose(fi);
  if (std::fclose(fo) != 0) return 2;
  std::printf("sections %zu cases %zu out_of_descriptor %llu\n", sections, cases,
              static_cast<unsigned long long>(dn_shim::oob_count));
  return dn_shim::oob_count ? 3 : 0;
}
