// sha256_check.cpp — the SHA-256 arithmetic of the commitment kernel
// (csrc/sha256_core.hpp) on the host: one hex message per line on stdin (an
// empty line is the empty message), its digest as 64 hex digits per line on
// stdout.  tests/test_commit_host.py builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer and compares the digests with hashlib.
//
// The message is hashed twice through sha::digest: once with a getter that
// reads a copy cut to the message's length and answers 0xA5 for every byte
// past it (what load_block must mask off), once with one that answers zero
// there; the two must agree.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sha256_core.hpp"

using namespace dn;

static int nibble(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.size() % 2) {
      std::fprintf(stderr, "odd number of hex digits\n");
      return 2;
    }
    std::vector<uint8_t> m(line.size() / 2);  // exactly the message: a read past it is a sanitizer report
    for (size_t i = 0; i < m.size(); ++i) {
      const int hi = nibble(line[2 * i]), lo = nibble(line[2 * i + 1]);
      if (hi < 0 || lo < 0) {
        std::fprintf(stderr, "not a hex digit\n");
        return 2;
      }
      m[i] = static_cast<uint8_t>(16 * hi + lo);
    }
    const uint64_t len = m.size();
    uint32_t d[2][8];
    for (int pass = 0; pass < 2; ++pass) {
      const uint8_t fill = pass ? 0x00 : 0xA5;
      auto get = [&](uint64_t p) {
        uint32_t v = 0;
        for (uint64_t i = 0; i < 4; ++i) v = (v << 8) | (p + i < len ? m[p + i] : fill);
        return v;
      };
      sha::digest(d[pass], get, len);
    }
    for (int i = 0; i < 8; ++i)
      if (d[0][i] != d[1][i]) {
        std::fprintf(stderr, "bytes past the end of a %llu-byte message reached the digest\n",
                     (unsigned long long)len);
        return 3;
      }
    for (int i = 0; i < 8; ++i) std::printf("%08x", d[0][i]);
    std::printf("\n");
  }
  return 0;
}
