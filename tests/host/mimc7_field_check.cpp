// mimc7_field_check.cpp — the BN254 arithmetic of the MiMC7 kernels
// (csrc/mimc7_field.hpp, the text the kernels compile) run on the host, one
// operation per input line, for tests/test_mimc7_field_host.py to compare with
// Python integers.  Stand-alone: built with AddressSanitizer and
// UndefinedBehaviorSanitizer, never loaded into another process.
//
// stdin: `op operand...` lines, operands as hex integers (at most 256 bits);
// stdout: one line per input line, the result as a hex integer.
//
//   mul a b        a b mod q                          (a, b < q)
//   sqr a b        (a + b)^2 mod q, the sum lazy as in a hash round:
//                  Montgomery forms added limb-wise, carry-normalized, not
//                  reduced, then mont_sqr             (a, b < q)
//   hash x k       mimc7_hash(x, k) mod q             (x, k < q)
//   arr_step r x   (r + x + mimc7_hash(x, r)) mod q   (r, x < q)
//   raw_mul a b    mont_mul on the 29-bit limbs of a, b as given (anything
//                  below 3 q): a b R^-1 mod q.  The program checks that the
//                  result is canonical (< q) and that every column
//                  accumulator of the product stays below 2^63.
//   raw_sqr a      the same for mont_sqr
//   f2f bits p     float_to_field(double with these bits, 10^p): the field
//                  value, or `bad` where the conversion refuses
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mimc7_field.hpp"

using namespace dn::mimc;

namespace {

[[noreturn]] void die(const char* what, long line) {
  std::fprintf(stderr, "mimc7_field_check: %s (input line %ld)\n", what, line);
  std::exit(2);
}

bool parse_hex(const char* s, uint32_t out[L]) {
  for (int i = 0; i < L; ++i) out[i] = 0;
  const size_t n = std::strlen(s);
  if (n == 0 || n > 8 * L) return false;
  for (size_t i = 0; i < n; ++i) {
    const char c = s[n - 1 - i];
    uint32_t d;
    if (c >= '0' && c <= '9') d = static_cast<uint32_t>(c - '0');
    else if (c >= 'a' && c <= 'f') d = static_cast<uint32_t>(c - 'a' + 10);
    else return false;
    out[i / 8] |= d << (4 * (i % 8));
  }
  return true;
}

void print_hex(const uint32_t v[L]) {
  for (int i = L - 1; i >= 0; --i) std::printf("%08" PRIx32, v[i]);
  std::putchar('\n');
}

// The column accumulators of mont_mul / mont_sqr in 128 bits, the same
// schedule: the largest value any column reaches.
typedef unsigned __int128 u128;

u128 reduce_columns(u128 T[2 * N], u128 top, const Consts& k) {
  for (int i = 0; i < N; ++i) {
    const uint32_t m = (static_cast<uint32_t>(T[i]) * k.qinv) & kM29;
    for (int j = 0; j < N; ++j) {
      T[i + j] += static_cast<u128>(m) * k.q29[j];
      if (T[i + j] > top) top = T[i + j];
    }
    T[i + 1] += T[i] >> 29;
    if (T[i + 1] > top) top = T[i + 1];
  }
  u128 c = 0;
  for (int i = 0; i < N; ++i) {
    const u128 v = T[N + i] + c;
    if (v > top) top = v;
    c = v >> 29;
  }
  return top;
}

u128 mul_columns_max(const uint32_t a[N], const uint32_t b[N], const Consts& k) {
  u128 T[2 * N] = {}, top = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      T[i + j] += static_cast<u128>(a[i]) * b[j];
      if (T[i + j] > top) top = T[i + j];
    }
  return reduce_columns(T, top, k);
}

u128 sqr_columns_max(const uint32_t a[N], const Consts& k) {
  u128 T[2 * N] = {}, top = 0;
  for (int i = 0; i < N; ++i) {
    T[2 * i] += static_cast<u128>(a[i]) * a[i];
    if (T[2 * i] > top) top = T[2 * i];
    for (int j = i + 1; j < N; ++j) {
      T[i + j] += static_cast<u128>(a[i]) * (static_cast<u128>(a[j]) << 1);
      if (T[i + j] > top) top = T[i + j];
    }
  }
  return reduce_columns(T, top, k);
}

void print_raw(const uint32_t r[N], u128 top, const Consts& k, long line) {
  if (top >> 63) die("a column accumulator reached 2^63", line);
  for (int i = 0; i < N; ++i)
    if (r[i] > kM29) die("a result limb is not normalized", line);
  if (geq29(r, k.q29)) die("the result is not canonical (>= q)", line);
  uint32_t out[L];
  from29(r, out);
  print_hex(out);
}

}  // namespace

int main() {
  Consts k;
  std::memset(&k, 0, sizeof(k));
  make_consts(k);
  for (int c = 0; c < kRounds; ++c) {  // as consts() in mimc7_bn254.hip
    uint32_t plain[L];
    dec_to_limbs(kCtsDec[c], plain);
    to_mont(k.cts[c], plain, k);
  }
  char op[16], s1[80], s2[80];
  char buf[256];
  long line = 0;
  while (std::fgets(buf, sizeof(buf), stdin)) {
    ++line;
    s1[0] = s2[0] = 0;
    const int got = std::sscanf(buf, "%15s %79s %79s", op, s1, s2);
    if (got < 2) die("malformed line", line);
    if (!std::strcmp(op, "f2f")) {
      if (got != 3) die("f2f takes bits and a precision", line);
      const uint64_t bits = std::strtoull(s1, nullptr, 16);
      const int p = std::atoi(s2);
      if (p < 0 || p > 22) die("precision 0..22", line);
      double v;
      std::memcpy(&v, &bits, sizeof(v));
      uint32_t out[L];
      if (float_to_field(v, pow10d(p), out, k)) {
        if (geq(out, k.q)) die("float_to_field result >= q", line);
        print_hex(out);
      } else {
        std::puts("bad");
      }
      continue;
    }
    uint32_t a[L], b[L] = {0};
    const bool unary = !std::strcmp(op, "raw_sqr");
    if (!parse_hex(s1, a) || (!unary && (got != 3 || !parse_hex(s2, b)))) die("bad operand", line);
    if (!std::strcmp(op, "raw_mul") || unary) {
      uint32_t a29[N], b29[N], r[N];
      to29(a, a29);
      to29(b, b29);
      if (unary) {
        mont_sqr(r, a29, k);
        print_raw(r, sqr_columns_max(a29, k), k, line);
      } else {
        mont_mul(r, a29, b29, k);
        print_raw(r, mul_columns_max(a29, b29, k), k, line);
      }
      continue;
    }
    if (geq(a, k.q) || geq(b, k.q)) die("operand >= q", line);
    uint32_t am[N], bm[N], rm[N], out[L];
    to_mont(am, a, k);
    to_mont(bm, b, k);
    if (!std::strcmp(op, "mul")) {
      mont_mul(rm, am, bm, k);
    } else if (!std::strcmp(op, "sqr")) {
      uint32_t t[N];
      for (int i = 0; i < N; ++i) t[i] = am[i] + bm[i];  // < 2 q: not reduced
      norm29(t);
      mont_sqr(rm, t, k);
    } else if (!std::strcmp(op, "hash")) {
      hash_m(rm, am, bm, k);
    } else if (!std::strcmp(op, "arr_step")) {
      for (int i = 0; i < N; ++i) rm[i] = am[i];
      arr_step(rm, bm, k);
    } else {
      die("unknown op", line);
    }
    from_mont(out, rm, k);
    if (geq(out, k.q)) die("result >= q", line);
    print_hex(out);
  }
  return 0;
}
