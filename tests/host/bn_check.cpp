// bn_check.cpp — the big-integer arithmetic of the host byte API
// (csrc/host_shamir.cpp) run one operation per input line, for
// tests/test_bigint_edges_host.py to compare with Python integers.
// Stand-alone: built with AddressSanitizer and UndefinedBehaviorSanitizer,
// never loaded into another process.  The library's sources are included as
// text, so the functions of their anonymous namespaces are called directly.
//
// stdin: `op operand...` lines; integers as hex, `-` in front for a negative
// one; byte strings as hex digit pairs, `-` for the empty string.
// stdout: one line per input line.
//
//   divmod a b            divmod_mag: `q r`                     (a >= 0, b > 0)
//   mod a b               bn_mod: Python's a % b                (b > 0)
//   floordiv a b          bn_floordiv: Python's a // b          (b != 0)
//   inverse k p           bn_inverse: the value, `ZERODIV` or `ASSERT`
//   mul a b               bn_mul
//   fold10 v              fold10 of the ten words of v          (v < 2^640)
//   mulsmalladd v x c     mul_small_add                         (v, c < p; x < 2^64)
//   fmul a b              mul                                   (a, b < p)
//   fneg a                neg                                   (a < p)
//   frombe bytes          from_be
//   invsmall d            inv_small                             (0 < d < 2^64)
//   make t p n value c... dn_shamir_make_shares_host: the n records as bytes;
//                         p `-` is 2^521 - 1 passed as NULL
//   evalat p x c...       dn_shamir_eval_at_host, all operands signed
//   resolve t p rec...    dn_shamir_resolve_shares_host: the secret's bytes,
//                         or `ERR code message`
// The three entry points get output buffers of exactly the capacity they
// document, allocated on the heap, so a write past one is reported.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host_m521.cpp"
#include "host_shamir.cpp"

namespace {

[[noreturn]] void die(const char* what, long line) {
  std::fprintf(stderr, "bn_check: %s (input line %ld)\n", what, line);
  std::exit(2);
}

int nibble(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

// hex digit pairs -> bytes; `-` is the empty string
bool parse_bytes(const std::string& s, std::vector<uint8_t>& out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  for (size_t i = 0; i < s.size(); i += 2) {
    const int h = nibble(s[i]), l = nibble(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out.push_back(static_cast<uint8_t>(h * 16 + l));
  }
  return true;
}

// a hex integer -> big-endian magnitude bytes and sign
bool parse_int(const std::string& s, std::vector<uint8_t>& mag, bool& neg) {
  neg = !s.empty() && s[0] == '-';
  std::string d = s.substr(neg ? 1 : 0);
  if (d.empty()) return false;
  if (d.size() % 2) d = "0" + d;
  return parse_bytes(d, mag);
}

bool parse_bn(const std::string& s, BN& out) {
  std::vector<uint8_t> mag;
  bool neg;
  if (!parse_int(s, mag, neg)) return false;
  out = bn_from_be(mag.data(), mag.size());
  out.neg = neg && !out.zero();
  return true;
}

// a hex integer below 2^640 -> ten 64-bit words (not through from_be)
bool parse_words(const std::string& s, uint64_t v[10]) {
  for (int i = 0; i < 10; ++i) v[i] = 0;
  if (s.empty() || s.size() > 160) return false;
  for (size_t i = 0; i < s.size(); ++i) {
    const int d = nibble(s[s.size() - 1 - i]);
    if (d < 0) return false;
    v[i / 16] |= static_cast<uint64_t>(d) << (4 * (i % 16));
  }
  return true;
}

bool parse_f(const std::string& s, F& f) {
  uint64_t v[10];
  if (!parse_words(s, v) || v[9] || v[8] > kTop) return false;
  std::memcpy(f.w, v, sizeof(f.w));
  return true;
}

std::string hex_words(const uint64_t* w, int n) {
  std::string out;
  char buf[20];
  for (int i = n - 1; i >= 0; --i) {
    if (out.empty()) {
      if (w[i] == 0) continue;
      std::snprintf(buf, sizeof(buf), "%" PRIx64, w[i]);
    } else {
      std::snprintf(buf, sizeof(buf), "%016" PRIx64, w[i]);
    }
    out += buf;
  }
  return out.empty() ? "0" : out;
}

std::string hex_f(const F& f) { return hex_words(f.w, kW); }

std::string hex_bn(const BN& a) {
  // the magnitude as stored: a leading zero limb (a missing trim) would show
  std::string out = a.neg ? "-" : "";
  if (a.m.empty()) return a.neg ? "-0" : "0";
  char buf[12];
  for (size_t i = a.m.size(); i-- > 0;) {
    std::snprintf(buf, sizeof(buf), i + 1 == a.m.size() ? "%" PRIx32 : "%08" PRIx32, a.m[i]);
    out += buf;
  }
  if (a.m.back() == 0) out = "untrimmed:" + out;
  return out;
}

std::string hex_bytes(const uint8_t* p, uint64_t n) {
  if (n == 0) return "-";
  std::string out;
  char buf[4];
  for (uint64_t i = 0; i < n; ++i) {
    std::snprintf(buf, sizeof(buf), "%02x", p[i]);
    out += buf;
  }
  return out;
}

// an exactly sized heap buffer (at least one byte, so that it is a real block)
struct Heap {
  uint8_t* p;
  explicit Heap(uint64_t n) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))) {}
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

struct Prime {
  std::vector<uint8_t> be;
  bool neg = false, m521 = false;
  const uint8_t* ptr() const { return m521 ? nullptr : be.data(); }
  uint32_t len() const { return m521 ? 0u : static_cast<uint32_t>(be.size()); }
  uint32_t width() const { return m521 ? 66u : static_cast<uint32_t>(be.size()); }
};

bool parse_prime(const std::string& s, Prime& p) {
  if (s == "-") {
    p.m521 = true;
    return true;
  }
  return parse_int(s, p.be, p.neg);
}

std::string error_line(int rc) { return "ERR " + std::to_string(rc) + " " + dn_last_error(); }

}  // namespace

int main() {
  std::string line;
  long ln = 0;
  while (std::getline(std::cin, line)) {
    ++ln;
    std::istringstream in(line);
    std::vector<std::string> tok;
    for (std::string t; in >> t;) tok.push_back(t);
    if (tok.empty()) die("empty line", ln);
    const std::string& op = tok[0];
    const size_t argc = tok.size() - 1;
    std::string res;
    if (op == "divmod" || op == "mod" || op == "floordiv" || op == "inverse" || op == "mul") {
      BN a, b;
      if (argc != 2 || !parse_bn(tok[1], a) || !parse_bn(tok[2], b)) die("bad operands", ln);
      if (op == "divmod") {
        if (a.neg || b.neg || b.zero()) die("divmod needs a >= 0, b > 0", ln);
        BN q, r;
        divmod_mag(a, b, q, r);
        res = hex_bn(q) + " " + hex_bn(r);
      } else if (op == "mod") {
        if (b.neg || b.zero()) die("mod needs b > 0", ln);
        res = hex_bn(bn_mod(a, b));
      } else if (op == "floordiv") {
        if (b.zero()) die("floordiv needs b != 0", ln);
        res = hex_bn(bn_floordiv(a, b));
      } else if (op == "mul") {
        res = hex_bn(bn_mul(a, b));
      } else {
        if (b.neg || b.zero()) die("inverse needs p > 0", ln);
        BN out;
        const int rc = bn_inverse(a, b, out);
        res = rc == DN_OK ? hex_bn(out) : rc == DN_ERR_ZERODIV ? "ZERODIV" : rc == DN_ERR_ASSERT ? "ASSERT" : "?";
      }
    } else if (op == "fold10") {
      uint64_t v[10];
      F r;
      if (argc != 1 || !parse_words(tok[1], v)) die("bad operands", ln);
      fold10(v, r);
      res = hex_f(r);
    } else if (op == "mulsmalladd") {
      F v, c, r;
      uint64_t x[10];
      if (argc != 3 || !parse_f(tok[1], v) || !parse_words(tok[2], x) || !parse_f(tok[3], c)) die("bad operands", ln);
      for (int i = 1; i < 10; ++i)
        if (x[i]) die("x needs 64 bits", ln);
      mul_small_add(v, x[0], c, r);
      res = hex_f(r);
    } else if (op == "fmul") {
      F a, b, r;
      if (argc != 2 || !parse_f(tok[1], a) || !parse_f(tok[2], b)) die("bad operands", ln);
      mul(a, b, r);
      res = hex_f(r);
    } else if (op == "fneg") {
      F a, r;
      if (argc != 1 || !parse_f(tok[1], a)) die("bad operands", ln);
      neg(a, r);
      res = hex_f(r);
    } else if (op == "frombe") {
      std::vector<uint8_t> b;
      if (argc != 1 || !parse_bytes(tok[1], b)) die("bad operands", ln);
      Heap exact(b.size());  // (an exactly sized copy: a read past the bytes is reported)
      if (!b.empty()) std::memcpy(exact.p, b.data(), b.size());
      F r;
      from_be(exact.p, b.size(), r);
      res = hex_f(r);
    } else if (op == "invsmall") {
      uint64_t d[10];
      if (argc != 1 || !parse_words(tok[1], d) || d[0] == 0) die("bad operands", ln);
      for (int i = 1; i < 10; ++i)
        if (d[i]) die("d needs 64 bits", ln);
      F r;
      inv_small(d[0], r);
      res = hex_f(r);
    } else if (op == "make") {
      Prime p;
      std::vector<uint8_t> value;
      if (argc < 4 || !parse_prime(tok[2], p) || !parse_bytes(tok[4], value)) die("bad operands", ln);
      const int t = std::atoi(tok[1].c_str());
      const uint64_t n = std::strtoull(tok[3].c_str(), nullptr, 10);
      const uint32_t w = p.width();
      std::vector<uint8_t> coeffs;
      for (size_t i = 5; i < tok.size(); ++i) {
        std::vector<uint8_t> mag;
        bool cneg;
        if (!parse_int(tok[i], mag, cneg) || cneg) die("bad coefficient", ln);
        size_t lead = 0;
        while (lead < mag.size() && mag[lead] == 0) ++lead;
        if (mag.size() - lead > w) die("coefficient wider than the prime", ln);
        coeffs.insert(coeffs.end(), w - (mag.size() - lead), 0);
        coeffs.insert(coeffs.end(), mag.begin() + static_cast<long>(lead), mag.end());
      }
      if (static_cast<int>(tok.size()) - 5 != (t > 1 ? t - 1 : 0)) die("t - 1 coefficients expected", ln);
      const uint64_t cap = n * (9ull + w);
      Heap out(cap), offs(8 * (n + 1));
      uint64_t* o = reinterpret_cast<uint64_t*>(offs.p);
      const int rc = dn_shamir_make_shares_host(value.data(), value.size(), coeffs.data(), w, t, p.ptr(), p.len(), n,
                                                out.p, cap, o);
      if (rc != DN_OK) {
        res = error_line(rc);
      } else {
        for (uint64_t i = 0; i < n; ++i) res += (i ? " " : "") + hex_bytes(out.p + o[i], o[i + 1] - o[i]);
        if (n == 0) res = "none";
      }
    } else if (op == "evalat") {
      Prime p;
      std::vector<uint8_t> x;
      bool xneg;
      if (argc < 2 || !parse_prime(tok[1], p) || p.m521 || !parse_int(tok[2], x, xneg)) die("bad operands", ln);
      std::vector<uint8_t> cs, cneg;
      std::vector<uint64_t> offs{0};
      for (size_t i = 3; i < tok.size(); ++i) {
        std::vector<uint8_t> mag;
        bool ng;
        if (!parse_int(tok[i], mag, ng)) die("bad coefficient", ln);
        cs.insert(cs.end(), mag.begin(), mag.end());
        offs.push_back(cs.size());
        cneg.push_back(ng ? 1 : 0);
      }
      // the least capacity the entry point accepts for any result below |p|
      const uint64_t cap = 4 * ((p.be.size() + 3) / 4);
      Heap out(cap);
      uint64_t n = 0;
      int sgn = 0;
      const int k = static_cast<int>(tok.size()) - 3;
      const int rc = dn_shamir_eval_at_host(cs.data(), offs.data(), cneg.data(), k, x.data(),
                                            static_cast<uint32_t>(x.size()), xneg, p.be.data(),
                                            static_cast<uint32_t>(p.be.size()), p.neg, out.p, cap, &n, &sgn);
      if (rc != DN_OK) {
        res = error_line(rc);
      } else {
        std::string h = n == 0 ? "0" : hex_bytes(out.p, n);
        if (n && out.p[0] == 0) h = "leading-zero:" + h;  // the result is minimal big-endian
        if (n && h[0] == '0') h.erase(0, 1);
        res = (sgn ? "-" : "") + h;
      }
    } else if (op == "resolve") {
      Prime p;
      if (argc < 2 || !parse_prime(tok[2], p) || p.neg) die("bad operands", ln);
      const int t = std::atoi(tok[1].c_str());
      std::vector<uint8_t> all;
      std::vector<uint64_t> offs{0};
      for (size_t i = 3; i < tok.size(); ++i) {
        std::vector<uint8_t> rec;
        if (!parse_bytes(tok[i], rec)) die("bad record", ln);
        all.insert(all.end(), rec.begin(), rec.end());
        offs.push_back(all.size());
      }
      Heap shares(all.size());  // exactly sized: a parse past the last record is reported
      if (!all.empty()) std::memcpy(shares.p, all.data(), all.size());
      const uint64_t cap = p.width();
      Heap out(cap);
      uint64_t n = 0;
      const int rc = dn_shamir_resolve_shares_host(shares.p, offs.data(), static_cast<int>(tok.size()) - 3, t, p.ptr(),
                                                   p.len(), out.p, cap, &n);
      res = rc == DN_OK ? hex_bytes(out.p, n) : error_line(rc);
    } else {
      die("unknown operation", ln);
    }
    std::puts(res.c_str());
  }
  return 0;
}
