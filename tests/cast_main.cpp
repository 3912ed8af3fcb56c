// Stand-alone driver of the per-row rules of chapterhouseqe_amd/csrc/cast_device.h, built by tests/test_cast_host.py with the
// system C++ compiler and -fsanitize=address,undefined.  Reads cases from the file named on the command line, one per line:
//   fixed <from> <to> <value bits, decimal> <expected bits of the target's width, decimal | fail>
//   parse 12 <to> <string as hex or -> <expected bits of the target's width, decimal | fail>
//   print <from> 12 <value bits, decimal> <expected bytes as hex>
// <from> / <to> are CastType numbers; value bits are the 64-bit form of cast_device.h (integers extended by their signedness).
// Every string is copied into a heap block of exactly its length, and every printed value is written into a heap block of
// exactly the length cast_decimal_len / cast_bool_len announced, so a read or write one byte outside trips the sanitizer.
// Exit status: 0 = every case as expected, 1 = a mismatch (listed on stderr), 2 = unreadable input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../chapterhouseqe_amd/csrc/cast_device.h"

static bool unhex(const char* h, std::vector<uint8_t>* out) {
  out->clear();
  if (!strcmp(h, "-")) return true;
  const size_t n = strlen(h);
  if (n % 2) return false;
  for (size_t i = 0; i < n; i += 2) {
    unsigned v;
    if (sscanf(h + i, "%2x", &v) != 1) return false;
    out->push_back((uint8_t)v);
  }
  return true;
}
static std::string hexed(const uint8_t* p, size_t n) {
  if (!n) return "-";
  std::string out;
  char b[3];
  for (size_t i = 0; i < n; ++i) { snprintf(b, sizeof b, "%02x", p[i]); out += b; }
  return out;
}
// the low bytes a column of type `to` stores
static uint64_t narrowed(uint64_t bits, int to) {
  const int w = to == chq::CT_BOOL ? 1 : chq::cast_width(to);
  return w >= 8 ? bits : bits & ((1ull << (8 * w)) - 1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char op[16], in[1 << 12], want[1 << 12];
  int from, to, bad = 0, n = 0;
  while (fscanf(f, "%15s %d %d %4095s %4095s", op, &from, &to, in, want) == 5) {
    ++n;
    std::string got;
    const std::string name = op;
    if (name == "fixed") {
      uint64_t out = 0;
      const bool ok = chq::cast_fixed_value(strtoull(in, nullptr, 10), from, to, &out);
      got = ok ? std::to_string(narrowed(out, to)) : "fail";
      // the lazy-error flag must cover every failure
      if (!ok && !chq::cast_can_fail(from, to)) got = "failed although cast_can_fail says it cannot";
    } else if (name == "parse") {
      std::vector<uint8_t> s;
      if (!unhex(in, &s)) { fclose(f); return 2; }
      uint8_t* block = new uint8_t[s.size()];
      if (!s.empty()) memcpy(block, s.data(), s.size());
      uint64_t out = 0;
      const bool ok = chq::cast_parse_int(block, (int32_t)s.size(), to, &out);
      delete[] block;
      got = ok ? std::to_string(narrowed(out, to)) : "fail";
    } else if (name == "print") {
      const uint64_t bits = strtoull(in, nullptr, 10);
      const int32_t len = from == chq::CT_BOOL ? chq::cast_bool_len(bits != 0) : chq::cast_decimal_len(bits, chq::cast_is_signed(from));
      uint8_t* block = new uint8_t[(size_t)len];
      if (from == chq::CT_BOOL) chq::cast_write_bool(bits != 0, block);
      else chq::cast_write_decimal(bits, chq::cast_is_signed(from), block, len);
      got = hexed(block, (size_t)len);
      delete[] block;
    } else {
      fclose(f);
      return 2;
    }
    if (got != want) { fprintf(stderr, "case %d: %s %d -> %d %s: got %s, expected %s\n", n, op, from, to, in, got.c_str(), want); ++bad; }
  }
  fclose(f);
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : (n ? 0 : 2);
}
