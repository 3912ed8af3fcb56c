// Stand-alone driver of the per-row rules of chapterhouseqe_amd/csrc/strfn_device.h, built by tests/test_strfn_host.py with
// the system C++ compiler and -fsanitize=address,undefined.  Reads cases from the file named on the command line, one per
// line: <function> <string as hex or -> <p> <has n: 0 / 1> <n> <expected: result bytes as hex or -, or a decimal for length>.
// Functions: upper lower length substring trim ltrim rtrim (octet_length and `||` are deliberately absent: the first is the
// row's byte count, the second a copy, and neither has a per-row rule in the header).  Every string is copied into a heap
// block of exactly its length, so a read one byte before or behind it trips the sanitizer.  Exit status: 0 = every case as
// expected, 1 = a mismatch (listed on stderr), 2 = unreadable input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../chapterhouseqe_amd/csrc/strfn_device.h"

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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char fn[64], sh[1 << 16], wh[1 << 16];
  int p, has_n, cnt, bad = 0, n = 0;
  while (fscanf(f, "%63s %65535s %d %d %d %65535s", fn, sh, &p, &has_n, &cnt, wh) == 6) {
    std::vector<uint8_t> s;
    if (!unhex(sh, &s)) { fclose(f); return 2; }
    ++n;
    const int32_t len = (int32_t)s.size();
    uint8_t* block = new uint8_t[s.size()];
    if (!s.empty()) memcpy(block, s.data(), s.size());
    std::string got;
    const std::string name = fn;
    if (name == "upper" || name == "lower") {
      std::vector<uint8_t> out(s.size());
      for (int32_t i = 0; i < len; ++i) out[(size_t)i] = chq::strfn_map_byte(block[i], name == "upper");
      got = hexed(out.data(), out.size());
    } else if (name == "length") {
      got = std::to_string(chq::strfn_count_starts(block, len));
    } else {
      int32_t first = -1, count = -1;
      if (name == "substring") chq::strfn_substr_window(block, len, p, has_n != 0, cnt, &first, &count);
      else if (name == "trim" || name == "ltrim" || name == "rtrim") chq::strfn_trim_window(block, len, name != "rtrim", name != "ltrim", &first, &count);
      else { fclose(f); return 2; }
      if (first < 0 || count < 0 || first + count > len) got = "window out of the row";
      else got = hexed(block + first, (size_t)count);
    }
    delete[] block;
    if (got != wh) { fprintf(stderr, "case %d: %s %s p=%d has_n=%d n=%d: got %s, expected %s\n", n, fn, sh, p, has_n, cnt, got.c_str(), wh); ++bad; }
  }
  fclose(f);
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : (n ? 0 : 2);
}
