// Stand-alone driver of the LIKE matcher of chapterhouseqe_amd/csrc/like_device.h, built by tests/test_like_host.py with
// the system C++ compiler and -fsanitize=address,undefined.  Reads cases from the file named on the command line, one per
// line: <string as hex or -> <pattern as hex or -> <escape byte or -1> <expected: 0, 1, E = trailing escape, L = too long>.
// Every string is copied into a heap block of exactly its length, so a read one byte before or behind it trips the
// sanitizer.  Exit status: 0 = every case as expected, 1 = a mismatch (listed on stderr), 2 = unreadable input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../chapterhouseqe_amd/csrc/like_device.h"

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

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char sh[1 << 16], ph[1 << 16];
  char want;
  int escape, bad = 0, n = 0;
  while (fscanf(f, "%65535s %65535s %d %c", sh, ph, &escape, &want) == 4) {
    std::vector<uint8_t> s, p;
    if (!unhex(sh, &s) || !unhex(ph, &p)) { fclose(f); return 2; }
    ++n;
    uint8_t* ptext = new uint8_t[p.size()];
    if (!p.empty()) memcpy(ptext, p.data(), p.size());
    chq::LikePattern* pat = new chq::LikePattern;
    const chq::LikeCompileStatus st = chq::like_compile(ptext, (int64_t)p.size(), escape, pat);
    delete[] ptext;
    char got;
    if (st == chq::LIKE_TRAILING_ESCAPE) got = 'E';
    else if (st == chq::LIKE_TOO_LONG) got = 'L';
    else {
      uint8_t* block = new uint8_t[s.size()];
      if (!s.empty()) memcpy(block, s.data(), s.size());
      got = chq::like_match(*pat, block, (int32_t)s.size()) ? '1' : '0';
      delete[] block;
    }
    delete pat;
    if (got != want) { fprintf(stderr, "case %d: string %s pattern %s escape %d: got %c, expected %c\n", n, sh, ph, escape, got, want); ++bad; }
  }
  fclose(f);
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : (n ? 0 : 2);
}
