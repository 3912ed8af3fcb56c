// Stand-alone driver of the per-row rules of chapterhouseqe_amd/csrc/temporal_device.h, built by tests/test_temporal_host.py with
// the system C++ compiler and -fsanitize=address,undefined.  Reads cases from the file named on the command line, one per line:
//   part  <kind> <field> <raw value, decimal> <expected Int32, decimal | null>
//   trunc <kind> <unit>  <raw value, decimal> <expected raw value, decimal | null>
//   lit   <0 DATE | 1 TIMESTAMP> <kind> <the literal's bytes as hex or -> <expected raw value, decimal | bad | finer | range>
// <kind>, <field> and <unit> are the TemporalKind / TemporalField / TemporalUnit numbers.  Every literal is copied into a heap
// block of exactly its length, so a read one byte outside trips the sanitizer.
// Exit status: 0 = every case as expected, 1 = a mismatch (listed on stderr), 2 = unreadable input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../chapterhouseqe_amd/csrc/temporal_device.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char op[16], in[1 << 10], want[64];
  int a, b, bad = 0, n = 0;
  while (fscanf(f, "%15s %d %d %1023s %63s", op, &a, &b, in, want) == 5) {
    ++n;
    std::string got;
    const std::string name = op;
    if (name == "part") {
      int32_t out = 0;
      got = chq::temporal_part(a, b, strtoll(in, nullptr, 10), &out) ? std::to_string(out) : "null";
    } else if (name == "trunc") {
      int64_t out = 0;
      got = chq::temporal_trunc(a, b, strtoll(in, nullptr, 10), &out) ? std::to_string(out) : "null";
    } else if (name == "lit") {
      std::vector<char> s;
      if (strcmp(in, "-") != 0) {
        const size_t len = strlen(in);
        if (len % 2) { fclose(f); return 2; }
        for (size_t i = 0; i < len; i += 2) { unsigned v; if (sscanf(in + i, "%2x", &v) != 1) { fclose(f); return 2; } s.push_back((char)v); }
      }
      char* block = new char[s.size()];
      if (!s.empty()) memcpy(block, s.data(), s.size());
      chq::TemporalLiteral lit;
      if (!chq::temporal_parse_literal(a, block, (int64_t)s.size(), &lit)) got = "bad";
      else {
        int64_t raw = 0;
        const int rc = chq::temporal_literal_raw(lit, b, &raw);
        got = rc == 0 ? std::to_string(raw) : rc == 1 ? "finer" : "range";
      }
      delete[] block;
    } else {
      fclose(f);
      return 2;
    }
    if (got != want) { fprintf(stderr, "case %d: %s %d %d %s: got %s, expected %s\n", n, op, a, b, in, got.c_str(), want); ++bad; }
  }
  fclose(f);
  printf("%d cases, %d mismatches\n", n, bad);
  return bad ? 1 : (n ? 0 : 2);
}
