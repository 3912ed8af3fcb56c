// avg_main.cpp -- avg_rn128 of avg_rn.h alone, for the address and undefined-behaviour sanitizers (host code; built and run by
// tests/test_aggregate_ext_host.py).  The expectations are not computed here: the test writes a table of totals with the bits
// of Python's float(int), which is correctly rounded, and this program compares avg_rn128 with every row of it.
//
//   avg_main TABLE     TABLE: one "<hi> <lo> <signed> <bits>" per line, hexadecimal 64-bit words of the two's complement (or
//                      unsigned) 128-bit total, 0 / 1, and the expected binary64 bits
//                      prints "<checks> checks, <mismatches> mismatches"
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../chapterhouseqe_amd/csrc/avg_rn.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: avg_main TABLE\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  long checks = 0, mismatches = 0;
  uint64_t hi, lo, bits;
  int is_signed;
  while (fscanf(f, "%" SCNx64 " %" SCNx64 " %d %" SCNx64, &hi, &lo, &is_signed, &bits) == 4) {
    const double d = chq::avg_rn128(lo, hi, is_signed != 0);
    uint64_t got;
    memcpy(&got, &d, 8);
    ++checks;
    if (got != bits && ++mismatches <= 20)
      printf("MISMATCH hi=%016" PRIx64 " lo=%016" PRIx64 " signed=%d: got %016" PRIx64 ", expected %016" PRIx64 "\n", hi, lo, is_signed, got, bits);
  }
  fclose(f);
  printf("%ld checks, %ld mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
