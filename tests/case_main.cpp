// case_main.cpp -- the CASE rules of case_device.h alone, for the address and undefined-behaviour sanitizers (host code; built
// and run by tests/test_case_host.py).  Every buffer is a heap block of exactly the bytes its rows need, so a load past a
// bitmap's last byte, a value's last byte or an offsets array's last entry is reported.  The expectations come from a
// bit-by-bit and row-by-row restatement of the rule below, not from the word functions under test.
//
//   case_main [seed]      prints "<checks> checks, <mismatches> mismatches"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../chapterhouseqe_amd/csrc/case_device.h"

using namespace chq;

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// a bitmap of `n` bits that begins at bit `off` of an exact heap block
struct Bits {
  uint8_t* p = nullptr; int64_t off = 0, n = 0;
  Bits(int64_t off_, int64_t n_, int density) : off(off_), n(n_) {
    const size_t bytes = (size_t)((off + n + 7) / 8);
    p = (uint8_t*)malloc(bytes ? bytes : 1);
    for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();                 // (the bits around the rows are noise)
    for (int64_t i = 0; i < n; ++i) set(i, (int)(rnd() % 100) < density);
  }
  Bits(const Bits&) = delete;
  ~Bits() { free(p); }
  bool get(int64_t i) const { return (p[(off + i) >> 3] >> ((off + i) & 7)) & 1; }
  void set(int64_t i, bool v) { uint8_t& b = p[(off + i) >> 3]; const uint8_t m = (uint8_t)(1u << ((off + i) & 7)); b = v ? (b | m) : (b & ~m); }
};

static long checks = 0, mismatches = 0;
static void expect(bool ok, const char* what, int64_t n, int64_t off, int64_t at) {
  ++checks;
  if (!ok && ++mismatches <= 20) printf("MISMATCH %s nrows=%lld offset=%lld at=%lld\n", what, (long long)n, (long long)off, (long long)at);
}

template <int W>
static void check_fixed(const CaseSelectParams& sp, const std::vector<int>& choice, const std::vector<Bits*>& rvalid, const std::vector<uint8_t*>& rvals, int64_t n, int64_t off) {
  uint8_t* out = (uint8_t*)malloc((size_t)(n * W ? n * W : 1));
  for (int64_t i = 0; i < n; ++i) {
    const int k = case_choice(sp.masks, sp.words, sp.n_when, i);
    expect(k == choice[(size_t)i], "choice", n, off, i);
    const CaseBranch& b = sp.br[k];
    const bool valid = case_branch_valid(b, i);
    bool want_valid = b.kind == CASE_CONST || (b.kind == CASE_COLUMN && (!rvalid[(size_t)k] || rvalid[(size_t)k]->get(i)));
    expect(valid == want_valid, "valid", n, off, i);
    if (!valid) continue;
    case_copy_value<W>(b, i, out + i * W);
    uint8_t want[16];
    if (b.kind == CASE_CONST) { memcpy(want, &b.const_lo, 8); memcpy(want + 8, &b.const_hi, 8); }
    else memcpy(want, rvals[(size_t)k] + i * W, W);
    expect(memcmp(out + i * W, want, W) == 0, "value", n, off, i);
  }
  free(out);
}

static void one_shape(int64_t n, int64_t off, int n_when, bool has_else) {
  const int64_t words = (n + 63) / 64;
  // ---- conditions and the masks ----
  std::vector<Bits*> cval, cvalid;
  for (int k = 0; k < n_when; ++k) {
    cval.push_back(new Bits(off + k, n, 30));
    cvalid.push_back(k % 3 == 1 ? nullptr : new Bits(off + 2 * k, n, 80));
  }
  uint64_t* masks = (uint64_t*)malloc((size_t)((n_when + 1) * words ? (n_when + 1) * words * 8 : 1));
  for (int64_t w = 0; w < words; ++w) {
    uint64_t remaining = case_rows_mask(w, n);
    for (int k = 0; k < n_when; ++k) {
      const uint64_t c = case_load_word(cval[(size_t)k]->p, cval[(size_t)k]->off, w, n);
      const uint64_t v = case_load_word(cvalid[(size_t)k] ? cvalid[(size_t)k]->p : nullptr, cvalid[(size_t)k] ? cvalid[(size_t)k]->off : 0, w, n);
      masks[k * words + w] = case_take(&remaining, c, v);
    }
    masks[n_when * words + w] = remaining;
  }
  // bit by bit: the first condition that is true and valid
  std::vector<int> choice((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int k = 0;
    while (k < n_when && !(cval[(size_t)k]->get(i) && (!cvalid[(size_t)k] || cvalid[(size_t)k]->get(i)))) ++k;
    choice[(size_t)i] = k;
    for (int j = 0; j <= n_when; ++j) expect((int)((masks[j * words + (i >> 6)] >> (i & 63)) & 1) == (j == k), "mask bit", n, off, i);
  }
  for (int j = 0; j <= n_when && words > 0; ++j)   // no bit of a row >= n
    expect((masks[j * words + words - 1] & ~case_rows_mask(words - 1, n)) == 0, "mask tail", n, off, j);

  // ---- branches: columns with and without validity, a constant, a null ----
  CaseSelectParams sp{};
  sp.n_when = n_when; sp.nrows = n; sp.words = words; sp.masks = (const unsigned long long*)masks;
  std::vector<Bits*> rvalid((size_t)n_when + 1, nullptr), rbits((size_t)n_when + 1, nullptr);
  std::vector<uint8_t*> rvals((size_t)n_when + 1, nullptr);
  std::vector<int32_t*> roffs((size_t)n_when + 1, nullptr);
  std::vector<uint8_t*> rdata((size_t)n_when + 1, nullptr);
  const int widths[5] = {1, 2, 4, 8, 16};
  for (int wi = 0; wi < 5; ++wi) {
    const int W = widths[wi];
    for (int k = 0; k <= n_when; ++k) {
      CaseBranch& b = sp.br[k];
      b = CaseBranch{};
      if (k == n_when && !has_else) { b.kind = CASE_NULL; continue; }
      if (k % 4 == 2) { b.kind = CASE_CONST; b.const_lo = rnd(); b.const_hi = rnd(); continue; }
      if (k % 4 == 3) { b.kind = CASE_NULL; continue; }
      b.kind = CASE_COLUMN;
      rvals[(size_t)k] = (uint8_t*)malloc((size_t)(n * W ? n * W : 1));
      for (int64_t j = 0; j < n * W; ++j) rvals[(size_t)k][j] = (uint8_t)rnd();
      b.values = rvals[(size_t)k];
      if (k % 2 == 0) { rvalid[(size_t)k] = new Bits(off + 3 * k + 1, n, 70); b.validity = rvalid[(size_t)k]->p; b.offset = rvalid[(size_t)k]->off; }
    }
    switch (W) {
      case 1: check_fixed<1>(sp, choice, rvalid, rvals, n, off); break;
      case 2: check_fixed<2>(sp, choice, rvalid, rvals, n, off); break;
      case 4: check_fixed<4>(sp, choice, rvalid, rvals, n, off); break;
      case 8: check_fixed<8>(sp, choice, rvalid, rvals, n, off); break;
      default: check_fixed<16>(sp, choice, rvalid, rvals, n, off); break;
    }
    for (int k = 0; k <= n_when; ++k) { free(rvals[(size_t)k]); rvals[(size_t)k] = nullptr; delete rvalid[(size_t)k]; rvalid[(size_t)k] = nullptr; }
  }
  // ---- Boolean results, word-wise: values and validity share the branch's bit offset ----
  for (int k = 0; k <= n_when; ++k) {
    CaseBranch& b = sp.br[k];
    b = CaseBranch{};
    if (k == n_when && !has_else) { b.kind = CASE_NULL; continue; }
    if (k % 4 == 1) { b.kind = CASE_CONST; b.const_lo = (uint64_t)(k & 2 ? 1 : 0); continue; }
    if (k % 4 == 3) { b.kind = CASE_NULL; continue; }
    b.kind = CASE_COLUMN;
    const int64_t boff = (off + 5 * k + 2) % 64 + (k % 2) * 64;
    rbits[(size_t)k] = new Bits(boff, n, 50);
    b.values = rbits[(size_t)k]->p; b.offset = boff;
    if (k % 4 == 0) { rvalid[(size_t)k] = new Bits(boff, n, 70); b.validity = rvalid[(size_t)k]->p; }
  }
  for (int64_t w = 0; w < words; ++w) {
    uint64_t val, valid;
    case_select_bool_word(sp, w, &val, &valid);
    for (int64_t i = 64 * w; i < 64 * w + 64; ++i) {
      const bool gv = (valid >> (i & 63)) & 1, gb = (val >> (i & 63)) & 1;
      if (i >= n) { expect(!gv && !gb, "bool tail", n, off, i); continue; }
      const CaseBranch& b = sp.br[choice[(size_t)i]];
      const int k = choice[(size_t)i];
      const bool wv = b.kind == CASE_CONST || (b.kind == CASE_COLUMN && (!rvalid[(size_t)k] || rvalid[(size_t)k]->get(i)));
      const bool wb = wv && (b.kind == CASE_CONST ? (b.const_lo & 1) != 0 : rbits[(size_t)k]->get(i));
      expect(gv == wv && gb == wb, "bool word", n, off, i);
    }
  }
  for (int k = 0; k <= n_when; ++k) { delete rvalid[(size_t)k]; rvalid[(size_t)k] = nullptr; delete rbits[(size_t)k]; rbits[(size_t)k] = nullptr; }
  // ---- Utf8 results: the chosen range of a sliced offsets array, or a literal ----
  for (int k = 0; k <= n_when; ++k) {
    CaseBranch& b = sp.br[k];
    b = CaseBranch{};
    if (k == n_when && !has_else) { b.kind = CASE_NULL; continue; }
    if (k % 3 == 1) { b.kind = CASE_CONST; b.lit_len = k; rdata[(size_t)k] = (uint8_t*)malloc((size_t)(k ? k : 1)); b.data = rdata[(size_t)k]; continue; }
    b.kind = CASE_COLUMN;
    roffs[(size_t)k] = (int32_t*)malloc((size_t)(n + 1) * 4);
    int32_t at = (int32_t)(rnd() % 5);
    for (int64_t i = 0; i <= n; ++i) { roffs[(size_t)k][i] = at; at += (int32_t)(rnd() % 4); }
    b.values = (const uint8_t*)roffs[(size_t)k];
  }
  for (int64_t i = 0; i < n; ++i) {
    const CaseBranch& b = sp.br[choice[(size_t)i]];
    if (b.kind == CASE_NULL) continue;
    int32_t first = -1, len = -1;
    case_string_range(b, i, &first, &len);
    const int k = choice[(size_t)i];
    const bool ok = b.kind == CASE_CONST ? (first == 0 && len == b.lit_len) : (first == roffs[(size_t)k][i] && len == roffs[(size_t)k][i + 1] - roffs[(size_t)k][i]);
    expect(ok, "string range", n, off, i);
  }
  for (int k = 0; k <= n_when; ++k) { free(roffs[(size_t)k]); free(rdata[(size_t)k]); roffs[(size_t)k] = nullptr; rdata[(size_t)k] = nullptr; }
  free(masks);
  for (Bits* b : cval) delete b;
  for (Bits* b : cvalid) delete b;
}

int main(int argc, char** argv) {
  if (argc > 1) rng_state ^= strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull;
  // case_load_word alone: every bit offset, every row count around the word boundaries, against single bits
  const int64_t counts[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200};
  for (int64_t n : counts)
    for (int64_t off = 0; off < 64; ++off) {
      Bits b(off, n, 50);
      for (int64_t w = 0; w < (n + 63) / 64; ++w) {
        const uint64_t got = case_load_word(b.p, b.off, w, n);
        uint64_t want = 0;
        for (int64_t i = 64 * w; i < n && i < 64 * w + 64; ++i) want |= (uint64_t)b.get(i) << (i & 63);
        expect(got == want, "load word", n, off, w);
        expect(case_load_word(nullptr, off, w, n) == case_rows_mask(w, n), "load word without a bitmap", n, off, w);
      }
    }
  // the mask rule and the selects: every bit offset 0..63 at every count, 1 / 2 / 8 WHENs, with and without ELSE
  for (int64_t n : counts)
    for (int64_t off = 0; off < 64; ++off) {
      one_shape(n, off, 1 + (int)(off % 2), off % 4 < 2);
      if (off % 8 == 3) one_shape(n, off, CASE_MAX_WHENS, off % 16 == 3);
    }
  printf("%ld checks, %ld mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
