// aggregate_acc.h -- device side only: the one accumulator of every aggregate (AggAcc, aggregate_device.h) -- identity,
// combine, load through the permutation, conversion to the output value (the small loads around it: scan_device.h).  Shared by the
// GROUP BY kernels (aggregate.hip: segmented reduce) and the window-function kernels (window.hip: segmented scan); the
// parameter block P is AggReduceParams or WinAggParams, which name these fields alike.
#pragma once
#include <hip/hip_runtime.h>

#include "aggregate_device.h"
#include "avg_rn.h"        // avg_rn128
#include "scan_device.h"   // lane_id, bit_at, load_uint, load_int

namespace chq {

__device__ __forceinline__ double as_double(uint64_t u) { return __longlong_as_double((long long)u); }
__device__ __forceinline__ uint64_t as_bits(double d) { return (uint64_t)__double_as_longlong(d); }
// the averages accumulate as the sums of their kind
constexpr bool acc_int_total(int op) { return op == AO_SUM_INT || op == AO_AVG_INT; }
constexpr bool acc_float_total(int op) { return op == AO_SUM_FLOAT || op == AO_AVG_FLOAT; }

template <int OP>
__device__ __forceinline__ AggAcc acc_identity() {
  AggAcc x{0, 0, 0};
  if (acc_float_total(OP)) x.a = 1ull << 63;   // -0.0: v + -0.0 == v for every v, -0.0 and +0.0 included
  if (OP == AO_MIN) x.a = ~0ull;
  return x;
}

// x covers earlier sorted positions than y
template <int OP>
__device__ __forceinline__ AggAcc acc_combine(const AggAcc& x, const AggAcc& y) {
  AggAcc r;
  r.cnt = x.cnt + y.cnt;
  r.b = 0;
  if (acc_int_total(OP)) {
    r.a = x.a + y.a;
    r.b = x.b + y.b + (r.a < x.a ? 1 : 0);
  } else if (acc_float_total(OP)) {
    r.a = as_bits(as_double(x.a) + as_double(y.a));
  } else if (OP == AO_MIN) {
    r.a = x.a < y.a ? x.a : y.a;
  } else if (OP == AO_MAX) {
    r.a = x.a > y.a ? x.a : y.a;
  } else {
    r.a = 0;
  }
  return r;
}

template <int OP, class P>
__device__ __forceinline__ AggAcc acc_load(const P& p, int64_t pos) {
  const uint32_t r = p.perm ? p.perm[pos] : (uint32_t)pos;
  if (p.validity && !bit_at(p.validity, p.bit_offset + r)) return acc_identity<OP>();
  AggAcc x{0, 0, 1};
  if (acc_int_total(OP)) {
    if (p.value_kind == AV_SIGNED) {
      const int64_t v = load_int(p.values, r, p.width);
      x.a = (uint64_t)v;
      x.b = v < 0 ? ~0ull : 0ull;
    } else {
      x.a = load_uint(p.values, r, p.width);
    }
  } else if (acc_float_total(OP)) {
    x.a = as_bits(p.width == 4 ? (double)((const float*)p.values)[r] : ((const double*)p.values)[r]);   // Float32 widens exactly
  } else if (OP == AO_MIN || OP == AO_MAX) {
    if (p.value_kind == AV_SIGNED) {
      x.a = (uint64_t)load_int(p.values, r, p.width) ^ (1ull << 63);
    } else if (p.value_kind == AV_UNSIGNED) {
      x.a = load_uint(p.values, r, p.width);
    } else {   // totalOrder: sign set -> every bit inverted, else the sign bit set
      const int bits = 8 * p.width;
      const uint64_t u = load_uint(p.values, r, p.width);
      const uint64_t sign = 1ull << (bits - 1), mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
      x.a = (u & sign) ? (~u & mask) : (u | sign);
    }
  }
  return x;
}

// the finished accumulator of group g (window functions: of the frame of input row g) -> its output value
template <int OP, class P>
__device__ __forceinline__ void acc_finalize(const P& p, uint32_t g, const AggAcc& acc) {
  if (OP == AO_COUNT) {
    ((int64_t*)p.out)[g] = (int64_t)acc.cnt;
    return;
  }
  p.cnt_out[g] = acc.cnt;
  if (OP == AO_SUM_INT) {
    const bool fits = p.value_kind == AV_SIGNED ? acc.b == ((acc.a >> 63) ? ~0ull : 0ull) : acc.b == 0;
    if (!fits) atomicOr(p.overflow, 1u);
    ((uint64_t*)p.out)[g] = acc.a;
  } else if (OP == AO_SUM_FLOAT) {
    ((uint64_t*)p.out)[g] = acc.cnt ? acc.a : 0;
  } else if (OP == AO_AVG_INT) {   // RN(exact total) / count: one rounding of the total, one IEEE division; no overflow
    ((uint64_t*)p.out)[g] = acc.cnt ? as_bits(avg_rn128(acc.a, acc.b, p.value_kind == AV_SIGNED) / (double)acc.cnt) : 0;
  } else if (OP == AO_AVG_FLOAT) {   // the SUM's bits over the count, in one IEEE division
    ((uint64_t*)p.out)[g] = acc.cnt ? as_bits(as_double(acc.a) / (double)acc.cnt) : 0;
  } else {
    uint64_t u = 0;
    if (acc.cnt) {
      if (p.value_kind == AV_SIGNED) {
        u = acc.a ^ (1ull << 63);
      } else if (p.value_kind == AV_UNSIGNED) {
        u = acc.a;
      } else {
        const int bits = 8 * p.width;
        const uint64_t sign = 1ull << (bits - 1), mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
        u = (acc.a & sign) ? (acc.a & ~sign) : (~acc.a & mask);
      }
    }
    switch (p.width) {
      case 1: p.out[g] = (uint8_t)u; break;
      case 2: ((uint16_t*)p.out)[g] = (uint16_t)u; break;
      case 4: ((uint32_t*)p.out)[g] = (uint32_t)u; break;
      default: ((uint64_t*)p.out)[g] = u; break;
    }
  }
}

__device__ __forceinline__ AggAcc shfl_up_acc(const AggAcc& x, int o) {
  AggAcc y;
  y.a = __shfl_up((unsigned long long)x.a, (unsigned)o, 64);
  y.b = __shfl_up((unsigned long long)x.b, (unsigned)o, 64);
  y.cnt = __shfl_up((unsigned long long)x.cnt, (unsigned)o, 64);
  return y;
}
__device__ __forceinline__ AggAcc shfl_down_acc(const AggAcc& x, int o) {
  AggAcc y;
  y.a = __shfl_down((unsigned long long)x.a, (unsigned)o, 64);
  y.b = __shfl_down((unsigned long long)x.b, (unsigned)o, 64);
  y.cnt = __shfl_down((unsigned long long)x.cnt, (unsigned)o, 64);
  return y;
}

}  // namespace chq
