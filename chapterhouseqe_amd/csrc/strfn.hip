// strfn.hip -- gfx950 kernels of the scalar string functions.  Like the other typed operations they
// write a temporary column -- Utf8 or Int32 here -- that replaces the node before the rest of the expression is lowered.
//
//   strfn_bytemap_kernel   UPPER / LOWER: a flat map over the column's byte range, oblivious of rows.  16-byte aligned loads
//                          in the body (stores at whatever phase the output has), single bytes at the ragged ends.
//   strfn_rebase_kernel    the offsets of a length-preserving function: the input's, rebased to 0.
//   strfn_rows_kernel      LENGTH / OCTET_LENGTH values, the SUBSTRING / TRIM window of each row, the row lengths of `||`, on
//                          the row-wise scheme of wave_rows.h.  Two modes like like.hip: lane per row, or -- more than
//                          STRFN_WAVE_MODE_BYTES in the wave's rows -- wave per row with a ballot + popcount per 64-byte step.
//   (scan.hip)             exclusive scan of the row lengths -> Int32 offsets and the 64-bit byte total: launch_offsets_scan.
//   strfn_gather_kernel    the bytes of every output row from 1 source range (copy_rows) or up to STRFN_MAX_PARTS parts (its
//                          own loops: the parts of a row are written one behind the other before the next row); same two modes.
// Every load of string data is a byte load inside [offsets[i], offsets[i + 1]) of a VALID row i < nrows (the byte map: inside
// [offsets[0], offsets[nrows])): no padding is assumed, and data may be null when there are no bytes.
#include <hip/hip_runtime.h>

#include "strfn_device.h"
#include "typed_ops.h"   // rows_grid
#include "wave_rows.h"

namespace chq {
namespace {
typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// ---- UPPER / LOWER -------------------------------------------------------------------------------------------------------
// four bytes at once: bit 7 of each byte of `m` marks an ASCII letter of the case that changes; its bit 5 is flipped
__device__ __forceinline__ uint32_t map_word(uint32_t x, uint32_t add_ge, uint32_t add_gt) {
  const uint32_t y = x & 0x7f7f7f7fu;
  const uint32_t m = (y + add_ge) & ~(y + add_gt) & ~x & 0x80808080u;
  return x ^ (m >> 2);
}

__global__ __launch_bounds__(256) void strfn_bytemap_kernel(const StrByteMapParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
  int64_t head = (int64_t)((16 - ((uintptr_t)p.in & 15)) & 15);
  if (head > p.n) head = p.n;
  const int64_t nvec = (p.n - head) >> 4, tail0 = head + (nvec << 4);
  if (tid < head) p.out[tid] = strfn_map_byte(p.in[tid], p.upper != 0);
  if (tid < p.n - tail0) p.out[tail0 + tid] = strfn_map_byte(p.in[tail0 + tid], p.upper != 0);
  // 'a' = 0x61, 'z' + 1 = 0x7b, 'A' = 0x41, 'Z' + 1 = 0x5b: adding 0x80 - bound sets bit 7 exactly from the bound up
  const uint32_t ge = p.upper ? 0x1f1f1f1fu : 0x3f3f3f3fu, gt = p.upper ? 0x05050505u : 0x25252525u;
  const u32x4* src = (const u32x4*)(p.in + head);
  uint8_t* dst = p.out + head;
  for (int64_t v = tid; v < nvec; v += nthreads) {
    u32x4 w = src[v];
    w.x = map_word(w.x, ge, gt); w.y = map_word(w.y, ge, gt); w.z = map_word(w.z, ge, gt); w.w = map_word(w.w, ge, gt);
    *(u32x4_unaligned*)(dst + (v << 4)) = w;
  }
}

__global__ __launch_bounds__(256) void strfn_rebase_kernel(const StrRebaseParams p) {
  const int32_t first = p.in[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) p.out[i] = p.in[i] - first;
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
// wave-per-row helpers: every argument but `lane` is wave-uniform
__device__ int32_t wave_count_starts(const uint8_t* s, int32_t n, int lane) {
  int32_t c = 0;
  for (int32_t pos = 0; pos < n; pos += 64) {
    const int32_t q = pos + lane;
    c += __popcll(__ballot(q < n && strfn_is_start(s[q])));
  }
  return c;
}
struct WaveKth {
  const uint8_t* s; int lane;
  __device__ int32_t operator()(int32_t off, int32_t m, int64_t k) const {
    for (int32_t pos = 0; pos < m; pos += 64) {
      const int32_t q = pos + lane;
      u64 starts = __ballot(q < m && strfn_is_start(s[off + q]));
      const int c = __popcll(starts);
      if (k <= c) {
        for (; k > 1; --k) starts &= starts - 1;
        return pos + __ffsll((long long)starts) - 1;
      }
      k -= c;
    }
    return m;
  }
};
__device__ void wave_trim(const uint8_t* s, int32_t n, bool left, bool right, int lane, int32_t* first, int32_t* len) {
  int32_t b = 0, e = n;
  if (left) {
    b = n;
    for (int32_t pos = 0; pos < n; pos += 64) {
      const int32_t q = pos + lane;
      const u64 m = __ballot(q < n && s[q] != 0x20);
      if (m) { b = pos + __ffsll((long long)m) - 1; break; }
    }
  }
  if (right) {
    e = b;
    for (int32_t hi = n; hi > b; hi -= 64) {
      const int32_t q = hi - 1 - lane;   // lane 0 looks at the last byte
      const u64 m = __ballot(q >= b && s[q] != 0x20);
      if (m) { e = hi - (__ffsll((long long)m) - 1); break; }
    }
  }
  *first = b; *len = e - b;
}

__global__ __launch_bounds__(kRowsBlock) void strfn_rows_kernel(const StrRowsParams p) {
  const int lane = lane_id();
  const StrPart& a = p.part[0];
  const int fn = p.fn;
  // (SUBSTRING from the row's first byte to its end needs no data at all)
  const bool reads_data = fn == STRFN_LENGTH || fn == STRFN_TRIM || fn == STRFN_LTRIM || fn == STRFN_RTRIM ||
                          (fn == STRFN_SUBSTRING && (p.p > 1 || p.has_cnt));
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    bool valid = false;
    int32_t b = 0, e = 0;
    if (i < p.nrows) {
      valid = true;
      for (int k = 0; k < p.n_parts; ++k)
        if (!row_valid(p.part[k].validity, p.part[k].validity_offset, i)) valid = false;
      if (a.offsets) { b = a.offsets[i]; e = a.offsets[i + 1]; }
    }
    const u64 vm = __ballot(valid);
    int32_t out = 0, start = 0;
    if (fn == STRFN_CONCAT) {
      if (valid) {
        u64 sum = 0;
        for (int k = 0; k < p.n_parts; ++k)
          sum += p.part[k].offsets ? (u64)(uint32_t)(p.part[k].offsets[i + 1] - p.part[k].offsets[i]) : (u64)(uint32_t)p.part[k].lit_len;
        out = (int32_t)(uint32_t)(sum > 0xffffffffull ? 0xffffffffull : sum);
      }
    } else if (fn == STRFN_OCTET_LENGTH) {
      if (valid) out = e - b;
    } else if (reads_data && wave_spans_more_than(a.offsets, base, wave_end, STRFN_WAVE_MODE_BYTES)) {
      for (u64 todo = vm; todo; todo &= todo - 1) {
        const int row = __ffsll((long long)todo) - 1;
        const int32_t rb = __shfl(b, row), n = __shfl(e, row) - rb;
        const uint8_t* s = a.data + rb;
        int32_t first = 0, len = 0;
        if (fn == STRFN_LENGTH) len = wave_count_starts(s, n, lane);
        else if (fn == STRFN_SUBSTRING) strfn_substr_window_with(WaveKth{s, lane}, n, p.p, p.has_cnt != 0, p.cnt, &first, &len);
        else wave_trim(s, n, fn != STRFN_RTRIM, fn != STRFN_LTRIM, lane, &first, &len);
        if (lane == row) { out = len; start = rb + first; }
      }
    } else if (valid) {
      const uint8_t* s = a.data + b;
      int32_t first = 0;
      if (fn == STRFN_LENGTH) out = strfn_count_starts(s, e - b);
      else if (fn == STRFN_SUBSTRING) strfn_substr_window(s, e - b, p.p, p.has_cnt != 0, p.cnt, &first, &out);
      else strfn_trim_window(s, e - b, fn != STRFN_RTRIM, fn != STRFN_LTRIM, &first, &out);
      start = b + first;
    }
    if (i < p.nrows) {
      p.out_i32[i] = out;
      if (p.out_start) p.out_start[i] = start;
    }
    store_validity_word(p.out_validity, p.null_count, base, wave_end, vm);
  }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowsBlock) void strfn_gather_kernel(const StrGatherParams p) {
  const int lane = lane_id();
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    int32_t ob = 0, oe = 0;
    if (i < p.nrows) { ob = p.out_offsets[i]; oe = p.out_offsets[i + 1]; }
    const bool wave_mode = wave_spans_more_than(p.out_offsets, base, wave_end, STRFN_WAVE_MODE_BYTES);
    if (p.start) {
      copy_rows(wave_mode, oe > ob ? p.part[0].data + p.start[i] : nullptr, p.out_data, ob, oe - ob);
    } else if (wave_mode) {
      for (u64 todo = __ballot(oe > ob); todo; todo &= todo - 1) {
        const int row = __ffsll((long long)todo) - 1;
        const int64_t r = base + row;
        uint8_t* dst = p.out_data + __shfl(ob, row);
        for (int k = 0; k < p.n_parts; ++k) {
          const StrPart& q = p.part[k];
          const int32_t sb = q.offsets ? q.offsets[r] : 0;
          const int32_t n = q.offsets ? q.offsets[r + 1] - sb : q.lit_len;
          for (int32_t j = lane; j < n; j += 64) dst[j] = q.data[sb + j];
          dst += n;
        }
      }
    } else if (oe > ob) {
      uint8_t* dst = p.out_data + ob;
      for (int k = 0; k < p.n_parts; ++k) {
        const StrPart& q = p.part[k];
        const int32_t sb = q.offsets ? q.offsets[i] : 0;
        const int32_t n = q.offsets ? q.offsets[i + 1] - sb : q.lit_len;
        for (int32_t j = 0; j < n; ++j) dst[j] = q.data[sb + j];
        dst += n;
      }
    }
  }
}
}  // namespace

hipError_t launch_strfn_bytemap(const StrByteMapParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(strfn_bytemap_kernel, dim3(rows_grid(p.n / 16 + 1, 256 * 16)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_strfn_rebase(const StrRebaseParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(strfn_rebase_kernel, dim3(rows_grid(p.n, 256 * 16)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_strfn_rows(const StrRowsParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(strfn_rows_kernel, dim3(rows_grid(p.nrows, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_strfn_gather(const StrGatherParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(strfn_gather_kernel, dim3(rows_grid(p.nrows, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
}  // namespace chq
