// parquet_jobs.h -- the plain structs the Parquet scan's host plans (parquet_scan_plan.cpp) fill and the kernels of parquet.hip /
// parquet_codec.hip read: page descriptors and inflate jobs.  Standard headers only (parquet_device.h includes this and adds
// what needs HIP), so the planning unit and its CPU test program compile without a GPU toolchain.
#pragma once
#include <stdint.h>

namespace chq {

// One data page of a column chunk.  Offsets are relative to the chunk buffer (the chunk as it lies in the file).
struct PqPageDesc {
  uint32_t levels_at;    // definition levels (RLE / bit-packed hybrid, bit width 1), behind their length prefix
  uint32_t levels_len;   // 0: none (required column, or statistics say there are no nulls)
  uint32_t values_at;
  uint32_t values_len;
  uint32_t num_rows;     // values of the page including nulls (flat schema: = rows)
  uint32_t pad;
  int64_t first_row;     // of the page inside the row group
};

// ---- page decompression (parquet_codec.hip) ---------------------------------------------------------------------------
// A compressed chunk is inflated page by page into an uncompressed image of the chunk; the page descriptors point into that
// image.  One job = one byte range of the raw chunk -> its place in the image.
enum : uint32_t { PQ_CODEC_STORED = 0, PQ_CODEC_SNAPPY = 1,
                  // a snappy page of several 64 KiB blocks, inflated block by block (parquet_codec.hip): three jobs in three launches
                  PQ_CODEC_SNAPPY_INDEX = 2,    // walks the element chain, writes where every block starts in the input
                  PQ_CODEC_SNAPPY_BLOCK = 3,    // inflates block `block` (one per block of the page)
                  PQ_CODEC_SNAPPY_FINISH = 4,   // patches the page descriptor; inflates the whole page if the blocks gave up
                  // ... and the INDEX walk of a large page as two launches of one wave per SEGMENT of its input (`block` = segment)
                  PQ_CODEC_SNAPPY_SEG = 5,      // walks a segment from a guessed start; notes where it entered, left, and the output in between
                  PQ_CODEC_SNAPPY_RESOLVE = 6 };// if the segments' entries and exits chain up exactly: walks the segment again, noting block starts
constexpr uint32_t PQ_SNAPPY_SEGMENTS = 16;     // at most; a segment is at least 32 KiB of compressed bytes (`block` = segment | segments << 16)
constexpr uint32_t PQ_SNAPPY_LEAD = 2048;       // bytes in front of a segment from where its wave looks for the chain
enum : uint32_t { PQ_JOB_KEEP_LEVELS = 1,       // with `page`: the column's definition levels are decoded (else only skipped)
                  PQ_JOB_FORCE_FALLBACK = 2 };  // INDEX job: report "not block-aligned" (tests of the FINISH path)
struct PqCodecJob {
  const uint8_t* raw;         // the chunk as it lies in the file (in HBM)
  uint8_t* image;             // the chunk's uncompressed image
  PqPageDesc* pages;          // the chunk's page descriptors (in HBM)
  uint32_t* err;              // the column's error word
  uint32_t src_at, src_len;   // in `raw`
  uint32_t dst_at, dst_len;   // in `image`; dst_at is a multiple of 16, dst_len is what the page header promises
  uint32_t codec;             // PQ_CODEC_*
  int32_t page;               // >= 0: a V1 data page of an optional column -- [4-byte length][levels][values] can only be told
                              // apart after inflation: the kernel fills levels_at / levels_len / values_at / values_len of pages[page]
  uint32_t flags;             // PQ_JOB_*
  uint32_t block;             // SNAPPY_BLOCK: which 64 KiB block of the page
  uint32_t* index;            // SNAPPY_INDEX / _BLOCK / _FINISH: [0] != 0: the blocks gave up; [1 + k]: input position of block k;
                              // [1 + blocks]: the page's compressed length; [2 + blocks ...]: PQ_SNAPPY_SEGMENTS x {entered at, left at,
                              // output bytes, ok} of a segmented walk (zero-filled before the launches)
};
// A launch serves every compressed page of every column and row group of a call's wave (jobs carry their own buffers):
// a page is a serial chain, so the pages (and, after the index walk, their 64 KiB blocks) in flight are the parallelism --
// per-column launches on the columns' streams left the twenty slowest pages of a twenty-row-group file sharing the handful of
// hardware queues the streams map to.  Launch order on a stream: INDEX jobs, then BLOCK + whole-page jobs, then FINISH jobs.
struct PqCodecParams {
  const PqCodecJob* jobs;
  int32_t n_jobs;
  int32_t pad;
};

}  // namespace chq
