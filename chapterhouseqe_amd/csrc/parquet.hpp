// parquet.hpp -- Parquet scan with the page decode on the GPU.
//
// Replaces, for the step in front of the filter path, what the reference does with the third-party `parquet` crate inside
// read_files_task.rs:233-282 (ParquetRecordBatchStreamBuilder ... with_batch_size(max_rows_per_batch)): here the file's
// bytes are parsed on the host only as far as the METADATA goes (footer, page headers: a few hundred bytes per MB), the
// column chunks are uploaded as they lie in the file, and the pages are decoded into Arrow buffers in HBM by the kernels
// of parquet.hip -- the batch the filter kernels consume never exists in host memory.
//
// Scope: flat schemas (no repetition), optional or required columns (definition level <= 1), physical types BOOLEAN,
// INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY (as Utf8); encodings PLAIN and RLE_DICTIONARY / PLAIN_DICTIONARY; data pages
// V1 and V2; codecs UNCOMPRESSED (what the reference's own writers produce: AsyncArrowWriter::try_new(.., None),
// create_sample_data.rs:222, materialize_files_task.rs:128-133) and SNAPPY (what the writers users have produce by default),
// inflated on the GPU (parquet_codec.hip).  Anything else: CHQ_ERR_NOT_SUPPORTED with the reason.
// Input: the whole file in host memory, or a range reader (the caller's storage reader fetches the footer and exactly the
// column chunks a call decodes: read_files_task.rs:233-250 reads through opendal ranges the same way); a call decodes the
// columns it is asked for (DEV_NOTES.md:123: column pruning).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "parquet_jobs.h"

namespace chq {

enum PqType : int { PQ_BOOLEAN = 0, PQ_INT32 = 1, PQ_INT64 = 2, PQ_INT96 = 3, PQ_FLOAT = 4, PQ_DOUBLE = 5, PQ_BYTE_ARRAY = 6, PQ_FIXED_LEN_BYTE_ARRAY = 7 };
enum PqEncoding : int { PQ_PLAIN = 0, PQ_PLAIN_DICTIONARY = 2, PQ_RLE = 3, PQ_BIT_PACKED = 4, PQ_DELTA_BINARY_PACKED = 5,
                        PQ_DELTA_LENGTH_BYTE_ARRAY = 6, PQ_DELTA_BYTE_ARRAY = 7, PQ_RLE_DICTIONARY = 8, PQ_BYTE_STREAM_SPLIT = 9 };
enum PqPageType : int { PQ_DATA_PAGE = 0, PQ_INDEX_PAGE = 1, PQ_DICTIONARY_PAGE = 2, PQ_DATA_PAGE_V2 = 3 };

struct PqColumnSchema {
  std::string name;
  int type = -1;            // PqType
  int type_length = 0;
  int repetition = 0;       // 0 required, 1 optional, 2 repeated
  int converted_type = -1;  // 0 = UTF8
  bool logical_string = false;
  bool logical_other = false;   // a logical type this scan does not map (decimal, timestamp, ...)
};

struct PqPage {
  int type = 0;                 // PqPageType
  int64_t header_at = 0;        // offset of the page header, relative to the first byte of its column chunk
  int64_t payload_at = 0;       // offset of the first byte behind the header, relative to the chunk
  int64_t compressed_size = 0, uncompressed_size = 0;
  int64_t num_values = 0;       // rows of a data page (flat schema), entries of a dictionary page
  int encoding = 0;             // of the values
  int def_encoding = PQ_RLE;
  int64_t num_nulls = -1;       // V2 only
  int64_t def_bytes = 0, rep_bytes = 0;   // V2: byte lengths of the level sections (uncompressed, in front of the values)
  bool v2_compressed = true;    // V2: is_compressed (the values section; the level sections never are)
};

struct PqColumnChunk {
  int type = -1;
  int codec = 0;
  int64_t num_values = 0;
  int64_t total_compressed_size = 0;
  int64_t data_page_offset = 0, dictionary_page_offset = -1;
  int64_t stat_null_count = -1;   // from the chunk's Statistics, -1 = not recorded
  std::vector<int> encodings;
  bool pages_parsed = false;    // a file opened over a range reader parses a chunk's page headers when the chunk is fetched
  std::vector<PqPage> pages;    // in file order, dictionary page (if any) first
  int64_t first_byte() const {   // (an empty chunk has a dictionary page and no data page: data_page_offset is 0 then)
    return dictionary_page_offset > 0 && (data_page_offset <= 0 || dictionary_page_offset < data_page_offset) ? dictionary_page_offset : data_page_offset;
  }
};

struct PqRowGroup {
  int64_t num_rows = 0;
  std::vector<PqColumnChunk> columns;
};

// 0 = `length` bytes of the file starting at `offset` were written to `dst`; anything else fails the call
typedef int (*PqReadRange)(void* user, int64_t offset, int64_t length, uint8_t* dst);

struct PqFile {
  const uint8_t* data = nullptr;   // borrowed: the whole file in host memory, or null for a file behind a range reader
  PqReadRange read = nullptr;      // range reader (data == null)
  void* read_user = nullptr;
  int64_t size = 0;
  int64_t num_rows = 0;
  std::string created_by;
  std::vector<PqColumnSchema> columns;   // leaves of a flat schema, in file order
  std::vector<PqRowGroup> row_groups;
};

// Footer + every page header of every column chunk.  Throws ChqError (INVALID_ARGUMENT for a malformed file,
// NOT_SUPPORTED for nested schemas).
PqFile parquet_open(const uint8_t* data, int64_t size);
// The same over a range reader: reads the tail of the file (footer), nothing else; page headers are parsed per chunk when a
// call fetches the chunk.
PqFile parquet_open_reader(int64_t size, PqReadRange read, void* user);
// Page headers of one column chunk whose `csize` bytes start at `chunk`: fills c.pages (offsets relative to the chunk)
void parquet_parse_pages(const uint8_t* chunk, int64_t csize, PqColumnChunk& c);
// "rows R row_groups G created_by ..." / "column <name> <physical> <required|optional> [utf8]" /
// "rg <i> rows <n>" / "chunk <col> values <n> codec <c> pages <p>" / "page <type> values <n> enc <e> bytes <b> header <h>" lines
std::string parquet_describe(const PqFile& f);

struct Context;
struct Batch;
struct Buffer;
// One row group decoded into a device-resident batch (parquet_scan.cpp + parquet.hip).
Batch parquet_read_row_group(Context& ctx, const PqFile& f, int row_group);
// Several consecutive row groups, one batch each: their decodes overlap, the host synchronises twice per call.
// `columns` (n_columns >= 0 entries, or null = every column): the columns to decode, in the order they are wanted -- only
// their chunks are fetched, uploaded and decoded.
std::vector<Batch> parquet_read_row_groups(Context& ctx, const PqFile& f, int first, int count, const int32_t* columns = nullptr,
                                           int n_columns = -1);

// One record batch -> one complete Parquet file (one row group) in host memory (parquet_write.cpp + parquet_write.hip).
struct ParquetImage {
  std::shared_ptr<Buffer> bytes;   // host memory
  int64_t len = 0;
};
ParquetImage record_to_parquet(Context& ctx, const Batch& rec);
// several batches of one schema -> one file, one row group per batch
ParquetImage records_to_parquet(Context& ctx, const std::vector<const Batch*>& recs);

// ---- the scan's host plans (parquet_scan_plan.cpp) -----------------------------------------------------------------------
// Pure host arithmetic in front of the uploads and launches of parquet_scan.cpp: what a column is, where every page of its
// chunk lies (the chunk itself, or the uncompressed image of a compressed one), the inflate jobs, the cut of a call into waves
// and of a wave's jobs into launch chains -- every "malformed" / "unsupported" decision of a scan that the host can make.
// Plain structs and offsets (no device pointers, no HIP): tests/parquet_scan_plan_main.cpp runs it without a GPU.
struct PqColumnClass {
  const char* format = nullptr;   // Arrow format string
  int width = 0;                  // fixed-width types
  bool byte_array = false, boolean = false, optional = false, compressed = false;
  bool has_levels = false;        // definition levels are decoded (optional column whose statistics do not rule nulls out)
  int64_t first = 0, csize = 0;   // the chunk's bytes in the file (0, 0 for a row group without rows)
};
// Refuses what the scan does not decode (repeated, logical / converted / physical type, codec) and a chunk that cannot be
// (values != rows, outside the file, 4 GiB).
PqColumnClass parquet_classify_column(const PqColumnSchema& cs, const PqColumnChunk& cc, int64_t rows, int64_t file_size);

struct PqColumnPlan {
  std::vector<PqPageDesc> descs;                          // one per data page; offsets into the chunk or its image
  std::vector<int32_t> plain_list, dict_list, rle_list;   // the data pages by encoding: a partition of `descs`
  std::vector<uint32_t> h_nonnull, h_base;                // per page: values and first value, if the column has no levels
  uint32_t dict_at = 0, dict_len = 0, dict_count = 0;     // dictionary page payload
  int64_t image_bytes = 0;                                // compressed chunk: size of the uncompressed image
  std::vector<PqCodecJob> jobs;                           // compressed chunk: its inflate jobs, pointer fields null
  bool dict_walked = false;                               // uncompressed Utf8 dictionary: walked here, on the host
  std::vector<uint32_t> h_src, h_len;                     // ... position and length of every entry
};
// `pages`: the chunk's page headers; `chunk_bytes`: its k.csize bytes (only read where the chunk is uncompressed).
PqColumnPlan parquet_plan_column(const PqColumnClass& k, const PqColumnSchema& cs, const std::vector<PqPage>& pages, int64_t rows,
                                 const uint8_t* chunk_bytes);

// A call's row groups in waves of at most 1 GiB of selected chunk bytes (at least one row group): `bytes` per row group ->
// the boundaries 0 = c[0] < c[1] < ... = bytes.size().
std::vector<int> parquet_wave_cuts(const std::vector<int64_t>& bytes);
// The compressed pages of a wave of n row groups are inflated in 1, 2 or 3 parts of consecutive row groups ...
size_t parquet_inflate_parts(size_t n);
// ... and part `part` ends behind row group j of the wave
inline bool parquet_part_ends(size_t j, size_t n_parts, size_t n, size_t part) { return (j + 1) * n_parts / n != part; }

// One chain of inflate launches: SEG, INDEX (+ RESOLVE), BLOCK (+ whole-page), FINISH jobs, in that order on one stream.
struct PqChain {
  std::vector<PqCodecJob> seg, index, blocks, finish;
  size_t words = 0;   // of the chain's index table; the jobs' `index` is a byte offset into it until the table exists
  std::vector<PqCodecJob> flat() const;   // seg, index, blocks, finish
};
// An indexed page: its INDEX (or SEG + RESOLVE), BLOCK and FINISH jobs.
void parquet_chain_add_page(PqChain& ch, const PqCodecJob& j, bool segments, bool force_fallback);
// Routes a part's jobs by the option `snappy_blocks`: whole-page jobs and the indexed pages below 512 KiB of compressed
// bytes into `part`, the larger ones into the wave's `large` chain.
void parquet_route_jobs(const PqCodecJob* jobs, size_t n, int64_t snappy_blocks, PqChain& part, PqChain& large);

// ---- the writer's file layout (parquet_layout.cpp) --------------------------------------------------------------------
// Pure host arithmetic between the device encode and the assembly of parquet_write.cpp: page cuts, level runs, Thrift page
// headers, chunk offsets, statistics bytes and the footer, over plain structs and offsets (no pointers, no HIP), so that
// tests/parquet_layout_main.cpp runs it without a GPU.
constexpr int PW_LAYOUT_BLOCK_ROWS = 4096;   // = PW_BLOCK_ROWS of parquet_device.h: page boundaries are multiples of it

// What the device produced for one column chunk.
struct PwChunk {
  std::string name;
  int physical = PQ_INT32;      // PqType: BOOLEAN (bit-packed), INT32 / INT64 / FLOAT / DOUBLE (4 or 8 bytes a value), BYTE_ARRAY (Utf8)
  bool optional = false;
  int64_t rows = 0;
  int64_t stream_bytes = 0;     // the PLAIN value stream: non-null values only, without gaps
  bool has_levels = false;      // a level bitmap exists: ceil(rows / 8) bytes, the validity bits from bit 0
  std::vector<unsigned long long> prefix;   // bytes of the stream in front of every 4096-row block (empty where pages are cut by arithmetic)
  int64_t null_count = 0;
  bool has_minmax = false;
  std::string min_value, max_value;   // Statistics.min_value / max_value: PLAIN encoding of the value (Utf8: the bytes)
};

// One data page: `head` from the host, then a slice of the chunk's level bitmap, then a slice of its value stream.
struct PwPage {
  int64_t rows = 0;
  std::vector<uint8_t> head;    // Thrift PageHeader + the host part of the level section ([u32 length][run header])
  int64_t levels_at = 0, levels_bytes = 0;
  int64_t stream_at = 0, stream_bytes = 0;
  int64_t total() const { return (int64_t)head.size() + levels_bytes + stream_bytes; }
};
struct PwChunkLayout {
  std::vector<PwPage> pages;
  int64_t at = 0, bytes = 0;    // file offset of the first page header (set by parquet_layout_group), length of the chunk
};
// One row group of the file: a batch's chunks and where they lie.
struct PwGroup {
  int64_t rows = 0;
  std::vector<PwChunk> chunks;
  std::vector<PwChunkLayout> layout;
};

// Rows per page of a row group: `opt_page_rows` rounded down to a multiple of 4096, at least 4096, widened so that a chunk
// has at most 64 pages.
int64_t parquet_write_page_rows(int64_t opt_page_rows, int64_t rows);
PwChunkLayout parquet_layout_chunk(const PwChunk& c, int64_t page_rows);
// Lays out every chunk of `g` one behind the other from file offset `at` (advanced past the last page).
void parquet_layout_group(PwGroup& g, int64_t page_rows, int64_t& at);
// FileMetaData: the schema of the first group, every group's chunks.
std::vector<uint8_t> parquet_write_footer(const std::vector<PwGroup>& groups);
// min_value / max_value of a fixed-width or Boolean chunk from the order-preserving int64 keys of pw_stats_kernel.
void parquet_statistics_bytes(int64_t min_key, int64_t max_key, PwChunk& c);

}  // namespace chq
