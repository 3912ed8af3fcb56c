// parquet_scan_plan.cpp -- the Parquet scan's host plans: everything in front of the uploads and launches of parquet_scan.cpp
// that is host arithmetic (declarations in parquet.hpp).  Column classification, the page loop of a column chunk (descriptors,
// page lists, the uncompressed image of a compressed chunk and its inflate jobs, the host walk of a Utf8 dictionary), wave
// cuts and the construction of the inflate launch chains.  Every "malformed" / "unsupported" decision of a scan that does not
// need the device is made here.  Standard headers only: tests/parquet_scan_plan_main.cpp runs it on the CPU, under the host
// sanitizers.
#include <algorithm>
#include <cstring>

#include "parquet.hpp"
#include "plan.hpp"   // ChqError

namespace chq {
namespace {

[[noreturn]] void unsupported(const std::string& what) { throw ChqError{CHQ_ERR_NOT_SUPPORTED, "parquet: " + what}; }
[[noreturn]] void malformed(const std::string& what) { throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: " + what}; }

}  // namespace

PqColumnClass parquet_classify_column(const PqColumnSchema& cs, const PqColumnChunk& cc, int64_t rows, int64_t file_size) {
  PqColumnClass k;
  if (cs.repetition > 1) unsupported("repeated column '" + cs.name + "'");
  if (cs.logical_other) unsupported("logical type of column '" + cs.name + "'");
  if (cc.codec != 0 && cc.codec != 1) {
    static const char* kCodec[] = {"UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"};
    unsupported(std::string("compression codec ") + (cc.codec >= 0 && cc.codec < 8 ? kCodec[cc.codec] : std::to_string(cc.codec).c_str()) +
                " (column '" + cs.name + "'); UNCOMPRESSED and SNAPPY pages are decoded");
  }
  k.compressed = cc.codec == 1;
  if (cc.num_values != rows) malformed("column '" + cs.name + "' holds " + std::to_string(cc.num_values) + " values for " + std::to_string(rows) + " rows");
  const bool is_string = cs.logical_string || cs.converted_type == 0;
  if (cs.converted_type > 0 && !((cs.converted_type == 17 && cs.type == PQ_INT32) || (cs.converted_type == 18 && cs.type == PQ_INT64)))
    unsupported("converted type " + std::to_string(cs.converted_type) + " of column '" + cs.name + "'");
  switch (cs.type) {
    case PQ_BOOLEAN: k.format = "b"; k.boolean = true; k.width = 1; break;
    case PQ_INT32: k.format = "i"; k.width = 4; break;
    case PQ_INT64: k.format = "l"; k.width = 8; break;
    case PQ_FLOAT: k.format = "f"; k.width = 4; break;
    case PQ_DOUBLE: k.format = "g"; k.width = 8; break;
    case PQ_BYTE_ARRAY:
      if (!is_string) unsupported("BYTE_ARRAY column '" + cs.name + "' without the String annotation");
      k.format = "u"; k.byte_array = true; break;
    default: unsupported("physical type " + std::to_string(cs.type) + " of column '" + cs.name + "'");
  }
  k.first = rows ? cc.first_byte() : 0; k.csize = rows ? cc.total_compressed_size : 0;
  if (k.csize < 0 || k.first < 0 || k.csize > file_size - k.first) malformed("column chunk outside the file");
  if (k.csize >= (1ll << 32) - 64) unsupported("column chunk of " + std::to_string(k.csize) + " bytes");
  k.optional = cs.repetition == 1;
  k.has_levels = k.optional && cc.stat_null_count != 0;
  return k;
}

PqColumnPlan parquet_plan_column(const PqColumnClass& k, const PqColumnSchema& cs, const std::vector<PqPage>& pages, int64_t rows,
                                 const uint8_t* chunk_host) {
  const bool compressed = k.compressed, optional = k.optional;
  const int64_t csize = k.csize;
  PqColumnPlan pl;
  std::vector<PqPageDesc>& descs = pl.descs;
  uint32_t& dict_at = pl.dict_at; uint32_t& dict_len = pl.dict_len; uint32_t& dict_count = pl.dict_count;
  bool have_dict = false;
  int64_t row_at = 0;
  // Compressed chunk: every page is inflated into an uncompressed IMAGE of the chunk (pages back to back, 16-byte
  // aligned) and `rel` / the descriptors below point into that image; uncompressed chunk: the image is the chunk itself.
  std::vector<PqCodecJob>& jobs = pl.jobs;
  int64_t& image_at = pl.image_bytes;
  for (const PqPage& pg : pages) {
    if (!compressed && pg.compressed_size != pg.uncompressed_size) malformed("uncompressed page whose sizes differ");
    const int64_t raw_rel = pg.payload_at;   // (page offsets are relative to the chunk)
    if (raw_rel < 0 || pg.compressed_size < 0 || pg.compressed_size > csize - raw_rel) malformed("page outside its column chunk");
    if (pg.uncompressed_size < 0 || pg.uncompressed_size >= (1ll << 31)) malformed("page size");
    int64_t rel = raw_rel;
    int64_t v2_values_at = 0, v2_values_len = 0;   // compressed V2 page: where its values section lands in the image
    if (compressed) {
      if (pg.type == PQ_INDEX_PAGE) continue;
      rel = image_at;
      image_at += (pg.uncompressed_size + 15) / 16 * 16;
      if (image_at >= (1ll << 32) - 64) unsupported("column chunk of more than 4 GiB uncompressed");
      PqCodecJob j{};
      j.src_at = (uint32_t)raw_rel; j.src_len = (uint32_t)pg.compressed_size; j.dst_at = (uint32_t)rel; j.dst_len = (uint32_t)pg.uncompressed_size;
      j.codec = PQ_CODEC_SNAPPY; j.page = -1;
      if (pg.type == PQ_DATA_PAGE_V2) {
        // the level sections lie uncompressed in front of the values section, which is compressed unless the header says not
        const int64_t lv = pg.def_bytes + pg.rep_bytes;
        if (pg.def_bytes < 0 || pg.rep_bytes < 0 || lv > pg.compressed_size || lv > pg.uncompressed_size) malformed("level sections run past the page");
        if (lv > 0) {
          PqCodecJob l = j;
          l.src_len = (uint32_t)lv; l.dst_len = (uint32_t)lv; l.codec = PQ_CODEC_STORED;
          jobs.push_back(l);
        }
        // (the values section starts at an arbitrary byte of the image: the inflate kernel wants 16-byte aligned
        // destinations, so the values get their own aligned slot and the levels stay where they are)
        const int64_t vrel = image_at;
        image_at += (pg.uncompressed_size - lv + 15) / 16 * 16;
        j.src_at = (uint32_t)(raw_rel + lv); j.src_len = (uint32_t)(pg.compressed_size - lv);
        j.dst_at = (uint32_t)vrel; j.dst_len = (uint32_t)(pg.uncompressed_size - lv);
        if (!pg.v2_compressed) j.codec = PQ_CODEC_STORED;
        if (j.dst_len > 0 || j.src_len > 0) jobs.push_back(j);
        v2_values_at = vrel; v2_values_len = pg.uncompressed_size - lv;
      } else {
        if (pg.type == PQ_DATA_PAGE && cs.repetition == 1) {   // [4-byte length][levels][values]: told apart on the device
          j.page = -2;   // patched to the descriptor's index below
        }
        jobs.push_back(j);
      }
    }
    if (pg.type == PQ_DICTIONARY_PAGE) {
      if (pg.encoding != PQ_PLAIN && pg.encoding != PQ_PLAIN_DICTIONARY) unsupported("dictionary page encoding " + std::to_string(pg.encoding));
      if (pg.num_values < 0 || pg.num_values >= (1ll << 31)) malformed("dictionary size");
      dict_at = (uint32_t)rel; dict_len = (uint32_t)pg.uncompressed_size; dict_count = (uint32_t)pg.num_values; have_dict = true;
      continue;
    }
    if (pg.type == PQ_INDEX_PAGE) continue;
    if (pg.type != PQ_DATA_PAGE && pg.type != PQ_DATA_PAGE_V2) unsupported("page type " + std::to_string(pg.type));
    PqPageDesc d{};
    if (pg.num_values < 0 || pg.num_values > rows - row_at) malformed("page of column '" + cs.name + "' holds more rows than the row group has left");
    d.num_rows = (uint32_t)pg.num_values; d.first_row = row_at;
    int64_t at = rel, left = pg.uncompressed_size;
    if (pg.type == PQ_DATA_PAGE) {
      if (optional) {   // [4-byte length][RLE hybrid levels]
        if (pg.def_encoding != PQ_RLE) unsupported("definition level encoding " + std::to_string(pg.def_encoding));
        if (left < 4) malformed("page too short for its definition levels");
        if (compressed) {
          // the length prefix is inside the compressed payload: the inflate kernel reads it and fills in the descriptor
          // (levels_at / levels_len / values_at / values_len) before the decode kernels, queued behind it, read it
          for (size_t q = jobs.size(); q-- > 0;) if (jobs[q].page == -2) { jobs[q].page = (int32_t)descs.size(); jobs[q].flags = k.has_levels ? PQ_JOB_KEEP_LEVELS : 0; break; }
          d.levels_at = (uint32_t)at; d.levels_len = k.has_levels ? 1 : 0;   // (placeholder: "has levels", see the check below)
          at = rel; left = 0;
        } else {
          uint32_t l; memcpy(&l, chunk_host + raw_rel, 4);
          if ((int64_t)l + 4 > left) malformed("definition levels run past the page");
          d.levels_at = (uint32_t)(at + 4); d.levels_len = l;
          at += 4 + l; left -= 4 + l;
        }
      }
    } else {
      if (pg.rep_bytes != 0) unsupported("repetition levels");
      if (pg.def_bytes < 0 || pg.def_bytes > left) malformed("definition levels run past the page");
      d.levels_at = (uint32_t)at; d.levels_len = (uint32_t)pg.def_bytes;
      if (compressed) { at = v2_values_at; left = v2_values_len; }
      else { at += pg.def_bytes; left -= pg.def_bytes; }
      if (!optional && pg.def_bytes != 0) malformed("definition levels on a required column");
    }
    if (optional && k.has_levels && d.levels_len == 0 && d.num_rows > 0) malformed("optional column without definition levels");
    if (!k.has_levels) d.levels_len = 0;
    d.values_at = (uint32_t)at; d.values_len = (uint32_t)left;
    const int page_index = (int)descs.size();
    if (pg.encoding == PQ_PLAIN) pl.plain_list.push_back(page_index);
    else if (pg.encoding == PQ_RLE_DICTIONARY || pg.encoding == PQ_PLAIN_DICTIONARY) {
      if (!have_dict) malformed("dictionary-encoded page without a dictionary page in front of it");
      pl.dict_list.push_back(page_index);
    } else if (pg.encoding == PQ_RLE && k.boolean) pl.rle_list.push_back(page_index);
    else unsupported("encoding " + std::to_string(pg.encoding) + " (column '" + cs.name + "')");
    pl.h_nonnull.push_back(d.num_rows); pl.h_base.push_back((uint32_t)row_at);
    row_at += pg.num_values;
    descs.push_back(d);
  }
  if (row_at != rows) malformed("pages of column '" + cs.name + "' hold " + std::to_string(row_at) + " rows, the row group has " + std::to_string(rows));
  if (k.byte_array && !pl.dict_list.empty() && !compressed) {
    // The dictionary page is ONE page: on the GPU a single workgroup would walk its length prefixes (5 ms for 1 MB of
    // ragged strings).  The host has the bytes and walks them in ~0.2 ms while it prepares the launches.
    pl.dict_walked = true;
    pl.h_src.resize(dict_count); pl.h_len.resize(dict_count);
    const uint8_t* dp = chunk_host + dict_at;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < dict_count; ++i) {
      if (pos + 4 > dict_len) malformed("dictionary page of column '" + cs.name + "' ends inside an entry");
      uint32_t l; memcpy(&l, dp + pos, 4);
      if ((uint64_t)l > dict_len - pos - 4) malformed("dictionary entry of column '" + cs.name + "' runs past its page");
      pl.h_src[i] = dict_at + (uint32_t)pos + 4; pl.h_len[i] = l;
      pos += 4 + (uint64_t)l;
    }
  }
  // (the last two refusals of a column: they stood among the launches, where only a HIP error may throw)
  if (rows != 0 && !descs.empty() && !k.byte_array) {
    if (dict_count > 0 && (uint64_t)dict_count * k.width > dict_len) malformed("dictionary page shorter than its entries");
    if (!pl.dict_list.empty() && k.boolean) unsupported("dictionary-encoded BOOLEAN column");
  }
  return pl;
}

std::vector<int> parquet_wave_cuts(const std::vector<int64_t>& bytes) {
  std::vector<int> cuts{0};
  const int n = (int)bytes.size();
  int next = 0;
  while (next < n) {
    int wave_end = next;
    int64_t wave_bytes = 0;
    while (wave_end < n) {   // a wave: about 1 GiB of column chunks resident at once (at least one row group)
      const int64_t b = bytes[(size_t)wave_end];
      if (wave_end > next && wave_bytes + b > ((int64_t)1 << 30)) break;
      wave_bytes += b; ++wave_end;
    }
    cuts.push_back(wave_end);
    next = wave_end;
  }
  return cuts;
}

size_t parquet_inflate_parts(size_t n) { return n >= 12 ? 3 : (n >= 6 ? 2 : 1); }

std::vector<PqCodecJob> PqChain::flat() const {
  std::vector<PqCodecJob> all;
  for (const std::vector<PqCodecJob>* v : {&seg, &index, &blocks, &finish}) all.insert(all.end(), v->begin(), v->end());
  return all;
}

void parquet_chain_add_page(PqChain& ch, const PqCodecJob& j, bool segments, bool force_fallback) {
  const uint32_t nblk = (j.dst_len + 65535u) / 65536u;
  PqCodecJob a = j;
  a.index = (uint32_t*)(uintptr_t)(ch.words * sizeof(uint32_t));   // (an offset until the table exists)
  ch.words += nblk + 2 + 4 * PQ_SNAPPY_SEGMENTS;
  PqCodecJob c = a; c.codec = PQ_CODEC_SNAPPY_FINISH;
  ch.finish.push_back(c);
  a.page = -1; a.flags = force_fallback ? PQ_JOB_FORCE_FALLBACK : 0u;
  a.codec = PQ_CODEC_SNAPPY_BLOCK;
  for (uint32_t k = 0; k < nblk; ++k) { a.block = k; ch.blocks.push_back(a); }
  const uint32_t n_seg = segments ? std::min<uint32_t>(PQ_SNAPPY_SEGMENTS, j.src_len >> 15) : 1u;
  if (n_seg >= 2) {   // (the walk of the page: one wave per segment of its input, twice)
    for (uint32_t k = 0; k < n_seg; ++k) { a.block = k | (n_seg << 16); a.codec = PQ_CODEC_SNAPPY_SEG; ch.seg.push_back(a); a.codec = PQ_CODEC_SNAPPY_RESOLVE; ch.index.push_back(a); }
  } else {
    a.codec = PQ_CODEC_SNAPPY_INDEX; a.block = 0;
    ch.index.push_back(a);
  }
}

void parquet_route_jobs(const PqCodecJob* jobs, size_t n, int64_t snappy_blocks, PqChain& part, PqChain& large) {
  for (size_t q = 0; q < n; ++q) {
    const PqCodecJob& pj = jobs[q];
    if (snappy_blocks == 0 || pj.codec != PQ_CODEC_SNAPPY || pj.dst_len < 3u * 65536u) part.blocks.push_back(pj);
    else parquet_chain_add_page(pj.src_len >= (512u << 10) ? large : part, pj, snappy_blocks != 3, snappy_blocks == 2);
  }
}

}  // namespace chq
