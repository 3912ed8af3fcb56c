// sort.hpp -- ORDER BY: the stable multi-key sort of a record batch, or of a group of them joined into one (sort.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "engine.hpp"
#include "sort_device.h"

namespace chq {

// sort.hip
hipError_t launch_sort_norm(const SortNormParams& p, hipStream_t stream);
hipError_t launch_sort_hist(const SortHistParams& p, int grid, hipStream_t stream);
hipError_t launch_sort_pass(const SortPassParams& p, hipStream_t stream);   // count, scan, scatter: 3 launches
hipError_t launch_sort_utf8_maxlen(const SortMaxLenParams& p, int grid, hipStream_t stream);
hipError_t launch_sort_gather_fixed(const SortGatherParams& p, hipStream_t stream, bool pad = false);
hipError_t launch_sort_gather_bits(const SortGatherParams& p, hipStream_t stream, bool pad = false);
hipError_t launch_sort_utf8_sizes(const SortGatherParams& p, hipStream_t stream, bool pad = false);   // 2 launches
hipError_t launch_sort_utf8_copy(const SortGatherParams& p, hipStream_t stream, bool pad = false);    // 2 launches

// one ORDER BY key as the C ABI hands it over (chq_sort_key)
struct SortKeyArg {
  const Expr* column = nullptr;   // Identifier / CompoundIdentifier, resolved like compute_value resolves them
  bool descending = false;
  bool nulls_first = false;
};

// bytes the kernels move, for chq_call_stats (algorithmic: every byte read or written once)
struct Traffic {
  int64_t read = 0, written = 0;
};

// The pieces of the sort that the operators on top of it (aggregate.cpp, join.cpp, window.cpp, partition.cpp) stand on.
// the column an argument names: the resolver of compute_value (plan.cpp), which must come back with a bare column.  `what`
// says which argument in "<what> must be a column, not <text>"
int resolve_key(const Expr& e, const std::vector<PlanColumn>& pcols, int64_t nrows, const std::string& what = "a sort key");
// temporal types and decimals of up to 8 bytes: they order, and MIN / MAX compare them, as their signed integers.  The ONE
// place the list of their formats stands: the key words, sortable() and the typing of the aggregates all ask here.
bool orders_as_signed(const Column& c);
// does the column's type have an order here?  The key types of ORDER BY, JOIN (join.cpp) and the hash partitioning (partition.cpp)
bool sortable(const Column& c);
// out row i = in row perm[i] (perm null: identity) for rows [0, m), on the device; a validity bitmap's set bits are added to
// *ones and the column's null_count left at -1 for the caller to fill in.  `pad`: perm may hold kSortNoRow ("no row", the
// padded side of an outer join): such a row comes out null over zeroed value bytes, and the column nullable with a bitmap,
// through the padded variants of the kernels -- the kernels of a call with pad = false are the ones without the test.
Column gather_column(Context& ctx, const Column& c, const uint32_t* perm, int64_t m, uint64_t* ones, Traffic& t, bool pad = false);
// the permutation of rows [0, n) that orders `rec` by `keys` on the columns `cols` (null: identity -- no key, or fewer than 2 rows)
BufferPtr sort_permutation(Context& ctx, const Batch& rec, const std::vector<int>& cols, const std::vector<SortKeyArg>& keys, Traffic& t);

// The end of an operator's call: closes the kernel span, copies the call's `n` counter words (u64: set validity bits, overflow
// flags) back -- nothing when n is 0 --, synchronises the stream and sets kernel_ns and the two byte counters of ctx.stats.
std::vector<uint64_t> finish_call(Context& ctx, const void* words, size_t n, const Traffic& t, const char* what = "read back null counts");
// every null_count that gather_column (or validity_from_counts, aggregate.hpp) left at -1: rows - ones[i] for column i
void fill_null_counts(std::vector<Column>& cols, int64_t rows, const std::vector<uint64_t>& ones);

// The batches of `in` (one schema, host or device resident) in key order, stable (batch order, then row order), cut to
// the first `limit` rows (-1: all).  The result is ONE device batch with the schema of the input.  Throws ChqError.
Batch sort_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<SortKeyArg>& keys,
                   int64_t limit);

// group_concat.cpp: the batches of a group joined into ONE device batch by the concat kernels (a single batch: its device view).
// A Utf8 column whose joined bytes pass int32 offsets is CHQ_ERR_ARROW_INVALID_ARGUMENT, naming the column.
Batch join_group(Context& ctx, const std::vector<Batch>& recs);

}  // namespace chq
