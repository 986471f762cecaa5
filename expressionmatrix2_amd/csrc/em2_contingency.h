// em2_contingency.h -- internal interface of em2_contingency.hip for the C ABI glue (em2_capi.hip).
#ifndef EM2_CONTINGENCY_H
#define EM2_CONTINGENCY_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

namespace em2 {

// The contingency table of two labelings of n items (the `matrix` of ExpressionMatrix::computeMetaDataRandIndex,
// src/ExpressionMatrix.cpp:1369-1381, and what computeRandIndex, src/randIndex.hpp:38-85, sums over it), in host memory.
//   rowTotals [n0], columnTotals [n1]       the items with id0 == i / id1 == j;
//   i0 / i1 / count                         the table cells that are not zero, ascending by (i0, i1);
//   sumCells, sumRows, sumColumns           the sums of v (v - 1) over the cells, of t (t - 1) over the row totals and over
//                                           the column totals.  All three are at most n (n - 1) < 2^64 (n < 2^32).
struct ContingencyResult {
    uint32_t n0 = 0, n1 = 0;
    uint64_t n = 0;
    int path = 0;                                  // the path that ran: kContingencyLds or kContingencySort
    std::vector<uint64_t> rowTotals, columnTotals;
    std::vector<uint32_t> i0, i1;
    std::vector<uint64_t> count;
    uint64_t sumCells = 0, sumRows = 0, sumColumns = 0;
};

constexpr int kContingencyAutomatic = 0;
constexpr int kContingencyLds = 1;                 // a private 32-bit table per workgroup in LDS
constexpr int kContingencySort = 2;                // radix sort of the (id0, id1) keys, then the runs
constexpr uint64_t kContingencyLdsCells = 16384;   // n0 * n1 at most, for the LDS path: 64 KiB of counters

// d_id0 / d_id1 [n] in device memory, n < 2^32, n0 and n1 positive; path: one of the three constants, the LDS path only where
// n0 * n1 <= kContingencyLdsCells (the caller checks all of this).  *inputError is set to 1 and nothing is computed where an
// id0 is not below n0 or an id1 is not below n1: the kernels test an id before they form an address with it.
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
hipError_t runContingency(const uint32_t* d_id0, const uint32_t* d_id1, uint64_t n, uint32_t n0, uint32_t n1, int path,
                          ContingencyResult& out, uint32_t* inputError, hipStream_t stream);

}  // namespace em2

#endif
