// em2_contingency.hip -- the contingency table of two labelings of n cells: what ExpressionMatrix::computeMetaDataRandIndex
// (src/ExpressionMatrix.cpp:1328-1390) fills with two std::map look-ups per cell and what computeRandIndex (src/randIndex.hpp:38-85)
// sums over it, as a histogram of n pairs of integers.  Integer work only: every output is exact, and no
// floating-point number is formed on the device.
//
// The table is kept sparse -- the cells that are not zero as (i0, i1, count), ascending -- because a field with many values
// (createMetaDataFromClusterGraph gives every unclustered cell a value of its own) makes n0 x n1 far larger than n.  Two paths:
//   * LDS path, n0 * n1 <= 16384:
//       ldsCountKernel       every workgroup keeps a private copy of the table as 32-bit counters in LDS (at most 64 KiB), reads
//                            its slice of the two id arrays with 16-byte loads, counts with LDS atomics and adds the counters
//                            that are not zero to the 64-bit table in memory with vector atomics;
//       denseTriplesKernel   one workgroup turns that table into the ascending triples (a scan over its 256 threads);
//   * sort path, any n0 and n1:
//       keysKernel           key = id0 << bits(n1) | id1;
//       a radix sort of the keys over exactly bits(n0) + bits(n1) bits;
//       headFlagsKernel, an inclusive scan of the flags, runStartsKernel, runCountsKernel: a run of equal keys is a table cell.
// Both end the same way: triplesTotalsKernel adds every triple to its row and column total (vector atomics on 64-bit words) and
// sums v (v - 1); pairSumKernel sums t (t - 1) over the row totals and over the column totals.
// Every kernel that reads an id tests it against n0 / n1 before an address is formed with it, writes nothing for an element
// that fails and raises the error word; the host reads that word before anything derived from the ids is used.

#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_runs.h"
#include "em2_scratch.h"
#include "em2_wave.h"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

// What the device code and the C entry points at the end of this file share.
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
static hipError_t runContingency(const uint32_t* d_id0, const uint32_t* d_id1, uint64_t n, uint32_t n0, uint32_t n1, int path,
                                 ContingencyResult& out, uint32_t* inputError, hipStream_t stream);

namespace {

typedef unsigned long long u64;      // (the type HIP's 64-bit atomicAdd takes)

// The bits that hold every id below n (n >= 1): 0 for n == 1.
inline uint32_t bitsFor(uint32_t n)
{
    uint32_t bits = 0;
    while (bits < 32u && (uint64_t(1) << bits) < n) bits++;
    return bits;
}

// The sum of `value` over the 64 lanes, in every lane.
__device__ __forceinline__ u64 waveSumU64(u64 value)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) value += __shfl_xor(value, step, 64);
    return value;
}

// Block b counts the elements [b * perBlock, min(n, (b + 1) * perBlock)); perBlock is a multiple of 4.  Wide: both id arrays
// are 16-byte aligned, so is then every slice's first element.  Dynamic LDS: n0 * n1 counters.
template <bool Wide>
__global__ void __launch_bounds__(256)
ldsCountKernel(const uint32_t* __restrict__ id0, const uint32_t* __restrict__ id1, uint64_t n, uint32_t n0, uint32_t n1,
               uint64_t perBlock, u64* __restrict__ table, uint32_t* __restrict__ error)
{
    extern __shared__ uint32_t counters[];
    const uint32_t cells = n0 * n1;
    for (uint32_t c = threadIdx.x; c < cells; c += 256u) counters[c] = 0u;
    __syncthreads();

    const uint64_t begin = uint64_t(blockIdx.x) * perBlock;
    const uint64_t end = begin < n ? (n - begin < perBlock ? n : begin + perBlock) : begin;
    bool bad = false;
    const auto add = [&](uint32_t a, uint32_t b) {
        if (a < n0 && b < n1) atomicAdd(&counters[a * n1 + b], 1u);
        else bad = true;
    };
    if (Wide) {
        const uint64_t wholeEnd = begin + ((end - begin) & ~uint64_t(3));
        for (uint64_t i = begin + 4u * threadIdx.x; i < wholeEnd; i += 1024u) {
            const uint4 a = *reinterpret_cast<const uint4*>(id0 + i);
            const uint4 b = *reinterpret_cast<const uint4*>(id1 + i);
            add(a.x, b.x);
            add(a.y, b.y);
            add(a.z, b.z);
            add(a.w, b.w);
        }
        const uint64_t i = wholeEnd + threadIdx.x;               // (at most 3 elements, in the last slice only)
        if (i < end) add(id0[i], id1[i]);
    } else {
        for (uint64_t i = begin + threadIdx.x; i < end; i += 256u) add(id0[i], id1[i]);
    }
    __syncthreads();

    for (uint32_t c = threadIdx.x; c < cells; c += 256u) {
        const uint32_t v = counters[c];
        if (v) atomicAdd(&table[c], u64(v));
    }
    if (bad) atomicOr(error, 1u);
}

// One workgroup: the cells of table[cells] that are not zero as (c / n1, c % n1, value), ascending by c; their number to *nnz.
__global__ void __launch_bounds__(256)
denseTriplesKernel(const u64* __restrict__ table, uint32_t cells, uint32_t n1, uint32_t* __restrict__ i0, uint32_t* __restrict__ i1,
                   u64* __restrict__ count, u64* __restrict__ nnz)
{
    __shared__ uint32_t waveTotals[4];
    const uint32_t chunk = (cells + 255u) / 256u;
    const uint32_t begin = threadIdx.x * chunk < cells ? threadIdx.x * chunk : cells;
    const uint32_t end = cells - begin < chunk ? cells : begin + chunk;
    uint32_t mine = 0u;
    for (uint32_t c = begin; c < end; c++) mine += table[c] != 0u ? 1u : 0u;
    const uint32_t inclusive = waveInclusiveScan(mine);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) waveTotals[wave] = inclusive;
    __syncthreads();
    uint32_t at = inclusive - mine;
    for (uint32_t w = 0; w < wave; w++) at += waveTotals[w];
    if (threadIdx.x == 255u) *nnz = u64(at) + mine;
    for (uint32_t c = begin; c < end; c++) {
        const u64 v = table[c];
        if (!v) continue;
        i0[at] = c / n1;
        i1[at] = c % n1;
        count[at] = v;
        at++;
    }
}

// keys[i] = id0[i] << bits1 | id1[i] for the elements whose ids are in range.
__global__ void __launch_bounds__(256)
keysKernel(const uint32_t* __restrict__ id0, const uint32_t* __restrict__ id1, uint64_t n, uint32_t n0, uint32_t n1, uint32_t bits1,
           uint64_t* __restrict__ keys, uint32_t* __restrict__ error)
{
    bool bad = false;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t a = id0[i], b = id1[i];
        if (a < n0 && b < n1) keys[i] = uint64_t(a) << bits1 | b;
        else bad = true;
    }
    if (bad) atomicOr(error, 1u);
}

// rank: the inclusive scan of the flags.  Run r = rank[i] - 1 begins at the i whose flag is set: its first element and its ids.
__global__ void __launch_bounds__(256)
runStartsKernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ rank, uint64_t n,
                uint32_t bits1, uint32_t* __restrict__ starts, uint32_t* __restrict__ i0, uint32_t* __restrict__ i1)
{
    const uint64_t mask1 = (uint64_t(1) << bits1) - 1u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (!flags[i]) continue;
        const uint32_t r = rank[i] - 1u;                         // (rank[i] in [1, i + 1]: r <= i < n, the arrays' size)
        const uint64_t key = keys[i];
        starts[r] = uint32_t(i);
        i0[r] = uint32_t(key >> bits1);
        i1[r] = uint32_t(key & mask1);
    }
}

// count[r] = the length of run r; *nnz = the number of runs = rank[n - 1].
__global__ void __launch_bounds__(256)
runCountsKernel(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ rank, uint64_t n, u64* __restrict__ count,
                u64* __restrict__ nnz)
{
    const uint64_t runs = rank[n - 1u];
    for (uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < runs; r += uint64_t(gridDim.x) * blockDim.x) {
        count[r] = (r + 1u < runs ? uint64_t(starts[r + 1u]) : n) - starts[r];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *nnz = runs;
}

// rowTotals[i0] += count, columnTotals[i1] += count for every triple (the ids were tested where the triples were made);
// *sumCells += v (v - 1).
__global__ void __launch_bounds__(256)
triplesTotalsKernel(const uint32_t* __restrict__ i0, const uint32_t* __restrict__ i1, const u64* __restrict__ count,
                    const u64* __restrict__ nnz, u64* __restrict__ rowTotals, u64* __restrict__ columnTotals, u64* __restrict__ sumCells)
{
    const uint64_t triples = *nnz;
    u64 sum = 0u;
    for (uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < triples; r += uint64_t(gridDim.x) * blockDim.x) {
        const u64 v = count[r];
        atomicAdd(&rowTotals[i0[r]], v);
        atomicAdd(&columnTotals[i1[r]], v);
        sum += v * (v - 1u);
    }
    sum = waveSumU64(sum);
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(sumCells, sum);
}

// *sum += t (t - 1) over totals[count].
__global__ void __launch_bounds__(256)
pairSumKernel(const u64* __restrict__ totals, uint32_t count, u64* __restrict__ sum)
{
    u64 mine = 0u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const u64 t = totals[i];
        if (t) mine += t * (t - 1u);
    }
    mine = waveSumU64(mine);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(sum, mine);
}

template <class T> hipError_t toHost(std::vector<T>& to, const void* from, size_t count, hipStream_t stream)
{
    to.resize(count);
    if (count == 0) return hipSuccess;
    return hipMemcpyAsync(to.data(), from, count * sizeof(T), hipMemcpyDeviceToHost, stream);
}

}  // namespace

hipError_t runContingency(const uint32_t* d_id0, const uint32_t* d_id1, uint64_t n, uint32_t n0, uint32_t n1, int path,
                          ContingencyResult& out, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    out = ContingencyResult();
    out.n0 = n0;
    out.n1 = n1;
    out.n = n;
    const uint64_t cells64 = uint64_t(n0) * n1;
    const bool lds = path == kContingencyLds || (path == kContingencyAutomatic && cells64 <= kContingencyLdsCells);
    out.path = lds ? kContingencyLds : kContingencySort;
    out.rowTotals.assign(n0, 0u);
    out.columnTotals.assign(n1, 0u);
    if (n == 0) return hipSuccess;

    StageTimer timer(lds ? "contingency (LDS)" : "contingency (sort)");
    const dim3 threads(256);
    const size_t capacity = lds ? size_t(cells64) : size_t(n);            // of the triples: the cells that are not zero
    ArenaPlan plan;
    // (everything up to offZeroEnd starts as zero)
    const size_t offWords = plan.take(256);                                 // error, nnz, the three sums
    const size_t offRowTotals = plan.takeFor<u64>(n0);
    const size_t offColumnTotals = plan.takeFor<u64>(n1);
    const size_t offTable = plan.take(lds ? size_t(cells64) * sizeof(u64) : 0u);
    const size_t offZeroEnd = plan.bytes;
    const size_t offI0 = plan.takeFor<uint32_t>(capacity);
    const size_t offI1 = plan.takeFor<uint32_t>(capacity);
    const size_t offCount = plan.takeFor<u64>(capacity);
    size_t offKeysA = 0, offKeysB = 0, offFlags = 0, offRank = 0, offStarts = 0, offTemp = 0, sortBytes = 0, scanBytes = 0;
    const uint32_t bits1 = bitsFor(n1);
    const uint32_t keyBits = bitsFor(n0) + bits1 ? bitsFor(n0) + bits1 : 1u;      // (n0 == n1 == 1: every key is 0, one bit)
    if (!lds) {
        offKeysA = plan.takeFor<uint64_t>(n);
        offKeysB = plan.takeFor<uint64_t>(n);
        offFlags = plan.takeFor<uint32_t>(n);
        offRank = plan.takeFor<uint32_t>(n);
        offStarts = plan.takeFor<uint32_t>(n);
        EM2_TRY(sortKeysBufferBytes(size_t(n), 0u, keyBits, sortBytes));
        EM2_TRY(inclusiveScanBytes(size_t(n), scanBytes));
        offTemp = plan.take(sortBytes > scanBytes ? sortBytes : scanBytes);
    }
    CachedBuffer arena;
    EM2_TRY(arena.allocate(plan.bytes));
    char* base = arena.as<char>();
    uint32_t* error = arenaAt<uint32_t>(base, offWords);
    u64* nnz = arenaAt<u64>(base, offWords + 8);
    u64* sums = arenaAt<u64>(base, offWords + 16);                          // cells, rows, columns
    u64* rowTotals = arenaAt<u64>(base, offRowTotals);
    u64* columnTotals = arenaAt<u64>(base, offColumnTotals);
    u64* table = arenaAt<u64>(base, offTable);
    uint32_t* i0 = arenaAt<uint32_t>(base, offI0);
    uint32_t* i1 = arenaAt<uint32_t>(base, offI1);
    u64* count = arenaAt<u64>(base, offCount);
    EM2_TRY(hipMemsetAsync(base, 0, offZeroEnd, stream));

    // an id out of range: nothing was written for it, and nothing below may use what the kernel left
    const auto inputChecked = [&]() -> hipError_t {
        EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        return hipStreamSynchronize(stream);
    };

    if (lds) {
        // slices of at least four elements per table cell, so that adding a workgroup's table to memory does not cost more
        // than counting; at most two workgroups for each of the 256 CUs
        const uint64_t atLeast = 4u * cells64 > 4096u ? 4u * cells64 : 4096u;
        uint64_t blocks = (n + atLeast - 1u) / atLeast;
        if (blocks > 512u) blocks = 512u;
        const uint64_t perBlock = ((n + blocks - 1u) / blocks + 3u) & ~uint64_t(3);
        blocks = (n + perBlock - 1u) / perBlock;
        const size_t ldsBytes = size_t(cells64) * sizeof(uint32_t);
        const bool wide = ((reinterpret_cast<uintptr_t>(d_id0) | reinterpret_cast<uintptr_t>(d_id1)) & 15u) == 0u;
        const void* kernel = wide ? reinterpret_cast<const void*>(&ldsCountKernel<true>) : reinterpret_cast<const void*>(&ldsCountKernel<false>);
        EM2_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(kContingencyLdsCells * sizeof(uint32_t))));
        if (wide) {
            ldsCountKernel<true><<<dim3(uint32_t(blocks)), threads, ldsBytes, stream>>>(d_id0, d_id1, n, n0, n1, perBlock, table, error);
        } else {
            ldsCountKernel<false><<<dim3(uint32_t(blocks)), threads, ldsBytes, stream>>>(d_id0, d_id1, n, n0, n1, perBlock, table, error);
        }
        EM2_TRY(hipGetLastError());
        EM2_TRY(inputChecked());
        if (*inputError) {
            arena.idle = true;
            return hipSuccess;
        }
        EM2_TRY(timer.stage("count", stream));
        denseTriplesKernel<<<dim3(1), threads, 0, stream>>>(table, uint32_t(cells64), n1, i0, i1, count, nnz);
        EM2_TRY(hipGetLastError());
    } else {
        DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, offKeysA), arenaAt<uint64_t>(base, offKeysB)};
        uint32_t* flags = arenaAt<uint32_t>(base, offFlags);
        uint32_t* rank = arenaAt<uint32_t>(base, offRank);
        uint32_t* starts = arenaAt<uint32_t>(base, offStarts);
        keysKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(d_id0, d_id1, n, n0, n1, bits1, keys.current(), error);
        EM2_TRY(hipGetLastError());
        EM2_TRY(inputChecked());
        if (*inputError) {
            arena.idle = true;
            return hipSuccess;
        }
        EM2_TRY(timer.stage("keys", stream));
        EM2_TRY(sortKeys(base + offTemp, sortBytes, keys, size_t(n), 0u, keyBits, stream));
        EM2_TRY(timer.stage("sort", stream));
        const uint64_t* sorted = keys.current();
        headFlagsKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(sorted, n, flags);
        EM2_TRY(hipGetLastError());
        EM2_TRY(inclusiveScan(base + offTemp, scanBytes, flags, rank, size_t(n), stream));
        runStartsKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(sorted, flags, rank, n, bits1, starts, i0, i1);
        EM2_TRY(hipGetLastError());
        runCountsKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(starts, rank, n, count, nnz);
        EM2_TRY(hipGetLastError());
    }
    EM2_TRY(timer.stage("triples", stream));

    triplesTotalsKernel<<<dim3(gridFor(capacity)), threads, 0, stream>>>(i0, i1, count, nnz, rowTotals, columnTotals, sums);
    EM2_TRY(hipGetLastError());
    pairSumKernel<<<dim3(gridFor(n0)), threads, 0, stream>>>(rowTotals, n0, sums + 1);
    EM2_TRY(hipGetLastError());
    pairSumKernel<<<dim3(gridFor(n1)), threads, 0, stream>>>(columnTotals, n1, sums + 2);
    EM2_TRY(hipGetLastError());
    u64 words[4] = {0, 0, 0, 0};                                            // nnz and the three sums
    EM2_TRY(hipMemcpyAsync(words, nnz, sizeof(words), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("totals and sums", stream));
    if (words[0] > capacity) {
        arena.idle = true;
        return hipErrorUnknown;
    }
    out.sumCells = words[1];
    out.sumRows = words[2];
    out.sumColumns = words[3];
    EM2_TRY(toHost(out.rowTotals, rowTotals, n0, stream));
    EM2_TRY(toHost(out.columnTotals, columnTotals, n1, stream));
    EM2_TRY(toHost(out.i0, i0, size_t(words[0]), stream));
    EM2_TRY(toHost(out.i1, i1, size_t(words[0]), stream));
    EM2_TRY(toHost(out.count, count, size_t(words[0]), stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("results to the host", stream));
    arena.idle = true;                                                      // (everything that used the block has been waited for)
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

struct em2_contingency {
    em2::ContingencyResult result;
};

static int contingencyCreate(const char* who, bool idsOnDevice, const uint32_t* id0, const uint32_t* id1, uint64_t n, uint32_t n0,
                             uint32_t n1, int path, em2_contingency** out)
{
    if (!out) return failNull(who);
    *out = nullptr;
    if (n && (!id0 || !id1)) return failNull(who);
    if (n0 == 0 || n1 == 0) return failArgument(who, "n0 and n1 must be positive");
    if (path != em2::kContingencyAutomatic && path != em2::kContingencyLds && path != em2::kContingencySort) {
        return failArgument(who, "path must be 0 (automatic), 1 (LDS) or 2 (sort)");
    }
    if (path == em2::kContingencyLds && uint64_t(n0) * n1 > em2::kContingencyLdsCells) {
        return fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the LDS path holds a table of at most " +
                                                    std::to_string(em2::kContingencyLdsCells) + " cells");
    }
    // (the three sums are at most n (n - 1), and a run's first element is kept in 32 bits)
    if (n > 0xffffffffull) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 elements are not supported");
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer d0, d1;
    if (!idsOnDevice && n) {
        EM2_HIP(d0.upload(id0, size_t(n)));
        EM2_HIP(d1.upload(id1, size_t(n)));
    }
    std::unique_ptr<em2_contingency> c(new em2_contingency);
    uint32_t inputError = 0;
    const hipError_t status = em2::runContingency(idsOnDevice || !n ? id0 : d0.as<uint32_t>(), idsOnDevice || !n ? id1 : d1.as<uint32_t>(), n,
                                                  n0, n1, path, c->result, &inputError, nullptr);
    if (status != hipSuccess || inputError) {
        EM2_HIP(status);
        return failArgument(who, "an id is not below its count (id0 < n0, id1 < n1)");
    }
    *out = c.release();
    return EM2_OK;
}

int em2_contingency_create(const uint32_t* id0, const uint32_t* id1, uint64_t n, uint32_t n0, uint32_t n1, int path, em2_contingency** out)
{
    return contingencyCreate("em2_contingency", false, id0, id1, n, n0, n1, path, out);
}

int em2_dev_contingency(const uint32_t* d_id0, const uint32_t* d_id1, uint64_t n, uint32_t n0, uint32_t n1, int path, em2_contingency** out)
{
    return contingencyCreate("em2_dev_contingency", true, d_id0, d_id1, n, n0, n1, path, out);
}

int em2_contingency_sizes(const em2_contingency* table, uint32_t* n0, uint32_t* n1, uint64_t* n, uint64_t* nonZeroCount, int* path)
{
    if (!table) return failNull("em2_contingency_sizes");
    const em2::ContingencyResult& r = table->result;
    if (n0) *n0 = r.n0;
    if (n1) *n1 = r.n1;
    if (n) *n = r.n;
    if (nonZeroCount) *nonZeroCount = r.count.size();
    if (path) *path = r.path;
    return EM2_OK;
}

int em2_contingency_get(const em2_contingency* table, uint64_t* rowTotals, uint64_t* columnTotals, uint32_t* i0, uint32_t* i1,
                        uint64_t* count, uint64_t* sums)
{
    if (!table) return failNull("em2_contingency_get");
    const em2::ContingencyResult& r = table->result;
    if (rowTotals) std::copy(r.rowTotals.begin(), r.rowTotals.end(), rowTotals);
    if (columnTotals) std::copy(r.columnTotals.begin(), r.columnTotals.end(), columnTotals);
    if (i0) std::copy(r.i0.begin(), r.i0.end(), i0);
    if (i1) std::copy(r.i1.begin(), r.i1.end(), i1);
    if (count) std::copy(r.count.begin(), r.count.end(), count);
    if (sums) {
        sums[0] = r.sumCells;
        sums[1] = r.sumRows;
        sums[2] = r.sumColumns;
    }
    return EM2_OK;
}

void em2_contingency_free(em2_contingency* table) { delete table; }

}  // extern "C"
