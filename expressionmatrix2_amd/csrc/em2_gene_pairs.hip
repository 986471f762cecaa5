// em2_gene_pairs.hip -- ExpressionMatrix::findSimilarGenePairs0 (src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198): the
// Pearson correlation of every pair of genes over the cells of a cell set, the k best partners of every gene.
//
// The reference builds a dense float vector per gene (ExpressionMatrixSubset::getDenseRepresentation,
// src/ExpressionMatrixSubset.cpp:142-174), normalises the cells (L1 / L2 / none), shifts and scales every gene to zero mean
// and unit norm (:117-135), and then computes r(g0, g1) = std::inner_product(x0, x1, 0.f) for every unordered pair (:153-177):
// a float multiplication, then a float addition, per cell, in ascending cell order.  Here:
//   * cellSumsKernel        computeSums and the checks the scatter's bounds rest on (em2_expression.h);
//   * denseCellsKernel      the dense matrix, CELL-major (dense[cell][gene], the gene pitch a multiple of the tile), and the
//                           cell normalisation: a block per cell, so the walk is contiguous;
//   * standardizeKernel     :117-135 literally, a thread per gene walking the cells in ascending order (neighbouring threads
//                           read neighbouring floats); the two double sums keep the reference's order;
//   * genePairsKernel       the hot path.  A block owns a 128 x 128 tile of gene pairs of the upper triangle (tile row <=
//                           tile column: every unordered pair once); 16 cells of both gene ranges are staged through LDS per
//                           step while the next 16 are in flight in registers; a thread keeps 8 x 8 accumulators, each a
//                           strict chain acc = acc + (a * b) over the cells in ascending order (two accumulators per packed
//                           instruction; -ffp-contract=off, no FMA: the reference targets SSE4.2).  A pair with double(r) >
//                           similarityThreshold is written in both directions as (gene << 32 | partner, r) into one stream
//                           behind a cursor that one atomic per wave advances and that keeps counting past the capacity;
//   * rocPRIM's radix sort on the 64-bit key puts every gene's candidates together in ascending partner id, the order in which
//     the reference's loop appends them (:165-166);
//   * selectGenesKernel     keepBest (src/heap.hpp:116-126) per gene: where a list is longer than k, em2_select.h's
//                           introselect over {partner, -r} (x.key < y.key  <=>  x.second > y.second, +-0 included; NaN never
//                           gets here), in LDS where the list fits and on the segment in global memory where it does not; the
//                           first k are kept in the arrangement it leaves.
// The final std::sort by similarity alone (:186) runs on the host on that arrangement (em2_host.cpp: libstdc++'s introsort
// itself, as in the reference).

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"
#include "em2_primitives.h"
#include "em2_wave.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <string>

namespace em2 {
namespace {

constexpr uint32_t kTile = 128;                  // genes per side of a block's tile
constexpr uint32_t kChunk = 16;                  // cells staged through LDS per step
constexpr uint32_t kPairThreads = 256;           // 16 x 16 threads, 8 x 8 pairs each
constexpr uint32_t kSelectLdsEntries = 8192;     // a list of up to this many candidates is selected in LDS (64 KiB)

typedef float Float2 __attribute__((ext_vector_type(2)));
typedef float Float4 __attribute__((ext_vector_type(4)));

struct CellSums {
    double sum1, sum2;        // ExpressionMatrixSubset::Sum
};

// {partner, -similarity}: the element em2_select.h's introselect works on.
struct GeneEntry {
    uint32_t gene;
    float key;
};

// computeSums and the input check (em2_expression.h).  A thread per cell, striding over the grid (gridFor caps it).
__global__ void __launch_bounds__(256)
cellSumsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
               CellSums* __restrict__ sums, uint32_t* __restrict__ error)
{
    uint32_t bad = 0u;
    for (uint64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cellCount; c += uint64_t(gridDim.x) * blockDim.x) {
        const CellWalk w = walkCell(toc, data, c, geneCount);
        sums[c].sum1 = w.sum1;
        sums[c].sum2 = w.sum2;
        bad |= w.bad;
    }
    if (bad) atomicOr(error, bad);
}

// getDenseRepresentation (:142-174) for the cells blockIdx.x, + gridDim.x, ...: the row is zero on entry.  Every entry of the
// cell is multiplied by the factor, zeros included, so a factor that is not finite makes the whole cell NaN, as in the reference.
__global__ void __launch_bounds__(256)
denseCellsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const CellSums* __restrict__ sums,
                 uint32_t cellCount, uint32_t geneCount, uint32_t pitch, int method, float* __restrict__ dense)
{
    for (uint32_t cell = blockIdx.x; cell < cellCount; cell += gridDim.x) {
        float* row = dense + size_t(cell) * pitch;
        const uint64_t end = toc[cell + 1u];
        for (uint64_t p = toc[cell] + threadIdx.x; p < end; p += blockDim.x) {
            const CountIn e = data[p];
            row[e.gene] = e.count;
        }
        if (method == 0) continue;
        const CellSums s = sums[cell];
        const double scaling = method == 1 ? s.sum1 : __dsqrt_rn(s.sum2);
        if (scaling != 0.) {                                                   // (uniform over the block)
            const float factor = float(__ddiv_rn(1., scaling));
            __syncthreads();
            for (uint32_t g = threadIdx.x; g < geneCount; g += blockDim.x) row[g] *= factor;
        }
    }
}

// :117-135 for gene g: sum (double) over the cells ascending, average = float(sum / cellCount), x -= average, sum2 (double) of
// the float products x*x, factor = float(1 / sqrt(sum2)), x *= factor.  x - average is computed twice (for sum2 and for the
// result) instead of being stored in between: the same float operation on the same operands.  The loads of a batch do not
// depend on the sums and are issued together; the sums stay sequential.
__global__ void __launch_bounds__(64)
standardizeKernel(float* __restrict__ dense, uint32_t cellCount, uint32_t geneCount, uint32_t pitch)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= geneCount) return;
    float* column = dense + g;
    constexpr uint32_t kBatch = 16;
    float v[kBatch];
    double sum = 0.;
    uint32_t c = 0;
    for (; c + kBatch <= cellCount; c += kBatch) {
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) v[i] = column[size_t(c + i) * pitch];
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) sum += double(v[i]);
    }
    for (; c < cellCount; ++c) sum += double(column[size_t(c) * pitch]);
    const float average = float(__ddiv_rn(sum, double(cellCount)));
    double sum2 = 0.;
    for (c = 0; c + kBatch <= cellCount; c += kBatch) {
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) v[i] = column[size_t(c + i) * pitch];
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) {
            const float x = v[i] - average;
            sum2 += double(x * x);
        }
    }
    for (; c < cellCount; ++c) {
        const float x = column[size_t(c) * pitch] - average;
        sum2 += double(x * x);
    }
    const float factor = float(__ddiv_rn(1., __dsqrt_rn(sum2)));
    for (c = 0; c + kBatch <= cellCount; c += kBatch) {
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) v[i] = column[size_t(c + i) * pitch];
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) column[size_t(c + i) * pitch] = (v[i] - average) * factor;
    }
    for (; c < cellCount; ++c) column[size_t(c) * pitch] = (column[size_t(c) * pitch] - average) * factor;
}

// One cell of the tile: 8 genes of the row range and 8 of the column range from LDS (two 16-byte reads each: the 16 threads
// of a row read 256 contiguous bytes), 64 multiplications and 64 additions.
__device__ __forceinline__ void pairStep(const Float4 (*tileA)[kTile / 4], const Float4 (*tileB)[kTile / 4], uint32_t c, uint32_t ty,
                                         uint32_t tx, Float2 (&acc)[8][4])
{
    const Float4 a0 = tileA[c][ty], a1 = tileA[c][16u + ty];
    const Float4 b0 = tileB[c][tx], b1 = tileB[c][16u + tx];
    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const Float2 b[4] = {Float2{b0.x, b0.y}, Float2{b0.z, b0.w}, Float2{b1.x, b1.y}, Float2{b1.z, b1.w}};
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const Float2 product = Float2{a[i], a[i]} * b[j];        // rounded
            acc[i][j] = acc[i][j] + product;                          // rounded again: never an FMA
        }
    }
}

// dense[cellRows][pitch] with pitch a multiple of kTile and cellRows a multiple of kChunk; the genes from geneCount on and the
// cells from cellCount on are zero.  The former are never emitted.  The latter are walked, behind the last cell, and change
// no bit: their products are 0 * 0 = +0, and acc + (+0) is acc for every acc but -0, which a chain that starts at +0 never
// holds (a float sum is -0 only if both terms are); NaN and inf stay what they are.
// keys / values: the stream, `capacity` records; *cursor counts every record, written or not.  all: NULL or [geneCount][geneCount].
__global__ void __launch_bounds__(kPairThreads, 4)
genePairsKernel(const float* __restrict__ dense, uint32_t pitch, uint32_t cellCount, uint32_t geneCount, double similarityThreshold,
                uint64_t* __restrict__ keys, float* __restrict__ values, uint64_t capacity, unsigned long long* __restrict__ cursor,
                float* __restrict__ all)
{
    const uint32_t tileRow = blockIdx.y, tileColumn = blockIdx.x;
    if (tileRow > tileColumn) return;                                         // the triangle (uniform over the block)
    __shared__ Float4 tileA[kChunk][kTile / 4];
    __shared__ Float4 tileB[kChunk][kTile / 4];
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15u;
    // staging: a tile step is kChunk rows of 32 Float4; thread tid moves Float4 (tid & 31) of the rows (tid >> 5) and + 8
    const uint32_t stageColumn = tid & 31u, stageRow = tid >> 5;
    const size_t pitch4 = pitch / 4u;
    const Float4* sourceA = reinterpret_cast<const Float4*>(dense) + size_t(tileRow) * (kTile / 4) + stageColumn;
    const Float4* sourceB = reinterpret_cast<const Float4*>(dense) + size_t(tileColumn) * (kTile / 4) + stageColumn;

    Float2 acc[8][4];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = Float2{0.f, 0.f};
    }

    const uint32_t chunks = (cellCount + kChunk - 1u) / kChunk;
    Float4 nextA[2], nextB[2];
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        nextA[h] = sourceA[size_t(stageRow + 8u * h) * pitch4];
        nextB[h] = sourceB[size_t(stageRow + 8u * h) * pitch4];
    }
    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
        __syncthreads();                                                       // the previous step's reads are done
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            tileA[stageRow + 8u * h][stageColumn] = nextA[h];
            tileB[stageRow + 8u * h][stageColumn] = nextB[h];
        }
        __syncthreads();
        if (chunk + 1u < chunks) {
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                const size_t row = size_t(chunk + 1u) * kChunk + stageRow + 8u * h;
                nextA[h] = sourceA[row * pitch4];
                nextB[h] = sourceB[row * pitch4];
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < kChunk; ++c) pairStep(tileA, tileB, c, ty, tx, acc);
    }

    // the thread's pairs: rows {4 ty + i, 64 + 4 ty + i}, columns {4 tx + j, 64 + 4 tx + j} of the tile, i, j < 4
    const uint32_t rowBase = tileRow * kTile + 4u * ty, columnBase = tileColumn * kTile + 4u * tx;
    const bool diagonal = tileRow == tileColumn;
    uint32_t mine = 0;
    uint64_t survivorBits = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t g0 = rowBase + (i & 3u) + 64u * (i >> 2), g1 = columnBase + (j & 3u) + 64u * (j >> 2);
            const float r = (j & 1u) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
            const bool valid = g0 < geneCount && g1 < geneCount && (diagonal ? g0 < g1 : true);
            if (valid && all) {
                all[size_t(g0) * geneCount + g1] = r;
                all[size_t(g1) * geneCount + g0] = r;
            }
            if (valid && double(r) > similarityThreshold) {                  // :163, float > double; false for NaN
                ++mine;
                survivorBits |= 1ull << (i * 8u + j);
            }
        }
    }
    // one cursor advance per wave: the lanes' counts, an inclusive scan, the last lane draws for all
    const uint32_t lane = tid & 63u;
    const uint32_t inclusive = waveInclusiveScan(mine);
    const uint32_t total = uint32_t(__shfl(int(inclusive), 63, 64));
    if (total == 0u) return;                                                   // (uniform over the wave)
    unsigned long long base = 0;
    if (lane == 63u) base = atomicAdd(cursor, 2ull * total);
    base = (unsigned long long)(__shfl((long long)(base), 63, 64));
    uint64_t at = base + 2ull * (inclusive - mine);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (!((survivorBits >> (i * 8u + j)) & 1ull)) continue;
            const uint32_t g0 = rowBase + (i & 3u) + 64u * (i >> 2), g1 = columnBase + (j & 3u) + 64u * (j >> 2);
            const float r = (j & 1u) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
            if (at < capacity) {
                keys[at] = uint64_t(g0) << 32 | g1;
                values[at] = r;
            }
            if (at + 1u < capacity) {
                keys[at + 1u] = uint64_t(g1) << 32 | g0;
                values[at + 1u] = r;
            }
            at += 2u;
        }
    }
}

__device__ __forceinline__ uint64_t lowerBound(const uint64_t* __restrict__ sorted, uint64_t count, uint64_t key)
{
    uint64_t low = 0, high = count;
    while (low < high) {
        const uint64_t middle = low + (high - low) / 2u;
        if (sorted[middle] < key) low = middle + 1u;
        else high = middle;
    }
    return low;
}

// offsets[g] = the first record of gene g in the sorted stream, offsets[geneCount] = count; *longest = the longest list that
// needs a selection (longer than k).  A thread per gene, striding over the grid.
__global__ void __launch_bounds__(256)
geneOffsetsKernel(const uint64_t* __restrict__ sortedKeys, uint64_t count, uint32_t geneCount, uint32_t k, uint64_t* __restrict__ offsets,
                  uint32_t* __restrict__ longest)
{
    for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < geneCount; g += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t begin = lowerBound(sortedKeys, count, g << 32);
        const uint64_t end = g + 1u == geneCount ? count : lowerBound(sortedKeys, count, (g + 1u) << 32);
        offsets[g] = begin;
        if (g + 1u == geneCount) offsets[geneCount] = count;
        if (end - begin > k) atomicMax(longest, uint32_t(end - begin));
    }
}

// keepBest for the genes blockIdx.x, + gridDim.x, ...: a wave per gene.  entries: 8 bytes per record of the stream (the sort's
// input buffer, free by now), used by the lists that do not fit ldsEntries.
__global__ void __launch_bounds__(64)
selectGenesKernel(const uint64_t* __restrict__ sortedKeys, const float* __restrict__ sortedValues, const uint64_t* __restrict__ offsets,
                  uint32_t geneCount, uint32_t k, uint32_t ldsEntries, GeneEntry* __restrict__ entries, PairOut* __restrict__ outPairs,
                  uint32_t* __restrict__ outUsed)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    GeneEntry* inLds = reinterpret_cast<GeneEntry*>(ldsRaw);
    const uint32_t lane = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < geneCount; g += gridDim.x) {
        const uint64_t begin = offsets[g];
        const uint32_t n = uint32_t(offsets[g + 1u] - begin);
        PairOut* out = outPairs + size_t(g) * k;
        if (n <= k) {                                                          // keepBest leaves the list alone (heap.hpp:118)
            for (uint32_t t = lane; t < n; t += 64u) out[t] = PairOut{uint32_t(sortedKeys[begin + t]), sortedValues[begin + t]};
            if (lane == 0) outUsed[g] = n;
            continue;
        }
        if (n <= ldsEntries) {
            for (uint32_t t = lane; t < n; t += 64u) inLds[t] = GeneEntry{uint32_t(sortedKeys[begin + t]), -sortedValues[begin + t]};
            waveSync();
            if (lane == 0) nthElement(inLds, int(k), int(n));
            waveSync();
            for (uint32_t t = lane; t < k; t += 64u) out[t] = PairOut{inLds[t].gene, -inLds[t].key};
            waveSync();
        } else {
            GeneEntry* inMemory = entries + begin;
            for (uint32_t t = lane; t < n; t += 64u) inMemory[t] = GeneEntry{uint32_t(sortedKeys[begin + t]), -sortedValues[begin + t]};
            waveSyncGlobal();
            if (lane == 0) nthElement(inMemory, int(k), int(n));
            waveSyncGlobal();
            for (uint32_t t = lane; t < k; t += 64u) out[t] = PairOut{inMemory[t].gene, -inMemory[t].key};
        }
        if (lane == 0) outUsed[g] = k;
    }
}

class GenePairsTimer {
public:
    GenePairsTimer() : on_(getenv("EM2_TIMING") && getenv("EM2_TIMING")[0] == '1'), last_(std::chrono::steady_clock::now()) {}
    // (the caller has synchronised the stream)
    void stage(const char* name)
    {
        if (!on_) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[em2 timing] findSimilarGenePairs0: %s %.3f ms\n", name, std::chrono::duration<double, std::milli>(now - last_).count());
        last_ = now;
    }
    bool on() const { return on_; }
private:
    bool on_;
    std::chrono::steady_clock::time_point last_;
};

}  // namespace


// The stream's budget.  Process-wide; the library reads no environment variable for it (its table of those is full,
// tests/test_capi_cpu.py): em2_set_gene_pairs_buffer_mb sets it, and the Python binding calls that with EM2_GENE_PAIRS_BUFFER_MB.
static std::atomic<uint64_t> genePairsBudgetMegabytes{4096};

void setGenePairsBudgetMegabytes(uint64_t megabytes) { genePairsBudgetMegabytes.store(megabytes); }

uint64_t genePairsBudgetRecords() { return genePairsBudgetMegabytes.load() * (1024ull * 1024ull) / kGenePairsBytesPerRecord; }

// d_toc / d_data: the subset's CSR on the device (toc from 0).  d_pairs [geneCount][k] and d_used [geneCount] receive every
// gene's kept candidates in the arrangement keepBest leaves (unused slots zero); the caller sorts them.  d_all: NULL or
// [geneCount][geneCount] floats, every r (the diagonal is left as it is).  Allocates its own scratch; synchronises the stream.
hipError_t runGenePairs(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, int method, uint32_t k,
                        double similarityThreshold, PairOut* d_pairs, uint32_t* d_used, float* d_all, GenePairsStatus* status,
                        hipStream_t stream)
{
    *status = GenePairsStatus();
    GenePairsTimer timer;
    const uint32_t pitch = blocksOf(geneCount, kTile) * kTile, cellRows = blocksOf(cellCount, kChunk) * kChunk;
    DeviceBuffer sums, words, dense;
    EM2_TRY(sums.allocate(size_t(cellCount) * sizeof(CellSums)));
    EM2_TRY(words.allocate(256));                         // [0] input error, [1] longest list, [2..3] the cursor
    EM2_TRY(hipMemsetAsync(words.p, 0, 256, stream));
    uint32_t* error = words.as<uint32_t>();
    uint32_t* longest = error + 1;
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(error + 2);
    cellSumsKernel<<<dim3(gridFor(cellCount)), dim3(256), 0, stream>>>(d_toc, d_data, cellCount, geneCount, sums.as<CellSums>(), error);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(&status->inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (status->inputError) return hipSuccess;

    EM2_TRY(dense.allocate(size_t(cellRows) * pitch * sizeof(float)));
    EM2_TRY(hipMemsetAsync(dense.p, 0, size_t(cellRows) * pitch * sizeof(float), stream));
    EM2_TRY(hipMemsetAsync(d_pairs, 0, size_t(geneCount) * k * sizeof(PairOut), stream));
    EM2_TRY(hipMemsetAsync(d_used, 0, size_t(geneCount) * sizeof(uint32_t), stream));
    denseCellsKernel<<<dim3(cellCount < 65536u ? cellCount : 65536u), dim3(256), 0, stream>>>(
        d_toc, d_data, sums.as<CellSums>(), cellCount, geneCount, pitch, method, dense.as<float>());
    standardizeKernel<<<dim3((geneCount + 63u) / 64u), dim3(64), 0, stream>>>(dense.as<float>(), cellCount, geneCount, pitch);
    EM2_TRY(hipGetLastError());
    if (timer.on()) EM2_TRY(hipStreamSynchronize(stream));
    timer.stage("dense vectors");

    // the stream: the worst case where the budget holds it, else the budget; once more with the exact size when that was too small
    const uint64_t worstCase = uint64_t(geneCount) * (geneCount - 1u);
    uint64_t capacity = worstCase < genePairsBudgetRecords() ? worstCase : genePairsBudgetRecords();
    const uint32_t tiles = pitch / kTile;
    DeviceBuffer keysA, keysB, valuesA, valuesB, temp, offsets;
    uint64_t count = 0;
    for (int run = 0; run < 2; ++run) {
        EM2_TRY(keysA.allocate(capacity * sizeof(uint64_t)));
        EM2_TRY(valuesA.allocate(capacity * sizeof(float)));
        EM2_TRY(hipMemsetAsync(cursor, 0, sizeof(unsigned long long), stream));
        if (timer.on()) EM2_TRY(hipStreamSynchronize(stream));
        timer.stage("stream allocation");                                      // (kept out of the pair kernel's time)
        genePairsKernel<<<dim3(tiles, tiles), dim3(kPairThreads), 0, stream>>>(
            dense.as<float>(), pitch, cellCount, geneCount, similarityThreshold, keysA.as<uint64_t>(), valuesA.as<float>(), capacity,
            cursor, run == 0 ? d_all : nullptr);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(&count, cursor, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        timer.stage(run == 0 ? "pair kernel" : "pair kernel (again, exact size)");
        status->records = count;
        status->runs = run + 1;
        if (count <= capacity) break;
        // too small: the exact size, if the device has it (the sort needs every buffer twice, and its own scratch)
        keysA.release();
        valuesA.release();
        size_t freeBytes = 0, totalBytes = 0;
        EM2_TRY(hipMemGetInfo(&freeBytes, &totalBytes));
        if (run == 1 || count > freeBytes / (kGenePairsBytesPerRecord + 8u)) {
            status->overflow = true;
            status->freeBytes = freeBytes;
            return hipSuccess;
        }
        capacity = count;
    }

    // (the sort alternates between the stream and a second buffer of its size and says where the result is)
    EM2_TRY(keysB.allocate(count * sizeof(uint64_t)));
    EM2_TRY(valuesB.allocate(count * sizeof(float)));
    EM2_TRY(offsets.allocate((size_t(geneCount) + 1u) * sizeof(uint64_t)));
    DoubleBuffer<uint64_t> keys{keysA.as<uint64_t>(), keysB.as<uint64_t>()};
    DoubleBuffer<float> values{valuesA.as<float>(), valuesB.as<float>()};
    if (count) {
        uint32_t geneBits = 1;
        while (geneBits < 32u && (1ull << geneBits) < geneCount) ++geneBits;
        size_t tempBytes = 0;
        EM2_TRY(sortPairsU64F32BufferBytes(size_t(count), 0u, 32u + geneBits, tempBytes));
        EM2_TRY(temp.allocate(tempBytes));
        EM2_TRY(sortPairs(temp.p, tempBytes, keys, values, size_t(count), 0u, 32u + geneBits, stream));
    }
    geneOffsetsKernel<<<dim3(gridFor(geneCount)), dim3(256), 0, stream>>>(keys.current(), count, geneCount, k, offsets.as<uint64_t>(), longest);
    EM2_TRY(hipGetLastError());
    uint32_t longestList = 0;
    EM2_TRY(hipMemcpyAsync(&longestList, longest, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    timer.stage("sort");

    const uint32_t ldsEntries = longestList < kSelectLdsEntries ? longestList : kSelectLdsEntries;
    const size_t ldsBytes = size_t(ldsEntries) * sizeof(GeneEntry);
    EM2_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&selectGenesKernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(ldsBytes)));
    selectGenesKernel<<<dim3(geneCount < 65536u ? geneCount : 65536u), dim3(64), ldsBytes, stream>>>(
        keys.current(), values.current(), offsets.as<uint64_t>(), geneCount, k, ldsEntries, reinterpret_cast<GeneEntry*>(keys.alternate()),
        d_pairs, d_used);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    timer.stage("selection");
    status->longestList = longestList;
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

// std::sort by similarity alone, per gene (em2_host.cpp).
extern "C" void em2_internal_sort_gene_pairs(em2_pair* pairs, const uint32_t* usedCount, uint32_t geneCount, uint32_t k);

static const uint32_t kAllSimilaritiesMaxGenes = 8192;          // allSimilarities: 256 MB of floats at most

void em2_set_gene_pairs_buffer_mb(uint64_t megabytes) { em2::setGenePairsBudgetMegabytes(megabytes); }

int em2_find_similar_gene_pairs0(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                 int normalizationMethod, uint32_t k, double similarityThreshold, em2_pair* pairs,
                                 uint32_t* usedCount, float* allSimilarities)
{
    const char* who = "em2_find_similar_gene_pairs0";
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (!toc || !usedCount || (!pairs && k)) return failNull(who);
    if (allSimilarities && geneCount > kAllSimilaritiesMaxGenes) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": allSimilarities is an aid for at most " +
                                               std::to_string(kAllSimilaritiesMaxGenes) + " genes");
    }
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(csr.upload());                     // (the device checks the gene ids before any kernel indexes with them)
    const size_t allCount = allSimilarities ? size_t(geneCount) * geneCount : 0;
    DeviceBuffer dPairs, dUsed, dAll;
    EM2_HIP(dPairs.allocateFor<em2_pair>(size_t(geneCount) * k));
    EM2_HIP(dUsed.allocateFor<uint32_t>(geneCount));
    if (allSimilarities) {
        EM2_HIP(dAll.allocateFor<float>(allCount));
        EM2_HIP(hipMemset(dAll.p, 0, allCount * sizeof(float)));                   // (the diagonal: the reference computes none)
    }
    em2::GenePairsStatus status;
    EM2_HIP(em2::runGenePairs(csr.toc.as<uint64_t>(), csr.data.as<em2::CountIn>(), cellCount, geneCount, normalizationMethod, k,
                              similarityThreshold, dPairs.as<em2::PairOut>(), dUsed.as<uint32_t>(), dAll.as<float>(), &status, nullptr));
    if (status.inputError) return failArgument(who, em2::inputErrorText(status.inputError));
    if (status.overflow) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": " + std::to_string(status.records) + " candidate records (" +
                                               std::to_string(status.records * em2::kGenePairsBytesPerRecord >> 20) +
                                               " MB with the sort's second buffer) fit neither the candidate buffer (" +
                                               std::to_string(em2::genePairsBudgetRecords() * em2::kGenePairsBytesPerRecord >> 20) +
                                               " MB, em2_set_gene_pairs_buffer_mb; the Python binding sets it from its environment variable) nor "
                                               "the free device memory (" + std::to_string(status.freeBytes >> 20) +
                                               " MB), so a larger buffer cannot help: raise the similarity threshold");
    }
    EM2_HIP(dPairs.download(pairs, size_t(geneCount) * k));
    EM2_HIP(dUsed.download(usedCount, geneCount));
    EM2_HIP(dAll.download(allSimilarities, allCount));
    if (k) em2_internal_sort_gene_pairs(pairs, usedCount, geneCount, k);          // :186, the library's own std::sort
    return EM2_OK;
}

}  // extern "C"
