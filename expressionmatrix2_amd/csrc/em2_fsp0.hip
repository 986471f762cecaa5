// em2_fsp0.hip -- ExpressionMatrix::findSimilarPairs0 (src/ExpressionMatrixFindSimilarPairs.cpp:16-99): the exact
// similarity (ExpressionMatrixSubset::computeCellSimilarity, src/ExpressionMatrixSubset.cpp:83-133) of every pair of cells
// of an expression matrix subset, the pairs above the threshold offered to SimilarPairs::add (src/SimilarPairs.cpp:170-232)
// and the per-cell lists sorted at the end (:399-405) -- and the device half of ExpressionMatrix::analyzeSimilarPairs
// (src/ExpressionMatrixLsh.cpp:55-150): the exact similarity of every STORED pair.
//
// The reference walks the unordered pairs (c0 ascending, c1 > c0 ascending) and offers each survivor to both cells, so
// every cell sees its candidates in ascending id of the other cell: the cells are independent.  Here a block owns a row
// cell and evaluates ALL its ordered pairs (twice the reference's arithmetic, no ordering problem between blocks):
//   * the row's counts are scattered into a dense float vector with a presence bitmap (LDS, or global scratch for gene
//     sets that do not fit), as in em2_analyze.hip; a stored zero, inf or NaN count takes part in the product exactly as in
//     the reference's merge loop, because the bitmap and not the value decides;
//   * the lanes take the columns j = 0 .. N-1, j != row, in ascending batches of one column per lane; per pair: the sparse
//     scalar product (float products, double sum, ascending gene order), the correlation coefficient (separate
//     multiplications and subtraction, correctly rounded square root and division), the double comparison with the
//     threshold and the conversion to float;
//   * the batch's survivors are compacted in column order (ballot + prefix over the waves) and wave 0 replays
//     SimilarPairs::add over them: the slots in LDS, usedCount / lowestSimilarityIndex / lowestSimilarity in registers,
//     the rescan after a replacement as a wave-wide (value, first index) minimum.  Once a cell is full a survivor at or
//     below lowestSimilarity is dropped before the compaction (the lowest value only rises);
//   * the slots are sorted by (similarity descending, id ascending) -- a total order, ids being distinct -- and written
//     out with the three CellInfo fields, the index referring to the slot BEFORE the sort as in the reference.
// Where the reference is undefined -- a replacement while lowestSimilarityIndex is 0xffffffff, which needs k stored
// similarities of +inf or FLT_MAX, or k = 0 and a similarity of +inf -- the candidate is dropped.

#include "em2_device.h"

#include <cfloat>

namespace em2 {
namespace {

constexpr uint32_t kMaxThreads = 1024;               // columns per batch at most; the survivors' buffer holds that many
constexpr uint32_t kMaxSlots = 4096;                 // min(k, cellCount - 1) at most: 32 KiB of slots
constexpr size_t kLdsBytes = 160u * 1024u;           // per workgroup on gfx950
constexpr uint32_t kGlobalFormBlocks = 1024;         // blocks (hence scratch vectors) of the global-memory form
constexpr uint32_t kInvalidIndex = 0xffffffffu;

struct CellSums {
    double sum1;        // ExpressionMatrixSubset::computeSums (:47-58)
    double spread;      // n * sum2 - sum1 * sum1, the factor of the denominator (:116-117)
};

// computeSums, and the checks the kernels' bounds rest on: gene ids below geneCount, strictly ascending within a cell.
__global__ void __launch_bounds__(256)
fsp0SumsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
               CellSums* __restrict__ sums, uint32_t* __restrict__ error)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cellCount) return;
    double sum1 = 0., sum2 = 0.;
    uint32_t bad = 0u, previous = 0u;
    const uint64_t begin = toc[c], end = toc[c + 1u];
    for (uint64_t p = begin; p < end; ++p) {
        const CountIn e = data[p];
        if (e.gene >= geneCount) bad |= 1u;
        if (p != begin && e.gene <= previous) bad |= 2u;
        previous = e.gene;
        sum1 += double(e.count);
        sum2 += double(e.count * e.count);               // count*count is a float product (:55)
    }
    const double n = double(geneCount);
    sums[c].sum1 = sum1;
    sums[c].spread = n * sum2 - sum1 * sum1;
    if (bad) atomicOr(error, bad);
}

struct RowVector {
    const float* dense;
    const uint32_t* present;
};

__device__ __forceinline__ void addProduct(const RowVector& row, const CountIn c, double& scalarProduct)
{
    if ((row.present[c.gene >> 5] >> (c.gene & 31u)) & 1u) {
        const float product = row.dense[c.gene] * c.count;       // it0->second * it1->second: a float product (:103)
        scalarProduct += double(product);
    }
}

// The scalar product of the row cell with cell j over the genes both have, in ascending gene order (:86-108).  Four
// entries of cell j are loaded ahead of their use (the addresses do not depend on the values); the sum stays in order.
__device__ __forceinline__ double scalarProductWithRow(const RowVector& row, const uint64_t* __restrict__ toc,
                                                       const CountIn* __restrict__ data, uint32_t j)
{
    double scalarProduct = 0.;
    const uint64_t end = toc[j + 1u];
    uint64_t p = toc[j];
    for (; p + 4u <= end; p += 4u) {
        const CountIn c0 = data[p], c1 = data[p + 1u], c2 = data[p + 2u], c3 = data[p + 3u];
        addProduct(row, c0, scalarProduct);
        addProduct(row, c1, scalarProduct);
        addProduct(row, c2, scalarProduct);
        addProduct(row, c3, scalarProduct);
    }
    for (; p < end; ++p) addProduct(row, data[p], scalarProduct);
    return scalarProduct;
}

// :111-132.  Every step is one correctly rounded IEEE operation, as compiled for the reference (-ffp-contract=off here).
__device__ __forceinline__ double similarityOf(double n, double scalarProduct, const CellSums a, const CellSums b)
{
    const double numerator = n * scalarProduct - a.sum1 * b.sum1;
    const double denominator = __dsqrt_rn(a.spread * b.spread);
    return __ddiv_rn(numerator, denominator);
}

// Clears the bitmap and scatters the row cell's counts.  Ends with a barrier.
__device__ __forceinline__ void loadRow(float* dense, uint32_t* present, uint32_t bitmapWords, const uint64_t* __restrict__ toc,
                                        const CountIn* __restrict__ data, uint32_t row)
{
    for (uint32_t w = threadIdx.x; w < bitmapWords; w += blockDim.x) present[w] = 0u;
    __syncthreads();
    const uint64_t end = toc[row + 1u];
    for (uint64_t p = toc[row] + threadIdx.x; p < end; p += blockDim.x) {
        const CountIn c = data[p];
        dense[c.gene] = c.count;
        atomicOr(present + (c.gene >> 5), 1u << (c.gene & 31u));
    }
    __syncthreads();
}

// OrderPairsBySecondGreaterThenByFirstLess (src/orderPairs.hpp).
__device__ __forceinline__ bool sortsBefore(const PairOut a, const PairOut b)
{
    if (a.similarity > b.similarity) return true;
    if (a.similarity < b.similarity) return false;
    return a.cell < b.cell;
}

struct Fsp0Lds {
    uint32_t denseOffset, presentOffset, slotsOffset, survivorsOffset, stateOffset, totalBytes;
};

__host__ __device__ inline Fsp0Lds fsp0Lds(bool inLds, uint32_t geneCount, uint32_t slotCapacity)
{
    Fsp0Lds l;
    uint32_t at = 0;
    l.denseOffset = at;
    if (inLds) at += (geneCount * 4u + 7u) & ~7u;
    l.presentOffset = at;
    if (inLds) at += (((geneCount + 31u) / 32u) * 4u + 7u) & ~7u;
    l.slotsOffset = at;
    at += slotCapacity * 8u;
    l.survivorsOffset = at;
    at += kMaxThreads * 8u;
    l.stateOffset = at;
    at += 32u * 4u;                   // [0] usedCount [1] lowestSimilarityIndex [2] lowestSimilarity bits, [8..24) the waves' counts
    l.totalBytes = at;
    return l;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(kMaxThreads)
fsp0RowsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const CellSums* __restrict__ sums,
               uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t k, uint32_t slotCapacity,
               double similarityThreshold, float* __restrict__ denseScratch, uint32_t* __restrict__ presentScratch,
               PairOut* __restrict__ outPairs, uint32_t* __restrict__ outUsed, uint32_t* __restrict__ outLowestIndex,
               float* __restrict__ outLowestSimilarity)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const Fsp0Lds l = fsp0Lds(IN_LDS, geneCount, slotCapacity);
    const uint32_t bitmapWords = (geneCount + 31u) / 32u;
    float* dense = IN_LDS ? reinterpret_cast<float*>(ldsRaw + l.denseOffset) : denseScratch + size_t(blockIdx.x) * geneCount;
    uint32_t* present = IN_LDS ? reinterpret_cast<uint32_t*>(ldsRaw + l.presentOffset) : presentScratch + size_t(blockIdx.x) * bitmapWords;
    PairOut* slots = reinterpret_cast<PairOut*>(ldsRaw + l.slotsOffset);
    PairOut* survivors = reinterpret_cast<PairOut*>(ldsRaw + l.survivorsOffset);
    volatile uint32_t* state = reinterpret_cast<uint32_t*>(ldsRaw + l.stateOffset);
    volatile uint32_t* waveCounts = state + 8;
    const RowVector rowVector{dense, present};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const double n = double(geneCount);

    for (uint32_t row = rowBegin + blockIdx.x; row < rowEnd; row += gridDim.x) {
        if (threadIdx.x == 0) {
            state[0] = 0u;                                   // the constructor's values (src/SimilarPairs.cpp:36-40)
            state[1] = kInvalidIndex;
            state[2] = __float_as_uint(FLT_MAX);
        }
        loadRow(dense, present, bitmapWords, toc, data, row);
        const CellSums mine = sums[row];

        for (uint32_t base = 0; base < cellCount; base += blockDim.x) {
            const uint32_t j = base + threadIdx.x;
            const bool full = state[0] == k;
            const float lowestAtStart = __uint_as_float(state[2]);
            bool keep = false;
            float similarityFloat = 0.f;
            if (j < cellCount && j != row) {
                const double scalarProduct = scalarProductWithRow(rowVector, toc, data, j);
                const double similarity = similarityOf(n, scalarProduct, mine, sums[j]);
                if (similarity > similarityThreshold) {                              // double > double; false for NaN
                    similarityFloat = float(similarity);                             // make_pair(cellId1, similarity) -> Pair
                    keep = !(full && similarityFloat <= lowestAtStart);              // :203 would reject it: lowest only rises
                }
            }
            const uint64_t ballot = __ballot(keep);
            if (lane == 0) waveCounts[wave] = uint32_t(__popcll(ballot));
            __syncthreads();
            uint32_t offset = 0, total = 0;
            for (uint32_t w = 0; w < waves; ++w) {
                const uint32_t count = waveCounts[w];
                if (w < wave) offset += count;
                total += count;
            }
            if (keep) survivors[offset + uint32_t(__popcll(ballot & ((1ull << lane) - 1ull)))] = PairOut{j, similarityFloat};
            __syncthreads();
            if (total == 0) continue;                                                // (uniform over the block)
            if (wave == 0) {
                // SimilarPairs::add (:170-232) over the batch's survivors, in ascending id of the other cell
                uint32_t used = state[0], lowestIndex = state[1];
                float lowest = __uint_as_float(state[2]);
                for (uint32_t t = 0; t < total; ++t) {
                    const PairOut candidate = survivors[t];
                    if (used < k) {
                        if (candidate.similarity < lowest) {                         // :185-188
                            lowestIndex = used;
                            lowest = candidate.similarity;
                        }
                        if (lane == 0) slots[used] = candidate;                      // :191-192
                        ++used;
                        continue;
                    }
                    if (candidate.similarity <= lowest) continue;                    // :203
                    if (lowestIndex == kInvalidIndex) continue;                      // undefined in the reference, see above
                    const uint32_t replaced = lowestIndex;
                    if (lane == 0) slots[replaced] = candidate;                      // :217
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    // :220-228: the first slot, by index, that holds the strict minimum
                    float best = FLT_MAX;
                    uint32_t bestIndex = kInvalidIndex;
                    for (uint32_t i = lane; i < k; i += 64u) {
                        const float value = i == replaced ? candidate.similarity : slots[i].similarity;
                        if (value < best) {
                            best = value;
                            bestIndex = i;
                        }
                    }
                    for (uint32_t step = 32u; step > 0u; step >>= 1) {
                        const float otherValue = __shfl_xor(best, int(step), 64);
                        const uint32_t otherIndex = uint32_t(__shfl_xor(int(bestIndex), int(step), 64));
                        if (otherValue < best || (otherValue == best && otherIndex < bestIndex)) {
                            best = otherValue;
                            bestIndex = otherIndex;
                        }
                    }
                    lowest = best;
                    lowestIndex = bestIndex;
                }
                if (lane == 0) {
                    state[0] = used;
                    state[1] = lowestIndex;
                    state[2] = __float_as_uint(lowest);
                }
            }
            __syncthreads();
        }

        // SimilarPairs::sort (:399-405): bitonic over the used slots padded to a power of two with entries that sort last
        // (a stored similarity is above the threshold, hence never -inf)
        const uint32_t used = state[0];
        uint32_t sortCount = 1u;
        while (sortCount < used) sortCount <<= 1;
        for (uint32_t i = used + threadIdx.x; i < sortCount; i += blockDim.x) slots[i] = PairOut{kInvalidIndex, -INFINITY};
        __syncthreads();
        for (uint32_t size = 2u; size <= sortCount; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
                for (uint32_t t = threadIdx.x; t < sortCount / 2u; t += blockDim.x) {
                    const uint32_t lo = 2u * t - (t & (stride - 1u)), hi = lo + stride;
                    const bool ascending = (lo & size) == 0u;
                    const PairOut a = slots[lo], b = slots[hi];
                    if (sortsBefore(b, a) == ascending) {
                        slots[lo] = b;
                        slots[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        PairOut* out = outPairs + size_t(row - rowBegin) * k;
        for (uint32_t t = threadIdx.x; t < k; t += blockDim.x) out[t] = t < used ? slots[t] : PairOut{0u, 0.f};
        if (threadIdx.x == 0) {
            outUsed[row - rowBegin] = used;
            outLowestIndex[row - rowBegin] = state[1];
            outLowestSimilarity[row - rowBegin] = __uint_as_float(state[2]);
        }
        __syncthreads();
    }
}

// analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:95-106): one block per cell 0, one lane per stored neighbour.
template <bool IN_LDS>
__global__ void __launch_bounds__(256)
storedPairsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const CellSums* __restrict__ sums,
                  uint32_t geneCount, uint32_t rowBegin, uint32_t rowEnd, const PairOut* __restrict__ pairs,
                  const uint32_t* __restrict__ usedCount, uint32_t k, float* __restrict__ denseScratch,
                  uint32_t* __restrict__ presentScratch, double* __restrict__ exact)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const uint32_t bitmapWords = (geneCount + 31u) / 32u;
    float* dense = IN_LDS ? reinterpret_cast<float*>(ldsRaw) : denseScratch + size_t(blockIdx.x) * geneCount;
    uint32_t* present = IN_LDS ? reinterpret_cast<uint32_t*>(ldsRaw + ((size_t(geneCount) * 4u + 7u) & ~size_t(7u)))
                               : presentScratch + size_t(blockIdx.x) * bitmapWords;
    const RowVector rowVector{dense, present};
    const double n = double(geneCount);
    for (uint32_t row = rowBegin + blockIdx.x; row < rowEnd; row += gridDim.x) {
        const uint32_t used = usedCount[row];
        if (used == 0u) continue;                                                     // (uniform over the block)
        loadRow(dense, present, bitmapWords, toc, data, row);
        const CellSums mine = sums[row];
        for (uint32_t t = threadIdx.x; t < used; t += blockDim.x) {
            const uint32_t j = pairs[size_t(row) * k + t].cell;
            exact[size_t(row - rowBegin) * k + t] = similarityOf(n, scalarProductWithRow(rowVector, toc, data, j), mine, sums[j]);
        }
        __syncthreads();
    }
}

size_t alignUp256(size_t x) { return (x + 255u) & ~size_t(255u); }

uint32_t slotCapacityOf(uint32_t cellCount, uint32_t k)
{
    const uint32_t needed = cellCount ? (k < cellCount - 1u ? k : cellCount - 1u) : 0u;     // a cell has cellCount - 1 candidates
    uint32_t capacity = 1u;
    while (capacity < needed) capacity <<= 1;
    return capacity;
}

bool rowFitsLds(uint32_t geneCount, uint32_t slotCapacity) { return fsp0Lds(true, geneCount, slotCapacity).totalBytes <= kLdsBytes; }

size_t rowScratchBytes(uint32_t geneCount, uint32_t blocks)
{
    return alignUp256(size_t(geneCount) * 4u * blocks) + alignUp256(size_t((geneCount + 31u) / 32u) * 4u * blocks);
}

}  // namespace


uint32_t fsp0MaxSlots() { return kMaxSlots; }

bool fsp0Supported(uint32_t cellCount, uint32_t k) { return slotCapacityOf(cellCount, k) <= kMaxSlots; }

// sums | error word | the dense vectors and bitmaps of the global-memory form
size_t fsp0WorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, uint32_t k)
{
    size_t bytes = alignUp256(size_t(cellCount) * sizeof(CellSums)) + 256u;
    if (!rowFitsLds(geneCount, slotCapacityOf(cellCount, k))) bytes += rowScratchBytes(geneCount, rowCount < kGlobalFormBlocks ? rowCount : kGlobalFormBlocks);
    return bytes;
}

// Rows [rowBegin, rowEnd): outPairs[(row - rowBegin) * k ..], outUsed / outLowestIndex / outLowestSimilarity[row - rowBegin].
// *inputError: bit 0 a gene id not below geneCount, bit 1 gene ids not strictly ascending within a cell; the rows are
// not computed then.  Synchronises the stream.
hipError_t runFsp0(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin, uint32_t rowEnd,
                   uint32_t k, double similarityThreshold, PairOut* outPairs, uint32_t* outUsed, uint32_t* outLowestIndex,
                   float* outLowestSimilarity, void* workspace, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0u;
    if (rowEnd <= rowBegin) return hipSuccess;
    char* base = static_cast<char*>(workspace);
    CellSums* sums = reinterpret_cast<CellSums*>(base);
    uint32_t* error = reinterpret_cast<uint32_t*>(base + alignUp256(size_t(cellCount) * sizeof(CellSums)));
    char* scratch = reinterpret_cast<char*>(error) + 256u;
    hipError_t e = hipMemsetAsync(error, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    fsp0SumsKernel<<<dim3((cellCount + 255u) / 256u), dim3(256), 0, stream>>>(toc, data, cellCount, geneCount, sums, error);
    e = hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess || *inputError) return e;

    const uint32_t rows = rowEnd - rowBegin;
    const uint32_t slotCapacity = slotCapacityOf(cellCount, k);
    const bool inLds = rowFitsLds(geneCount, slotCapacity);
    const Fsp0Lds l = fsp0Lds(inLds, geneCount, slotCapacity);
    // waves per CU: a row that fills the LDS leaves room for one block, which then brings 16 waves
    const uint32_t threads = l.totalBytes <= 40u * 1024u ? 256u : l.totalBytes <= 80u * 1024u ? 512u : kMaxThreads;
    if (inLds) {
        const void* kernel = reinterpret_cast<const void*>(&fsp0RowsKernel<true>);
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(l.totalBytes));
        if (e != hipSuccess) return e;
        fsp0RowsKernel<true><<<dim3(rows), dim3(threads), l.totalBytes, stream>>>(
            toc, data, sums, cellCount, geneCount, rowBegin, rowEnd, k, slotCapacity, similarityThreshold, nullptr, nullptr, outPairs,
            outUsed, outLowestIndex, outLowestSimilarity);
    } else {
        const uint32_t blocks = rows < kGlobalFormBlocks ? rows : kGlobalFormBlocks;
        float* dense = reinterpret_cast<float*>(scratch);
        uint32_t* present = reinterpret_cast<uint32_t*>(scratch + alignUp256(size_t(geneCount) * 4u * blocks));
        const void* kernel = reinterpret_cast<const void*>(&fsp0RowsKernel<false>);
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(l.totalBytes));
        if (e != hipSuccess) return e;
        fsp0RowsKernel<false><<<dim3(blocks), dim3(256), l.totalBytes, stream>>>(
            toc, data, sums, cellCount, geneCount, rowBegin, rowEnd, k, slotCapacity, similarityThreshold, dense, present, outPairs,
            outUsed, outLowestIndex, outLowestSimilarity);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}


size_t storedPairsWorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount)
{
    size_t bytes = alignUp256(size_t(cellCount) * sizeof(CellSums)) + 256u;
    if (!rowFitsLds(geneCount, 1u)) bytes += rowScratchBytes(geneCount, rowCount < kGlobalFormBlocks ? rowCount : kGlobalFormBlocks);
    return bytes;
}

// The sums of all cells into the workspace (once per matrix), with the input checks of runFsp0.
hipError_t prepareStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, void* workspace,
                              uint32_t* inputError, hipStream_t stream)
{
    char* base = static_cast<char*>(workspace);
    uint32_t* error = reinterpret_cast<uint32_t*>(base + alignUp256(size_t(cellCount) * sizeof(CellSums)));
    hipError_t e = hipMemsetAsync(error, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    fsp0SumsKernel<<<dim3((cellCount + 255u) / 256u), dim3(256), 0, stream>>>(toc, data, cellCount, geneCount,
                                                                               reinterpret_cast<CellSums*>(base), error);
    e = hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}

// exact[(row - rowBegin) * k + t] = the exact similarity of cell `row` and its t-th stored neighbour, t < usedCount[row];
// pairs / usedCount cover all cells and every stored id is below cellCount (the caller checked).
hipError_t launchStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin,
                             uint32_t rowEnd, const PairOut* pairs, const uint32_t* usedCount, uint32_t k, void* workspace,
                             double* exact, hipStream_t stream)
{
    if (rowEnd <= rowBegin || k == 0) return hipSuccess;
    char* base = static_cast<char*>(workspace);
    const CellSums* sums = reinterpret_cast<const CellSums*>(base);
    char* scratch = base + alignUp256(size_t(cellCount) * sizeof(CellSums)) + 256u;
    const uint32_t rows = rowEnd - rowBegin;
    if (rowFitsLds(geneCount, 1u)) {
        const size_t lds = ((size_t(geneCount) * 4u + 7u) & ~size_t(7u)) + size_t((geneCount + 31u) / 32u) * 4u;
        const void* kernel = reinterpret_cast<const void*>(&storedPairsKernel<true>);
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
        storedPairsKernel<true><<<dim3(rows), dim3(256), lds, stream>>>(toc, data, sums, geneCount, rowBegin, rowEnd, pairs, usedCount, k,
                                                                       nullptr, nullptr, exact);
    } else {
        const uint32_t blocks = rows < kGlobalFormBlocks ? rows : kGlobalFormBlocks;
        float* dense = reinterpret_cast<float*>(scratch);
        uint32_t* present = reinterpret_cast<uint32_t*>(scratch + alignUp256(size_t(geneCount) * 4u * blocks));
        storedPairsKernel<false><<<dim3(blocks), dim3(256), 0, stream>>>(toc, data, sums, geneCount, rowBegin, rowEnd, pairs, usedCount, k,
                                                                        dense, present, exact);
    }
    return hipGetLastError();
}

}  // namespace em2
