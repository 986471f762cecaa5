// em2_fsp0.hip -- ExpressionMatrix::findSimilarPairs0 (src/ExpressionMatrixFindSimilarPairs.cpp:16-99): the exact
// similarity (ExpressionMatrixSubset::computeCellSimilarity, src/ExpressionMatrixSubset.cpp:83-133) of every pair of cells
// of an expression matrix subset, the pairs above the threshold offered to SimilarPairs::add (src/SimilarPairs.cpp:170-232)
// and the per-cell lists sorted at the end (:399-405) -- and the device half of ExpressionMatrix::analyzeSimilarPairs
// (src/ExpressionMatrixLsh.cpp:55-150): the exact similarity of every STORED pair.
//
// The reference walks the unordered pairs (c0 ascending, c1 > c0 ascending) and offers each survivor to both cells, so
// every cell sees its candidates in ascending id of the other cell: the cells are independent.  Here a block owns a row
// cell and evaluates ALL its ordered pairs (twice the reference's arithmetic, no ordering problem between blocks):
//   * the row's counts are scattered into em2_expression.h's dense row vector (LDS, or global scratch if they do not fit);
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
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"

#include <cfloat>

#include <string>

namespace em2 {
namespace {

constexpr uint32_t kMaxThreads = 1024;               // columns per batch at most; the survivors' buffer holds that many
constexpr uint32_t kMaxSlots = 4096;                 // min(k, cellCount - 1) at most: 32 KiB of slots
constexpr uint32_t kInvalidIndex = 0xffffffffu;

struct CellSums {
    double sum1;        // ExpressionMatrixSubset::computeSums (:47-58)
    double spread;      // n * sum2 - sum1 * sum1, the factor of the denominator (:116-117)
};

// computeSums and the input check (em2_expression.h).  A thread per cell, striding over the grid (gridFor caps it).
__global__ void __launch_bounds__(256)
fsp0SumsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
               CellSums* __restrict__ sums, uint32_t* __restrict__ error)
{
    const double n = double(geneCount);
    uint32_t bad = 0u;
    for (uint64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cellCount; c += uint64_t(gridDim.x) * blockDim.x) {
        const CellWalk w = walkCell(toc, data, c, geneCount);
        sums[c].sum1 = w.sum1;
        sums[c].spread = n * w.sum2 - w.sum1 * w.sum1;
        bad |= w.bad;
    }
    if (bad) atomicOr(error, bad);
}

// :111-132.  Every step is one correctly rounded IEEE operation, as compiled for the reference (-ffp-contract=off here).
__device__ __forceinline__ double similarityOf(double n, double scalarProduct, const CellSums a, const CellSums b)
{
    const double numerator = n * scalarProduct - a.sum1 * b.sum1;
    const double denominator = __dsqrt_rn(a.spread * b.spread);
    return __ddiv_rn(numerator, denominator);
}

// OrderPairsBySecondGreaterThenByFirstLess (src/orderPairs.hpp).
__device__ __forceinline__ bool sortsBefore(const PairOut a, const PairOut b)
{
    if (a.similarity > b.similarity) return true;
    if (a.similarity < b.similarity) return false;
    return a.cell < b.cell;
}

// The kernel's own LDS, behind the row vector where that is in LDS.
struct Fsp0Lds {
    uint32_t slotsOffset, survivorsOffset, stateOffset, totalBytes;
};

__host__ __device__ inline Fsp0Lds fsp0Lds(uint32_t slotCapacity)
{
    Fsp0Lds l;
    l.slotsOffset = 0u;
    l.survivorsOffset = slotCapacity * 8u;
    l.stateOffset = l.survivorsOffset + kMaxThreads * 8u;
    l.totalBytes = l.stateOffset + 32u * 4u;       // [0] usedCount [1] lowestSimilarityIndex [2] lowestSimilarity bits, [8..24) the waves' counts
    return l;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(kMaxThreads)
fsp0RowsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const CellSums* __restrict__ sums,
               uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t k, uint32_t slotCapacity,
               double similarityThreshold, PairOut* __restrict__ outPairs, uint32_t* __restrict__ outUsed,
               uint32_t* __restrict__ outLowestIndex, float* __restrict__ outLowestSimilarity, char* rowScratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const RowVector rowVector = rowVectorOf<IN_LDS>(ldsRaw, rowScratch, geneCount);
    unsigned char* own = ldsRaw + (IN_LDS ? rowVectorBytes(geneCount) : 0u);
    const Fsp0Lds l = fsp0Lds(slotCapacity);
    PairOut* slots = reinterpret_cast<PairOut*>(own + l.slotsOffset);
    PairOut* survivors = reinterpret_cast<PairOut*>(own + l.survivorsOffset);
    volatile uint32_t* state = reinterpret_cast<uint32_t*>(own + l.stateOffset);
    volatile uint32_t* waveCounts = state + 8;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const double n = double(geneCount);

    for (uint32_t row = rowBegin + blockIdx.x; row < rowEnd; row += gridDim.x) {
        if (threadIdx.x == 0) {
            state[0] = 0u;                                   // the constructor's values (src/SimilarPairs.cpp:36-40)
            state[1] = kInvalidIndex;
            state[2] = __float_as_uint(FLT_MAX);
        }
        loadRow(rowVector, geneCount, toc, data, row);
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
                  const uint32_t* __restrict__ usedCount, uint32_t k, double* __restrict__ exact, char* rowScratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const RowVector rowVector = rowVectorOf<IN_LDS>(ldsRaw, rowScratch, geneCount);
    const double n = double(geneCount);
    for (uint32_t row = rowBegin + blockIdx.x; row < rowEnd; row += gridDim.x) {
        const uint32_t used = usedCount[row];
        if (used == 0u) continue;                                                     // (uniform over the block)
        loadRow(rowVector, geneCount, toc, data, row);
        const CellSums mine = sums[row];
        for (uint32_t t = threadIdx.x; t < used; t += blockDim.x) {
            const uint32_t j = pairs[size_t(row) * k + t].cell;
            exact[size_t(row - rowBegin) * k + t] = similarityOf(n, scalarProductWithRow(rowVector, toc, data, j), mine, sums[j]);
        }
        __syncthreads();
    }
}

uint32_t slotCapacityOf(uint32_t cellCount, uint32_t k)
{
    const uint32_t needed = cellCount ? (k < cellCount - 1u ? k : cellCount - 1u) : 0u;     // a cell has cellCount - 1 candidates
    uint32_t capacity = 1u;
    while (capacity < needed) capacity <<= 1;
    return capacity;
}

// Whether a row vector fits the LDS next to fsp0's own for that many slots (the stored pairs' kernel takes one slot's cut-over).
bool fsp0RowFitsLds(uint32_t geneCount, uint32_t slotCapacity) { return rowFitsLds(geneCount, fsp0Lds(slotCapacity).totalBytes); }

// sums | error word | the row vectors of the global-memory form
size_t workspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, bool inLds)
{
    return alignUp(size_t(cellCount) * sizeof(CellSums)) + 256u + (inLds ? 0u : rowScratchBytes(geneCount, rowCount));
}

char* rowScratchOf(void* workspace, uint32_t cellCount) { return static_cast<char*>(workspace) + alignUp(size_t(cellCount) * sizeof(CellSums)) + 256u; }

}  // namespace


uint32_t fsp0MaxSlots() { return kMaxSlots; }

// The sums of all cells into the workspace (once per matrix) and the input error word to the host.  Synchronises the stream.
hipError_t prepareStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, void* workspace,
                              uint32_t* inputError, hipStream_t stream)
{
    char* base = static_cast<char*>(workspace);
    uint32_t* error = reinterpret_cast<uint32_t*>(base + alignUp(size_t(cellCount) * sizeof(CellSums)));
    EM2_TRY(hipMemsetAsync(error, 0, sizeof(uint32_t), stream));
    fsp0SumsKernel<<<dim3(gridFor(cellCount)), dim3(256), 0, stream>>>(toc, data, cellCount, geneCount, reinterpret_cast<CellSums*>(base), error);
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

bool fsp0Supported(uint32_t cellCount, uint32_t k) { return slotCapacityOf(cellCount, k) <= kMaxSlots; }

size_t fsp0WorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, uint32_t k)
{
    return workspaceBytes(cellCount, rowCount, geneCount, fsp0RowFitsLds(geneCount, slotCapacityOf(cellCount, k)));
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
    const hipError_t e = prepareStoredPairs(toc, data, cellCount, geneCount, workspace, inputError, stream);
    if (e != hipSuccess || *inputError) return e;

    const uint32_t slotCapacity = slotCapacityOf(cellCount, k);
    const bool inLds = fsp0RowFitsLds(geneCount, slotCapacity);
    const size_t ownLdsBytes = fsp0Lds(slotCapacity).totalBytes;
    // waves per CU: a row that fills the LDS leaves room for one block, which then brings 16 waves
    const size_t ldsBytes = ownLdsBytes + rowVectorBytes(geneCount);
    const uint32_t threads = ldsBytes <= 40u * 1024u ? 256u : ldsBytes <= 80u * 1024u ? 512u : kMaxThreads;
    EM2_TRY(launchRowKernel(inLds, &fsp0RowsKernel<true>, &fsp0RowsKernel<false>, rowEnd - rowBegin, threads, geneCount, ownLdsBytes,
                            rowScratchOf(workspace, cellCount), stream, toc, data, static_cast<const CellSums*>(workspace), cellCount,
                            geneCount, rowBegin, rowEnd, k, slotCapacity, similarityThreshold, outPairs, outUsed, outLowestIndex,
                            outLowestSimilarity));
    return hipStreamSynchronize(stream);
}


size_t storedPairsWorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount)
{
    return workspaceBytes(cellCount, rowCount, geneCount, fsp0RowFitsLds(geneCount, 1u));
}

// exact[(row - rowBegin) * k + t] = the exact similarity of cell `row` and its t-th stored neighbour, t < usedCount[row];
// pairs / usedCount cover all cells and every stored id is below cellCount (the caller checked).
hipError_t launchStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin,
                             uint32_t rowEnd, const PairOut* pairs, const uint32_t* usedCount, uint32_t k, void* workspace,
                             double* exact, hipStream_t stream)
{
    if (rowEnd <= rowBegin || k == 0) return hipSuccess;
    return launchRowKernel(fsp0RowFitsLds(geneCount, 1u), &storedPairsKernel<true>, &storedPairsKernel<false>, rowEnd - rowBegin, 256u,
                           geneCount, 0u, rowScratchOf(workspace, cellCount), stream, toc, data, static_cast<const CellSums*>(workspace),
                           geneCount, rowBegin, rowEnd, pairs, usedCount, k, exact);
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

// The checks of findSimilarPairs0 that need no device.  CZI_ASSERT(similarityThreshold <= 1.)
// (src/ExpressionMatrixFindSimilarPairs.cpp:26) comes first in the reference.
static int prepareFsp0(const char* who, uint32_t cellCount, uint32_t geneCount, uint32_t k, double similarityThreshold)
{
    if (!(similarityThreshold <= 1.)) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": Assertion failed: similarityThreshold <= 1.");
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (!em2::fsp0Supported(cellCount, k)) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(em2::fsp0MaxSlots()) +
                                               " stored pairs per cell (min(k, cellCount-1)) is not supported");
    }
    return EM2_OK;
}

size_t em2_dev_find_similar_pairs0_workspace(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, uint32_t k)
{
    return em2::fsp0WorkspaceBytes(cellCount, rowCount, geneCount, k);
}

int em2_dev_find_similar_pairs0(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                                uint32_t rowBegin, uint32_t rowEnd, uint32_t k, double similarityThreshold, em2_pair* d_pairs,
                                uint32_t* d_usedCount, uint32_t* d_lowestSimilarityIndex, float* d_lowestSimilarity,
                                void* d_workspace, size_t workspaceBytes, void* stream)
{
    const char* who = "em2_dev_find_similar_pairs0";
    const int prc = prepareFsp0(who, cellCount, geneCount, k, similarityThreshold);
    if (prc != EM2_OK) return prc;
    if (rowBegin > rowEnd || rowEnd > cellCount) return failArgument(who, "bad row range");
    if (rowBegin == rowEnd) return EM2_OK;
    if (!d_toc || !d_usedCount || !d_lowestSimilarityIndex || !d_lowestSimilarity || (!d_pairs && k) || !d_workspace) return failNull(who);
    if (workspaceBytes < em2::fsp0WorkspaceBytes(cellCount, rowEnd - rowBegin, geneCount, k)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    EM2_HIP(em2::runFsp0(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), cellCount, geneCount, rowBegin, rowEnd, k,
                         similarityThreshold, reinterpret_cast<em2::PairOut*>(d_pairs), d_usedCount, d_lowestSimilarityIndex,
                         d_lowestSimilarity, d_workspace, &inputError, static_cast<hipStream_t>(stream)));
    if (inputError) return failArgument(who, em2::inputErrorText(inputError));
    return EM2_OK;
}

int em2_find_similar_pairs0(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, uint32_t k,
                            double similarityThreshold, em2_pair* pairs, uint32_t* usedCount, uint32_t* lowestSimilarityIndex,
                            float* lowestSimilarity)
{
    const char* who = "em2_find_similar_pairs0";
    const int prc = prepareFsp0(who, cellCount, geneCount, k, similarityThreshold);
    if (prc != EM2_OK) return prc;
    if (cellCount == 0) return EM2_OK;
    if (!toc || !usedCount || !lowestSimilarityIndex || !lowestSimilarity || (!pairs && k)) return failNull(who);
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(csr.upload());                     // (the device checks the gene ids before any kernel indexes with them)
    DeviceBuffer dPairs, dUsed, dIndex, dLowest, dWorkspace;
    const size_t workspaceBytes = em2::fsp0WorkspaceBytes(cellCount, cellCount, geneCount, k);
    EM2_HIP(dPairs.allocateFor<em2_pair>(size_t(cellCount) * k));
    EM2_HIP(dUsed.allocateFor<uint32_t>(cellCount));
    EM2_HIP(dIndex.allocateFor<uint32_t>(cellCount));
    EM2_HIP(dLowest.allocateFor<float>(cellCount));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int rc = em2_dev_find_similar_pairs0(csr.toc.as<uint64_t>(), csr.data.as<em2_count>(), cellCount, geneCount, 0, cellCount, k,
                                               similarityThreshold, dPairs.as<em2_pair>(), dUsed.as<uint32_t>(), dIndex.as<uint32_t>(),
                                               dLowest.as<float>(), dWorkspace.p, workspaceBytes, nullptr);
    if (rc != EM2_OK) return rc;
    EM2_HIP(dPairs.download(pairs, size_t(cellCount) * k));
    EM2_HIP(dUsed.download(usedCount, cellCount));
    EM2_HIP(dIndex.download(lowestSimilarityIndex, cellCount));
    EM2_HIP(dLowest.download(lowestSimilarity, cellCount));
    return EM2_OK;
}

}  // extern "C"
