// em2_dense.hip -- ExpressionMatrix::getDenseExpressionMatrix (src/PythonModule.cpp:112-138) for rows of a CSR in device
// memory: out[cell][gene], row-major, zero where nothing is stored.  NOT getDenseRepresentation
// (em2_gene_pairs.hip's denseCellsKernel): this one is cell-major, has no guard against a zero sum and multiplies only what
// is stored.
//
// The gene set and the cell list are applied on the way (what em2_subset.hip would materialise): an entry whose global gene id
// the gene set does not know is passed over, in the sums and in the fill alike.
//   * denseFactorsKernel   a thread per row: ExpressionMatrixSubset::computeSums (src/ExpressionMatrixSubset.cpp:47-58) over
//                          the row's kept entries in stored order with walkCell's checks (em2_expression.h), then the float
//                          factor of :117-130: 1.f, float(1. / sum1) or float(1. / sqrt(sum2)).  No guard: a zero sum gives
//                          an infinite factor, and inf * 0 is the reference's NaN.
//   * denseFillKernel<T>   a workgroup per row, striding over the rows: zeroes the row's geneCount elements (16-byte stores
//                          between a head and a tail of single elements, because a row begins on a 16-byte boundary only
//                          when pitch * sizeof(T) is a multiple of 16), a barrier, then every kept entry becomes
//                          T(factor * count): a float product (:135), widened for double (:136).  The padding behind
//                          geneCount is not touched.
// The fill runs only once the factors' pass has found the ids good: nothing is indexed with an unchecked gene id.
// No FMA can form (one product per element; -ffp-contract=off besides); the division and the square root are the
// correctly rounded __ddiv_rn / __dsqrt_rn.

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"

#include <string>

namespace em2 {
namespace {

constexpr uint32_t kInvalid = 0xffffffffu;
constexpr uint32_t kFillBlocks = 8192;            // blocks of the fill at most: 32 per CU, each strides over the rows

// The local id of a stored gene: itself without a table, else GeneSet::getLocalGeneId (kInvalid: not in the gene set).
__device__ __forceinline__ uint32_t localGeneOf(const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t gene)
{
    if (!geneLocalIds) return gene;
    return gene < globalGeneCount ? geneLocalIds[gene] : kInvalid;
}

// factors[r - rowBegin] for the rows [rowBegin, rowEnd); *error |= walkCell's word over the kept entries.
__global__ void __launch_bounds__(256)
denseFactorsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const uint32_t* __restrict__ cellIds,
                   const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int method,
                   uint32_t rowBegin, uint32_t rowEnd, float* __restrict__ factors, uint32_t* __restrict__ error)
{
    uint32_t bad = 0u;
    for (uint64_t r = uint64_t(rowBegin) + blockIdx.x * blockDim.x + threadIdx.x; r < rowEnd; r += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t cell = cellIds ? cellIds[r] : r;
        CellWalk w{0., 0., 0u};
        if (!geneLocalIds) {
            w = walkCell(toc, data, cell, geneCount);
        } else {
            // walkCell over the entries the gene set keeps, under their local ids
            bool first = true;
            uint32_t previous = 0u;
            const uint64_t end = toc[cell + 1u];
            for (uint64_t p = toc[cell]; p < end; ++p) {
                const CountIn e = data[p];
                const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, e.gene);
                if (local == kInvalid) continue;
                if (local >= geneCount) w.bad |= 1u;
                if (!first && local <= previous) w.bad |= 2u;
                first = false;
                previous = local;
                w.sum1 += double(e.count);
                w.sum2 += double(e.count * e.count);             // a float product (ExpressionMatrixSubset.cpp:55)
            }
        }
        bad |= w.bad;
        float factor = 1.f;                                                            // PythonModule.cpp:119-121
        if (method == 1) factor = float(__ddiv_rn(1., w.sum1));                        // :123
        else if (method == 2) factor = float(__ddiv_rn(1., __dsqrt_rn(w.sum2)));       // :126
        factors[r - rowBegin] = factor;
    }
    if (bad) atomicOr(error, bad);
}

template <class T>
__global__ void __launch_bounds__(256)
denseFillKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, const uint32_t* __restrict__ cellIds,
                const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, uint32_t rowBegin,
                uint32_t rowEnd, const float* __restrict__ factors, T* __restrict__ out, size_t pitchElements)
{
    constexpr uint32_t kPerStore = 16u / sizeof(T);
    for (uint64_t r = uint64_t(rowBegin) + blockIdx.x; r < rowEnd; r += gridDim.x) {
        T* const row = out + size_t(r - rowBegin) * pitchElements;
        // the row's first 256 entries are loaded before the zeroes are stored, so that the chain cell id -> toc -> entry -> local
        // id passes behind the stores instead of behind the barrier
        const uint64_t cell = cellIds ? cellIds[r] : r;
        const float factor = factors[r - rowBegin];
        const uint64_t end = toc[cell + 1u];
        uint64_t p = toc[cell] + threadIdx.x;
        float firstCount = 0.f;
        uint32_t firstLocal = kInvalid;
        if (p < end) {
            const CountIn e = data[p];
            firstCount = e.count;
            firstLocal = localGeneOf(geneLocalIds, globalGeneCount, e.gene);
        }
        // elements in front of the first 16-byte boundary (out is aligned to sizeof(T), so they are whole)
        uint32_t head = uint32_t(((16u - (reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / sizeof(T));
        if (head > geneCount) head = geneCount;
        const uint32_t wide = (geneCount - head) / kPerStore;
        const uint32_t tailBegin = head + wide * kPerStore;
        if (threadIdx.x < head) row[threadIdx.x] = T(0);
        uint4* const body = reinterpret_cast<uint4*>(row + head);
        for (uint32_t i = threadIdx.x; i < wide; i += blockDim.x) body[i] = make_uint4(0u, 0u, 0u, 0u);
        if (tailBegin + threadIdx.x < geneCount) row[tailBegin + threadIdx.x] = T(0);      // fewer than kPerStore <= 4 elements
        __syncthreads();
        if (firstLocal != kInvalid) {                            // (a checked id is below geneCount, so never kInvalid)
            const float count = factor * firstCount;             // :135
            row[firstLocal] = T(count);                          // :136
        }
        for (p += blockDim.x; p < end; p += blockDim.x) {
            const CountIn e = data[p];
            const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, e.gene);
            if (local == kInvalid) continue;
            const float count = factor * e.count;                // :135
            row[local] = T(count);                               // :136
        }
        // (the next row of this block is other memory: no barrier between the scatter and its zeroes)
    }
}

}  // namespace

size_t denseExpressionWorkspaceBytes(uint32_t rowCount) { return 256u + alignUp(size_t(rowCount) * sizeof(float)); }

hipError_t runDenseExpression(const uint64_t* d_toc, const CountIn* d_data, const uint32_t* d_cellIds, const uint32_t* d_geneLocalIds,
                              uint32_t globalGeneCount, uint32_t geneCount, int method, uint32_t rowBegin, uint32_t rowEnd,
                              bool elementsAreDouble, void* d_out, size_t pitchElements, void* workspace, size_t workspaceBytes,
                              uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    if (rowEnd <= rowBegin) return hipSuccess;
    const uint32_t rows = rowEnd - rowBegin;
    if (workspaceBytes < denseExpressionWorkspaceBytes(rows)) return hipErrorInvalidValue;
    uint32_t* error = static_cast<uint32_t*>(workspace);
    float* factors = reinterpret_cast<float*>(static_cast<char*>(workspace) + 256u);
    StageTimer timer("denseExpression");
    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    denseFactorsKernel<<<dim3(gridFor(rows)), dim3(256), 0, stream>>>(d_toc, d_data, d_cellIds, d_geneLocalIds, globalGeneCount, geneCount,
                                                                      method, rowBegin, rowEnd, factors, error);
    EM2_TRY(hipGetLastError());
    // the gene ids are the fill's indices: nothing is written before they are known to be good
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (*inputError) return hipSuccess;
    EM2_TRY(timer.stage("factors", stream));
    const uint32_t blocks = rows < kFillBlocks ? rows : kFillBlocks;
    if (elementsAreDouble) {
        denseFillKernel<double><<<dim3(blocks), dim3(256), 0, stream>>>(d_toc, d_data, d_cellIds, d_geneLocalIds, globalGeneCount, geneCount,
                                                                        rowBegin, rowEnd, factors, static_cast<double*>(d_out), pitchElements);
    } else {
        denseFillKernel<float><<<dim3(blocks), dim3(256), 0, stream>>>(d_toc, d_data, d_cellIds, d_geneLocalIds, globalGeneCount, geneCount,
                                                                       rowBegin, rowEnd, factors, static_cast<float*>(d_out), pitchElements);
    }
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("fill", stream));
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

size_t em2_dev_dense_expression_workspace(uint32_t rowCount) { return em2::denseExpressionWorkspaceBytes(rowCount); }

// The device call under the name of the entry point that makes it.
static int devDenseExpression(const char* who, const uint64_t* d_toc, const em2_count* d_data, const uint32_t* d_cellIds, uint32_t cellCount,
                              const uint32_t* d_geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                              uint32_t rowBegin, uint32_t rowEnd, int elementType, void* d_out, uint64_t pitchElements, void* d_workspace,
                              size_t workspaceBytes, void* stream)
{
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (elementType != EM2_DENSE_FLOAT64 && elementType != EM2_DENSE_FLOAT32) {
        return failArgument(who, "elementType must be 0 (float64) or 1 (float32)");
    }
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (rowBegin > rowEnd || rowEnd > cellCount) return failArgument(who, "rowBegin <= rowEnd <= cellCount is required");
    if (pitchElements < geneCount) return failArgument(who, "pitchElements is below geneCount");
    if (rowBegin == rowEnd) return EM2_OK;
    if (!d_toc || !d_out || !d_workspace) return failNull(who);
    const size_t elementBytes = elementType == EM2_DENSE_FLOAT64 ? sizeof(double) : sizeof(float);
    if (reinterpret_cast<uintptr_t>(d_out) % elementBytes) return failArgument(who, "d_out is not aligned to its element");
    if (workspaceBytes < em2::denseExpressionWorkspaceBytes(rowEnd - rowBegin)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    static_assert(EM2_DENSE_FLOAT64 == 0 && EM2_DENSE_FLOAT32 == 1, "the element types as numbers");
    const bool elementsAreDouble = elementType == 0;          // (not by name: EM2_HIP keeps the call's text)
    EM2_HIP(em2::runDenseExpression(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), d_cellIds, d_geneLocalIds, globalGeneCount, geneCount,
                                    normalizationMethod, rowBegin, rowEnd, elementsAreDouble, d_out, size_t(pitchElements),
                                    d_workspace, workspaceBytes, &inputError, static_cast<hipStream_t>(stream)));
    if (inputError) return failArgument(who, em2::inputErrorText(inputError));
    return EM2_OK;
}

int em2_dev_dense_expression(const uint64_t* d_toc, const em2_count* d_data, const uint32_t* d_cellIds, uint32_t cellCount,
                             const uint32_t* d_geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                             uint32_t rowBegin, uint32_t rowEnd, int elementType, void* d_out, uint64_t pitchElements,
                             void* d_workspace, size_t workspaceBytes, void* stream)
{
    return devDenseExpression("em2_dev_dense_expression", d_toc, d_data, d_cellIds, cellCount, d_geneLocalIds, globalGeneCount, geneCount,
                              normalizationMethod, rowBegin, rowEnd, elementType, d_out, pitchElements, d_workspace, workspaceBytes, stream);
}

static const size_t kDenseDeviceBufferBytes = size_t(1) << 30;          // em2_dense_expression's device buffer at most

int em2_dense_expression(const uint64_t* toc, const em2_count* data, uint32_t csrCellCount, const uint32_t* cellIds, uint32_t cellCount,
                         const uint32_t* geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                         int elementType, void* out, uint64_t pitchElements)
{
    const char* who = "em2_dense_expression";
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (elementType != EM2_DENSE_FLOAT64 && elementType != EM2_DENSE_FLOAT32) {
        return failArgument(who, "elementType must be 0 (float64) or 1 (float32)");
    }
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (pitchElements < geneCount) return failArgument(who, "pitchElements is below geneCount");
    if (!cellIds && cellCount != csrCellCount) return failArgument(who, "without cellIds cellCount must be csrCellCount");
    if (cellCount == 0) return EM2_OK;
    if (!toc || !out || (!geneLocalIds && globalGeneCount)) return failNull(who);
    for (uint32_t i = 0; cellIds && i < cellCount; ++i) {
        if (cellIds[i] >= csrCellCount) return failArgument(who, "a cell id is not below the cell count of the CSR");
    }
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), csrCellCount)) return failArgument(who, error);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(csr.upload());                     // (the device checks the gene ids before any kernel indexes with them)
    DeviceBuffer dCellIds, dLocalIds, dOut, dWorkspace;
    if (cellIds) EM2_HIP(dCellIds.upload(cellIds, cellCount));
    if (geneLocalIds) EM2_HIP(dLocalIds.upload(geneLocalIds, globalGeneCount));
    const size_t elementBytes = elementType == EM2_DENSE_FLOAT64 ? sizeof(double) : sizeof(float);
    const size_t rowBytes = size_t(geneCount) * elementBytes;
    const uint64_t rowsThatFit = kDenseDeviceBufferBytes / rowBytes;
    const uint32_t chunkRows = uint32_t(rowsThatFit < 1 ? 1 : (rowsThatFit > cellCount ? cellCount : rowsThatFit));
    const size_t workspaceBytes = em2::denseExpressionWorkspaceBytes(chunkRows);
    EM2_HIP(dOut.allocate(size_t(chunkRows) * rowBytes));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    for (uint32_t rowBegin = 0; rowBegin < cellCount; rowBegin += chunkRows) {
        const uint32_t rowEnd = cellCount - rowBegin < chunkRows ? cellCount : rowBegin + chunkRows;
        const int rc = devDenseExpression(who, csr.toc.as<uint64_t>(), csr.data.as<em2_count>(), cellIds ? dCellIds.as<uint32_t>() : nullptr,
                                          cellCount, geneLocalIds ? dLocalIds.as<uint32_t>() : nullptr, globalGeneCount, geneCount,
                                          normalizationMethod, rowBegin, rowEnd, elementType, dOut.p, geneCount, dWorkspace.p, workspaceBytes,
                                          nullptr);
        if (rc != EM2_OK) return rc;
        // the geneCount elements of every row; the caller's padding stays as it is
        char* const to = static_cast<char*>(out) + size_t(rowBegin) * size_t(pitchElements) * elementBytes;
        if (pitchElements == geneCount) {
            EM2_HIP(hipMemcpy(to, dOut.p, size_t(rowEnd - rowBegin) * rowBytes, hipMemcpyDeviceToHost));
        } else {
            EM2_HIP(hipMemcpy2D(to, size_t(pitchElements) * elementBytes, dOut.p, rowBytes, rowBytes, rowEnd - rowBegin, hipMemcpyDeviceToHost));
        }
    }
    return EM2_OK;
}

}  // extern "C"
