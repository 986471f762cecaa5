// em2_cell_values.hip -- one number per cell of a list, the two colourings of the cell graph that are device work
// (ExpressionMatrix::exploreCellGraph, src/ExpressionMatrixHttpServerGraphs.cpp:788-850):
//   * cellSimilaritiesKernel<IN_LDS>   ExpressionMatrix::computeCellSimilarity (src/ExpressionMatrix.cpp:1468-1537) of one cell
//                          against a list.  Every block puts cell 0 into a RowVector (em2_expression.h) indexed by the gene
//                          set's local ids -- LDS, or global scratch for gene sets that do not fit -- and thread 0 forms sum0
//                          and sum00 over its kept entries in stored order; then a lane per listed cell walks that cell's
//                          entries once: sum1 and sum11 in stored order, sum01 from the float products with the row vector in
//                          ascending gene order, widened to double.  n is the gene set's size; numerator / denominator with
//                          no guard (0/0 is the reference's NaN).
//   * geneExpressionKernel a lane per listed cell: the value computeExpressionVector (:1253-1296) gives one gene.  The factor
//                          pass is em2_dense.hip's (1.f, float(1. / sum1), float(1. / sqrt(sum2)) over the kept entries in
//                          stored order, count * count a float product) and picks the gene's entry up on its way; without
//                          normalization there is no pass and the gene is found by bisection of the ascending row.  The
//                          value is factor * count, a float product, and 0 where the cell stores nothing for the gene: column
//                          localGene of em2_dev_dense_expression's float32 matrix.
// A cell's sums are chains of double additions in stored order, so a wave cannot share a row's arithmetic; a lane per cell it is
// for rows of every length.  Nothing is indexed with an unchecked id: a cell id not below cellCount, a local id not below
// geneCount and local ids that do not ascend are reported and never used.
// No FMA can form (-ffp-contract=off); the divisions and square roots are the correctly rounded __ddiv_rn / __dsqrt_rn.

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"

#include <string>
#include <vector>

namespace em2 {
namespace {

constexpr uint32_t kInvalid = 0xffffffffu;
constexpr uint32_t kBadCellId = 4u;                // error bits 0 and 1 are walkCell's
constexpr uint32_t kGeneNotInSet = 8u;
constexpr size_t kOwnLdsBytes = 16;                // sum0 and sum00 behind the row vector
constexpr uint32_t kValueBlocks = 1024;            // blocks at most: each loads cell 0 for itself

__device__ __forceinline__ uint32_t localGeneOf(const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t gene)
{
    if (!geneLocalIds) return gene;
    return gene < globalGeneCount ? geneLocalIds[gene] : kInvalid;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(256)
cellSimilaritiesKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount,
                       const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0,
                       const uint32_t* __restrict__ cellIds, uint32_t count, double* __restrict__ out, uint32_t* __restrict__ error,
                       char* scratch)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const RowVector row = rowVectorOf<IN_LDS>(lds, scratch, geneCount);
    double* const sums0 = reinterpret_cast<double*>(lds + (IN_LDS ? rowVectorBytes(geneCount) : 0u));
    uint32_t bad = 0u;

    // loadRow under local ids: the bitmap decides, so what the scratch held before is never read
    const uint32_t bitmapWords = (geneCount + 31u) / 32u;
    for (uint32_t w = threadIdx.x; w < bitmapWords; w += blockDim.x) row.present[w] = 0u;
    __syncthreads();
    const uint64_t begin0 = toc[cellId0], end0 = toc[cellId0 + 1u];
    for (uint64_t p = begin0 + threadIdx.x; p < end0; p += blockDim.x) {
        const CountIn c = data[p];
        const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, c.gene);
        if (local == kInvalid) continue;
        if (local >= geneCount) {
            bad |= 1u;
            continue;
        }
        row.dense[local] = c.count;
        atomicOr(row.present + (local >> 5), 1u << (local & 31u));
    }
    if (threadIdx.x == 0) {
        double sum0 = 0., sum00 = 0.;                                  // :1504-1512, stored order
        bool first = true;
        uint32_t previous = 0u;
        for (uint64_t p = begin0; p < end0; ++p) {
            const CountIn c = data[p];
            const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, c.gene);
            if (local == kInvalid) continue;
            if (!first && local <= previous) bad |= 2u;
            first = false;
            previous = local;
            sum0 += double(c.count);
            sum00 += double(c.count * c.count);                        // a float product
        }
        sums0[0] = sum0;
        sums0[1] = sum00;
    }
    __syncthreads();
    const double sum0 = sums0[0], sum00 = sums0[1];
    const double n = double(geneCount);

    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t cell = cellIds ? cellIds[i] : uint32_t(i);
        if (cell >= cellCount) {
            bad |= kBadCellId;
            continue;
        }
        double sum01 = 0., sum1 = 0., sum11 = 0.;
        bool first = true;
        uint32_t previous = 0u;
        const uint64_t end = toc[cell + 1u];
        for (uint64_t p = toc[cell]; p < end; ++p) {
            const CountIn c = data[p];
            const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, c.gene);
            if (local == kInvalid) continue;
            if (local >= geneCount) {
                bad |= 1u;
                continue;
            }
            if (!first && local <= previous) bad |= 2u;
            first = false;
            previous = local;
            addProduct(row, CountIn{local, c.count}, sum01);           // :1480-1499
            sum1 += double(c.count);                                   // :1514-1523
            sum11 += double(c.count * c.count);
        }
        const double numerator = n * sum01 - sum0 * sum1;              // :1529-1535
        const double denominator = __dsqrt_rn((n * sum00 - sum0 * sum0) * (n * sum11 - sum1 * sum1));
        out[i] = __ddiv_rn(numerator, denominator);
    }
    if (bad) atomicOr(error, bad);
}

__global__ void __launch_bounds__(256)
geneExpressionKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount,
                     const uint32_t* __restrict__ geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId,
                     int method, const uint32_t* __restrict__ cellIds, uint32_t count, float* __restrict__ out,
                     uint32_t* __restrict__ error)
{
    const uint32_t localGene = localGeneOf(geneLocalIds, globalGeneCount, globalGeneId);
    if (localGene >= geneCount) {                                      // (kInvalid too) CZI_ASSERT, :821
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(error, kGeneNotInSet);
        return;
    }
    uint32_t bad = 0u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t cell = cellIds ? cellIds[i] : uint32_t(i);
        if (cell >= cellCount) {
            bad |= kBadCellId;
            continue;
        }
        const uint64_t begin = toc[cell], end = toc[cell + 1u];
        bool stored = false;
        float geneCountValue = 0.f;
        float factor = 1.f;
        if (method == 0) {
            // the first entry whose gene is not below globalGeneId, by bisection of the ascending row
            uint64_t low = begin, high = end;
            while (low < high) {
                const uint64_t middle = low + (high - low) / 2u;
                if (data[middle].gene < globalGeneId) low = middle + 1u;
                else high = middle;
            }
            if (low < end) {
                const CountIn c = data[low];
                if (c.gene == globalGeneId) {
                    stored = true;
                    geneCountValue = c.count;
                }
            }
        } else {
            double sum1 = 0., sum2 = 0.;
            bool first = true;
            uint32_t previous = 0u;
            for (uint64_t p = begin; p < end; ++p) {
                const CountIn c = data[p];
                const uint32_t local = localGeneOf(geneLocalIds, globalGeneCount, c.gene);
                if (local == kInvalid) continue;
                if (local >= geneCount) bad |= 1u;
                if (!first && local <= previous) bad |= 2u;
                first = false;
                previous = local;
                sum1 += double(c.count);
                sum2 += double(c.count * c.count);                     // a float product (:1286)
                if (local == localGene && !stored) {                   // the reference's loop breaks at the first (:827-832)
                    stored = true;
                    geneCountValue = c.count;
                }
            }
            factor = method == 1 ? float(__ddiv_rn(1., sum1)) : float(__ddiv_rn(1., __dsqrt_rn(sum2)));     // :1282, :1288
        }
        out[i] = stored ? factor * geneCountValue : 0.f;               // :1294, a float product
    }
    if (bad) atomicOr(error, bad);
}

size_t rowHomeBytes(uint32_t geneCount, uint32_t blocks)
{
    return rowFitsLds(geneCount, kOwnLdsBytes) ? 0u : rowScratchBytes(geneCount, blocks);
}

uint32_t valueBlocks(uint32_t count)
{
    const uint32_t blocks = blocksOf(count, 256u);
    return blocks > kValueBlocks ? kValueBlocks : (blocks ? blocks : 1u);
}

const char* valueErrorText(uint32_t bad)
{
    return (bad & kBadCellId) ? "a cell id is not below the cell count" : inputErrorText(bad);
}

}  // namespace

size_t cellSimilaritiesWorkspaceBytes(uint32_t geneCount, uint32_t count) { return 256u + rowHomeBytes(geneCount, valueBlocks(count)); }

hipError_t runCellSimilarities(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                               uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* d_cellIds, uint32_t count,
                               double* d_out, void* workspace, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    if (count == 0) return hipSuccess;
    uint32_t* error = static_cast<uint32_t*>(workspace);
    StageTimer timer("cellSimilarities");
    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    const bool inLds = rowFitsLds(geneCount, kOwnLdsBytes);
    EM2_TRY(launchRowKernel(inLds, cellSimilaritiesKernel<true>, cellSimilaritiesKernel<false>, valueBlocks(count), 256u, geneCount,
                            kOwnLdsBytes, static_cast<char*>(workspace) + 256u, stream, d_toc, d_data, cellCount, d_geneLocalIds,
                            globalGeneCount, geneCount, cellId0, d_cellIds, count, d_out, error));
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    return timer.stage("kernel", stream);
}

hipError_t runGeneExpression(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                             uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int method, const uint32_t* d_cellIds,
                             uint32_t count, float* d_out, void* workspace, uint32_t* inputError, hipStream_t stream)
{
    uint32_t* error = static_cast<uint32_t*>(workspace);
    StageTimer timer("geneExpression");
    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    geneExpressionKernel<<<dim3(gridFor(count)), dim3(256), 0, stream>>>(d_toc, d_data, cellCount, d_geneLocalIds, globalGeneCount, geneCount,
                                                                         globalGeneId, method, d_cellIds, count, d_out, error);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    return timer.stage("kernel", stream);
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

size_t em2_dev_cell_similarities_to_cell_workspace(uint32_t geneCount, uint32_t count) { return em2::cellSimilaritiesWorkspaceBytes(geneCount, count); }

int em2_cell_similarities_row_in_lds(uint32_t geneCount) { return em2::rowFitsLds(geneCount, em2::kOwnLdsBytes) ? 1 : 0; }

static int devCellSimilarities(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                               uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* d_cellIds, uint32_t count,
                               double* d_out, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellId0 >= cellCount) return failArgument(who, "cellId0 is not below the cell count");
    if (!d_cellIds && count > cellCount) return failArgument(who, "without cellIds count must not exceed the cell count");
    if (count == 0) return EM2_OK;
    if (!d_toc || !d_out || !d_workspace) return failNull(who);
    if (workspaceBytes < em2::cellSimilaritiesWorkspaceBytes(geneCount, count)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    EM2_HIP(em2::runCellSimilarities(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), cellCount, d_geneLocalIds, globalGeneCount,
                                     geneCount, cellId0, d_cellIds, count, d_out, d_workspace, &inputError,
                                     static_cast<hipStream_t>(stream)));
    if (inputError) return failArgument(who, em2::valueErrorText(inputError));
    return EM2_OK;
}

int em2_dev_cell_similarities_to_cell(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                                      uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* d_cellIds,
                                      uint32_t count, double* d_out, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return devCellSimilarities("em2_dev_cell_similarities_to_cell", d_toc, d_data, cellCount, d_geneLocalIds, globalGeneCount, geneCount,
                               cellId0, d_cellIds, count, d_out, d_workspace, workspaceBytes, stream);
}

// What the two host forms share: the checks of the list, the CSR and the tables on the device.
namespace {
struct UploadedValuesInput {
    em2::UploadedCsr csr;
    DeviceBuffer cellIds, localIds;
};
}  // namespace

static int uploadValuesInput(const char* who, const uint64_t* toc, const em2_count* data, uint32_t cellCount, const uint32_t* geneLocalIds,
                             uint32_t globalGeneCount, const uint32_t* cellIds, uint32_t count, UploadedValuesInput& in)
{
    if (!toc || (!geneLocalIds && globalGeneCount)) return failNull(who);
    if (!cellIds && count > cellCount) return failArgument(who, "without cellIds count must not exceed the cell count");
    for (uint32_t i = 0; cellIds && i < count; ++i) {
        if (cellIds[i] >= cellCount) return failArgument(who, "a cell id is not below the cell count");
    }
    if (const char* error = in.csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(in.csr.upload());
    if (cellIds) EM2_HIP(in.cellIds.upload(cellIds, count));
    if (geneLocalIds) EM2_HIP(in.localIds.upload(geneLocalIds, globalGeneCount));
    return EM2_OK;
}

int em2_cell_similarities_to_cell(const uint64_t* toc, const em2_count* data, uint32_t cellCount, const uint32_t* geneLocalIds,
                                  uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* cellIds, uint32_t count,
                                  double* out)
{
    const char* who = "em2_cell_similarities_to_cell";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellId0 >= cellCount) return failArgument(who, "cellId0 is not below the cell count");
    if (count && !out) return failNull(who);
    UploadedValuesInput in;
    const int rc = uploadValuesInput(who, toc, data, cellCount, geneLocalIds, globalGeneCount, cellIds, count, in);
    if (rc != EM2_OK || count == 0) return rc;
    DeviceBuffer dOut, dWorkspace;
    const size_t workspaceBytes = em2::cellSimilaritiesWorkspaceBytes(geneCount, count);
    EM2_HIP(dOut.allocateFor<double>(count));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int status = devCellSimilarities(who, in.csr.toc.as<uint64_t>(), in.csr.data.as<em2_count>(), cellCount,
                                           geneLocalIds ? in.localIds.as<uint32_t>() : nullptr, globalGeneCount, geneCount, cellId0,
                                           cellIds ? in.cellIds.as<uint32_t>() : nullptr, count, dOut.as<double>(), dWorkspace.p,
                                           workspaceBytes, nullptr);
    if (status != EM2_OK) return status;
    EM2_HIP(dOut.download(out, count));
    return EM2_OK;
}

size_t em2_dev_gene_expression_of_cells_workspace(void) { return 256u; }

static int devGeneExpression(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                             uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int normalizationMethod,
                             const uint32_t* d_cellIds, uint32_t count, float* d_out, void* d_workspace, size_t workspaceBytes, void* stream)
{
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (!d_cellIds && count > cellCount) return failArgument(who, "without cellIds count must not exceed the cell count");
    if (!d_workspace || (count && (!d_toc || !d_out))) return failNull(who);
    if (workspaceBytes < 256u) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    // (an empty list still asks whether the gene is in the gene set)
    EM2_HIP(em2::runGeneExpression(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), cellCount, d_geneLocalIds, globalGeneCount, geneCount,
                                   globalGeneId, normalizationMethod, d_cellIds, count, d_out, d_workspace, &inputError,
                                   static_cast<hipStream_t>(stream)));
    if (inputError & em2::kGeneNotInSet) {
        return fail(EM2_ERROR_RUNTIME, std::string(who) + ": Assertion failed: localGeneId != invalidGeneId (gene " +
                                           std::to_string(globalGeneId) + " is not in the gene set)");
    }
    if (inputError) return failArgument(who, em2::valueErrorText(inputError));
    return EM2_OK;
}

int em2_dev_gene_expression_of_cells(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                                     uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int normalizationMethod,
                                     const uint32_t* d_cellIds, uint32_t count, float* d_out, void* d_workspace, size_t workspaceBytes,
                                     void* stream)
{
    return devGeneExpression("em2_dev_gene_expression_of_cells", d_toc, d_data, cellCount, d_geneLocalIds, globalGeneCount, geneCount,
                             globalGeneId, normalizationMethod, d_cellIds, count, d_out, d_workspace, workspaceBytes, stream);
}

int em2_gene_expression_of_cells(const uint64_t* toc, const em2_count* data, uint32_t cellCount, const uint32_t* geneLocalIds,
                                 uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int normalizationMethod,
                                 const uint32_t* cellIds, uint32_t count, float* out)
{
    const char* who = "em2_gene_expression_of_cells";
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (count && !out) return failNull(who);
    UploadedValuesInput in;
    const int rc = uploadValuesInput(who, toc, data, cellCount, geneLocalIds, globalGeneCount, cellIds, count, in);
    if (rc != EM2_OK) return rc;
    DeviceBuffer dOut, dWorkspace;
    EM2_HIP(dOut.allocateFor<float>(count));
    EM2_HIP(dWorkspace.allocate(256u));
    const int status = devGeneExpression(who, in.csr.toc.as<uint64_t>(), in.csr.data.as<em2_count>(), cellCount,
                                         geneLocalIds ? in.localIds.as<uint32_t>() : nullptr, globalGeneCount, geneCount, globalGeneId,
                                         normalizationMethod, cellIds ? in.cellIds.as<uint32_t>() : nullptr, count, dOut.as<float>(),
                                         dWorkspace.p, 256u, nullptr);
    if (status != EM2_OK) return status;
    EM2_HIP(dOut.download(out, count));
    return EM2_OK;
}

}  // extern "C"
