// em2_expression.h -- what the kernels that read the expression counts themselves (the CSR of toc and (gene, count)
// entries, not the LSH signatures) share: a cell's sums with the input check, the row cell as a dense vector with a
// presence bitmap and the sparse scalar product against it, and where that vector lives (LDS, or global scratch for gene
// sets that do not fit).  The arithmetic is pinned bit for bit by ExpressionMatrixSubset::computeSums
// (src/ExpressionMatrixSubset.cpp:47-58) and ExpressionMatrixSubset::computeCellSimilarity (:83-133).
#ifndef EM2_EXPRESSION_H
#define EM2_EXPRESSION_H

#include "em2_device.h"
#include "em2_hip_util.h"

namespace em2 {

struct CellWalk {
    double sum1, sum2;      // ExpressionMatrixSubset::Sum
    uint32_t bad;           // bit 0: a gene id not below geneCount; bit 1: gene ids not strictly ascending
};

// computeSums over the entries of one cell in stored order.
__device__ __forceinline__ CellWalk walkCell(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint64_t cell,
                                             uint32_t geneCount)
{
    CellWalk w{0., 0., 0u};
    uint32_t previous = 0u;
    const uint64_t begin = toc[cell], end = toc[cell + 1u];
    for (uint64_t p = begin; p < end; ++p) {
        const CountIn e = data[p];
        if (e.gene >= geneCount) w.bad |= 1u;
        if (p != begin && e.gene <= previous) w.bad |= 2u;
        previous = e.gene;
        w.sum1 += double(e.count);
        w.sum2 += double(e.count * e.count);             // count*count is a float product (:55)
    }
    return w;
}

// The text of a nonzero error word of walkCell (the caller puts its own name in front).
inline const char* inputErrorText(uint32_t bad)
{
    return (bad & 1u) ? "a local gene id is not below geneCount" : "the gene ids of a cell are not strictly ascending";
}

// A stored zero, inf or NaN count takes part in the products exactly as in the reference's merge loop, because the bitmap
// and not the value decides; what an earlier row left in `dense` is never read for the same reason.
struct RowVector {
    float* dense;           // [geneCount]
    uint32_t* present;      // [(geneCount + 31) / 32]
};

// Clears the bitmap and scatters the row cell's counts.  Ends with a barrier; the caller puts one between the last use of
// a row and the next loadRow.
__device__ __forceinline__ void loadRow(const RowVector& row, uint32_t geneCount, const uint64_t* __restrict__ toc,
                                        const CountIn* __restrict__ data, uint32_t cell)
{
    const uint32_t bitmapWords = (geneCount + 31u) / 32u;
    for (uint32_t w = threadIdx.x; w < bitmapWords; w += blockDim.x) row.present[w] = 0u;
    __syncthreads();
    const uint64_t end = toc[cell + 1u];
    for (uint64_t p = toc[cell] + threadIdx.x; p < end; p += blockDim.x) {
        const CountIn c = data[p];
        row.dense[c.gene] = c.count;
        atomicOr(row.present + (c.gene >> 5), 1u << (c.gene & 31u));
    }
    __syncthreads();
}

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

// A kernel of this kind is a template <bool IN_LDS> whose last parameter is the scratch of the global-memory form.  In
// the LDS form a block owns one row and the vector is the front of its dynamic LDS; in the global-memory form at most
// kRowScratchBlocks blocks stride over the rows, each with a vector of its own in the scratch.

constexpr size_t kLdsBytes = 160u * 1024u;              // per workgroup on gfx950
constexpr uint32_t kRowScratchBlocks = 1024;

// The floats, then the bitmap, each padded to 8 bytes (what follows in LDS may hold 8-byte records).
__host__ __device__ inline uint32_t rowVectorBytes(uint32_t geneCount)
{
    return ((geneCount * 4u + 7u) & ~7u) + ((((geneCount + 31u) / 32u) * 4u + 7u) & ~7u);
}

inline uint32_t rowScratchBlocks(uint32_t rows) { return rows < kRowScratchBlocks ? rows : kRowScratchBlocks; }

// The scratch of the global-memory form for a launch over `rows` rows.
inline size_t rowScratchBytes(uint32_t geneCount, uint32_t rows) { return alignUp(size_t(rowVectorBytes(geneCount)) * rowScratchBlocks(rows)); }

// Whether the row vector and `ownLdsBytes` more fit the LDS of a workgroup.
inline bool rowFitsLds(uint32_t geneCount, size_t ownLdsBytes = 0) { return rowVectorBytes(geneCount) + ownLdsBytes <= kLdsBytes; }

// The block's row vector.  LDS of the kernel's own starts rowVectorBytes behind the dynamic LDS base in the LDS form.
template <bool IN_LDS>
__device__ __forceinline__ RowVector rowVectorOf(unsigned char* lds, char* scratch, uint32_t geneCount)
{
    unsigned char* base = IN_LDS ? lds : reinterpret_cast<unsigned char*>(scratch) + size_t(blockIdx.x) * rowVectorBytes(geneCount);
    return RowVector{reinterpret_cast<float*>(base), reinterpret_cast<uint32_t*>(base + ((geneCount * 4u + 7u) & ~7u))};
}

// Launches the form asked for over `rows` rows: the LDS form with a block of ldsFormThreads per row, the global-memory
// form with blocks of 256 threads; either with ownLdsBytes of dynamic LDS behind the row vector.
template <class... Parameters, class... Arguments>
hipError_t launchRowKernel(bool inLds, void (*ldsForm)(Parameters...), void (*globalForm)(Parameters...), uint32_t rows,
                           uint32_t ldsFormThreads, uint32_t geneCount, size_t ownLdsBytes, void* scratch, hipStream_t stream,
                           Arguments... arguments)
{
    void (*kernel)(Parameters...) = inLds ? ldsForm : globalForm;
    const size_t ldsBytes = ownLdsBytes + (inLds ? rowVectorBytes(geneCount) : 0u);
    EM2_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(ldsBytes)));
    kernel<<<dim3(inLds ? rows : rowScratchBlocks(rows)), dim3(inLds ? ldsFormThreads : 256u), ldsBytes, stream>>>(
        arguments..., inLds ? nullptr : static_cast<char*>(scratch));
    return hipGetLastError();
}

}  // namespace em2

#endif
