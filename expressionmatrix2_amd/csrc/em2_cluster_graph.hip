// em2_cluster_graph.hip -- the rest of ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2087-2185) after
// the label propagation: ClusterGraph (src/ClusterGraph.cpp:59-386), the clusters' average expression
// (ExpressionMatrix::computeAverageExpression / computeExpressionVector, src/ExpressionMatrix.cpp:1179-1296, L2 only) and
// the similarity of two clusters (src/regressionCoefficient.cpp:10-42).
//
// What the reference's arithmetic pins is the ORDER of its double sums:
//   * a cell's norm: sum += c*c (float product) over the cell's entries in stored order (:1285-1288);
//   * avg[g] += float(c * factor) over the cluster's cells in the order of ClusterGraphVertex::cells (:1194-1205);
//   * sum += a*a over g ascending (:1231-1235); sx, sxx (per vertex) and sxy (per edge) over g ascending.
// Additions into one (cluster, gene) accumulator are ordered; different accumulators are independent.  The device runs:
//   1. clusterFactorKernel    one lane per listed cell: the norm's sequential sum (em2_expression.h's cell walk, which
//                             checks the gene ids before any kernel builds an index from them), factor = float(1/sqrt(sum));
//   2. clusterGatherKernel    one wave per listed cell: (key = cluster * geneCount + gene, value = float(c * factor)) at
//                             the cell's place in the concatenation of the clusters' cell lists;
//   3. rocPRIM radix sort of the pairs by key (stable: equal keys keep the order of the cell lists);
//   4. clusterRunKernel       one lane per entry: the first entry of every key's run into the dense table slot of that key;
//      clusterSumKernel       one lane per (cluster, gene): walks its run front to back, sum += double(value);
//   5. clusterNormalizeKernel one wave per cluster: a *= 1/cellCount, then products a*a chunk by chunk through LDS by all
//                             lanes and their sum by lane 0 in ascending g, a *= 1/sqrt(sum);
//   6. clusterVertexSumsKernel (sx, sxx once per vertex) and clusterEdgeKernel (sxy per edge) in the same
//      products-in-parallel, sum-by-one-lane form.
// Every product is rounded before its addition (-ffp-contract=off, as for the projection and fsp0); square roots and
// divisions are the correctly rounded ones.  The handful of operations per edge after the sums (numerator, denominator,
// quotient) and all of the graph bookkeeping -- the label map, the connected components of the merge, the removals, makeKnn,
// the std::sort of the renumbering -- are host code.
//
// Two places the reference does not pin:
//   * makeKnn sorts pair<double, edge_descriptor> with std::greater: edges of one vertex with exactly equal similarity are
//     ordered by the descriptors, i.e. by addresses.  Here the edge created LATER in the construction ranks higher.
//   * a NaN similarity (a cluster without variance, or an all-zero average) survives removeWeakEdges and makes that sort
//     undefined: EM2_ERROR_RUNTIME.

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"
#include "em2_primitives.h"
#include "../../include/em2_lsh.h"

#include <cstring>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <unordered_map>
#include <unordered_set>

#include <memory>
#include <string>
#include <vector>

// What the device code and the C entry points at the end of this file share.
namespace em2 {

struct ClusterStatus {
    int code;                   // EM2_OK or an EM2_ERROR_* of include/em2_lsh.h
    std::string message;
};

// The device side of ClusterGraph::computeAverageGeneExpression / computeSimilarities (src/ClusterGraph.cpp:125-169):
// holds the expression counts and the table of averages [cluster][gene] in device memory between the calls.
class ClusterDevice {
public:
    ClusterDevice();
    ~ClusterDevice();
    ClusterDevice(const ClusterDevice&) = delete;
    ClusterDevice& operator=(const ClusterDevice&) = delete;
    ClusterStatus upload(const char* who, const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount);
    ClusterStatus setAverages(const double* averages, uint32_t clusterCount, uint32_t geneCount);
    ClusterStatus averages(const char* who, const uint32_t* cellRows, const uint64_t* offsets, uint32_t clusterCount, double* hostAverages);
    ClusterStatus similarities(const char* who, const uint32_t* edge0, const uint32_t* edge1, uint64_t edgeCount, double* similarity);

private:
    struct State;
    State* state;
};

// What ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2153-2181) leaves in the ClusterGraph.  Clusters in
// vertex order; cells and unclusteredCells are cell-graph vertex indices; edges in the order of their creation.
struct ClusterGraphResult {
    uint32_t geneCount = 0;
    std::vector<uint32_t> clusterIds;
    std::vector<uint64_t> cellOffsets;
    std::vector<uint32_t> cells, unclusteredCells;
    std::vector<double> averages;
    std::vector<uint32_t> edgeCluster0, edgeCluster1;
    std::vector<double> edgeSimilarity;
    uint32_t initialClusterCount = 0;       // vertices and edges of the constructor, before the merge
    uint64_t initialEdgeCount = 0;
    double averagesSeconds = 0., similaritiesSeconds = 0., totalSeconds = 0.;
};

static ClusterStatus createClusterGraph(const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount,
                                        const uint32_t* vertexRows, uint32_t vertexCount, const uint32_t* edgeVertex0,
                                        const uint32_t* edgeVertex1, uint64_t edgeCount, const uint32_t* labels, uint64_t minClusterSize,
                                        uint64_t k, double similarityThreshold, double similarityThresholdForMerge, ClusterGraphResult& out);

namespace {

constexpr uint32_t kChunk = 1024;                   // doubles of LDS per wave in the sequential-sum kernels
constexpr unsigned long long kNoRun = ~0ull;

__global__ void __launch_bounds__(256)
clusterFactorKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t geneCount,
                    const uint32_t* __restrict__ cellRows, uint64_t listCount, float* __restrict__ factor,
                    uint32_t* __restrict__ error)
{
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= listCount) return;
    const CellWalk w = walkCell(toc, data, cellRows[i], geneCount);  // sum2: p.second * p.second, a float product (:1286)
    factor[i] = float(__ddiv_rn(1., __dsqrt_rn(w.sum2)));            // :1288
    if (w.bad) atomicOr(error, w.bad);
}

__global__ void __launch_bounds__(256)
clusterGatherKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t geneCount,
                    const uint32_t* __restrict__ cellRows, const uint32_t* __restrict__ clusterOfPosition,
                    const uint64_t* __restrict__ entryOffset, const float* __restrict__ factor, uint64_t listCount,
                    uint64_t* __restrict__ keys, float* __restrict__ values)
{
    const uint64_t i = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= listCount) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = cellRows[i];
    const uint64_t begin = toc[row], count = toc[row + 1u] - begin, out = entryOffset[i];
    const uint64_t base = uint64_t(clusterOfPosition[i]) * geneCount;
    const float f = factor[i];
    for (uint64_t q = lane; q < count; q += 64u) {
        const CountIn e = data[begin + q];
        keys[out + q] = base + e.gene;
        values[out + q] = e.count * f;                               // p.second *= factor: float (:1293-1295)
    }
}

__global__ void __launch_bounds__(256)
clusterRunKernel(const uint64_t* __restrict__ keys, uint64_t entryCount, unsigned long long* __restrict__ table)
{
    const uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= entryCount) return;
    const uint64_t key = keys[p];
    if (p == 0u || keys[p - 1u] != key) table[key] = p;
}

// table[t]: in, the first entry of accumulator t's run or kNoRun; out, the accumulator (:1194-1205).  Four entries are
// loaded ahead of their use (the addresses do not depend on the values); the sum stays in order.
__global__ void __launch_bounds__(256)
clusterSumKernel(const uint64_t* __restrict__ keys, const float* __restrict__ values, uint64_t entryCount,
                 unsigned long long* table, uint64_t accumulatorCount)
{
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= accumulatorCount) return;
    uint64_t p = table[t];
    double sum = 0.;
    if (p != kNoRun) {
        for (;;) {
            uint64_t key[4];
            float value[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint64_t q = p + j < entryCount ? p + j : entryCount - 1u;
                key[j] = keys[q];
                value[j] = values[q];
            }
            bool live = true;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                live = live && p + j < entryCount && key[j] == t;
                if (live) sum += double(value[j]);                   // averageExpression[localGeneId] += normalizedCount
            }
            if (!live) break;
            p += 4u;
        }
    }
    reinterpret_cast<double*>(table)[t] = sum;
}

// :1209-1240 for cluster blockIdx.x.  One wave.
__global__ void __launch_bounds__(64)
clusterNormalizeKernel(double* __restrict__ table, uint32_t geneCount, const double* __restrict__ inverseCellCount)
{
    __shared__ double products[kChunk];
    __shared__ double shared;
    double* a = table + size_t(blockIdx.x) * geneCount;
    const double inverse = inverseCellCount[blockIdx.x];
    double sum = 0.;
    for (uint32_t g0 = 0; g0 < geneCount; g0 += kChunk) {
        const uint32_t m = geneCount - g0 < kChunk ? geneCount - g0 : kChunk;
        for (uint32_t i = threadIdx.x; i < m; i += 64u) {
            const double x = a[g0 + i] * inverse;                    // a *= factor (:1210-1213)
            a[g0 + i] = x;
            products[i] = x * x;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t i = 0; i < m; ++i) sum += products[i];     // sum += a * a, g ascending (:1231-1235)
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) shared = __ddiv_rn(1., __dsqrt_rn(sum));   // :1236
    __syncthreads();
    const double factor = shared;
    for (uint32_t g = threadIdx.x; g < geneCount; g += 64u) a[g] = a[g] * factor;
}

// sx and sxx of src/regressionCoefficient.cpp:22-35 depend on one vector only: once per vertex.
__global__ void __launch_bounds__(64)
clusterVertexSumsKernel(const double* __restrict__ table, uint32_t geneCount, double* __restrict__ sx, double* __restrict__ sxx)
{
    __shared__ double values[kChunk];
    __shared__ double products[kChunk];
    const double* a = table + size_t(blockIdx.x) * geneCount;
    double s = 0., ss = 0.;
    for (uint32_t g0 = 0; g0 < geneCount; g0 += kChunk) {
        const uint32_t m = geneCount - g0 < kChunk ? geneCount - g0 : kChunk;
        for (uint32_t i = threadIdx.x; i < m; i += 64u) {
            const double x = a[g0 + i];
            values[i] = x;
            products[i] = x * x;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t i = 0; i < m; ++i) {
                s += values[i];
                ss += products[i];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sx[blockIdx.x] = s;
        sxx[blockIdx.x] = ss;
    }
}

// sxy (:34) per edge.  One wave per block, edges strided over the grid.
__global__ void __launch_bounds__(64)
clusterEdgeKernel(const double* __restrict__ table, uint32_t geneCount, const uint32_t* __restrict__ edge0,
                  const uint32_t* __restrict__ edge1, uint64_t edgeCount, double* __restrict__ sxy)
{
    __shared__ double products[kChunk];
    for (uint64_t e = blockIdx.x; e < edgeCount; e += gridDim.x) {
        const double* x = table + size_t(edge0[e]) * geneCount;
        const double* y = table + size_t(edge1[e]) * geneCount;
        double s = 0.;
        for (uint32_t g0 = 0; g0 < geneCount; g0 += kChunk) {
            const uint32_t m = geneCount - g0 < kChunk ? geneCount - g0 : kChunk;
            for (uint32_t i = threadIdx.x; i < m; i += 64u) products[i] = x[g0 + i] * y[g0 + i];
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t i = 0; i < m; ++i) s += products[i];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) sxy[e] = s;
    }
}

ClusterStatus ok() { return ClusterStatus{EM2_OK, std::string()}; }

ClusterStatus hipFailure(hipError_t e, const char* what)
{
    return ClusterStatus{EM2_ERROR_HIP, std::string(what) + ": " + hipGetErrorString(e)};
}

#define EM2_TRYC(call)                                                    \
    do {                                                                  \
        const hipError_t em2Error_ = (call);                              \
        if (em2Error_ != hipSuccess) return hipFailure(em2Error_, #call); \
    } while (0)

double secondsSince(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace


struct ClusterDevice::State {
    UploadedCsr csr;
    DeviceBuffer table, sx, sxx;
    uint32_t rowCount = 0, geneCount = 0, clusterCount = 0;
};

ClusterDevice::ClusterDevice() : state(new State) {}
ClusterDevice::~ClusterDevice() { delete state; }

ClusterStatus ClusterDevice::upload(const char* who, const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount)
{
    State& s = *state;
    if (const char* error = s.csr.check(toc, data, rowCount)) return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": " + error};
    s.rowCount = rowCount;
    s.geneCount = geneCount;
    EM2_TRYC(s.csr.upload());
    return ok();
}

ClusterStatus ClusterDevice::setAverages(const double* averages, uint32_t clusterCount, uint32_t geneCount)
{
    State& s = *state;
    s.geneCount = geneCount;
    s.clusterCount = clusterCount;
    const size_t bytes = size_t(clusterCount) * geneCount * sizeof(double);
    EM2_TRYC(s.table.allocate(bytes));
    if (bytes) EM2_TRYC(hipMemcpy(s.table.p, averages, bytes, hipMemcpyHostToDevice));
    return ok();
}

// The averages of clusterCount clusters into the device table [cluster][gene]; cluster c holds the rows
// cellRows[offsets[c] .. offsets[c + 1]) in that order.  hostAverages may be null.
ClusterStatus ClusterDevice::averages(const char* who, const uint32_t* cellRows, const uint64_t* offsets, uint32_t clusterCount,
                                      double* hostAverages)
{
    State& s = *state;
    const uint32_t geneCount = s.geneCount;
    const uint64_t listCount = offsets[clusterCount];
    s.clusterCount = clusterCount;
    const uint64_t accumulatorCount = uint64_t(clusterCount) * geneCount;
    if (accumulatorCount == 0) return ok();

    std::vector<uint32_t> clusterOfPosition(listCount);
    std::vector<uint64_t> entryOffset(size_t(listCount) + 1);
    std::vector<double> inverseCellCount(clusterCount);
    uint64_t entryCount = 0;
    for (uint32_t c = 0; c < clusterCount; ++c) {
        if (offsets[c] > offsets[c + 1]) return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the cluster offsets are not ascending"};
        inverseCellCount[c] = 1. / double(offsets[c + 1] - offsets[c]);                     // :1210
        for (uint64_t i = offsets[c]; i < offsets[c + 1]; ++i) {
            const uint32_t row = cellRows[i];
            if (row >= s.rowCount) return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a cluster names a cell that does not exist"};
            clusterOfPosition[i] = c;
            entryOffset[i] = entryCount;
            entryCount += s.csr.hostToc[row + 1] - s.csr.hostToc[row];
        }
    }
    entryOffset[listCount] = entryCount;

    // the dense table and the sort's buffers against what the device has free
    const size_t tableBytes = size_t(accumulatorCount) * sizeof(double);
    size_t sortTempBytes = 0;
    if (entryCount) {
        EM2_TRYC(sortPairsU64F32Bytes(size_t(entryCount), 0u, 64u, sortTempBytes));
    }
    const size_t scratchBytes = size_t(entryCount) * 24u + sortTempBytes + size_t(listCount) * 16u + size_t(clusterCount) * 8u;
    s.table.release();
    size_t freeBytes = 0, totalBytes = 0;
    EM2_TRYC(hipMemGetInfo(&freeBytes, &totalBytes));
    if (tableBytes + scratchBytes > freeBytes) {
        return ClusterStatus{EM2_ERROR_HIP, std::string(who) + ": " + hipGetErrorString(hipErrorOutOfMemory) + ": the table of " +
                                                std::to_string(clusterCount) + " clusters x " + std::to_string(geneCount) + " genes takes " +
                                                std::to_string(tableBytes) + " bytes and the sort of " + std::to_string(entryCount) +
                                                " expression counts " + std::to_string(scratchBytes) + ", the device has " +
                                                std::to_string(freeBytes) + " free"};
    }
    EM2_TRYC(s.table.allocate(tableBytes));

    DeviceBuffer rows, positions, entryOffsets, factor, inverse, error, keysIn, keysOut, valuesIn, valuesOut, temp;
    EM2_TRYC(rows.allocate(listCount * sizeof(uint32_t)));
    EM2_TRYC(positions.allocate(listCount * sizeof(uint32_t)));
    EM2_TRYC(entryOffsets.allocate((listCount + 1) * sizeof(uint64_t)));
    EM2_TRYC(factor.allocate(listCount * sizeof(float)));
    EM2_TRYC(inverse.allocate(size_t(clusterCount) * sizeof(double)));
    EM2_TRYC(error.allocate(sizeof(uint32_t)));
    EM2_TRYC(hipMemcpy(inverse.p, inverseCellCount.data(), size_t(clusterCount) * sizeof(double), hipMemcpyHostToDevice));
    EM2_TRYC(hipMemset(error.p, 0, sizeof(uint32_t)));
    EM2_TRYC(hipMemset(s.table.p, 0xff, tableBytes));                                       // kNoRun everywhere
    hipStream_t stream = nullptr;
    if (listCount) {
        EM2_TRYC(hipMemcpy(rows.p, cellRows, listCount * sizeof(uint32_t), hipMemcpyHostToDevice));
        EM2_TRYC(hipMemcpy(positions.p, clusterOfPosition.data(), listCount * sizeof(uint32_t), hipMemcpyHostToDevice));
        EM2_TRYC(hipMemcpy(entryOffsets.p, entryOffset.data(), (listCount + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        clusterFactorKernel<<<dim3(blocksOf(listCount, 256u)), dim3(256), 0, stream>>>(
            s.csr.toc.as<uint64_t>(), s.csr.data.as<CountIn>(), geneCount, rows.as<uint32_t>(), listCount, factor.as<float>(), error.as<uint32_t>());
        EM2_TRYC(hipGetLastError());
        uint32_t inputError = 0;
        EM2_TRYC(hipMemcpy(&inputError, error.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (inputError) return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": " + inputErrorText(inputError)};
    }
    if (entryCount) {
        EM2_TRYC(keysIn.allocate(entryCount * sizeof(uint64_t)));
        EM2_TRYC(keysOut.allocate(entryCount * sizeof(uint64_t)));
        EM2_TRYC(valuesIn.allocate(entryCount * sizeof(float)));
        EM2_TRYC(valuesOut.allocate(entryCount * sizeof(float)));
        EM2_TRYC(temp.allocate(sortTempBytes));
        clusterGatherKernel<<<dim3(blocksOf(listCount, 4u)), dim3(256), 0, stream>>>(
            s.csr.toc.as<uint64_t>(), s.csr.data.as<CountIn>(), geneCount, rows.as<uint32_t>(), positions.as<uint32_t>(),
            entryOffsets.as<uint64_t>(), factor.as<float>(), listCount, keysIn.as<uint64_t>(), valuesIn.as<float>());
        EM2_TRYC(hipGetLastError());
        // the keys' live low bits only (begin_bit 0; the upper bits are zero)
        unsigned endBit = 1u;
        while (endBit < 64u && (accumulatorCount >> endBit) != 0u) ++endBit;
        EM2_TRYC(sortPairs(temp.p, sortTempBytes, keysIn.as<uint64_t>(), keysOut.as<uint64_t>(), valuesIn.as<float>(), valuesOut.as<float>(),
                           size_t(entryCount), 0u, endBit, stream));
        clusterRunKernel<<<dim3(blocksOf(entryCount, 256u)), dim3(256), 0, stream>>>(keysOut.as<uint64_t>(), entryCount,
                                                                                   s.table.as<unsigned long long>());
        EM2_TRYC(hipGetLastError());
    }
    clusterSumKernel<<<dim3(blocksOf(accumulatorCount, 256u)), dim3(256), 0, stream>>>(
        keysOut.as<uint64_t>(), valuesOut.as<float>(), entryCount, s.table.as<unsigned long long>(), accumulatorCount);
    EM2_TRYC(hipGetLastError());
    clusterNormalizeKernel<<<dim3(clusterCount), dim3(64), 0, stream>>>(s.table.as<double>(), geneCount, inverse.as<double>());
    EM2_TRYC(hipGetLastError());
    EM2_TRYC(hipStreamSynchronize(stream));
    if (hostAverages) EM2_TRYC(hipMemcpy(hostAverages, s.table.p, tableBytes, hipMemcpyDeviceToHost));
    return ok();
}

// similarity[e] = regressionCoefficient(average of edge0[e], average of edge1[e]) over the table averages() or
// setAverages() left on the device.
ClusterStatus ClusterDevice::similarities(const char* who, const uint32_t* edge0, const uint32_t* edge1, uint64_t edgeCount,
                                          double* similarity)
{
    State& s = *state;
    const uint32_t clusterCount = s.clusterCount, geneCount = s.geneCount;
    for (uint64_t e = 0; e < edgeCount; ++e) {
        if (edge0[e] >= clusterCount || edge1[e] >= clusterCount) {
            return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": an edge names a cluster that does not exist"};
        }
    }
    if (edgeCount == 0) return ok();
    DeviceBuffer sx, sxx, sxy, d0, d1;
    EM2_TRYC(sx.allocate(size_t(clusterCount) * sizeof(double)));
    EM2_TRYC(sxx.allocate(size_t(clusterCount) * sizeof(double)));
    EM2_TRYC(sxy.allocate(edgeCount * sizeof(double)));
    EM2_TRYC(d0.allocate(edgeCount * sizeof(uint32_t)));
    EM2_TRYC(d1.allocate(edgeCount * sizeof(uint32_t)));
    EM2_TRYC(hipMemcpy(d0.p, edge0, edgeCount * sizeof(uint32_t), hipMemcpyHostToDevice));
    EM2_TRYC(hipMemcpy(d1.p, edge1, edgeCount * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipStream_t stream = nullptr;
    clusterVertexSumsKernel<<<dim3(clusterCount), dim3(64), 0, stream>>>(s.table.as<double>(), geneCount, sx.as<double>(), sxx.as<double>());
    EM2_TRYC(hipGetLastError());
    const uint32_t blocks = uint32_t(std::min<uint64_t>(edgeCount, 1u << 20));
    clusterEdgeKernel<<<dim3(blocks), dim3(64), 0, stream>>>(s.table.as<double>(), geneCount, d0.as<uint32_t>(), d1.as<uint32_t>(), edgeCount,
                                                           sxy.as<double>());
    EM2_TRYC(hipGetLastError());
    std::vector<double> hostSx(clusterCount), hostSxx(clusterCount), hostSxy(edgeCount);
    EM2_TRYC(hipMemcpy(hostSx.data(), sx.p, size_t(clusterCount) * sizeof(double), hipMemcpyDeviceToHost));
    EM2_TRYC(hipMemcpy(hostSxx.data(), sxx.p, size_t(clusterCount) * sizeof(double), hipMemcpyDeviceToHost));
    EM2_TRYC(hipMemcpy(hostSxy.data(), sxy.p, edgeCount * sizeof(double), hipMemcpyDeviceToHost));
    const double n = double(geneCount);
    for (uint64_t e = 0; e < edgeCount; ++e) {                                              // src/regressionCoefficient.cpp:38-41
        const double x = hostSx[edge0[e]], y = hostSx[edge1[e]], xx = hostSxx[edge0[e]], yy = hostSxx[edge1[e]];
        const double numerator = n * hostSxy[e] - x * y;
        const double denominator = std::sqrt((n * xx - x * x) * (n * yy - y * y));
        similarity[e] = numerator / denominator;
    }
    return ok();
}


// ---- ClusterGraph (src/ClusterGraph.cpp:59-386) ----

namespace {

struct GraphVertex {
    std::vector<uint32_t> cells;        // cell-graph vertex indices, in the reference's order
    bool alive = true;
};

struct GraphEdge {
    uint32_t v0, v1;
    double similarity = 0.;
    bool alive = true;
};

// computeAverageGeneExpression + computeSimilarities (:125-169) over what is alive.  averages (may be null) receives
// [alive vertex in vertex order][gene].
ClusterStatus averagesAndSimilarities(const char* who, ClusterDevice& device, const uint32_t* vertexRows,
                                      const std::vector<GraphVertex>& vertices, std::vector<GraphEdge>& edges,
                                      std::vector<double>* averages, uint32_t geneCount, double* seconds)
{
    std::vector<uint32_t> position(vertices.size(), 0xffffffffu), rows, e0, e1;
    std::vector<uint64_t> offsets(1, 0);
    for (size_t v = 0; v < vertices.size(); ++v) {
        if (!vertices[v].alive) continue;
        position[v] = uint32_t(offsets.size() - 1);
        for (const uint32_t cell : vertices[v].cells) rows.push_back(vertexRows ? vertexRows[cell] : cell);
        offsets.push_back(rows.size());
    }
    const uint32_t clusterCount = uint32_t(offsets.size() - 1);
    if (averages) averages->assign(size_t(clusterCount) * geneCount, 0.);
    auto t0 = std::chrono::steady_clock::now();
    ClusterStatus status = device.averages(who, rows.data(), offsets.data(), clusterCount, averages ? averages->data() : nullptr);
    seconds[0] += secondsSince(t0);
    if (status.code != EM2_OK) return status;
    std::vector<size_t> which;
    for (size_t e = 0; e < edges.size(); ++e) {
        if (!edges[e].alive) continue;
        which.push_back(e);
        e0.push_back(position[edges[e].v0]);
        e1.push_back(position[edges[e].v1]);
    }
    std::vector<double> similarity(which.size());
    t0 = std::chrono::steady_clock::now();
    status = device.similarities(who, e0.data(), e1.data(), which.size(), similarity.data());
    seconds[1] += secondsSince(t0);
    if (status.code != EM2_OK) return status;
    for (size_t i = 0; i < which.size(); ++i) edges[which[i]].similarity = similarity[i];
    return status;
}

}  // namespace

ClusterStatus createClusterGraph(const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount,
                                 const uint32_t* vertexRows, uint32_t vertexCount, const uint32_t* edgeVertex0,
                                 const uint32_t* edgeVertex1, uint64_t edgeCount, const uint32_t* labels, uint64_t minClusterSize,
                                 uint64_t k, double similarityThreshold, double similarityThresholdForMerge, ClusterGraphResult& out)
{
    const char* who = "em2_cluster_graph_create";
    const auto tStart = std::chrono::steady_clock::now();
    double deviceSeconds[2] = {0., 0.};
    for (uint64_t e = 0; e < edgeCount; ++e) {
        if (edgeVertex0[e] >= vertexCount || edgeVertex1[e] >= vertexCount) {
            return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": an edge names a vertex that does not exist"};
        }
    }
    if (vertexRows) {
        for (uint32_t v = 0; v < vertexCount; ++v) {
            if (vertexRows[v] >= rowCount) return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a vertex names a row that does not exist"};
        }
    } else if (vertexCount > rowCount) {
        return ClusterStatus{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": more vertices than rows"};
    }
    ClusterDevice device;
    ClusterStatus status = device.upload(who, toc, data, rowCount, geneCount);
    if (status.code != EM2_OK) return status;

    // the constructor (:61-120): a vertex per label at its first occurrence, an edge per unordered pair of distinct clusters
    std::vector<GraphVertex> vertices;
    std::vector<uint32_t> vertexLabel;
    std::unordered_map<uint32_t, uint32_t> vertexOfLabel;
    std::vector<uint32_t> clusterVertexOf(vertexCount);
    for (uint32_t v = 0; v < vertexCount; ++v) {
        const auto it = vertexOfLabel.find(labels[v]);
        uint32_t at;
        if (it == vertexOfLabel.end()) {
            at = uint32_t(vertices.size());
            vertexOfLabel.emplace(labels[v], at);
            vertices.emplace_back();
            vertexLabel.push_back(labels[v]);
        } else {
            at = it->second;
        }
        vertices[at].cells.push_back(v);
        clusterVertexOf[v] = at;
    }
    std::vector<GraphEdge> edges;
    std::unordered_set<uint64_t> known;
    for (uint64_t e = 0; e < edgeCount; ++e) {
        const uint32_t v0 = clusterVertexOf[edgeVertex0[e]], v1 = clusterVertexOf[edgeVertex1[e]];
        if (v0 == v1) continue;
        const uint64_t key = (uint64_t(std::min(v0, v1)) << 32) | std::max(v0, v1);
        if (!known.insert(key).second) continue;
        GraphEdge edge;
        edge.v0 = v0;
        edge.v1 = v1;
        edges.push_back(edge);
    }
    known.clear();

    // mergeVertices (:174-270)
    status = averagesAndSimilarities(who, device, vertexRows, vertices, edges, nullptr, geneCount, deviceSeconds);
    if (status.code != EM2_OK) return status;
    {
        std::vector<uint32_t> parent(vertices.size());
        std::iota(parent.begin(), parent.end(), 0u);
        const auto find = [&parent](uint32_t v) {
            while (parent[v] != v) {
                parent[v] = parent[parent[v]];
                v = parent[v];
            }
            return v;
        };
        for (const GraphEdge& e : edges) {
            if (!(e.similarity > similarityThresholdForMerge)) continue;                    // IsHighSimilarityEdge
            const uint32_t a = find(e.v0), b = find(e.v1);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);                            // the root is the first vertex in vertex order
        }
        for (uint32_t v = 0; v < vertices.size(); ++v) {
            const uint32_t first = find(v);
            if (first == v) continue;
            vertices[first].cells.insert(vertices[first].cells.end(), vertices[v].cells.begin(), vertices[v].cells.end());
            vertices[v].cells.clear();
            vertices[v].alive = false;
        }
        for (GraphEdge& e : edges) {
            if (!vertices[e.v0].alive || !vertices[e.v1].alive) e.alive = false;            // not transferred to the survivor
        }
    }

    // removeSmallVertices (:304-319)
    out.unclusteredCells.clear();
    for (size_t v = 0; v < vertices.size(); ++v) {
        if (!vertices[v].alive || vertices[v].cells.size() >= minClusterSize) continue;
        out.unclusteredCells.insert(out.unclusteredCells.end(), vertices[v].cells.begin(), vertices[v].cells.end());
        vertices[v].alive = false;
    }
    for (GraphEdge& e : edges) {
        if (!vertices[e.v0].alive || !vertices[e.v1].alive) e.alive = false;
    }

    // :2165-2171, then removeWeakEdges (:324-336)
    status = averagesAndSimilarities(who, device, vertexRows, vertices, edges, &out.averages, geneCount, deviceSeconds);
    if (status.code != EM2_OK) return status;
    for (GraphEdge& e : edges) {
        if (e.alive && e.similarity < similarityThreshold) e.alive = false;
    }
    for (const GraphEdge& e : edges) {
        if (e.alive && std::isnan(e.similarity)) {
            return ClusterStatus{EM2_ERROR_RUNTIME, std::string(who) + ": the similarity of two clusters is NaN (a cluster without variance or with "
                                                        "an all-zero average expression): the reference's makeKnn sort is undefined then"};
        }
    }

    // makeKnn (:342-386); equal similarities: the edge created later ranks higher
    {
        std::vector<std::vector<uint32_t>> edgesOf(vertices.size());
        for (uint32_t e = 0; e < edges.size(); ++e) {
            if (!edges[e].alive) continue;
            edgesOf[edges[e].v0].push_back(e);
            edgesOf[edges[e].v1].push_back(e);
        }
        std::vector<char> keep(edges.size(), 0);
        for (std::vector<uint32_t>& mine : edgesOf) {
            std::sort(mine.begin(), mine.end(), [&edges](uint32_t a, uint32_t b) {
                if (edges[a].similarity != edges[b].similarity) return edges[a].similarity > edges[b].similarity;
                return a > b;
            });
            for (size_t i = 0; i < mine.size() && i < k; ++i) keep[mine[i]] = 1;
        }
        for (uint32_t e = 0; e < edges.size(); ++e) {
            if (!keep[e]) edges[e].alive = false;
        }
    }

    // renumberClusters (:276-299): std::sort itself, on the reference's sequence, with its comparator
    std::vector<std::pair<uint64_t, uint32_t>> vertexTable;
    for (size_t v = 0; v < vertices.size(); ++v) {
        if (vertices[v].alive) vertexTable.push_back(std::make_pair(uint64_t(v), uint32_t(vertices[v].cells.size())));
    }
    std::sort(vertexTable.begin(), vertexTable.end(),
              [](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) { return x.second > y.second; });
    std::vector<uint32_t> finalId(vertices.size(), 0xffffffffu);
    for (uint32_t id = 0; id < vertexTable.size(); ++id) finalId[vertexTable[id].first] = id;

    out.geneCount = geneCount;
    out.clusterIds.clear();
    out.cells.clear();
    out.cellOffsets.assign(1, 0);
    for (size_t v = 0; v < vertices.size(); ++v) {
        if (!vertices[v].alive) continue;
        out.clusterIds.push_back(finalId[v]);
        out.cells.insert(out.cells.end(), vertices[v].cells.begin(), vertices[v].cells.end());
        out.cellOffsets.push_back(out.cells.size());
    }
    out.edgeCluster0.clear();
    out.edgeCluster1.clear();
    out.edgeSimilarity.clear();
    for (const GraphEdge& e : edges) {
        if (!e.alive) continue;
        out.edgeCluster0.push_back(finalId[e.v0]);
        out.edgeCluster1.push_back(finalId[e.v1]);
        out.edgeSimilarity.push_back(e.similarity);
    }
    out.initialClusterCount = uint32_t(vertices.size());
    out.initialEdgeCount = edges.size();
    out.averagesSeconds = deviceSeconds[0];
    out.similaritiesSeconds = deviceSeconds[1];
    out.totalSeconds = secondsSince(tStart);
    return ok();
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;

extern "C" {

struct em2_cluster_graph {
    em2::ClusterGraphResult result;
};

static int clusterStatus(const em2::ClusterStatus& status) { return status.code == EM2_OK ? EM2_OK : fail(status.code, status.message); }

int em2_cluster_average_expression(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                   const uint32_t* clusterCells, const uint64_t* clusterOffsets, uint32_t clusterCount,
                                   double* averages)
{
    const char* who = "em2_cluster_average_expression";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (clusterCount == 0) return EM2_OK;
    if (!toc || !clusterOffsets || !averages || (clusterOffsets[clusterCount] && !clusterCells)) return failNull(who);
    if (clusterOffsets[0] != 0) return failArgument(who, "clusterOffsets must start at 0");
    if (!haveDevice()) return failNoDevice(who);
    em2::ClusterDevice device;
    int rc = clusterStatus(device.upload(who, toc, reinterpret_cast<const em2::CountIn*>(data), cellCount, geneCount));
    if (rc != EM2_OK) return rc;
    return clusterStatus(device.averages(who, clusterCells, clusterOffsets, clusterCount, averages));
}

int em2_cluster_similarities(const double* averages, uint32_t clusterCount, uint32_t geneCount, const uint32_t* edgeCluster0,
                             const uint32_t* edgeCluster1, uint64_t edgeCount, double* similarity)
{
    const char* who = "em2_cluster_similarities";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (edgeCount == 0) return EM2_OK;
    if (!averages || !edgeCluster0 || !edgeCluster1 || !similarity) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    em2::ClusterDevice device;
    const int rc = clusterStatus(device.setAverages(averages, clusterCount, geneCount));
    if (rc != EM2_OK) return rc;
    return clusterStatus(device.similarities(who, edgeCluster0, edgeCluster1, edgeCount, similarity));
}

int em2_cluster_graph_create(const uint64_t* toc, const em2_count* data, uint32_t rowCount, uint32_t geneCount,
                             const uint32_t* vertexRows, uint32_t vertexCount, const uint32_t* edgeVertex0,
                             const uint32_t* edgeVertex1, uint64_t edgeCount, const uint32_t* labels, uint64_t minClusterSize,
                             uint64_t k, double similarityThreshold, double similarityThresholdForMerge, em2_cluster_graph** graph)
{
    const char* who = "em2_cluster_graph_create";
    if (!graph) return failNull(who);
    *graph = nullptr;
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (!toc || (vertexCount && !labels) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    std::unique_ptr<em2_cluster_graph> g(new em2_cluster_graph);
    const int rc = clusterStatus(em2::createClusterGraph(toc, reinterpret_cast<const em2::CountIn*>(data), rowCount, geneCount, vertexRows,
                                                         vertexCount, edgeVertex0, edgeVertex1, edgeCount, labels, minClusterSize, k,
                                                         similarityThreshold, similarityThresholdForMerge, g->result));
    if (rc != EM2_OK) return rc;
    *graph = g.release();
    return EM2_OK;
}

int em2_cluster_graph_sizes(const em2_cluster_graph* graph, uint32_t* clusterCount, uint32_t* geneCount, uint64_t* clusteredCellCount,
                            uint64_t* unclusteredCellCount, uint64_t* edgeCount)
{
    if (!graph) return failNull("em2_cluster_graph_sizes");
    const em2::ClusterGraphResult& r = graph->result;
    if (clusterCount) *clusterCount = uint32_t(r.clusterIds.size());
    if (geneCount) *geneCount = r.geneCount;
    if (clusteredCellCount) *clusteredCellCount = r.cells.size();
    if (unclusteredCellCount) *unclusteredCellCount = r.unclusteredCells.size();
    if (edgeCount) *edgeCount = r.edgeSimilarity.size();
    return EM2_OK;
}

int em2_cluster_graph_get(const em2_cluster_graph* graph, uint32_t* clusterIds, uint64_t* cellOffsets, uint32_t* cells,
                          uint32_t* unclusteredCells, double* averages, uint32_t* edgeCluster0, uint32_t* edgeCluster1,
                          double* edgeSimilarity)
{
    if (!graph) return failNull("em2_cluster_graph_get");
    const em2::ClusterGraphResult& r = graph->result;
    if (clusterIds) std::copy(r.clusterIds.begin(), r.clusterIds.end(), clusterIds);
    if (cellOffsets) std::copy(r.cellOffsets.begin(), r.cellOffsets.end(), cellOffsets);
    if (cells) std::copy(r.cells.begin(), r.cells.end(), cells);
    if (unclusteredCells) std::copy(r.unclusteredCells.begin(), r.unclusteredCells.end(), unclusteredCells);
    if (averages) std::copy(r.averages.begin(), r.averages.end(), averages);
    if (edgeCluster0) std::copy(r.edgeCluster0.begin(), r.edgeCluster0.end(), edgeCluster0);
    if (edgeCluster1) std::copy(r.edgeCluster1.begin(), r.edgeCluster1.end(), edgeCluster1);
    if (edgeSimilarity) std::copy(r.edgeSimilarity.begin(), r.edgeSimilarity.end(), edgeSimilarity);
    return EM2_OK;
}

int em2_cluster_graph_facts(const em2_cluster_graph* graph, double* values, uint32_t valueCount)
{
    if (!graph || (valueCount && !values)) return failNull("em2_cluster_graph_facts");
    const em2::ClusterGraphResult& r = graph->result;
    const double facts[5] = {r.totalSeconds, r.averagesSeconds, r.similaritiesSeconds, double(r.initialClusterCount),
                             double(r.initialEdgeCount)};
    for (uint32_t i = 0; i < valueCount; ++i) values[i] = i < 5u ? facts[i] : 0.;
    return EM2_OK;
}

void em2_cluster_graph_free(em2_cluster_graph* graph) { delete graph; }

}  // extern "C"
