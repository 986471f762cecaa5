// em2_layout.hip -- the layout of a graph in the plane: Hu's spring-electrical model (the one Graphviz's sfdp minimises, which
// the reference shells out to at src/CellGraph.cpp:210-264), single level, exact N-body repulsion.
//
// The result is a function of the input alone, bit for bit: every floating-point operation below is written out (fmaf where a
// product is fused, separate operations elsewhere: the library is built with -ffp-contract=off; division and sqrtf are the
// correctly rounded ones), and every sum has a shape that depends on the vertex count N only.
//   * checkEdgesKernel     every edge end is below N -- nothing indexes with one before this has passed;
//   * the adjacency        as the gene graph builds it (em2_adjacency.h): two directed records per edge, a radix sort, a
//                          search for the offsets.  Per vertex the neighbours ascend; a repeated edge is there twice;
//   * initialKernel        the start positions: a hash of (seed, vertex), uniform on a square of side sqrt(N) about the origin;
//   * repulsionKernel      the hot path.  The j range is cut into kLayoutSliceCount slices of ceil(N / 16) consecutive
//                          vertices; a lane owns one vertex i and one slice and adds its terms in ascending j; a wave's 64 lanes
//                          are 64 vertices i against the same j, read from LDS as a broadcast.  One partial per (slice, vertex);
//   * forceKernel          per vertex: the slice partials in ascending slice order, the attraction in ascending neighbour order,
//                          gravity, |f|^2 in double; the move by step * f / |f| into the other position buffer; the energy of
//                          256 consecutive vertices by a fixed tree in LDS;
//   * energyStepKernel     one workgroup: the chunk energies by a fixed tree, then one thread updates the step (Hu's adaptive
//                          scheme) in device memory.  The host reads the new step, one double per iteration, to decide the end.

#include "em2_adjacency.h"
#include "em2_entry.h"
#include "em2_scratch.h"

#include <cmath>
#include <cstring>            // (rocPRIM calls memset without including it)
#include <limits>
#include <rocprim/rocprim.hpp>
#include <string>

// What the device code and the C entry points at the end of this file share.
namespace em2 {

// The constants of the model (Hu 2005) and of the summation shapes.  The shapes are part of the contract: they are functions
// of the vertex count alone, never of the device or the grid.
constexpr float kLayoutC = 0.2f;                    // C * K^2, with the natural length K = 1
constexpr float kLayoutFloor = 1e-30f;              // delta: d^2 is raised to it, so j = i and coincident vertices add an exact 0
constexpr double kLayoutT = 0.9;                    // the step is multiplied by t when the energy did not fall
constexpr uint32_t kLayoutProgress = 5;             // ... and divided by t after this many falls in a row
constexpr uint32_t kLayoutSliceCount = 16;          // slices of the j range of a repulsion sum: ceil(N / 16) consecutive vertices each
constexpr uint32_t kLayoutTile = 128;               // j positions staged in LDS at a time (no effect on any sum)
constexpr uint32_t kLayoutBlockVertices = 256;      // vertices of a workgroup, and the leaves of one chunk of the energy tree
constexpr uint32_t kLayoutMaxVertexCount = 1u << 30;

struct LayoutParameters {
    uint32_t seed;
    uint32_t maxIterationCount;
    double tolerance;
    double gravity;
    double initialStep;
};

struct LayoutResult {
    uint32_t iterationCount = 0;
    double step = 0.;
    double energy = 0.;
};

// Bit of *inputError (nothing was computed where it is not 0).
constexpr uint32_t kLayoutEdgeRange = 1u;           // an edge end >= vertexCount

// The layout of the graph of vertexCount > 0 vertices and the edges (d_edge0[e], d_edge1[e]) in device memory: initial
// positions from (seed, vertex), then Hu's adaptive iteration until maxIterationCount or step < tolerance.  d_x / d_y
// [vertexCount] in device memory receive the positions.  Every edge end is checked before anything indexes with it.
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
static hipError_t runGraphLayout(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                                 const LayoutParameters& parameters, float* d_x, float* d_y, LayoutResult& result, uint32_t* inputError,
                                 hipStream_t stream);

// One evaluation of the forces at the positions d_x / d_y, no move: d_fx / d_fy [vertexCount], *energy = the sum of |f|^2.
static hipError_t runGraphLayoutForces(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, double gravity,
                                       const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy, uint32_t* inputError,
                                       hipStream_t stream);

namespace {

struct LayoutState {
    double step;
    double energy;
    uint32_t progress;
    uint32_t unused;
};

__global__ void __launch_bounds__(256)
checkEdgesKernel(const uint32_t* __restrict__ edge0, const uint32_t* __restrict__ edge1, uint64_t edgeCount, uint32_t vertexCount,
                 uint32_t* __restrict__ error)
{
    uint32_t bad = 0u;
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        if (edge0[e] >= vertexCount || edge1[e] >= vertexCount) bad = kLayoutEdgeRange;
    }
    if (bad) atomicOr(error, bad);
}

__global__ void __launch_bounds__(256)
layoutRecordsKernel(const uint32_t* __restrict__ edge0, const uint32_t* __restrict__ edge1, uint64_t edgeCount, uint64_t* __restrict__ keys)
{
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t v0 = edge0[e], v1 = edge1[e];
        keys[2u * e] = v0 << 32 | v1;
        keys[2u * e + 1u] = v1 << 32 | v0;
    }
}

// offsets[v] = where the records of vertex v begin, v in [0, vertexCount]; neighbours[i] = the low half of the i-th sorted key.
__global__ void __launch_bounds__(256)
layoutOffsetsKernel(const uint64_t* __restrict__ keys, uint64_t recordCount, uint32_t vertexCount, uint64_t* __restrict__ offsets,
                    uint32_t* __restrict__ neighbours)
{
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t v = first; v <= vertexCount; v += stride) offsets[v] = lowerBound(keys, recordCount, v << 32);
    for (uint64_t i = first; i < recordCount; i += stride) neighbours[i] = uint32_t(keys[i]);
}

// A counter-based hash (the finaliser of splitmix64) of seed << 32 | vertex: 24 bits per coordinate, u in [-0.5, 0.5) exactly,
// times the side of the square.
__global__ void __launch_bounds__(256)
initialKernel(uint32_t seed, uint32_t vertexCount, float side, float2* __restrict__ position)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        uint64_t z = (uint64_t(seed) << 32 | i) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const float ux = float(uint32_t(z >> 40)) * 0x1p-24f - 0.5f;
        const float uy = float(uint32_t(z >> 16) & 0xffffffu) * 0x1p-24f - 0.5f;
        position[i] = make_float2(ux * side, uy * side);
    }
}

__global__ void __launch_bounds__(256)
packKernel(const float* __restrict__ x, const float* __restrict__ y, uint32_t vertexCount, float2* __restrict__ position)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        position[i] = make_float2(x[i], y[i]);
    }
}

__global__ void __launch_bounds__(256)
unpackKernel(const float2* __restrict__ position, uint32_t vertexCount, float* __restrict__ x, float* __restrict__ y)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const float2 p = position[i];
        x[i] = p.x;
        y[i] = p.y;
    }
}

// One pair: (fx, fy) += (p_i - p_j) * C / max(d^2, delta).  dy * dy is a product of its own, the rest are fmaf.
__device__ __forceinline__ void repel(float xi, float yi, float2 pj, float& fx, float& fy)
{
    const float dx = xi - pj.x, dy = yi - pj.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    const float w = kLayoutC / fmaxf(d2, kLayoutFloor);
    fx = fmaf(dx, w, fx);
    fy = fmaf(dy, w, fy);
}

// Workgroup (b, s): the vertices [256 b, 256 b + 256) against slice s of the j range, [s L, min(N, s L + L)).  The slice goes
// through LDS in tiles of kLayoutTile positions; every lane of a wave reads the same tile entry (a broadcast, no conflict).
// partial[s N + i] = the slice's sum for vertex i, terms added in ascending j from 0.  An empty slice writes zeros.
__global__ void __launch_bounds__(kLayoutBlockVertices)
repulsionKernel(const float2* __restrict__ position, uint32_t vertexCount, uint32_t sliceLength, float2* __restrict__ partial)
{
    __shared__ float2 tile[kLayoutTile];
    const uint32_t i = blockIdx.x * kLayoutBlockVertices + threadIdx.x;
    const uint32_t slice = blockIdx.y;
    const uint64_t sliceBegin = uint64_t(slice) * sliceLength;
    const uint32_t begin = sliceBegin < vertexCount ? uint32_t(sliceBegin) : vertexCount;
    const uint32_t end = vertexCount - begin < sliceLength ? vertexCount : begin + sliceLength;
    const float2 pi = i < vertexCount ? position[i] : make_float2(0.f, 0.f);
    float fx = 0.f, fy = 0.f;
    for (uint32_t t = begin; t < end; t += kLayoutTile) {
        const uint32_t count = end - t < kLayoutTile ? end - t : kLayoutTile;
        __syncthreads();                                        // (everybody has finished with the tile before)
        if (threadIdx.x < count) tile[threadIdx.x] = position[t + threadIdx.x];
        __syncthreads();
        if (count == kLayoutTile) {
#pragma unroll 8
            for (uint32_t j = 0; j < kLayoutTile; j++) repel(pi.x, pi.y, tile[j], fx, fy);
        } else {
            for (uint32_t j = 0; j < count; j++) repel(pi.x, pi.y, tile[j], fx, fy);
        }
    }
    if (i < vertexCount) partial[uint64_t(slice) * vertexCount + i] = make_float2(fx, fy);
}

// The sum of the 256 doubles the workgroup's threads hold: v[t] += v[t + stride] for stride = 128, 64, ... 1.  In thread 0.
__device__ __forceinline__ double blockTree(double value, double* shared)
{
    shared[threadIdx.x] = value;
    __syncthreads();
#pragma unroll
    for (uint32_t stride = kLayoutBlockVertices / 2u; stride >= 1u; stride /= 2u) {
        if (threadIdx.x < stride) shared[threadIdx.x] += shared[threadIdx.x + stride];
        __syncthreads();
    }
    return shared[0];
}

// Vertex i = one thread; the grid is exactly ceil(N / 256) workgroups (the chunks of the energy tree).
//   f = ((p_0 + p_1) + ... + p_15)  -  sum over the neighbours j ascending of (p_i - p_j) * d  -  g * p_i
// with d = sqrtf(fmaf(dx, dx, dy * dy)) and each attraction term an fmaf into the running sum; f = fmaf(-g, p_i, repulsion -
// attraction).  The move (nextPosition != NULL): p_i + f * (float(step) / |f|), |f| = sqrtf(fmaf(fx, fx, fy * fy)), nothing
// where |f| = 0.  chunkEnergy[block] = the tree sum of double(fx) * double(fx) + double(fy) * double(fy), 0 for the threads
// past N.
__global__ void __launch_bounds__(kLayoutBlockVertices)
forceKernel(const float2* __restrict__ position, uint32_t vertexCount, const float2* __restrict__ partial,
            const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ neighbours, float gravity,
            const LayoutState* __restrict__ state, float2* __restrict__ nextPosition, float2* __restrict__ force,
            double* __restrict__ chunkEnergy)
{
    __shared__ double shared[kLayoutBlockVertices];
    const uint32_t i = blockIdx.x * kLayoutBlockVertices + threadIdx.x;
    double energy = 0.;
    if (i < vertexCount) {
        const float2 pi = position[i];
        float2 sum = partial[i];
        float rx = sum.x, ry = sum.y;
        for (uint32_t s = 1; s < kLayoutSliceCount; s++) {
            sum = partial[uint64_t(s) * vertexCount + i];
            rx += sum.x;
            ry += sum.y;
        }
        float ax = 0.f, ay = 0.f;
        const uint64_t last = offsets[i + 1u];
        for (uint64_t k = offsets[i]; k < last; k++) {
            const float2 pj = position[neighbours[k]];
            const float dx = pi.x - pj.x, dy = pi.y - pj.y;
            const float d = sqrtf(fmaf(dx, dx, dy * dy));
            ax = fmaf(dx, d, ax);
            ay = fmaf(dy, d, ay);
        }
        float fx = rx - ax, fy = ry - ay;
        fx = fmaf(-gravity, pi.x, fx);
        fy = fmaf(-gravity, pi.y, fy);
        energy = double(fx) * double(fx) + double(fy) * double(fy);
        if (force) force[i] = make_float2(fx, fy);
        if (nextPosition) {
            const float m = sqrtf(fmaf(fx, fx, fy * fy));
            float2 next = pi;
            if (m > 0.f) {
                const float scale = float(state->step) / m;
                next.x = fmaf(fx, scale, pi.x);
                next.y = fmaf(fy, scale, pi.y);
            }
            nextPosition[i] = next;
        }
    }
    const double total = blockTree(energy, shared);
    if (threadIdx.x == 0) chunkEnergy[blockIdx.x] = total;
}

// One workgroup.  Thread t adds chunkEnergy[t], [t + 256], ... in that order from 0; the 256 sums go through the tree.  Then
// Hu's step control in thread 0: the step is multiplied by t where the energy did not fall, divided by t after five falls in a
// row.  (updateStep false: only the energy is stored, for the forces entry.)
__global__ void __launch_bounds__(kLayoutBlockVertices)
energyStepKernel(const double* __restrict__ chunkEnergy, uint32_t chunkCount, bool updateStep, LayoutState* __restrict__ state)
{
    __shared__ double shared[kLayoutBlockVertices];
    double sum = 0.;
    for (uint32_t c = threadIdx.x; c < chunkCount; c += kLayoutBlockVertices) sum += chunkEnergy[c];
    const double energy = blockTree(sum, shared);
    if (threadIdx.x != 0) return;
    const double energy0 = state->energy;
    state->energy = energy;
    if (!updateStep) return;
    if (energy < energy0) {
        if (++state->progress >= kLayoutProgress) {
            state->progress = 0u;
            state->step /= kLayoutT;
        }
    } else {
        state->progress = 0u;
        state->step *= kLayoutT;
    }
}

// What a run and the forces entry share: the edge check, the adjacency, the buffers.
struct LayoutWork {
    CachedBuffer arena, recordArena;
    uint32_t vertexCount = 0, chunkCount = 0, sliceLength = 0;
    float2* position[2] = {nullptr, nullptr};
    float2* partial = nullptr;
    float2* force = nullptr;
    double* chunkEnergy = nullptr;
    uint64_t* offsets = nullptr;
    uint32_t* neighbours = nullptr;
    LayoutState* state = nullptr;

    void idle() { arena.idle = recordArena.idle = true; }

    hipError_t prepare(uint32_t n, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, uint32_t* inputError,
                       hipStream_t stream)
    {
        *inputError = 0;
        vertexCount = n;
        chunkCount = blocksOf(n, kLayoutBlockVertices);
        sliceLength = blocksOf(n, kLayoutSliceCount);
        const dim3 threads(256);
        const uint64_t recordCount = 2u * edgeCount;
        size_t at = 0;
        const auto take = [&at](size_t bytes) {
            const size_t here = at;
            at += alignUp(bytes ? bytes : 1u);
            return here;
        };
        const size_t offError = take(256);
        const size_t offState = take(sizeof(LayoutState));
        const size_t offPosition0 = take(size_t(n) * sizeof(float2));
        const size_t offPosition1 = take(size_t(n) * sizeof(float2));
        const size_t offForce = take(size_t(n) * sizeof(float2));
        const size_t offPartial = take(size_t(n) * kLayoutSliceCount * sizeof(float2));
        const size_t offChunk = take(size_t(chunkCount) * sizeof(double));
        const size_t offOffsets = take((size_t(n) + 1u) * sizeof(uint64_t));
        const size_t offNeighbours = take(size_t(recordCount) * sizeof(uint32_t));
        EM2_TRY(arena.allocate(at));
        char* base = arena.as<char>();
        uint32_t* error = reinterpret_cast<uint32_t*>(base + offError);
        state = reinterpret_cast<LayoutState*>(base + offState);
        position[0] = reinterpret_cast<float2*>(base + offPosition0);
        position[1] = reinterpret_cast<float2*>(base + offPosition1);
        force = reinterpret_cast<float2*>(base + offForce);
        partial = reinterpret_cast<float2*>(base + offPartial);
        chunkEnergy = reinterpret_cast<double*>(base + offChunk);
        offsets = reinterpret_cast<uint64_t*>(base + offOffsets);
        neighbours = reinterpret_cast<uint32_t*>(base + offNeighbours);

        EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
        checkEdgesKernel<<<dim3(gridFor(edgeCount)), threads, 0, stream>>>(d_edge0, d_edge1, edgeCount, n, error);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (*inputError) return hipSuccess;

        // the adjacency: 2 E directed records in (vertex, neighbour) order.  Equal keys (a repeated edge, a self-loop) are
        // equal records, so the sorted array is a function of the input alone.
        const uint64_t* sortedKeys = nullptr;
        if (recordCount) {
            at = 0;
            const size_t offKeysA = take(recordCount * sizeof(uint64_t));
            const size_t offKeysB = take(recordCount * sizeof(uint64_t));
            size_t sortBytes = 0;
            {
                rocprim::double_buffer<uint64_t> keys(nullptr, nullptr);
                EM2_TRY(rocprim::radix_sort_keys(nullptr, sortBytes, keys, size_t(recordCount), 0u, 64u, stream));
            }
            const size_t offSortTemp = take(sortBytes);
            EM2_TRY(recordArena.allocate(at));
            char* recordBase = recordArena.as<char>();
            rocprim::double_buffer<uint64_t> keys(reinterpret_cast<uint64_t*>(recordBase + offKeysA),
                                                  reinterpret_cast<uint64_t*>(recordBase + offKeysB));
            layoutRecordsKernel<<<dim3(gridFor(edgeCount)), threads, 0, stream>>>(d_edge0, d_edge1, edgeCount, keys.current());
            EM2_TRY(hipGetLastError());
            EM2_TRY(rocprim::radix_sort_keys(recordBase + offSortTemp, sortBytes, keys, size_t(recordCount), 0u, 64u, stream));
            sortedKeys = keys.current();
        }
        // (with no record the searches find nothing and read nothing: every offset 0)
        layoutOffsetsKernel<<<dim3(gridFor(recordCount > n ? recordCount : uint64_t(n) + 1u)), threads, 0, stream>>>(
            sortedKeys, recordCount, n, offsets, neighbours);
        EM2_TRY(hipGetLastError());
        return hipSuccess;
    }

    // One evaluation at position[from]; the move goes to position[1 - from] where `move` is set, f to `force` where wanted.
    hipError_t evaluate(uint32_t from, float gravity, bool move, bool keepForce, hipStream_t stream)
    {
        const dim3 threads(kLayoutBlockVertices);
        repulsionKernel<<<dim3(chunkCount, kLayoutSliceCount), threads, 0, stream>>>(position[from], vertexCount, sliceLength, partial);
        EM2_TRY(hipGetLastError());
        forceKernel<<<dim3(chunkCount), threads, 0, stream>>>(position[from], vertexCount, partial, offsets, neighbours, gravity, state,
                                                             move ? position[1u - from] : nullptr, keepForce ? force : nullptr,
                                                             chunkEnergy);
        EM2_TRY(hipGetLastError());
        energyStepKernel<<<dim3(1), threads, 0, stream>>>(chunkEnergy, chunkCount, move, state);
        return hipGetLastError();
    }
};

}  // namespace

hipError_t runGraphLayout(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                          const LayoutParameters& parameters, float* d_x, float* d_y, LayoutResult& result, uint32_t* inputError,
                          hipStream_t stream)
{
    StageTimer timer("graphLayout");
    LayoutWork work;
    EM2_TRY(work.prepare(vertexCount, d_edge0, d_edge1, edgeCount, inputError, stream));
    if (*inputError) {
        work.idle();
        return hipSuccess;
    }
    EM2_TRY(timer.stage("check and adjacency", stream));

    LayoutState host;
    host.step = parameters.initialStep;
    host.energy = std::numeric_limits<double>::infinity();
    host.progress = host.unused = 0u;
    EM2_TRY(hipMemcpyAsync(work.state, &host, sizeof(host), hipMemcpyHostToDevice, stream));
    initialKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(parameters.seed, vertexCount, sqrtf(float(vertexCount)),
                                                                       work.position[0]);
    EM2_TRY(hipGetLastError());

    // The positions stay on the device; the new step, one double, comes back after every iteration.
    const float gravity = float(parameters.gravity);
    double step = parameters.initialStep;
    uint32_t iterations = 0, from = 0;
    while (iterations < parameters.maxIterationCount && !(step < parameters.tolerance)) {
        EM2_TRY(work.evaluate(from, gravity, true, false, stream));
        EM2_TRY(hipMemcpyAsync(&step, &work.state->step, sizeof(double), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        from = 1u - from;
        iterations++;
    }
    EM2_TRY(timer.stage("iterations", stream));

    unpackKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(work.position[from], vertexCount, d_x, d_y);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(&host, work.state, sizeof(host), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    result.iterationCount = iterations;
    result.step = host.step;
    result.energy = host.energy;
    work.idle();                                                // (everything that used the blocks has been waited for)
    return hipSuccess;
}

hipError_t runGraphLayoutForces(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, double gravity,
                                const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy, uint32_t* inputError,
                                hipStream_t stream)
{
    LayoutWork work;
    EM2_TRY(work.prepare(vertexCount, d_edge0, d_edge1, edgeCount, inputError, stream));
    if (*inputError) {
        work.idle();
        return hipSuccess;
    }
    LayoutState host;
    host.step = 0.;
    host.energy = std::numeric_limits<double>::infinity();
    host.progress = host.unused = 0u;
    EM2_TRY(hipMemcpyAsync(work.state, &host, sizeof(host), hipMemcpyHostToDevice, stream));
    packKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(d_x, d_y, vertexCount, work.position[0]);
    EM2_TRY(hipGetLastError());
    EM2_TRY(work.evaluate(0u, float(gravity), false, true, stream));
    unpackKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(work.force, vertexCount, d_fx, d_fy);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(&host, work.state, sizeof(host), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    *energy = host.energy;
    work.idle();
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

// The edge arrays of a host-pointer entry in device memory.
static int uploadEdges(const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount, DeviceBuffer& d0, DeviceBuffer& d1)
{
    EM2_HIP(d0.upload(edgeVertex0, size_t(edgeCount)));
    EM2_HIP(d1.upload(edgeVertex1, size_t(edgeCount)));
    return EM2_OK;
}

static int graphLayout(const char* who, bool onDevice, uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                       uint64_t edgeCount, const em2_layout_parameters* parameters, float* x, float* y, em2_layout_result* result)
{
    if (!parameters || (vertexCount && (!x || !y)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(parameters->tolerance >= 0.)) return failArgument(who, "tolerance must not be negative");
    if (!(parameters->gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (!(parameters->initialStep >= 0.)) return failArgument(who, "initialStep must not be negative");
    if (vertexCount > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": vertexCount is above 2^30");
    if (result) {
        result->iterationCount = result->reserved = 0u;
        result->step = parameters->initialStep;
        result->energy = std::numeric_limits<double>::infinity();
    }
    if (vertexCount == 0) {
        // (no vertex, so every edge end is out of range)
        return edgeCount ? failArgument(who, "an edge names a vertex outside the graph") : EM2_OK;
    }
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer d0, d1, dx, dy;
    if (!onDevice) {
        const int status = uploadEdges(edgeVertex0, edgeVertex1, edgeCount, d0, d1);
        if (status != EM2_OK) return status;
        EM2_HIP(dx.allocateFor<float>(vertexCount));
        EM2_HIP(dy.allocateFor<float>(vertexCount));
    }
    const em2::LayoutParameters p = {parameters->seed, parameters->maxIterationCount, parameters->tolerance, parameters->gravity,
                                     parameters->initialStep};
    em2::LayoutResult r;
    uint32_t inputError = 0;
    EM2_HIP(em2::runGraphLayout(vertexCount, onDevice ? edgeVertex0 : d0.as<uint32_t>(), onDevice ? edgeVertex1 : d1.as<uint32_t>(), edgeCount,
                                p, onDevice ? x : dx.as<float>(), onDevice ? y : dy.as<float>(), r, &inputError, nullptr));
    if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
    if (!onDevice) {
        EM2_HIP(dx.download(x, vertexCount));
        EM2_HIP(dy.download(y, vertexCount));
    }
    if (result) {
        result->iterationCount = r.iterationCount;
        result->step = r.step;
        result->energy = r.energy;
    }
    return EM2_OK;
}

int em2_graph_layout(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                     const em2_layout_parameters* parameters, float* x, float* y, em2_layout_result* result)
{
    return graphLayout("em2_graph_layout", false, vertexCount, edgeVertex0, edgeVertex1, edgeCount, parameters, x, y, result);
}

int em2_dev_graph_layout(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                         const em2_layout_parameters* parameters, float* d_x, float* d_y, em2_layout_result* result)
{
    return graphLayout("em2_dev_graph_layout", true, vertexCount, d_edgeVertex0, d_edgeVertex1, edgeCount, parameters, d_x, d_y, result);
}

int em2_graph_layout_forces(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                            double gravity, const float* x, const float* y, float* fx, float* fy, double* energy)
{
    const char* who = "em2_graph_layout_forces";
    if ((vertexCount && (!x || !y || !fx || !fy)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (vertexCount > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": vertexCount is above 2^30");
    if (energy) *energy = 0.;
    if (vertexCount == 0) return edgeCount ? failArgument(who, "an edge names a vertex outside the graph") : EM2_OK;
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer d0, d1, dx, dy, dfx, dfy;
    const int status = uploadEdges(edgeVertex0, edgeVertex1, edgeCount, d0, d1);
    if (status != EM2_OK) return status;
    EM2_HIP(dx.upload(x, vertexCount));
    EM2_HIP(dy.upload(y, vertexCount));
    EM2_HIP(dfx.allocateFor<float>(vertexCount));
    EM2_HIP(dfy.allocateFor<float>(vertexCount));
    uint32_t inputError = 0;
    double e = 0.;
    EM2_HIP(em2::runGraphLayoutForces(vertexCount, d0.as<uint32_t>(), d1.as<uint32_t>(), edgeCount, gravity, dx.as<float>(), dy.as<float>(),
                                      dfx.as<float>(), dfy.as<float>(), &e, &inputError, nullptr));
    if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
    EM2_HIP(dfx.download(fx, vertexCount));
    EM2_HIP(dfy.download(fy, vertexCount));
    if (energy) *energy = e;
    return EM2_OK;
}

}  // extern "C"
