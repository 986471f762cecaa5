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
// The pyramid entries replace repulsionKernel by an approximation of the far field and keep the rest:
//   * boxKernel            the four extremes of the positions, as unsigned maxima of order-preserving bit patterns;
//   * pyramidKeysKernel    per vertex the quantised coordinates q, the leaf, the sort key morton(leaf) << vertexBits | vertex,
//                          and the leaf's count and integer sums of q by atomics (integers: no order);
//   * rocPRIM's radix sort of the keys over the bits in use; pyramidGatherKernel: the positions in sorted order, where each
//                          leaf begins;
//   * pyramidLevelKernel   level by level from the leaves up: a parent is the sum of its four children; the centroid and
//                          float(count) of every cell as one 16-byte record;
//   * pyramidWalkKernel    the hot path: a lane per vertex in sorted order, the far cells of the levels 2 ... D in the stated
//                          order, then the vertices of the nine leaves around its own; far + near goes to the vertex's slot.

#include "em2_adjacency.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_scratch.h"

#include <cmath>
#include <limits>
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
// The pyramid.  The leaf target decides the automatic depth and is part of the contract.
constexpr uint32_t kLayoutLeafTarget = EM2_LAYOUT_LEAF_TARGET;
constexpr uint32_t kLayoutMaxDepth = EM2_LAYOUT_MAX_DEPTH;
constexpr uint32_t kLayoutDepthAuto = EM2_LAYOUT_DEPTH_AUTO;
constexpr uint32_t kLayoutDepthExact = 0xfffffffeu;  // (internal) no pyramid: the exact repulsion
constexpr uint32_t kLayoutBoxBlocks = 512;           // workgroups of the box kernel (no effect on any result: minima and maxima)

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
// depth: kLayoutDepthExact for the exact repulsion, else kLayoutDepthAuto or the depth of the pyramid (<= kLayoutMaxDepth).
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
static hipError_t runGraphLayout(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                                 const LayoutParameters& parameters, uint32_t depth, float* d_x, float* d_y, LayoutResult& result,
                                 uint32_t* inputError, hipStream_t stream);

// One evaluation of the forces at the positions d_x / d_y, no move: d_fx / d_fy [vertexCount], *energy = the sum of |f|^2.
static hipError_t runGraphLayoutForces(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, double gravity,
                                       uint32_t depth, const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy,
                                       uint32_t* inputError, hipStream_t stream);

// The depth of the pyramid for vertexCount vertices: the smallest D with kLayoutLeafTarget * 4^D >= vertexCount, at most
// kLayoutMaxDepth.
static inline uint32_t layoutAutomaticDepth(uint32_t vertexCount)
{
    uint32_t depth = 0;
    while (depth < kLayoutMaxDepth && (uint64_t(kLayoutLeafTarget) << (2u * depth)) < vertexCount) depth++;
    return depth;
}

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
// past N.  (kSliceCount: 16 for the exact repulsion; 1 for the pyramid, whose walk leaves one sum per vertex.)
template <uint32_t kSliceCount>
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
        for (uint32_t s = 1; s < kSliceCount; s++) {
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

// ---- the pyramid ----
// Level l has 2^l x 2^l cells, stored row-major (by << l | bx) from cell (4^l - 1) / 3 of one array over all levels.  Every
// index below is formed from a quantised coordinate q <= 2^31 or from a key made of such indices, never from a position.

struct LayoutMoment {
    unsigned long long sumX, sumY;                  // the sums of q over the cell's vertices: at most 2^30 * 2^31
    uint32_t count;
    uint32_t unused;
};

__host__ __device__ __forceinline__ uint32_t layoutLevelBegin(uint32_t level) { return ((1u << (2u * level)) - 1u) / 3u; }

// float <-> a uint32 of the same order (no NaN comes here).
__device__ __forceinline__ uint32_t orderedBits(float v)
{
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float fromOrderedBits(uint32_t e) { return __uint_as_float(e ^ ((e >> 31) ? 0x80000000u : 0xffffffffu)); }

// The bits 0 ... 15 of v at the even positions / back.
__device__ __forceinline__ uint32_t spreadBits(uint32_t v)
{
    v &= 0xffffu;
    v = (v | v << 8) & 0x00ff00ffu;
    v = (v | v << 4) & 0x0f0f0f0fu;
    v = (v | v << 2) & 0x33333333u;
    return (v | v << 1) & 0x55555555u;
}

__device__ __forceinline__ uint32_t gatherBits(uint32_t v)
{
    v &= 0x55555555u;
    v = (v | v >> 1) & 0x33333333u;
    v = (v | v >> 2) & 0x0f0f0f0fu;
    v = (v | v >> 4) & 0x00ff00ffu;
    return (v | v >> 8) & 0x0000ffffu;
}

// box[0 ... 3] = ~ordered(xmin), ordered(xmax), ~ordered(ymin), ordered(ymax): four unsigned maxima from 0, so one memset
// prepares them and the order of the atomics is of no account.  fminf / fmaxf pass a NaN over.
__global__ void __launch_bounds__(256)
boxKernel(const float2* __restrict__ position, uint32_t vertexCount, uint32_t* __restrict__ box)
{
    const float inf = std::numeric_limits<float>::infinity();
    float xmin = inf, xmax = -inf, ymin = inf, ymax = -inf;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const float2 p = position[i];
        xmin = fminf(xmin, p.x);
        xmax = fmaxf(xmax, p.x);
        ymin = fminf(ymin, p.y);
        ymax = fmaxf(ymax, p.y);
    }
    for (int offset = 32; offset >= 1; offset /= 2) {
        xmin = fminf(xmin, __shfl_xor(xmin, offset));
        xmax = fmaxf(xmax, __shfl_xor(xmax, offset));
        ymin = fminf(ymin, __shfl_xor(ymin, offset));
        ymax = fmaxf(ymax, __shfl_xor(ymax, offset));
    }
    // the workgroup's four waves through LDS, then four atomics per workgroup: all of them go to the same four words, so the
    // grid is small (kLayoutBoxBlocks) and the vertices are strided over
    __shared__ float4 waveExtremes[4];
    if ((threadIdx.x & 63u) == 0u) waveExtremes[threadIdx.x >> 6] = make_float4(xmin, xmax, ymin, ymax);
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < 4u; w++) {
            xmin = fminf(xmin, waveExtremes[w].x);
            xmax = fmaxf(xmax, waveExtremes[w].y);
            ymin = fminf(ymin, waveExtremes[w].z);
            ymax = fmaxf(ymax, waveExtremes[w].w);
        }
        atomicMax(box + 0, ~orderedBits(xmin));
        atomicMax(box + 1, orderedBits(xmax));
        atomicMax(box + 2, ~orderedBits(ymin));
        atomicMax(box + 3, orderedBits(ymax));
    }
}

struct LayoutBox {
    float xmin, ymin, side;
};

__device__ __forceinline__ LayoutBox readBox(const uint32_t* __restrict__ box)
{
    LayoutBox b;
    b.xmin = fromOrderedBits(~box[0]);
    b.ymin = fromOrderedBits(~box[2]);
    b.side = fmaxf(fromOrderedBits(box[1]) - b.xmin, fromOrderedBits(box[3]) - b.ymin);
    return b;
}

// q = uint32_t(clamp((v - lo) / S, 0, 1) * 2^31) <= 2^31; 0 where S == 0.  A NaN quotient becomes 0 in fmaxf.
__device__ __forceinline__ uint32_t quantise(float v, float lo, float side)
{
    if (side == 0.f) return 0u;
    const float u = fminf(fmaxf((v - lo) / side, 0.f), 1.f);
    return uint32_t(u * 2147483648.f);
}

// Vertex i: keys[i] = morton(leaf) << vertexBits | i, and the leaf's moments.  (moment: the leaf level, zeroed before.)
__global__ void __launch_bounds__(256)
pyramidKeysKernel(const float2* __restrict__ position, uint32_t vertexCount, const uint32_t* __restrict__ box, uint32_t depth,
                  uint32_t vertexBits, uint64_t* __restrict__ keys, LayoutMoment* __restrict__ moment)
{
    const LayoutBox b = readBox(box);
    const uint32_t last = (1u << depth) - 1u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const float2 p = position[i];
        const uint32_t qx = quantise(p.x, b.xmin, b.side), qy = quantise(p.y, b.ymin, b.side);
        const uint32_t cx = min(last, qx >> (31u - depth)), cy = min(last, qy >> (31u - depth));
        keys[i] = uint64_t(spreadBits(cx) | spreadBits(cy) << 1) << vertexBits | i;
        LayoutMoment* leaf = moment + (cy << depth | cx);
        atomicAdd(&leaf->count, 1u);
        atomicAdd(&leaf->sumX, (unsigned long long)qx);
        atomicAdd(&leaf->sumY, (unsigned long long)qy);
    }
}

// Sorted place k: the position of its vertex, and where a leaf begins (leafBegin is written for the leaves that hold a vertex).
__global__ void __launch_bounds__(256)
pyramidGatherKernel(const uint64_t* __restrict__ keys, const float2* __restrict__ position, uint32_t vertexCount, uint32_t depth,
                    uint32_t vertexBits, float2* __restrict__ sortedPosition, uint32_t* __restrict__ leafBegin)
{
    const uint32_t last = (1u << depth) - 1u;
    for (uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < vertexCount; k += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t key = keys[k];
        const uint32_t vertex = uint32_t(key & ((1ull << vertexBits) - 1u));
        const uint32_t morton = uint32_t(key >> vertexBits);
        if (vertex < vertexCount) sortedPosition[k] = position[vertex];
        if (k == 0 || uint32_t(keys[k - 1u] >> vertexBits) != morton) {
            leafBegin[(gatherBits(morton >> 1) & last) << depth | (gatherBits(morton) & last)] = uint32_t(k);
        }
    }
}

// The cells of one level: the sum of the four children (below the leaf level), then the record the walk reads:
// (m_x, m_y, float(count), unused), m = float(double(lo) + double(S) * (double(sum) / (double(count) * 2^31))).  At the leaf
// level also leafRange = (begin, count) in the sorted order.
__global__ void __launch_bounds__(256)
pyramidLevelKernel(uint32_t level, uint32_t depth, const uint32_t* __restrict__ box, LayoutMoment* __restrict__ moment,
                   float4* __restrict__ record, const uint32_t* __restrict__ leafBegin, uint2* __restrict__ leafRange)
{
    const LayoutBox b = readBox(box);
    const uint32_t cellCount = 1u << (2u * level);
    LayoutMoment* mine = moment + layoutLevelBegin(level);
    const LayoutMoment* below = moment + layoutLevelBegin(level + 1u);      // (not touched at the leaf level)
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cellCount; c += gridDim.x * blockDim.x) {
        LayoutMoment m;
        if (level < depth) {
            const uint32_t bx = c & ((1u << level) - 1u), by = c >> level;
            m.sumX = m.sumY = 0ull;
            m.count = m.unused = 0u;
            for (uint32_t child = 0; child < 4u; child++) {
                const LayoutMoment& other = below[(2u * by + (child >> 1)) << (level + 1u) | (2u * bx + (child & 1u))];
                m.sumX += other.sumX;
                m.sumY += other.sumY;
                m.count += other.count;
            }
            mine[c] = m;
        } else {
            m = mine[c];
            leafRange[c] = m.count ? make_uint2(leafBegin[c], m.count) : make_uint2(0u, 0u);
        }
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m.count) {
            const double scale = double(m.count) * 2147483648.0;
            const double tx = double(m.sumX) / scale, ty = double(m.sumY) / scale;
            r.x = float(double(b.xmin) + double(b.side) * tx);
            r.y = float(double(b.ymin) + double(b.side) * ty);
            r.z = float(m.count);
        }
        record[layoutLevelBegin(level) + c] = r;
    }
}

// One far cell: (fx, fy) += (p_i - m) * (C * count) / max(d^2, delta).
__device__ __forceinline__ void repelCell(float xi, float yi, float4 cell, float& fx, float& fy)
{
    const float dx = xi - cell.x, dy = yi - cell.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    const float w = (kLayoutC * cell.z) / fmaxf(d2, kLayoutFloor);
    fx = fmaf(dx, w, fx);
    fy = fmaf(dy, w, fy);
}

// Sorted place k = one lane, so that a wave's lanes sit in the same leaf or in a few adjacent ones and their cells and leaves
// mostly coincide: the loads are then broadcasts or hits of the same lines.  Far: the levels 2 ... depth ascending, the 6 x 6
// cells of the parent's neighbourhood (by ascending, bx inside) that are in the grid, not within Chebyshev distance 1 of the
// vertex's cell and not empty.  Near: the 3 x 3 leaves around its own, their vertices in sorted (= ascending index) order.  Two
// sums from +0; repulsion[vertex] = far + near.  Lanes whose lists differ in length run their own loops under the wave's mask.
__global__ void __launch_bounds__(kLayoutBlockVertices)
pyramidWalkKernel(const uint64_t* __restrict__ keys, const float2* __restrict__ sortedPosition, uint32_t vertexCount, uint32_t depth,
                  uint32_t vertexBits, const float4* __restrict__ record, const uint2* __restrict__ leafRange,
                  float2* __restrict__ repulsion)
{
    const uint32_t k = blockIdx.x * kLayoutBlockVertices + threadIdx.x;
    if (k >= vertexCount) return;
    const uint64_t key = keys[k];
    const uint32_t vertex = uint32_t(key & ((1ull << vertexBits) - 1u));
    const uint32_t morton = uint32_t(key >> vertexBits);
    const int last = int((1u << depth) - 1u);
    const int cx = int(gatherBits(morton)) & last, cy = int(gatherBits(morton >> 1)) & last;
    const float2 p = sortedPosition[k];

    float farX = 0.f, farY = 0.f;
    for (uint32_t level = 2; level <= depth; level++) {
        const int ax = cx >> (depth - level), ay = cy >> (depth - level);
        const int side = 1 << level;
        const int x0 = 2 * ((ax >> 1) - 1), y0 = 2 * ((ay >> 1) - 1);
        const float4* cells = record + layoutLevelBegin(level);
        for (int by = y0; by < y0 + 6; by++) {
            if (by < 0 || by >= side) continue;
            for (int bx = x0; bx < x0 + 6; bx++) {
                if (bx < 0 || bx >= side || (abs(bx - ax) <= 1 && abs(by - ay) <= 1)) continue;
                const float4 cell = cells[uint32_t(by) << level | uint32_t(bx)];
                if (cell.z > 0.f) repelCell(p.x, p.y, cell, farX, farY);
            }
        }
    }

    float nearX = 0.f, nearY = 0.f;
    for (int by = cy - 1; by <= cy + 1; by++) {
        if (by < 0 || by > last) continue;
        for (int bx = cx - 1; bx <= cx + 1; bx++) {
            if (bx < 0 || bx > last) continue;
            const uint2 range = leafRange[uint32_t(by) << depth | uint32_t(bx)];
            const uint32_t begin = range.x < vertexCount ? range.x : vertexCount;
            const uint32_t end = range.y < vertexCount - begin ? begin + range.y : vertexCount;
            for (uint32_t j = begin; j < end; j++) repel(p.x, p.y, sortedPosition[j], nearX, nearY);
        }
    }
    if (vertex < vertexCount) repulsion[vertex] = make_float2(farX + nearX, farY + nearY);
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
    // the pyramid (pyramid false: the exact repulsion, and none of these is set)
    bool pyramid = false;
    uint32_t depth = 0, vertexBits = 1;
    uint32_t* box = nullptr;                        // directly behind the leaf level of `moment`: one memset clears both
    LayoutMoment* moment = nullptr;
    float4* record = nullptr;
    uint32_t* leafBegin = nullptr;
    uint2* leafRange = nullptr;
    float2* sortedPosition = nullptr;
    uint64_t* pyramidKeys[2] = {nullptr, nullptr};
    void* sortTemp = nullptr;
    size_t sortTempBytes = 0;

    void idle() { arena.idle = recordArena.idle = true; }

    // wantedDepth: kLayoutDepthExact, kLayoutDepthAuto or a depth <= kLayoutMaxDepth (the entries have checked it).
    hipError_t prepare(uint32_t n, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, uint32_t wantedDepth,
                       uint32_t* inputError, hipStream_t stream)
    {
        *inputError = 0;
        vertexCount = n;
        chunkCount = blocksOf(n, kLayoutBlockVertices);
        sliceLength = blocksOf(n, kLayoutSliceCount);
        pyramid = wantedDepth != kLayoutDepthExact;
        depth = !pyramid ? 0u : wantedDepth == kLayoutDepthAuto ? layoutAutomaticDepth(n) : wantedDepth < kLayoutMaxDepth ? wantedDepth : kLayoutMaxDepth;
        vertexBits = 1u;                                        // the bits of n - 1, at least one (a sort needs a bit)
        while (vertexBits < 32u && (uint64_t(n) - 1u) >> vertexBits) vertexBits++;
        const uint32_t cellCount = layoutLevelBegin(depth + 1u), leafCount = 1u << (2u * depth);
        const dim3 threads(256);
        const uint64_t recordCount = 2u * edgeCount;
        ArenaPlan plan;
        const size_t offError = plan.take(256);
        const size_t offState = plan.take(sizeof(LayoutState));
        const size_t offPosition0 = plan.takeFor<float2>(n);
        const size_t offPosition1 = plan.takeFor<float2>(n);
        const size_t offForce = plan.takeFor<float2>(n);
        const size_t offPartial = plan.take(size_t(n) * (pyramid ? 1u : kLayoutSliceCount) * sizeof(float2));
        const size_t offChunk = plan.takeFor<double>(chunkCount);
        const size_t offOffsets = plan.take((size_t(n) + 1u) * sizeof(uint64_t));
        const size_t offNeighbours = plan.takeFor<uint32_t>(recordCount);
        size_t offMoment = 0, offRecord = 0, offLeafBegin = 0, offLeafRange = 0, offSorted = 0, offKeys0 = 0, offKeys1 = 0, offTemp = 0;
        if (pyramid) {
            offMoment = plan.take(size_t(cellCount) * sizeof(LayoutMoment) + 4u * sizeof(uint32_t));      // (and the box behind it)
            offRecord = plan.takeFor<float4>(cellCount);
            offLeafBegin = plan.takeFor<uint32_t>(leafCount);
            offLeafRange = plan.takeFor<uint2>(leafCount);
            offSorted = plan.takeFor<float2>(n);
            offKeys0 = plan.takeFor<uint64_t>(n);
            offKeys1 = plan.takeFor<uint64_t>(n);
            EM2_TRY(sortKeysBufferBytes(size_t(n), 0u, vertexBits + 2u * depth, sortTempBytes));
            offTemp = plan.take(sortTempBytes);
        }
        EM2_TRY(arena.allocate(plan.bytes));
        char* base = arena.as<char>();
        if (pyramid) {
            moment = arenaAt<LayoutMoment>(base, offMoment);
            box = reinterpret_cast<uint32_t*>(moment + cellCount);
            record = arenaAt<float4>(base, offRecord);
            leafBegin = arenaAt<uint32_t>(base, offLeafBegin);
            leafRange = arenaAt<uint2>(base, offLeafRange);
            sortedPosition = arenaAt<float2>(base, offSorted);
            pyramidKeys[0] = arenaAt<uint64_t>(base, offKeys0);
            pyramidKeys[1] = arenaAt<uint64_t>(base, offKeys1);
            sortTemp = base + offTemp;
        }
        uint32_t* error = arenaAt<uint32_t>(base, offError);
        state = arenaAt<LayoutState>(base, offState);
        position[0] = arenaAt<float2>(base, offPosition0);
        position[1] = arenaAt<float2>(base, offPosition1);
        force = arenaAt<float2>(base, offForce);
        partial = arenaAt<float2>(base, offPartial);
        chunkEnergy = arenaAt<double>(base, offChunk);
        offsets = arenaAt<uint64_t>(base, offOffsets);
        neighbours = arenaAt<uint32_t>(base, offNeighbours);

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
            ArenaPlan records;
            const size_t offKeysA = records.takeFor<uint64_t>(recordCount);
            const size_t offKeysB = records.takeFor<uint64_t>(recordCount);
            size_t sortBytes = 0;
            EM2_TRY(sortKeysBufferBytes(size_t(recordCount), 0u, 64u, sortBytes));
            const size_t offSortTemp = records.take(sortBytes);
            EM2_TRY(recordArena.allocate(records.bytes));
            char* recordBase = recordArena.as<char>();
            DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(recordBase, offKeysA), arenaAt<uint64_t>(recordBase, offKeysB)};
            layoutRecordsKernel<<<dim3(gridFor(edgeCount)), threads, 0, stream>>>(d_edge0, d_edge1, edgeCount, keys.current());
            EM2_TRY(hipGetLastError());
            EM2_TRY(sortKeys(recordBase + offSortTemp, sortBytes, keys, size_t(recordCount), 0u, 64u, stream));
            sortedKeys = keys.current();
        }
        // (with no record the searches find nothing and read nothing: every offset 0)
        layoutOffsetsKernel<<<dim3(gridFor(recordCount > n ? recordCount : uint64_t(n) + 1u)), threads, 0, stream>>>(
            sortedKeys, recordCount, n, offsets, neighbours);
        EM2_TRY(hipGetLastError());
        return hipSuccess;
    }

    // The approximate repulsion at `current`, one sum per vertex into partial[vertex].  Everything is rebuilt: the box, the
    // order, the pyramid.  (With EM2_TIMING=1 and a timer set, the stages of every evaluation go to stderr.)
    StageTimer* timer = nullptr;
    hipError_t stage(const char* name, hipStream_t stream) { return timer ? timer->stage(name, stream) : hipSuccess; }

    hipError_t pyramidRepulsion(const float2* current, hipStream_t stream)
    {
        const dim3 threads(256);
        const uint32_t n = vertexCount, leafCount = 1u << (2u * depth);
        LayoutMoment* leaves = moment + layoutLevelBegin(depth);
        EM2_TRY(hipMemsetAsync(leaves, 0, size_t(leafCount) * sizeof(LayoutMoment) + 4u * sizeof(uint32_t), stream));
        boxKernel<<<dim3(gridFor(n) < kLayoutBoxBlocks ? gridFor(n) : kLayoutBoxBlocks), threads, 0, stream>>>(current, n, box);
        EM2_TRY(hipGetLastError());
        EM2_TRY(stage("box", stream));
        pyramidKeysKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(current, n, box, depth, vertexBits, pyramidKeys[0], leaves);
        EM2_TRY(hipGetLastError());
        DoubleBuffer<uint64_t> keys{pyramidKeys[0], pyramidKeys[1]};
        EM2_TRY(sortKeys(sortTemp, sortTempBytes, keys, size_t(n), 0u, vertexBits + 2u * depth, stream));
        pyramidGatherKernel<<<dim3(gridFor(n)), threads, 0, stream>>>(keys.current(), current, n, depth, vertexBits, sortedPosition,
                                                                     leafBegin);
        EM2_TRY(hipGetLastError());
        EM2_TRY(stage("keys and sort", stream));
        // the leaf level (its ranges are the near field's), then the levels above it that the far field reads: down to 2
        for (uint32_t level = depth;; level--) {
            pyramidLevelKernel<<<dim3(gridFor(1u << (2u * level))), threads, 0, stream>>>(level, depth, box, moment, record, leafBegin,
                                                                                         leafRange);
            EM2_TRY(hipGetLastError());
            if (level <= 2u) break;
        }
        EM2_TRY(stage("pyramid", stream));
        pyramidWalkKernel<<<dim3(chunkCount), dim3(kLayoutBlockVertices), 0, stream>>>(keys.current(), sortedPosition, n, depth, vertexBits,
                                                                                      record, leafRange, partial);
        EM2_TRY(hipGetLastError());
        return stage("walk", stream);
    }

    // One evaluation at position[from]; the move goes to position[1 - from] where `move` is set, f to `force` where wanted.
    hipError_t evaluate(uint32_t from, float gravity, bool move, bool keepForce, hipStream_t stream)
    {
        const dim3 threads(kLayoutBlockVertices);
        float2* next = move ? position[1u - from] : nullptr;
        float2* kept = keepForce ? force : nullptr;
        if (pyramid) {
            EM2_TRY(pyramidRepulsion(position[from], stream));
            forceKernel<1u><<<dim3(chunkCount), threads, 0, stream>>>(position[from], vertexCount, partial, offsets, neighbours, gravity,
                                                                     state, next, kept, chunkEnergy);
        } else {
            repulsionKernel<<<dim3(chunkCount, kLayoutSliceCount), threads, 0, stream>>>(position[from], vertexCount, sliceLength, partial);
            EM2_TRY(hipGetLastError());
            forceKernel<kLayoutSliceCount><<<dim3(chunkCount), threads, 0, stream>>>(position[from], vertexCount, partial, offsets, neighbours,
                                                                                    gravity, state, next, kept, chunkEnergy);
        }
        EM2_TRY(hipGetLastError());
        energyStepKernel<<<dim3(1), threads, 0, stream>>>(chunkEnergy, chunkCount, move, state);
        EM2_TRY(hipGetLastError());
        return pyramid ? stage("force", stream) : hipSuccess;
    }
};

}  // namespace

hipError_t runGraphLayout(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                          const LayoutParameters& parameters, uint32_t depth, float* d_x, float* d_y, LayoutResult& result,
                          uint32_t* inputError, hipStream_t stream)
{
    StageTimer timer("graphLayout");
    LayoutWork work;
    EM2_TRY(work.prepare(vertexCount, d_edge0, d_edge1, edgeCount, depth, inputError, stream));
    if (*inputError) {
        work.idle();
        return hipSuccess;
    }
    EM2_TRY(timer.stage("check and adjacency", stream));
    work.timer = &timer;

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
                                uint32_t depth, const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy,
                                uint32_t* inputError, hipStream_t stream)
{
    LayoutWork work;
    EM2_TRY(work.prepare(vertexCount, d_edge0, d_edge1, edgeCount, depth, inputError, stream));
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

// A depth the pyramid entries accept.
static bool depthIsValid(uint32_t depth) { return depth == em2::kLayoutDepthAuto || depth <= em2::kLayoutMaxDepth; }
static const char* const kDepthText = "depth must be at most 10 or the automatic depth";

// depth: em2::kLayoutDepthExact from the exact entries, else what the caller of a pyramid entry gave.
static int graphLayout(const char* who, bool onDevice, uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                       uint64_t edgeCount, const em2_layout_parameters* parameters, uint32_t depth, float* x, float* y,
                       em2_layout_result* result)
{
    if (!parameters || (vertexCount && (!x || !y)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(parameters->tolerance >= 0.)) return failArgument(who, "tolerance must not be negative");
    if (!(parameters->gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (!(parameters->initialStep >= 0.)) return failArgument(who, "initialStep must not be negative");
    if (depth != em2::kLayoutDepthExact && !depthIsValid(depth)) return failArgument(who, kDepthText);
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
                                p, depth, onDevice ? x : dx.as<float>(), onDevice ? y : dy.as<float>(), r, &inputError, nullptr));
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
    return graphLayout("em2_graph_layout", false, vertexCount, edgeVertex0, edgeVertex1, edgeCount, parameters, em2::kLayoutDepthExact, x, y,
                       result);
}

int em2_dev_graph_layout(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                         const em2_layout_parameters* parameters, float* d_x, float* d_y, em2_layout_result* result)
{
    return graphLayout("em2_dev_graph_layout", true, vertexCount, d_edgeVertex0, d_edgeVertex1, edgeCount, parameters,
                       em2::kLayoutDepthExact, d_x, d_y, result);
}

int em2_graph_layout_pyramid(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                             const em2_layout_parameters* parameters, uint32_t depth, float* x, float* y, em2_layout_result* result)
{
    // (the internal value for "exact" is not a depth a caller may give)
    return graphLayout("em2_graph_layout_pyramid", false, vertexCount, edgeVertex0, edgeVertex1, edgeCount, parameters,
                       depth == em2::kLayoutDepthExact ? em2::kLayoutMaxDepth + 1u : depth, x, y, result);
}

int em2_dev_graph_layout_pyramid(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                                 const em2_layout_parameters* parameters, uint32_t depth, float* d_x, float* d_y, em2_layout_result* result)
{
    return graphLayout("em2_dev_graph_layout_pyramid", true, vertexCount, d_edgeVertex0, d_edgeVertex1, edgeCount, parameters,
                       depth == em2::kLayoutDepthExact ? em2::kLayoutMaxDepth + 1u : depth, d_x, d_y, result);
}

static int graphLayoutForces(const char* who, uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                             uint64_t edgeCount, double gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy,
                             double* energy)
{
    if ((vertexCount && (!x || !y || !fx || !fy)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (depth != em2::kLayoutDepthExact && !depthIsValid(depth)) return failArgument(who, kDepthText);
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
    EM2_HIP(em2::runGraphLayoutForces(vertexCount, d0.as<uint32_t>(), d1.as<uint32_t>(), edgeCount, gravity, depth, dx.as<float>(),
                                      dy.as<float>(), dfx.as<float>(), dfy.as<float>(), &e, &inputError, nullptr));
    if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
    EM2_HIP(dfx.download(fx, vertexCount));
    EM2_HIP(dfy.download(fy, vertexCount));
    if (energy) *energy = e;
    return EM2_OK;
}

int em2_graph_layout_forces(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                            double gravity, const float* x, const float* y, float* fx, float* fy, double* energy)
{
    return graphLayoutForces("em2_graph_layout_forces", vertexCount, edgeVertex0, edgeVertex1, edgeCount, gravity, em2::kLayoutDepthExact, x,
                             y, fx, fy, energy);
}

int em2_graph_layout_forces_pyramid(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                                    double gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy, double* energy)
{
    return graphLayoutForces("em2_graph_layout_forces_pyramid", vertexCount, edgeVertex0, edgeVertex1, edgeCount, gravity,
                             depth == em2::kLayoutDepthExact ? em2::kLayoutMaxDepth + 1u : depth, x, y, fx, fy, energy);
}

}  // extern "C"
