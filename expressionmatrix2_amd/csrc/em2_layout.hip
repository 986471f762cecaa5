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
// The multilevel entries run these kernels level by level over a hierarchy built with integers only:
//   * mergeKeysKernel, a pair sort, em2_runs.h's head flags, a scan, mergeRunsKernel: the merged, weighted edges of a level;
//   * matchPointKernel / matchPairKernel   one round of locally dominant edges, a lane per vertex; the rounds end in the greedy
//                          matching over the total key (weight, hash, a, b);
//   * groupFlagsKernel, a scan, groupMapKernel: the coarse ids and masses; prolongKernel: the positions of the finer level;
//   * the force kernels above as templates on kWeighted: masses in the repulsion and the pyramid, weights in the attraction.
//                          The unweighted instantiations are what the single-level entries and level 0 run.

#include "em2_adjacency.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_runs.h"
#include "em2_scratch.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

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
constexpr uint32_t kLayoutDepthExact = EM2_LAYOUT_DEPTH_EXACT;   // no pyramid: the exact repulsion (the pyramid entries refuse it)
// The multilevel layout.  All three are part of the contract.
constexpr uint32_t kLayoutCoarsest = EM2_LAYOUT_COARSEST;
constexpr uint32_t kLayoutMaxLevels = EM2_LAYOUT_MAX_LEVELS;
constexpr uint32_t kLayoutExactLimit = EM2_LAYOUT_EXACT_LIMIT;
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

// One pair: (fx, fy) += (p_i - p_j) * C / max(d^2, delta).  dy * dy is a product of its own, the rest are fmaf.  kWeighted (a
// coarse level of the multilevel layout): C is multiplied by the mass of j first; with a mass of 1 that is C.
template <bool kWeighted>
__device__ __forceinline__ void repel(float xi, float yi, float2 pj, float mj, float& fx, float& fy)
{
    const float dx = xi - pj.x, dy = yi - pj.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    const float w = (kWeighted ? kLayoutC * mj : kLayoutC) / fmaxf(d2, kLayoutFloor);
    fx = fmaf(dx, w, fx);
    fy = fmaf(dy, w, fy);
}

// Workgroup (b, s): the vertices [256 b, 256 b + 256) against slice s of the j range, [s L, min(N, s L + L)).  The slice goes
// through LDS in tiles of kLayoutTile positions; every lane of a wave reads the same tile entry (a broadcast, no conflict).
// partial[s N + i] = the slice's sum for vertex i, terms added in ascending j from 0.  An empty slice writes zeros.
// kWeighted: the masses of the tile's vertices go through LDS with their positions (mass is not read otherwise); the
// unweighted kernel's LDS is the positions alone, as before.
template <bool kWeighted> struct LayoutTile {
    float2 position[kLayoutTile];
    float mass[kLayoutTile];
};
template <> struct LayoutTile<false> {
    float2 position[kLayoutTile];
};
template <bool kWeighted> __device__ __forceinline__ float tileMassAt(const LayoutTile<kWeighted>& tile, uint32_t j)
{
    if constexpr (kWeighted) return tile.mass[j];
    else return 1.f;
}

template <bool kWeighted>
__global__ void __launch_bounds__(kLayoutBlockVertices)
repulsionKernel(const float2* __restrict__ position, const uint32_t* __restrict__ mass, uint32_t vertexCount, uint32_t sliceLength,
                float2* __restrict__ partial)
{
    __shared__ LayoutTile<kWeighted> tile;
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
        if (threadIdx.x < count) {
            tile.position[threadIdx.x] = position[t + threadIdx.x];
            if constexpr (kWeighted) tile.mass[threadIdx.x] = float(mass[t + threadIdx.x]);
        }
        __syncthreads();
        if (count == kLayoutTile) {
#pragma unroll 8
            for (uint32_t j = 0; j < kLayoutTile; j++) repel<kWeighted>(pi.x, pi.y, tile.position[j], tileMassAt(tile, j), fx, fy);
        } else {
            for (uint32_t j = 0; j < count; j++) repel<kWeighted>(pi.x, pi.y, tile.position[j], tileMassAt(tile, j), fx, fy);
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
// kWeighted: an attraction term is fmaf(dx, d * float(w_ij), ax) and the sum is divided by float(m_i) once, before it is
// subtracted; with weights and masses of 1 both are exact and the bits are those of the unweighted force.
template <uint32_t kSliceCount, bool kWeighted>
__global__ void __launch_bounds__(kLayoutBlockVertices)
forceKernel(const float2* __restrict__ position, uint32_t vertexCount, const float2* __restrict__ partial,
            const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ neighbours, const uint32_t* __restrict__ mass,
            const uint32_t* __restrict__ neighbourWeights, float gravity,
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
            float d = sqrtf(fmaf(dx, dx, dy * dy));
            if (kWeighted) d = d * float(neighbourWeights[k]);
            ax = fmaf(dx, d, ax);
            ay = fmaf(dy, d, ay);
        }
        if (kWeighted) {
            const float mi = float(mass[i]);
            ax = ax / mi;
            ay = ay / mi;
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
    uint32_t count;                                 // (with masses: the sum of the masses, and the sums above are of m * q)
    uint32_t vertices;                              // the vertices of a leaf where they are not its count: with masses only
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
// kWeighted: the vertex counts as mass[i] vertices at its place -- the masses of a graph sum to at most 2^30, so the sums stay
// below 2^61 -- and the leaf counts its vertices apart.
template <bool kWeighted>
__global__ void __launch_bounds__(256)
pyramidKeysKernel(const float2* __restrict__ position, const uint32_t* __restrict__ mass, uint32_t vertexCount,
                  const uint32_t* __restrict__ box, uint32_t depth, uint32_t vertexBits, uint64_t* __restrict__ keys,
                  LayoutMoment* __restrict__ moment)
{
    const LayoutBox b = readBox(box);
    const uint32_t last = (1u << depth) - 1u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const float2 p = position[i];
        const uint32_t qx = quantise(p.x, b.xmin, b.side), qy = quantise(p.y, b.ymin, b.side);
        const uint32_t cx = min(last, qx >> (31u - depth)), cy = min(last, qy >> (31u - depth));
        keys[i] = uint64_t(spreadBits(cx) | spreadBits(cy) << 1) << vertexBits | i;
        LayoutMoment* leaf = moment + (cy << depth | cx);
        if (kWeighted) {
            const uint32_t m = mass[i];
            atomicAdd(&leaf->count, m);
            atomicAdd(&leaf->sumX, (unsigned long long)m * qx);
            atomicAdd(&leaf->sumY, (unsigned long long)m * qy);
            atomicAdd(&leaf->vertices, 1u);
        } else {
            atomicAdd(&leaf->count, 1u);
            atomicAdd(&leaf->sumX, (unsigned long long)qx);
            atomicAdd(&leaf->sumY, (unsigned long long)qy);
        }
    }
}

// Sorted place k: the position of its vertex, and where a leaf begins (leafBegin is written for the leaves that hold a vertex).
// kWeighted: also float(its mass).
template <bool kWeighted>
__global__ void __launch_bounds__(256)
pyramidGatherKernel(const uint64_t* __restrict__ keys, const float2* __restrict__ position, const uint32_t* __restrict__ mass,
                    uint32_t vertexCount, uint32_t depth, uint32_t vertexBits, float2* __restrict__ sortedPosition,
                    float* __restrict__ sortedMass, uint32_t* __restrict__ leafBegin)
{
    const uint32_t last = (1u << depth) - 1u;
    for (uint64_t k = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < vertexCount; k += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t key = keys[k];
        const uint32_t vertex = uint32_t(key & ((1ull << vertexBits) - 1u));
        const uint32_t morton = uint32_t(key >> vertexBits);
        if (vertex < vertexCount) {
            sortedPosition[k] = position[vertex];
            if (kWeighted) sortedMass[k] = float(mass[vertex]);
        }
        if (k == 0 || uint32_t(keys[k - 1u] >> vertexBits) != morton) {
            leafBegin[(gatherBits(morton >> 1) & last) << depth | (gatherBits(morton) & last)] = uint32_t(k);
        }
    }
}

// The cells of one level: the sum of the four children (below the leaf level), then the record the walk reads:
// (m_x, m_y, float(count), unused), m = float(double(lo) + double(S) * (double(sum) / (double(count) * 2^31))).  At the leaf
// level also leafRange = (begin, vertices) in the sorted order.
template <bool kWeighted>
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
            m.count = m.vertices = 0u;
            for (uint32_t child = 0; child < 4u; child++) {
                const LayoutMoment& other = below[(2u * by + (child >> 1)) << (level + 1u) | (2u * bx + (child & 1u))];
                m.sumX += other.sumX;
                m.sumY += other.sumY;
                m.count += other.count;
            }
            mine[c] = m;
        } else {
            m = mine[c];
            leafRange[c] = m.count ? make_uint2(leafBegin[c], kWeighted ? m.vertices : m.count) : make_uint2(0u, 0u);
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
// kWeighted: a near pair carries the mass of j (a far cell's float(count) is its mass sum already).
template <bool kWeighted>
__global__ void __launch_bounds__(kLayoutBlockVertices)
pyramidWalkKernel(const uint64_t* __restrict__ keys, const float2* __restrict__ sortedPosition, const float* __restrict__ sortedMass,
                  uint32_t vertexCount, uint32_t depth, uint32_t vertexBits, const float4* __restrict__ record, const uint2* __restrict__ leafRange,
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
            for (uint32_t j = begin; j < end; j++) {
                repel<kWeighted>(p.x, p.y, sortedPosition[j], kWeighted ? sortedMass[j] : 1.f, nearX, nearY);
            }
        }
    }
    if (vertex < vertexCount) repulsion[vertex] = make_float2(farX + nearX, farY + nearY);
}

// ---- the levels of the multilevel layout: integers only ----
// A level is a graph of merged edges (a, b), a < b, each once, with a weight; its vertices have masses.  `none` stands for
// "no vertex" in mate and pointer, and an edge key of all ones for an edge that is dropped (a self-loop, an edge inside a group).

constexpr uint32_t kLayoutNone = 0xffffffffu;
constexpr uint64_t kLayoutDroppedEdge = ~0ull;

// The finaliser of splitmix64 after its increment (initialKernel's hash), and the hash of (seed, level, what): the caller
// passes salt = layoutMix(seed << 32 | level).
__host__ __device__ __forceinline__ uint64_t layoutMix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256)
fillKernel(uint32_t* __restrict__ out, uint64_t count, uint32_t value)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) out[i] = value;
}

// Edge e as an unordered pair of the images of its ends under `map` (null: the ends themselves): keys[e] = min << 32 | max,
// or the dropped key where the two coincide; values[e] = its weight (weight null: 1).
__global__ void __launch_bounds__(256)
mergeKeysKernel(const uint32_t* __restrict__ edge0, const uint32_t* __restrict__ edge1, const uint32_t* __restrict__ weight,
                uint64_t edgeCount, const uint32_t* __restrict__ map, uint64_t* __restrict__ keys, uint32_t* __restrict__ values)
{
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        uint32_t a = edge0[e], b = edge1[e];
        if (map) {
            a = map[a];
            b = map[b];
        }
        keys[e] = a == b ? kLayoutDroppedEdge : uint64_t(min(a, b)) << 32 | max(a, b);
        values[e] = weight ? weight[e] : 1u;
    }
}

// The sorted keys with their head flags and the inclusive scan of the flags: run r = scan - 1 becomes edge r, its weight the
// sum of the run's values (integer atomics into zeroed words: no order).  The dropped keys sort last and form the last run,
// which is not counted: *mergedCount = the runs before it.
__global__ void __launch_bounds__(256)
mergeRunsKernel(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ values, const uint32_t* __restrict__ flags,
                const uint32_t* __restrict__ scan, uint64_t count, uint32_t* __restrict__ edge0, uint32_t* __restrict__ edge1,
                uint32_t* __restrict__ weight, uint64_t* __restrict__ mergedCount)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t key = sorted[i];
        const bool dropped = key == kLayoutDroppedEdge;
        if (i == count - 1u) *mergedCount = uint64_t(scan[i]) - (dropped ? 1u : 0u);
        if (dropped) continue;
        const uint32_t run = scan[i] - 1u;
        if (flags[i]) {
            edge0[run] = uint32_t(key >> 32);
            edge1[run] = uint32_t(key);
        }
        atomicAdd(weight + run, values[i]);
    }
}

// Two directed records per edge, the weight as the value.
__global__ void __launch_bounds__(256)
weightedRecordsKernel(const uint32_t* __restrict__ edge0, const uint32_t* __restrict__ edge1, const uint32_t* __restrict__ weight,
                      uint64_t edgeCount, uint64_t* __restrict__ keys, uint32_t* __restrict__ values)
{
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t v0 = edge0[e], v1 = edge1[e];
        keys[2u * e] = v0 << 32 | v1;
        keys[2u * e + 1u] = v1 << 32 | v0;
        values[2u * e] = values[2u * e + 1u] = weight ? weight[e] : 1u;
    }
}

// layoutOffsetsKernel with the weights of the sorted records.
__global__ void __launch_bounds__(256)
weightedOffsetsKernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ values, uint64_t recordCount, uint32_t vertexCount,
                      uint64_t* __restrict__ offsets, uint32_t* __restrict__ neighbours, uint32_t* __restrict__ neighbourWeights)
{
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t v = first; v <= vertexCount; v += stride) offsets[v] = lowerBound(keys, recordCount, v << 32);
    for (uint64_t i = first; i < recordCount; i += stride) {
        neighbours[i] = uint32_t(keys[i]);
        neighbourWeights[i] = values[i];
    }
}

// One round of the matching, first half.  A lane per vertex: an unmatched vertex scans its whole adjacency (a hub serialises
// the round: a known limit) for its live edges, those to unmatched neighbours, and points at the other end of the one with the
// largest key (weight, hash of (seed, level, a, b), a, b); pointer[v] = none where it has none or is matched.  *liveCount: the
// vertices that point somewhere, one atomic per wave.  The hash is only computed where the weights tie.
__global__ void __launch_bounds__(256)
matchPointKernel(uint32_t vertexCount, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ neighbours,
                 const uint32_t* __restrict__ neighbourWeights, const uint32_t* __restrict__ mate, uint64_t salt,
                 uint32_t* __restrict__ pointer, uint32_t* __restrict__ liveCount)
{
    uint32_t live = 0u;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t v = uint32_t(i);
        uint32_t best = kLayoutNone, bestWeight = 0u;
        uint64_t bestHash = 0ull;
        bool bestHashed = false;
        if (mate[v] == kLayoutNone) {
            const uint64_t last = offsets[i + 1u];
            for (uint64_t k = offsets[i]; k < last; k++) {
                const uint32_t u = neighbours[k];
                if (u >= vertexCount || mate[u] != kLayoutNone) continue;
                const uint32_t w = neighbourWeights[k];
                if (best != kLayoutNone && w < bestWeight) continue;
                bool better = best == kLayoutNone || w > bestWeight;
                uint64_t hash = 0ull;
                bool hashed = false;
                if (!better) {
                    // equal weights: the hashes of the two edges, then (a, b) -- the edges share v, so the other ends decide
                    if (!bestHashed) {
                        bestHash = layoutMix(salt ^ (uint64_t(min(v, best)) << 32 | max(v, best)));
                        bestHashed = true;
                    }
                    hash = layoutMix(salt ^ (uint64_t(min(v, u)) << 32 | max(v, u)));
                    hashed = true;
                    if (hash != bestHash) {
                        better = hash > bestHash;
                    } else {
                        const uint32_t a = min(v, u), b = max(v, u), bestA = min(v, best), bestB = max(v, best);
                        better = a != bestA ? a > bestA : b > bestB;
                    }
                }
                if (better) {
                    best = u;
                    bestWeight = w;
                    bestHash = hash;
                    bestHashed = hashed;
                }
            }
        }
        pointer[v] = best;
        if (best != kLayoutNone) live++;
    }
    for (int offset = 32; offset >= 1; offset /= 2) live += __shfl_xor(live, offset);
    if ((threadIdx.x & 63u) == 0u && live) atomicAdd(liveCount, live);
}

// ... second half: two vertices that point at each other are matched.  Every thread writes its own vertex only.
__global__ void __launch_bounds__(256)
matchPairKernel(uint32_t vertexCount, const uint32_t* __restrict__ pointer, uint32_t* __restrict__ mate)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t p = pointer[i];
        if (p < vertexCount && pointer[p] == uint32_t(i)) mate[i] = p;
    }
}

// flags[v] = 1 where v is the representative of its group: unmatched, or the smaller index of its pair.
__global__ void __launch_bounds__(256)
groupFlagsKernel(uint32_t vertexCount, const uint32_t* __restrict__ mate, uint32_t* __restrict__ flags)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t m = mate[i];
        flags[i] = (m == kLayoutNone || uint32_t(i) < m) ? 1u : 0u;
    }
}

// scan: the exclusive scan of the flags, so the coarse id of a representative.  coarseOf[v] = the id of v's representative;
// the representative writes the group's mass; *coarseCount = the groups.
__global__ void __launch_bounds__(256)
groupMapKernel(uint32_t vertexCount, const uint32_t* __restrict__ mate, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ scan,
               const uint32_t* __restrict__ mass, uint32_t* __restrict__ coarseOf, uint32_t* __restrict__ coarseMass,
               uint32_t* __restrict__ coarseCount)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t m = mate[i];
        if (flags[i]) {
            coarseOf[i] = scan[i];
            coarseMass[scan[i]] = mass[i] + (m < vertexCount ? mass[m] : 0u);
        } else {
            coarseOf[i] = m < vertexCount ? scan[m] : 0u;
        }
        if (i == vertexCount - 1u) *coarseCount = scan[i] + flags[i];
    }
}

// From a level to the finer one below it: a representative takes its group's position, the other member of a pair that
// position plus an offset in [-0.5, 0.5)^2 hashed from (seed, the finer level, vertex) -- coincident vertices would never
// separate, their pair terms being exact zeros.  salt = layoutMix(seed << 32 | level).
__global__ void __launch_bounds__(256)
prolongKernel(uint32_t vertexCount, const uint32_t* __restrict__ mate, const uint32_t* __restrict__ coarseOf, uint32_t coarseCount,
              const float2* __restrict__ coarsePosition, uint64_t salt, float2* __restrict__ position)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < vertexCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t c = coarseOf[i];
        float2 p = c < coarseCount ? coarsePosition[c] : make_float2(0.f, 0.f);
        const uint32_t m = mate[i];
        if (m != kLayoutNone && m < uint32_t(i)) {
            const uint64_t z = layoutMix(salt ^ i);
            p.x += float(uint32_t(z >> 40)) * 0x1p-24f - 0.5f;
            p.y += float(uint32_t(z >> 16) & 0xffffffu) * 0x1p-24f - 0.5f;
        }
        position[i] = p;
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
    // a coarse level of the multilevel layout: the masses of the vertices and the weights of `neighbours`,
    // which then live with the level, like `offsets` and `neighbours`.  Null: the unweighted kernels run.
    const uint32_t* mass = nullptr;
    const uint32_t* neighbourWeights = nullptr;
    float* sortedMass = nullptr;
    uint32_t* error = nullptr;

    void idle() { arena.idle = recordArena.idle = true; }

    // The buffers of an evaluation over n vertices.  ownAdjacency: with `offsets` and `neighbours` for recordCount entries,
    // which the caller then fills; else those two stay null until borrowGraph() points them at a level's arrays.
    // wantedDepth: kLayoutDepthExact, kLayoutDepthAuto or a depth <= kLayoutMaxDepth (the entries have checked it).
    hipError_t allocate(uint32_t n, uint64_t recordCount, uint32_t wantedDepth, bool weighted, bool ownAdjacency = true)
    {
        vertexCount = n;
        chunkCount = blocksOf(n, kLayoutBlockVertices);
        sliceLength = blocksOf(n, kLayoutSliceCount);
        pyramid = wantedDepth != kLayoutDepthExact;
        depth = !pyramid ? 0u : wantedDepth == kLayoutDepthAuto ? layoutAutomaticDepth(n) : wantedDepth < kLayoutMaxDepth ? wantedDepth : kLayoutMaxDepth;
        vertexBits = 1u;                                        // the bits of n - 1, at least one (a sort needs a bit)
        while (vertexBits < 32u && (uint64_t(n) - 1u) >> vertexBits) vertexBits++;
        const uint32_t cellCount = layoutLevelBegin(depth + 1u), leafCount = 1u << (2u * depth);
        ArenaPlan plan;
        const size_t offError = plan.take(256);
        const size_t offState = plan.take(sizeof(LayoutState));
        const size_t offPosition0 = plan.takeFor<float2>(n);
        const size_t offPosition1 = plan.takeFor<float2>(n);
        const size_t offForce = plan.takeFor<float2>(n);
        const size_t offPartial = plan.take(size_t(n) * (pyramid ? 1u : kLayoutSliceCount) * sizeof(float2));
        const size_t offChunk = plan.takeFor<double>(chunkCount);
        const size_t offOffsets = ownAdjacency ? plan.take((size_t(n) + 1u) * sizeof(uint64_t)) : 0u;
        const size_t offNeighbours = ownAdjacency ? plan.takeFor<uint32_t>(recordCount) : 0u;
        size_t offMoment = 0, offRecord = 0, offLeafBegin = 0, offLeafRange = 0, offSorted = 0, offKeys0 = 0, offKeys1 = 0, offTemp = 0;
        size_t offSortedMass = 0;
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
            if (weighted) offSortedMass = plan.takeFor<float>(n);
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
            if (weighted) sortedMass = arenaAt<float>(base, offSortedMass);
        }
        error = arenaAt<uint32_t>(base, offError);
        state = arenaAt<LayoutState>(base, offState);
        position[0] = arenaAt<float2>(base, offPosition0);
        position[1] = arenaAt<float2>(base, offPosition1);
        force = arenaAt<float2>(base, offForce);
        partial = arenaAt<float2>(base, offPartial);
        chunkEnergy = arenaAt<double>(base, offChunk);
        offsets = ownAdjacency ? arenaAt<uint64_t>(base, offOffsets) : nullptr;
        neighbours = ownAdjacency ? arenaAt<uint32_t>(base, offNeighbours) : nullptr;
        return hipSuccess;
    }

    // The graph of a coarse level, which the level owns and outlives this work with: nothing of it is in `arena`.
    void borrowGraph(const uint64_t* levelOffsets, const uint32_t* levelNeighbours, const uint32_t* levelNeighbourWeights,
                     const uint32_t* levelMass)
    {
        offsets = const_cast<uint64_t*>(levelOffsets);          // (read only from here on: the kernels take them as const)
        neighbours = const_cast<uint32_t*>(levelNeighbours);
        neighbourWeights = levelNeighbourWeights;
        mass = levelMass;
    }

    // *inputError = kLayoutEdgeRange where an edge end is not below n, else 0.  Synchronises the stream.
    hipError_t checkEdges(uint32_t n, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, uint32_t* inputError,
                          hipStream_t stream)
    {
        *inputError = 0;
        EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
        checkEdgesKernel<<<dim3(gridFor(edgeCount)), dim3(256), 0, stream>>>(d_edge0, d_edge1, edgeCount, n, error);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        return hipStreamSynchronize(stream);
    }

    // The unweighted graph of the single-level entries and of level 0: the buffers, the edge check, the adjacency.
    hipError_t prepare(uint32_t n, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, uint32_t wantedDepth,
                       uint32_t* inputError, hipStream_t stream)
    {
        const dim3 threads(256);
        const uint64_t recordCount = 2u * edgeCount;
        EM2_TRY(allocate(n, recordCount, wantedDepth, false));
        EM2_TRY(checkEdges(n, d_edge0, d_edge1, edgeCount, inputError, stream));
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

    template <bool kWeighted> hipError_t pyramidRepulsion(const float2* current, hipStream_t stream)
    {
        const dim3 threads(256);
        const uint32_t n = vertexCount, leafCount = 1u << (2u * depth);
        LayoutMoment* leaves = moment + layoutLevelBegin(depth);
        EM2_TRY(hipMemsetAsync(leaves, 0, size_t(leafCount) * sizeof(LayoutMoment) + 4u * sizeof(uint32_t), stream));
        boxKernel<<<dim3(gridFor(n) < kLayoutBoxBlocks ? gridFor(n) : kLayoutBoxBlocks), threads, 0, stream>>>(current, n, box);
        EM2_TRY(hipGetLastError());
        EM2_TRY(stage("box", stream));
        pyramidKeysKernel<kWeighted><<<dim3(gridFor(n)), threads, 0, stream>>>(current, mass, n, box, depth, vertexBits, pyramidKeys[0], leaves);
        EM2_TRY(hipGetLastError());
        DoubleBuffer<uint64_t> keys{pyramidKeys[0], pyramidKeys[1]};
        EM2_TRY(sortKeys(sortTemp, sortTempBytes, keys, size_t(n), 0u, vertexBits + 2u * depth, stream));
        pyramidGatherKernel<kWeighted><<<dim3(gridFor(n)), threads, 0, stream>>>(keys.current(), current, mass, n, depth, vertexBits,
                                                                                sortedPosition, sortedMass, leafBegin);
        EM2_TRY(hipGetLastError());
        EM2_TRY(stage("keys and sort", stream));
        // the leaf level (its ranges are the near field's), then the levels above it that the far field reads: down to 2
        for (uint32_t level = depth;; level--) {
            pyramidLevelKernel<kWeighted><<<dim3(gridFor(1u << (2u * level))), threads, 0, stream>>>(level, depth, box, moment, record,
                                                                                                    leafBegin, leafRange);
            EM2_TRY(hipGetLastError());
            if (level <= 2u) break;
        }
        EM2_TRY(stage("pyramid", stream));
        pyramidWalkKernel<kWeighted><<<dim3(chunkCount), dim3(kLayoutBlockVertices), 0, stream>>>(
            keys.current(), sortedPosition, sortedMass, n, depth, vertexBits, record, leafRange, partial);
        EM2_TRY(hipGetLastError());
        return stage("walk", stream);
    }

    // One evaluation at position[from]; the move goes to position[1 - from] where `move` is set, f to `force` where wanted.
    hipError_t evaluate(uint32_t from, float gravity, bool move, bool keepForce, hipStream_t stream)
    {
        return mass ? evaluateAs<true>(from, gravity, move, keepForce, stream) : evaluateAs<false>(from, gravity, move, keepForce, stream);
    }

    template <bool kWeighted> hipError_t evaluateAs(uint32_t from, float gravity, bool move, bool keepForce, hipStream_t stream)
    {
        const dim3 threads(kLayoutBlockVertices);
        float2* next = move ? position[1u - from] : nullptr;
        float2* kept = keepForce ? force : nullptr;
        if (pyramid) {
            EM2_TRY(pyramidRepulsion<kWeighted>(position[from], stream));
            forceKernel<1u, kWeighted><<<dim3(chunkCount), threads, 0, stream>>>(position[from], vertexCount, partial, offsets, neighbours, mass,
                                                                                neighbourWeights, gravity, state, next, kept, chunkEnergy);
        } else {
            repulsionKernel<kWeighted><<<dim3(chunkCount, kLayoutSliceCount), threads, 0, stream>>>(position[from], mass, vertexCount,
                                                                                                   sliceLength, partial);
            EM2_TRY(hipGetLastError());
            forceKernel<kLayoutSliceCount, kWeighted><<<dim3(chunkCount), threads, 0, stream>>>(
                position[from], vertexCount, partial, offsets, neighbours, mass, neighbourWeights, gravity, state, next, kept, chunkEnergy);
        }
        EM2_TRY(hipGetLastError());
        energyStepKernel<<<dim3(1), threads, 0, stream>>>(chunkEnergy, chunkCount, move, state);
        EM2_TRY(hipGetLastError());
        return pyramid ? stage("force", stream) : hipSuccess;
    }

    // Hu's adaptive iteration from position[from], at initialStep and an energy of +infinity, until maxIterationCount or
    // step < tolerance.  The positions stay on the device; the new step, one double, comes back after every iteration.
    // Afterwards position[from] holds the result, and the stream has been waited for.
    hipError_t iterate(const LayoutParameters& parameters, uint32_t& from, LayoutResult& result, hipStream_t stream)
    {
        LayoutState host;
        host.step = parameters.initialStep;
        host.energy = std::numeric_limits<double>::infinity();
        host.progress = host.unused = 0u;
        EM2_TRY(hipMemcpyAsync(state, &host, sizeof(host), hipMemcpyHostToDevice, stream));
        const float gravity = float(parameters.gravity);
        double step = parameters.initialStep;
        uint32_t iterations = 0;
        while (iterations < parameters.maxIterationCount && !(step < parameters.tolerance)) {
            EM2_TRY(evaluate(from, gravity, true, false, stream));
            EM2_TRY(hipMemcpyAsync(&step, &state->step, sizeof(double), hipMemcpyDeviceToHost, stream));
            EM2_TRY(hipStreamSynchronize(stream));
            from = 1u - from;
            iterations++;
        }
        EM2_TRY(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        result.iterationCount = iterations;
        result.step = host.step;
        result.energy = host.energy;
        return hipSuccess;
    }

    // One evaluation at the positions d_x / d_y, no move: d_fx / d_fy and *energy.  Synchronises the stream.
    hipError_t evaluateOnce(double gravity, const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy, hipStream_t stream)
    {
        LayoutState host;
        host.step = 0.;
        host.energy = std::numeric_limits<double>::infinity();
        host.progress = host.unused = 0u;
        EM2_TRY(hipMemcpyAsync(state, &host, sizeof(host), hipMemcpyHostToDevice, stream));
        packKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(d_x, d_y, vertexCount, position[0]);
        EM2_TRY(hipGetLastError());
        EM2_TRY(evaluate(0u, float(gravity), false, true, stream));
        unpackKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(force, vertexCount, d_fx, d_fy);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        *energy = host.energy;
        return hipSuccess;
    }
};

// One level of the multilevel layout, in device memory for the whole run: the masses, the merged edges with their weights, the
// adjacency over them (neighbours ascending and distinct), and, once the level has been coarsened, the matching and the map
// to the next level.  Two blocks: what is sized by the vertices, and what is sized by the edges.
struct LayoutLevel {
    CachedBuffer vertexArena, edgeArena;
    uint32_t vertexCount = 0;
    uint64_t edgeCount = 0;
    uint32_t rounds = 0;                            // of the matching that made this level from the one below it
    uint32_t* mass = nullptr;
    uint32_t* mate = nullptr;
    uint32_t* coarseOf = nullptr;
    uint64_t* offsets = nullptr;
    uint32_t* edge0 = nullptr;
    uint32_t* edge1 = nullptr;
    uint32_t* edgeWeight = nullptr;
    uint32_t* neighbours = nullptr;
    uint32_t* neighbourWeights = nullptr;

    void idle() { vertexArena.idle = edgeArena.idle = true; }

    hipError_t allocateVertices(uint32_t n)
    {
        vertexCount = n;
        ArenaPlan plan;
        const size_t offMass = plan.takeFor<uint32_t>(n), offMate = plan.takeFor<uint32_t>(n), offCoarse = plan.takeFor<uint32_t>(n);
        const size_t offOffsets = plan.takeFor<uint64_t>(size_t(n) + 1u);
        EM2_TRY(vertexArena.allocate(plan.bytes));
        char* base = vertexArena.as<char>();
        mass = arenaAt<uint32_t>(base, offMass);
        mate = arenaAt<uint32_t>(base, offMate);
        coarseOf = arenaAt<uint32_t>(base, offCoarse);
        offsets = arenaAt<uint64_t>(base, offOffsets);
        return hipSuccess;
    }

    // Room for at most `capacity` merged edges.
    hipError_t allocateEdges(uint64_t capacity)
    {
        ArenaPlan plan;
        const size_t off0 = plan.takeFor<uint32_t>(capacity), off1 = plan.takeFor<uint32_t>(capacity), offWeight = plan.takeFor<uint32_t>(capacity);
        const size_t offNeighbours = plan.takeFor<uint32_t>(2u * capacity), offNeighbourWeights = plan.takeFor<uint32_t>(2u * capacity);
        EM2_TRY(edgeArena.allocate(plan.bytes));
        char* base = edgeArena.as<char>();
        edge0 = arenaAt<uint32_t>(base, off0);
        edge1 = arenaAt<uint32_t>(base, off1);
        edgeWeight = arenaAt<uint32_t>(base, offWeight);
        neighbours = arenaAt<uint32_t>(base, offNeighbours);
        neighbourWeights = arenaAt<uint32_t>(base, offNeighbourWeights);
        return hipSuccess;
    }
};

// offsets / neighbours / neighbourWeights of the graph of n vertices and the edges (edge0, edge1, weight; weight null: 1), as
// LayoutWork::prepare builds the unweighted one: two records per edge, one stable radix sort of (key, weight) pairs, a search.
// Synchronises the stream (the scratch goes back to the cache).
hipError_t buildWeightedAdjacency(uint32_t n, const uint32_t* edge0, const uint32_t* edge1, const uint32_t* weight, uint64_t edgeCount,
                                  uint64_t* offsets, uint32_t* neighbours, uint32_t* neighbourWeights, hipStream_t stream)
{
    const dim3 threads(256);
    const uint64_t recordCount = 2u * edgeCount;
    CachedBuffer scratch;
    const uint64_t* sortedKeys = nullptr;
    const uint32_t* sortedValues = nullptr;
    if (recordCount) {
        ArenaPlan plan;
        const size_t offKeysA = plan.takeFor<uint64_t>(recordCount), offKeysB = plan.takeFor<uint64_t>(recordCount);
        const size_t offValuesA = plan.takeFor<uint32_t>(recordCount), offValuesB = plan.takeFor<uint32_t>(recordCount);
        size_t sortBytes = 0;
        EM2_TRY(sortPairsU64U32BufferBytes(size_t(recordCount), 0u, 64u, sortBytes));
        const size_t offSortTemp = plan.take(sortBytes);
        EM2_TRY(scratch.allocate(plan.bytes));
        char* base = scratch.as<char>();
        DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, offKeysA), arenaAt<uint64_t>(base, offKeysB)};
        DoubleBuffer<uint32_t> values{arenaAt<uint32_t>(base, offValuesA), arenaAt<uint32_t>(base, offValuesB)};
        weightedRecordsKernel<<<dim3(gridFor(edgeCount)), threads, 0, stream>>>(edge0, edge1, weight, edgeCount, keys.current(), values.current());
        EM2_TRY(hipGetLastError());
        EM2_TRY(sortPairs(base + offSortTemp, sortBytes, keys, values, size_t(recordCount), 0u, 64u, stream));
        sortedKeys = keys.current();
        sortedValues = values.current();
    }
    weightedOffsetsKernel<<<dim3(gridFor(recordCount > n ? recordCount : uint64_t(n) + 1u)), threads, 0, stream>>>(
        sortedKeys, sortedValues, recordCount, n, offsets, neighbours, neighbourWeights);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    scratch.idle = true;
    return hipSuccess;
}

// The merged edges of `level` (its vertices are allocated) from the edges (edge0, edge1, weight; weight null: 1) with their
// ends mapped through `map` (null: as they are), and the adjacency over them.  Every end, mapped, is below level.vertexCount.
hipError_t buildLevelEdges(LayoutLevel& level, const uint32_t* edge0, const uint32_t* edge1, const uint32_t* weight, uint64_t edgeCount,
                           const uint32_t* map, hipStream_t stream)
{
    const dim3 threads(256);
    EM2_TRY(level.allocateEdges(edgeCount));
    level.edgeCount = 0;
    if (edgeCount) {
        CachedBuffer scratch;
        ArenaPlan plan;
        const size_t offKeysA = plan.takeFor<uint64_t>(edgeCount), offKeysB = plan.takeFor<uint64_t>(edgeCount);
        const size_t offValuesA = plan.takeFor<uint32_t>(edgeCount), offValuesB = plan.takeFor<uint32_t>(edgeCount);
        const size_t offFlags = plan.takeFor<uint32_t>(edgeCount), offScan = plan.takeFor<uint32_t>(edgeCount);
        const size_t offCount = plan.take(sizeof(uint64_t));
        size_t sortBytes = 0, scanBytes = 0;
        EM2_TRY(sortPairsU64U32BufferBytes(size_t(edgeCount), 0u, 64u, sortBytes));
        EM2_TRY(inclusiveScanBytes(size_t(edgeCount), scanBytes));
        const size_t offSortTemp = plan.take(sortBytes), offScanTemp = plan.take(scanBytes);
        EM2_TRY(scratch.allocate(plan.bytes));
        char* base = scratch.as<char>();
        DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, offKeysA), arenaAt<uint64_t>(base, offKeysB)};
        DoubleBuffer<uint32_t> values{arenaAt<uint32_t>(base, offValuesA), arenaAt<uint32_t>(base, offValuesB)};
        uint32_t* flags = arenaAt<uint32_t>(base, offFlags);
        uint32_t* scan = arenaAt<uint32_t>(base, offScan);
        uint64_t* mergedCount = arenaAt<uint64_t>(base, offCount);
        const dim3 grid(gridFor(edgeCount));
        mergeKeysKernel<<<grid, threads, 0, stream>>>(edge0, edge1, weight, edgeCount, map, keys.current(), values.current());
        EM2_TRY(hipGetLastError());
        EM2_TRY(sortPairs(base + offSortTemp, sortBytes, keys, values, size_t(edgeCount), 0u, 64u, stream));
        headFlagsKernel<<<grid, threads, 0, stream>>>(keys.current(), edgeCount, flags);
        EM2_TRY(hipGetLastError());
        EM2_TRY(inclusiveScan(base + offScanTemp, scanBytes, flags, scan, size_t(edgeCount), stream));
        EM2_TRY(hipMemsetAsync(level.edgeWeight, 0, size_t(edgeCount) * sizeof(uint32_t), stream));
        mergeRunsKernel<<<grid, threads, 0, stream>>>(keys.current(), values.current(), flags, scan, edgeCount, level.edge0, level.edge1,
                                                     level.edgeWeight, mergedCount);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(&level.edgeCount, mergedCount, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        scratch.idle = true;
    }
    return buildWeightedAdjacency(level.vertexCount, level.edge0, level.edge1, level.edgeWeight, level.edgeCount, level.offsets,
                                  level.neighbours, level.neighbourWeights, stream);
}

// One coarsening step: the matching of `fine` by rounds of locally dominant edges (one counter comes back per round), the
// groups, and `coarse` with its masses, edges and adjacency.  fine.mate and fine.coarseOf are filled.
hipError_t coarsenLevel(LayoutLevel& fine, uint32_t seed, uint32_t levelIndex, LayoutLevel& coarse, hipStream_t stream)
{
    const dim3 threads(256);
    const uint32_t n = fine.vertexCount;
    const dim3 grid(gridFor(n));
    CachedBuffer scratch;
    ArenaPlan plan;
    const size_t offPointer = plan.takeFor<uint32_t>(n), offFlags = plan.takeFor<uint32_t>(n), offScan = plan.takeFor<uint32_t>(n);
    const size_t offMass = plan.takeFor<uint32_t>(n), offCounter = plan.take(sizeof(uint32_t));
    size_t scanBytes = 0;
    EM2_TRY(exclusiveScanU32Bytes(size_t(n), scanBytes));
    const size_t offScanTemp = plan.take(scanBytes);
    EM2_TRY(scratch.allocate(plan.bytes));
    char* base = scratch.as<char>();
    uint32_t* pointer = arenaAt<uint32_t>(base, offPointer);
    uint32_t* flags = arenaAt<uint32_t>(base, offFlags);
    uint32_t* scan = arenaAt<uint32_t>(base, offScan);
    uint32_t* coarseMass = arenaAt<uint32_t>(base, offMass);
    uint32_t* counter = arenaAt<uint32_t>(base, offCounter);

    const uint64_t salt = layoutMix(uint64_t(seed) << 32 | levelIndex);
    EM2_TRY(hipMemsetAsync(fine.mate, 0xff, size_t(n) * sizeof(uint32_t), stream));
    coarse.rounds = 0;
    for (;;) {
        uint32_t live = 0;
        EM2_TRY(hipMemsetAsync(counter, 0, sizeof(uint32_t), stream));
        matchPointKernel<<<grid, threads, 0, stream>>>(n, fine.offsets, fine.neighbours, fine.neighbourWeights, fine.mate, salt, pointer, counter);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(&live, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (!live) break;
        // (the best live edge of all is dominant at both of its ends, so every round matches a pair: at most n / 2 rounds)
        matchPairKernel<<<grid, threads, 0, stream>>>(n, pointer, fine.mate);
        EM2_TRY(hipGetLastError());
        if (++coarse.rounds > n) return hipErrorUnknown;         // (cannot be: the loop must not depend on that)
    }

    uint32_t coarseCount = 0;
    groupFlagsKernel<<<grid, threads, 0, stream>>>(n, fine.mate, flags);
    EM2_TRY(hipGetLastError());
    EM2_TRY(exclusiveScan(base + offScanTemp, scanBytes, flags, scan, size_t(n), stream));
    groupMapKernel<<<grid, threads, 0, stream>>>(n, fine.mate, flags, scan, fine.mass, fine.coarseOf, coarseMass, counter);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(&coarseCount, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(coarse.allocateVertices(coarseCount));
    EM2_TRY(hipMemcpyAsync(coarse.mass, coarseMass, size_t(coarseCount) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    EM2_TRY(buildLevelEdges(coarse, fine.edge0, fine.edge1, fine.edgeWeight, fine.edgeCount, fine.coarseOf, stream));
    scratch.idle = true;                                        // (buildLevelEdges has waited for the stream)
    return hipSuccess;
}

// Level 0 of a graph whose edge ends have been checked: the masses (null: 1) and the merged edges.
hipError_t buildFinestLevel(LayoutLevel& level, uint32_t n, const uint32_t* d_mass, const uint32_t* d_edge0, const uint32_t* d_edge1,
                            const uint32_t* d_weight, uint64_t edgeCount, hipStream_t stream)
{
    EM2_TRY(level.allocateVertices(n));
    if (d_mass) {
        EM2_TRY(hipMemcpyAsync(level.mass, d_mass, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    } else {
        fillKernel<<<dim3(gridFor(n)), dim3(256), 0, stream>>>(level.mass, n, 1u);
        EM2_TRY(hipGetLastError());
    }
    return buildLevelEdges(level, d_edge0, d_edge1, d_weight, edgeCount, nullptr, stream);
}

// What a level of n vertices evaluates its repulsion with, from the entry's depth argument: level 0 is the single-level
// entry of that argument; under kLayoutDepthAuto a coarse level of at most kLayoutExactLimit vertices is exact.
uint32_t depthOfLevel(uint32_t depth, uint32_t level, uint32_t n)
{
    if (depth == kLayoutDepthAuto && level > 0u && n <= kLayoutExactLimit) return kLayoutDepthExact;
    return depth;
}

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

    initialKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(parameters.seed, vertexCount, sqrtf(float(vertexCount)),
                                                                       work.position[0]);
    EM2_TRY(hipGetLastError());
    uint32_t from = 0;
    EM2_TRY(work.iterate(parameters, from, result, stream));
    EM2_TRY(timer.stage("iterations", stream));

    unpackKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(work.position[from], vertexCount, d_x, d_y);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
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
    EM2_TRY(work.evaluateOnce(gravity, d_x, d_y, d_fx, d_fy, energy, stream));
    work.idle();
    return hipSuccess;
}

// The multilevel layout: the levels by matching and contraction until the stop rule, the coarsest level from
// the hashed start positions, then level by level down to level 0, each from the prolonged positions of the one above, at
// initialStep and with the whole iteration budget.  Level 0 runs the unweighted kernels on the input as it is.  depth as
// runGraphLayout takes it.  result: the iterations of all levels, the step and energy of level 0's end.  levels: what was done.
static hipError_t runGraphLayoutMultilevel(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                                    const LayoutParameters& parameters, uint32_t depth, float* d_x, float* d_y, LayoutResult& result,
                                    em2_layout_levels& report, uint32_t* inputError, hipStream_t stream)
{
    StageTimer timer("graphLayoutMultilevel");
    const dim3 threads(256);
    LayoutWork finest;
    EM2_TRY(finest.prepare(vertexCount, d_edge0, d_edge1, edgeCount, depthOfLevel(depth, 0u, vertexCount), inputError, stream));
    if (*inputError) {
        finest.idle();
        return hipSuccess;
    }

    std::vector<std::unique_ptr<LayoutLevel>> levels;
    levels.emplace_back(new LayoutLevel);
    EM2_TRY(buildFinestLevel(*levels[0], vertexCount, nullptr, d_edge0, d_edge1, nullptr, edgeCount, stream));
    while (levels.back()->vertexCount > kLayoutCoarsest && levels.size() < kLayoutMaxLevels) {
        std::unique_ptr<LayoutLevel> next(new LayoutLevel);
        LayoutLevel& fine = *levels.back();
        EM2_TRY(coarsenLevel(fine, parameters.seed, uint32_t(levels.size() - 1u), *next, stream));
        const bool shrinks = 4ull * next->vertexCount <= 3ull * fine.vertexCount;
        if (!shrinks) {
            next->idle();                                       // (coarsenLevel has waited for the stream)
            break;
        }
        levels.push_back(std::move(next));
    }
    EM2_TRY(timer.stage("levels", stream));

    const uint32_t last = uint32_t(levels.size() - 1u);
    std::unique_ptr<LayoutWork> above;                          // the work of the level above the current one, whose positions it holds
    uint32_t aboveFrom = 0, total = 0;
    memset(&report, 0, sizeof(report));
    report.levelCount = uint32_t(levels.size());
    for (uint32_t l = last;; l--) {
        LayoutLevel& level = *levels[l];
        std::unique_ptr<LayoutWork> own;
        LayoutWork* work = &finest;
        if (l > 0u) {
            own.reset(new LayoutWork);
            work = own.get();
            EM2_TRY(work->allocate(level.vertexCount, 0u, depthOfLevel(depth, l, level.vertexCount), true, false));
            work->borrowGraph(level.offsets, level.neighbours, level.neighbourWeights, level.mass);
        }
        const dim3 grid(gridFor(level.vertexCount));
        if (l == last) {
            initialKernel<<<grid, threads, 0, stream>>>(parameters.seed, level.vertexCount, sqrtf(float(vertexCount)), work->position[0]);
        } else {
            prolongKernel<<<grid, threads, 0, stream>>>(level.vertexCount, level.mate, level.coarseOf, levels[l + 1u]->vertexCount,
                                                       above->position[aboveFrom], layoutMix(uint64_t(parameters.seed) << 32 | l),
                                                       work->position[0]);
        }
        EM2_TRY(hipGetLastError());
        if (above) {
            EM2_TRY(hipStreamSynchronize(stream));
            above->idle();
            above.reset();
        }
        uint32_t from = 0;
        LayoutResult levelResult;
        EM2_TRY(work->iterate(parameters, from, levelResult, stream));
        report.vertexCount[l] = level.vertexCount;
        report.edgeCount[l] = level.edgeCount;
        report.matchingRounds[l] = level.rounds;
        report.iterationCount[l] = levelResult.iterationCount;
        total += levelResult.iterationCount;
        EM2_TRY(timer.stage(("level " + std::to_string(l)).c_str(), stream));
        if (l == 0u) {
            result = levelResult;
            result.iterationCount = total;
            unpackKernel<<<grid, threads, 0, stream>>>(finest.position[from], vertexCount, d_x, d_y);
            EM2_TRY(hipGetLastError());
            EM2_TRY(hipStreamSynchronize(stream));
            break;
        }
        above = std::move(own);
        aboveFrom = from;
    }
    for (auto& level : levels) level->idle();
    finest.idle();
    return hipSuccess;
}

// For tests: one coarsening step of the graph (d_mass, d_weight null: 1) at `level`.  The outputs in device memory: d_mate,
// d_coarseOf, d_coarseMass [vertexCount], d_coarseEdge0 / 1 / Weight [edgeCount]; counts: the coarse vertices, the rounds,
// the coarse edges.
static hipError_t runGraphLayoutCoarsen(uint32_t vertexCount, const uint32_t* d_mass, const uint32_t* d_edge0, const uint32_t* d_edge1,
                                 const uint32_t* d_weight, uint64_t edgeCount, uint32_t seed, uint32_t level, uint32_t* d_mate,
                                 uint32_t* d_coarseOf, uint32_t* d_coarseMass, uint32_t* d_coarseEdge0, uint32_t* d_coarseEdge1,
                                 uint32_t* d_coarseWeight, uint64_t counts[3], uint32_t* inputError, hipStream_t stream)
{
    LayoutWork check;
    EM2_TRY(check.allocate(1u, 0u, kLayoutDepthExact, false, false));   // (for its error word)
    EM2_TRY(check.checkEdges(vertexCount, d_edge0, d_edge1, edgeCount, inputError, stream));
    check.idle();
    if (*inputError) return hipSuccess;
    LayoutLevel fine, coarse;
    EM2_TRY(buildFinestLevel(fine, vertexCount, d_mass, d_edge0, d_edge1, d_weight, edgeCount, stream));
    EM2_TRY(coarsenLevel(fine, seed, level, coarse, stream));
    const size_t word = sizeof(uint32_t);
    EM2_TRY(hipMemcpyAsync(d_mate, fine.mate, vertexCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipMemcpyAsync(d_coarseOf, fine.coarseOf, vertexCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipMemcpyAsync(d_coarseMass, coarse.mass, coarse.vertexCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipMemcpyAsync(d_coarseEdge0, coarse.edge0, coarse.edgeCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipMemcpyAsync(d_coarseEdge1, coarse.edge1, coarse.edgeCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipMemcpyAsync(d_coarseWeight, coarse.edgeWeight, coarse.edgeCount * word, hipMemcpyDeviceToDevice, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    counts[0] = coarse.vertexCount;
    counts[1] = coarse.rounds;
    counts[2] = coarse.edgeCount;
    fine.idle();
    coarse.idle();
    return hipSuccess;
}

// For tests: one evaluation with masses and weighted edges (d_mass, d_weight null: 1) through the weighted kernels.  The
// edges are taken as they are: two entries of a vertex for the same neighbour stay two, in the order of the edges.
static hipError_t runGraphLayoutForcesWeighted(uint32_t vertexCount, const uint32_t* d_mass, const uint32_t* d_edge0, const uint32_t* d_edge1,
                                        const uint32_t* d_weight, uint64_t edgeCount, double gravity, uint32_t depth, const float* d_x,
                                        const float* d_y, float* d_fx, float* d_fy, double* energy, uint32_t* inputError, hipStream_t stream)
{
    LayoutWork work;
    EM2_TRY(work.allocate(vertexCount, 2u * edgeCount, depth, true));
    EM2_TRY(work.checkEdges(vertexCount, d_edge0, d_edge1, edgeCount, inputError, stream));
    if (*inputError) {
        work.idle();
        return hipSuccess;
    }
    CachedBuffer extra;
    ArenaPlan plan;
    const size_t offMass = plan.takeFor<uint32_t>(vertexCount), offWeights = plan.takeFor<uint32_t>(2u * edgeCount);
    EM2_TRY(extra.allocate(plan.bytes));
    uint32_t* mass = arenaAt<uint32_t>(extra.p, offMass);
    uint32_t* neighbourWeights = arenaAt<uint32_t>(extra.p, offWeights);
    if (d_mass) {
        EM2_TRY(hipMemcpyAsync(mass, d_mass, size_t(vertexCount) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    } else {
        fillKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(mass, vertexCount, 1u);
        EM2_TRY(hipGetLastError());
    }
    EM2_TRY(buildWeightedAdjacency(vertexCount, d_edge0, d_edge1, d_weight, edgeCount, work.offsets, work.neighbours, neighbourWeights, stream));
    work.mass = mass;
    work.neighbourWeights = neighbourWeights;
    EM2_TRY(work.evaluateOnce(gravity, d_x, d_y, d_fx, d_fy, energy, stream));
    work.idle();
    extra.idle = true;
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

static int graphLayoutMultilevel(const char* who, bool onDevice, uint32_t vertexCount, const uint32_t* edgeVertex0,
                                 const uint32_t* edgeVertex1, uint64_t edgeCount, const em2_layout_parameters* parameters, uint32_t depth,
                                 float* x, float* y, em2_layout_result* result, em2_layout_levels* levels)
{
    if (!parameters || (vertexCount && (!x || !y)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(parameters->tolerance >= 0.)) return failArgument(who, "tolerance must not be negative");
    if (!(parameters->gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (!(parameters->initialStep >= 0.)) return failArgument(who, "initialStep must not be negative");
    if (depth != em2::kLayoutDepthExact && !depthIsValid(depth)) return failArgument(who, kDepthText);
    if (vertexCount > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": vertexCount is above 2^30");
    if (edgeCount >> 32) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": edgeCount is 2^32 or more");
    em2_layout_levels report;
    memset(&report, 0, sizeof(report));
    em2::LayoutResult r;
    r.step = parameters->initialStep;
    r.energy = std::numeric_limits<double>::infinity();
    if (vertexCount == 0) {
        if (edgeCount) return failArgument(who, "an edge names a vertex outside the graph");
    } else {
        if (!haveDevice()) return failNoDevice(who);
        DeviceBuffer d0, d1, dx, dy;
        if (!onDevice) {
            const int status = uploadEdges(edgeVertex0, edgeVertex1, edgeCount, d0, d1);
            if (status != EM2_OK) return status;
        }
        // (also for the device entry: a run that fails half-way must not have written the caller's arrays)
        EM2_HIP(dx.allocateFor<float>(vertexCount));
        EM2_HIP(dy.allocateFor<float>(vertexCount));
        const em2::LayoutParameters p = {parameters->seed, parameters->maxIterationCount, parameters->tolerance, parameters->gravity,
                                         parameters->initialStep};
        uint32_t inputError = 0;
        EM2_HIP(em2::runGraphLayoutMultilevel(vertexCount, onDevice ? edgeVertex0 : d0.as<uint32_t>(), onDevice ? edgeVertex1 : d1.as<uint32_t>(),
                                              edgeCount, p, depth, dx.as<float>(), dy.as<float>(), r, report, &inputError, nullptr));
        if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
        if (onDevice) {
            EM2_HIP(hipMemcpy(x, dx.p, size_t(vertexCount) * sizeof(float), hipMemcpyDeviceToDevice));
            EM2_HIP(hipMemcpy(y, dy.p, size_t(vertexCount) * sizeof(float), hipMemcpyDeviceToDevice));
        } else {
            EM2_HIP(dx.download(x, vertexCount));
            EM2_HIP(dy.download(y, vertexCount));
        }
    }
    if (result) {
        result->iterationCount = r.iterationCount;
        result->reserved = 0u;
        result->step = r.step;
        result->energy = r.energy;
    }
    if (levels) *levels = report;
    return EM2_OK;
}

int em2_graph_layout_multilevel(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                                const em2_layout_parameters* parameters, uint32_t depth, float* x, float* y, em2_layout_result* result,
                                em2_layout_levels* levels)
{
    return graphLayoutMultilevel("em2_graph_layout_multilevel", false, vertexCount, edgeVertex0, edgeVertex1, edgeCount, parameters, depth, x,
                                 y, result, levels);
}

int em2_dev_graph_layout_multilevel(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                                    const em2_layout_parameters* parameters, uint32_t depth, float* d_x, float* d_y,
                                    em2_layout_result* result, em2_layout_levels* levels)
{
    return graphLayoutMultilevel("em2_dev_graph_layout_multilevel", true, vertexCount, d_edgeVertex0, d_edgeVertex1, edgeCount, parameters,
                                 depth, d_x, d_y, result, levels);
}

// The masses and weights of a test entry: each mass >= 1, their sum at most 2^30; the weights' sum below 2^32.
static int checkMassesAndWeights(const char* who, uint32_t vertexCount, const uint32_t* mass, const uint32_t* edgeWeight, uint64_t edgeCount)
{
    uint64_t massSum = 0, weightSum = 0;
    for (uint32_t v = 0; mass && v < vertexCount; v++) {
        if (!mass[v]) return failArgument(who, "a mass is 0");
        massSum += mass[v];
    }
    for (uint64_t e = 0; e < edgeCount; e++) weightSum += edgeWeight ? edgeWeight[e] : 1u;
    if (massSum > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": the masses sum to more than 2^30");
    if (weightSum >> 32) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": the edge weights sum to 2^32 or more");
    return EM2_OK;
}

int em2_graph_layout_coarsen(uint32_t vertexCount, const uint32_t* mass, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                             const uint32_t* edgeWeight, uint64_t edgeCount, uint32_t seed, uint32_t level, uint32_t* mate,
                             uint32_t* coarseOf, uint32_t* coarseVertexCount, uint32_t* matchingRounds, uint32_t* coarseMass,
                             uint32_t* coarseEdge0, uint32_t* coarseEdge1, uint32_t* coarseWeight, uint64_t* coarseEdgeCount)
{
    const char* who = "em2_graph_layout_coarsen";
    if (!mate || !coarseOf || !coarseVertexCount || !matchingRounds || !coarseMass || !coarseEdgeCount ||
        (edgeCount && (!edgeVertex0 || !edgeVertex1 || !coarseEdge0 || !coarseEdge1 || !coarseWeight))) {
        return failNull(who);
    }
    if (vertexCount == 0) return failArgument(who, "vertexCount must not be 0");
    if (vertexCount > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": vertexCount is above 2^30");
    const int checked = checkMassesAndWeights(who, vertexCount, mass, edgeWeight, edgeCount);
    if (checked != EM2_OK) return checked;
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer d0, d1, dMass, dWeight, dMate, dCoarseOf, dCoarseMass, dC0, dC1, dCw;
    const int status = uploadEdges(edgeVertex0, edgeVertex1, edgeCount, d0, d1);
    if (status != EM2_OK) return status;
    if (mass) EM2_HIP(dMass.upload(mass, vertexCount));
    if (edgeWeight) EM2_HIP(dWeight.upload(edgeWeight, size_t(edgeCount)));
    EM2_HIP(dMate.allocateFor<uint32_t>(vertexCount));
    EM2_HIP(dCoarseOf.allocateFor<uint32_t>(vertexCount));
    EM2_HIP(dCoarseMass.allocateFor<uint32_t>(vertexCount));
    EM2_HIP(dC0.allocateFor<uint32_t>(size_t(edgeCount)));
    EM2_HIP(dC1.allocateFor<uint32_t>(size_t(edgeCount)));
    EM2_HIP(dCw.allocateFor<uint32_t>(size_t(edgeCount)));
    uint32_t inputError = 0;
    uint64_t counts[3] = {0, 0, 0};
    EM2_HIP(em2::runGraphLayoutCoarsen(vertexCount, mass ? dMass.as<uint32_t>() : nullptr, d0.as<uint32_t>(), d1.as<uint32_t>(),
                                       edgeWeight ? dWeight.as<uint32_t>() : nullptr, edgeCount, seed, level, dMate.as<uint32_t>(),
                                       dCoarseOf.as<uint32_t>(), dCoarseMass.as<uint32_t>(), dC0.as<uint32_t>(), dC1.as<uint32_t>(),
                                       dCw.as<uint32_t>(), counts, &inputError, nullptr));
    if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
    EM2_HIP(dMate.download(mate, vertexCount));
    EM2_HIP(dCoarseOf.download(coarseOf, vertexCount));
    EM2_HIP(dCoarseMass.download(coarseMass, size_t(counts[0])));
    EM2_HIP(dC0.download(coarseEdge0, size_t(counts[2])));
    EM2_HIP(dC1.download(coarseEdge1, size_t(counts[2])));
    EM2_HIP(dCw.download(coarseWeight, size_t(counts[2])));
    *coarseVertexCount = uint32_t(counts[0]);
    *matchingRounds = uint32_t(counts[1]);
    *coarseEdgeCount = counts[2];
    return EM2_OK;
}

int em2_graph_layout_forces_weighted(uint32_t vertexCount, const uint32_t* mass, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                                     const uint32_t* edgeWeight, uint64_t edgeCount, double gravity, uint32_t depth, const float* x,
                                     const float* y, float* fx, float* fy, double* energy)
{
    const char* who = "em2_graph_layout_forces_weighted";
    if ((vertexCount && (!x || !y || !fx || !fy)) || (edgeCount && (!edgeVertex0 || !edgeVertex1))) return failNull(who);
    if (!(gravity >= 0.)) return failArgument(who, "gravity must not be negative");
    if (depth != em2::kLayoutDepthExact && !depthIsValid(depth)) return failArgument(who, kDepthText);
    if (vertexCount > em2::kLayoutMaxVertexCount) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": vertexCount is above 2^30");
    const int checked = checkMassesAndWeights(who, vertexCount, mass, edgeWeight, edgeCount);
    if (checked != EM2_OK) return checked;
    if (vertexCount == 0) {
        if (edgeCount) return failArgument(who, "an edge names a vertex outside the graph");
        if (energy) *energy = 0.;
        return EM2_OK;
    }
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer d0, d1, dMass, dWeight, dx, dy, dfx, dfy;
    const int status = uploadEdges(edgeVertex0, edgeVertex1, edgeCount, d0, d1);
    if (status != EM2_OK) return status;
    if (mass) EM2_HIP(dMass.upload(mass, vertexCount));
    if (edgeWeight) EM2_HIP(dWeight.upload(edgeWeight, size_t(edgeCount)));
    EM2_HIP(dx.upload(x, vertexCount));
    EM2_HIP(dy.upload(y, vertexCount));
    EM2_HIP(dfx.allocateFor<float>(vertexCount));
    EM2_HIP(dfy.allocateFor<float>(vertexCount));
    uint32_t inputError = 0;
    double e = 0.;
    EM2_HIP(em2::runGraphLayoutForcesWeighted(vertexCount, mass ? dMass.as<uint32_t>() : nullptr, d0.as<uint32_t>(), d1.as<uint32_t>(),
                                              edgeWeight ? dWeight.as<uint32_t>() : nullptr, edgeCount, gravity, depth, dx.as<float>(),
                                              dy.as<float>(), dfx.as<float>(), dfy.as<float>(), &e, &inputError, nullptr));
    if (inputError) return failArgument(who, "an edge names a vertex outside the graph");
    EM2_HIP(dfx.download(fx, vertexCount));
    EM2_HIP(dfy.download(fy, vertexCount));
    if (energy) *energy = e;
    return EM2_OK;
}

}  // extern "C"
