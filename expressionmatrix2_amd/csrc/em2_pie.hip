// em2_pie.hip -- the device code of the signature graph's picture (the definitions are in include/em2_lsh.h).
//
// The colour census (ExpressionMatrix::colorByMetaDataInterpretedAsCategory, src/ExpressionMatrixSignatureGraph.cpp:230-262):
// per vertex the cells of each of the 13 colour indices, the colours that occur ordered by count descending and then by first
// occurrence, and every count as a fraction of the vertex's cells.
//   * censusLaneKernel   a lane per vertex of at most kPieWaveCells cells: 13 counters and 13 first positions in registers (every
//                        loop over the colours is unrolled, so no array is indexed by a run-time value); a vertex of more cells
//                        goes to a list;
//   * censusWaveKernel   a wave per listed vertex: 64 cells at a time, per colour a ballot, its population count and, the first
//                        time the colour shows, its lowest set lane.  The tallies are the same in every lane; lane 0 writes.
//   Both run twice: once for the number of slices per vertex, then, after a scan of those numbers, to fill the slices.  The rank
//   of a colour among the vertex's slices is the number of colours that come before it, counted directly: no sort.
//   Every id is tested before an address is formed with it; the count pass raises the error word, and nothing is written for an
//   input that fails.  A vertex of 10^6 cells is worked by one wave, 64 cells per step: a known limit.
//
// The raster with pies: em2_graph_draw's view, subpixels, checks and edge layer (em2_draw.h), then
//   * pieClassifyKernel  R_v = llround(radius[v] * s256), the checks of the radii and the slice offsets, and the vertices compacted
//                        into three lists by radius class (a ballot per class, one atomic per wave and class);
//   * pieVerticesKernel  1, 64 or 256 lanes per listed vertex stride over the pixels of its bounding box inside the image;
//   * pieSlicesKernel    a thread per pixel, once vertexTop is final: the slice of the top vertex that holds the pixel's centre,
//                        by cross products of 64-bit integers.
// Maximum and integer addition do not depend on the order of their operands; the order of the lists does depend on how the
// threads run, and nothing reads it but the kernels that work every member.

#include "em2_device.h"
#include "em2_draw.h"
#include "em2_entry.h"
#include "em2_hip_util.h"
#include "em2_pie.h"
#include "em2_primitives.h"
#include "em2_wave.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace em2 {
namespace {

constexpr uint32_t kPieColors = 13;                // 12 palette colours and "black"
constexpr uint32_t kPieWaveCells = 32;             // a vertex of more cells gets a wave
constexpr int64_t kPieLaneRadius = 4 * 256;        // a lane per vertex up to 4 pixels, as em2_graph_draw
constexpr int64_t kPieWaveRadius = 32 * 256;       // a wave per vertex up to 32 pixels, a workgroup above
constexpr double kPieMaxRadiusPixels = 8192.;

constexpr uint32_t kBadRadius = 4u;                // (1 and 2 are the prepare kernel's)
constexpr uint32_t kBadSlices = 8u;

struct PieCensusInput {
    const uint64_t* cellOffsets;       // [vertexCount + 1]
    const uint32_t* cells;             // [cellCount]
    uint64_t cellCount;
    const uint32_t* idOfCell;          // [cellSetSize]
    uint32_t cellSetSize;
    const uint8_t* colorOfValue;       // [valueCount]
    uint32_t valueCount;
    uint32_t vertexCount;
};

struct PieCensusOutput {
    uint32_t* sliceCount;              // the count pass: [vertexCount]
    const uint64_t* sliceOffsets;      // the fill pass
    uint8_t* sliceColor;
    uint32_t* sliceCells;
    double* sliceFraction;
};

struct PieTally {
    uint32_t count[kPieColors];
    uint32_t first[kPieColors];
};

// The colour index of cells[i]; kPieColors, which matches no colour, and `bad` set where an id is out of range.
__device__ __forceinline__ uint32_t colorOfCell(const PieCensusInput& in, uint64_t i, bool& bad)
{
    const uint32_t cell = in.cells[i];
    if (cell < in.cellSetSize) {
        const uint32_t id = in.idOfCell[cell];
        if (id < in.valueCount) {
            const uint32_t color = in.colorOfValue[id];
            if (color < kPieColors) return color;
        }
    }
    bad = true;
    return kPieColors;
}

// The cells [begin, end) of vertex v, or false and `bad` set where the offsets do not ascend or leave cells[].
__device__ __forceinline__ bool cellsOfVertex(const PieCensusInput& in, uint32_t v, uint64_t& begin, uint64_t& end, bool& bad)
{
    begin = in.cellOffsets[v];
    end = in.cellOffsets[v + 1u];
    if (begin <= end && end <= in.cellCount) return true;
    bad = true;
    return false;
}

template <bool Fill>
__device__ __forceinline__ void emitSlices(const PieTally& t, uint32_t v, const PieCensusOutput& out)
{
    uint32_t slices = 0u;
    uint64_t sum = 0u;
#pragma unroll
    for (uint32_t c = 0; c < kPieColors; ++c) {
        slices += t.count[c] ? 1u : 0u;
        sum += t.count[c];
    }
    if (!Fill) {
        out.sliceCount[v] = slices;
        return;
    }
    if (!slices) return;
    const double factor = __ddiv_rn(1., double(sum));                  // :258
    const uint64_t base = out.sliceOffsets[v];
#pragma unroll
    for (uint32_t c = 0; c < kPieColors; ++c) {
        if (!t.count[c]) continue;
        uint32_t rank = 0u;                                            // the colours std::sort leaves before this one (:251)
#pragma unroll
        for (uint32_t o = 0; o < kPieColors; ++o) {
            if (t.count[o] > t.count[c] || (t.count[o] == t.count[c] && t.count[o] && t.first[o] < t.first[c])) ++rank;
        }
        out.sliceColor[base + rank] = uint8_t(c);
        out.sliceCells[base + rank] = t.count[c];
        out.sliceFraction[base + rank] = double(t.count[c]) * factor;  // :260
    }
}

template <bool Fill>
__global__ void __launch_bounds__(256)
censusLaneKernel(PieCensusInput in, PieCensusOutput out, uint32_t* __restrict__ longVertices, uint32_t* __restrict__ longCount,
                 uint32_t* __restrict__ error)
{
    bool bad = false;
    for (uint64_t at = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; at < in.vertexCount; at += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t v = uint32_t(at);
        uint64_t begin, end;
        if (!cellsOfVertex(in, v, begin, end, bad)) continue;
        if (end - begin > kPieWaveCells) {
            if (!Fill) longVertices[atomicAdd(longCount, 1u)] = v;     // (at most one entry per vertex: the list holds vertexCount)
            continue;
        }
        PieTally t;
#pragma unroll
        for (uint32_t c = 0; c < kPieColors; ++c) t.count[c] = t.first[c] = 0u;
        const uint32_t n = uint32_t(end - begin);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t color = colorOfCell(in, begin + i, bad);
#pragma unroll
            for (uint32_t c = 0; c < kPieColors; ++c) {
                if (color == c) {
                    if (!t.count[c]) t.first[c] = i;
                    ++t.count[c];
                }
            }
        }
        if (!Fill || !bad) emitSlices<Fill>(t, v, out);
    }
    if (bad) atomicOr(error, 1u);
}

template <bool Fill>
__global__ void __launch_bounds__(256)
censusWaveKernel(PieCensusInput in, PieCensusOutput out, const uint32_t* __restrict__ longVertices, const uint32_t* __restrict__ longCount,
                 uint32_t* __restrict__ error)
{
    bool bad = false;
    const uint32_t listed = *longCount;
    const uint32_t waves = gridDim.x * (blockDim.x / 64u), lane = threadIdx.x & 63u;
    for (uint32_t at = blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6); at < listed; at += waves) {
        const uint32_t v = longVertices[at];
        uint64_t begin, end;
        if (!cellsOfVertex(in, v, begin, end, bad)) continue;          // (the lane kernel has passed it: the same for all lanes)
        PieTally t;
#pragma unroll
        for (uint32_t c = 0; c < kPieColors; ++c) t.count[c] = t.first[c] = 0u;
        const uint64_t n = end - begin;                                // below 2^32: the entry checks cellCount
        for (uint64_t base = 0; base < n; base += 64u) {
            const uint64_t i = base + lane;
            const uint32_t color = i < n ? colorOfCell(in, begin + i, bad) : kPieColors;
#pragma unroll
            for (uint32_t c = 0; c < kPieColors; ++c) {
                const uint64_t mask = __ballot(color == c);
                if (mask) {
                    if (!t.count[c]) t.first[c] = uint32_t(base) + uint32_t(__builtin_ctzll(mask));
                    t.count[c] += uint32_t(__popcll(mask));
                }
            }
        }
        const bool anyBad = __ballot(bad) != 0u;
        if (lane == 0u && (!Fill || !anyBad)) emitSlices<Fill>(t, v, out);
    }
    if (bad) atomicOr(error, 1u);
}

// ---- the raster ----

// One block-uniform trip per 256 vertices, so that every lane of a wave takes part in the ballots.
__global__ void __launch_bounds__(256)
pieClassifyKernel(uint32_t vertexCount, const double* __restrict__ radius, double s256, const uint64_t* __restrict__ sliceOffsets,
                  uint64_t sliceCount, int32_t* __restrict__ radius256, uint32_t* __restrict__ lists, uint64_t listPitch,
                  uint32_t* __restrict__ words)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t bad = 0u;
    for (uint64_t start = uint64_t(blockIdx.x) * blockDim.x; start < vertexCount; start += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t v = start + threadIdx.x;
        uint32_t radiusClass = 3u;                                     // none: past the end, or an error
        if (v < vertexCount) {
            const double r = radius[v] * s256;                         // in 1/256 pixel
            const uint64_t a = sliceOffsets[v], b = sliceOffsets[v + 1u];
            const bool slicesFine = a < b && b <= sliceCount && (v != 0u || a == 0u) && (v + 1u != vertexCount || b == sliceCount);
            if (!slicesFine) bad |= kBadSlices;
            if (!(r >= 0.) || r > kPieMaxRadiusPixels * 256.) {
                bad |= kBadRadius;
            } else if (slicesFine) {
                const int64_t R = llround(r);
                radius256[v] = int32_t(R);
                radiusClass = R <= kPieLaneRadius ? 0u : (R <= kPieWaveRadius ? 1u : 2u);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) {
            const uint64_t mask = __ballot(radiusClass == k);
            if (!mask) continue;
            const uint32_t leader = uint32_t(__builtin_ctzll(mask));
            uint32_t base = 0u;
            if (lane == leader) base = atomicAdd(words + 1u + k, uint32_t(__popcll(mask)));
            base = uint32_t(__shfl(int(base), int(leader), 64));
            if (radiusClass == k) lists[k * listPitch + base + lanesBelow(mask)] = uint32_t(v);       // (a list holds vertexCount)
        }
    }
    if (bad) atomicOr(words, bad);
}

// `lanes` lanes (1, 64 or the 256 of a block) per listed vertex; em2_graph_draw's coverage test with the vertex's own radius.
__global__ void __launch_bounds__(256)
pieVerticesKernel(const uint32_t* __restrict__ list, uint32_t listed, const int32_t* __restrict__ ux, const int32_t* __restrict__ uy,
                  const int32_t* __restrict__ radius256, int32_t size, uint32_t lanes, uint32_t* __restrict__ vertexTop)
{
    const int64_t S = size;
    const uint64_t groups = uint64_t(gridDim.x) * blockDim.x / lanes;
    const uint32_t lane = threadIdx.x % lanes;
    for (uint64_t at = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / lanes; at < listed; at += groups) {
        const uint32_t v = list[at];
        const int64_t cx = ux[v], cy = uy[v], R = radius256[v];
        const int64_t ownI = cx >> 8, ownJ = cy >> 8;
        // the pixels whose centre can lie within R: 256 i + 128 in [cx - R, cx + R]; the own pixel is among them
        int64_t iLow = (cx - R - 128 + 255) >> 8, iHigh = (cx + R - 128) >> 8;
        int64_t jLow = (cy - R - 128 + 255) >> 8, jHigh = (cy + R - 128) >> 8;
        if (ownI < iLow) iLow = ownI;
        if (ownI > iHigh) iHigh = ownI;
        if (ownJ < jLow) jLow = ownJ;
        if (ownJ > jHigh) jHigh = ownJ;
        if (iLow < 0) iLow = 0;
        if (jLow < 0) jLow = 0;
        if (iHigh > S - 1) iHigh = S - 1;
        if (jHigh > S - 1) jHigh = S - 1;
        if (iLow > iHigh || jLow > jHigh) continue;
        const uint64_t width = uint64_t(iHigh - iLow + 1), area = width * uint64_t(jHigh - jLow + 1);
        for (uint64_t t = lane; t < area; t += lanes) {
            const int64_t i = iLow + int64_t(t % width), j = jLow + int64_t(t / width);
            const int64_t dx = 256 * i + 128 - cx, dy = 256 * j + 128 - cy;
            if (dx * dx + dy * dy <= R * R || (i == ownI && j == ownJ)) atomicMax(vertexTop + uint64_t(j) * uint64_t(S) + uint64_t(i), v + 1u);
        }
    }
}

__device__ __forceinline__ int64_t cross(int64_t px, int64_t py, int64_t qx, int64_t qy) { return px * qy - py * qx; }

__global__ void __launch_bounds__(256)
pieSlicesKernel(int32_t size, const uint32_t* __restrict__ vertexTop, const int32_t* __restrict__ ux, const int32_t* __restrict__ uy,
                const uint64_t* __restrict__ sliceOffsets, const int32_t* __restrict__ boundaryX, const int32_t* __restrict__ boundaryY,
                const uint8_t* __restrict__ largeArc, uint32_t* __restrict__ sliceTop)
{
    const uint64_t S = uint64_t(size), pixels = S * S;
    for (uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < pixels; p += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t top = vertexTop[p];
        if (!top) {
            sliceTop[p] = 0u;
            continue;
        }
        const uint32_t v = top - 1u;
        const uint64_t first = sliceOffsets[v], m = sliceOffsets[v + 1u] - first;
        const int64_t dx = 256 * int64_t(p % S) + 128 - ux[v], dy = 256 * int64_t(p / S) + 128 - uy[v];
        uint64_t slice = 0u;
        if (m >= 2u && (dx != 0 || dy != 0)) {
            // |d| <= R <= 2^21 (or 256 on the own pixel) and a boundary component is below 2^31: the products stay below 2^53
            slice = m - 1u;
            for (uint64_t k = 0; k + 1u < m; ++k) {
                const int64_t ax = boundaryX[first + k], ay = boundaryY[first + k];
                const int64_t bx = boundaryX[first + k + 1u], by = boundaryY[first + k + 1u];
                const bool inside = largeArc[first + k] ? !(cross(bx, by, dx, dy) >= 0 && cross(dx, dy, ax, ay) > 0)
                                                        : (cross(ax, ay, dx, dy) >= 0 && cross(dx, dy, bx, by) > 0);
                if (inside) {
                    slice = k;
                    break;
                }
            }
        }
        sliceTop[p] = uint32_t(first + slice) + 1u;
    }
}

template <class T> hipError_t toHost(std::vector<T>& to, const void* from, size_t count, hipStream_t stream)
{
    to.resize(count);
    if (count == 0) return hipSuccess;
    return hipMemcpyAsync(to.data(), from, count * sizeof(T), hipMemcpyDeviceToHost, stream);
}

}  // namespace

// All pointers are device memory.  *inputError is set, and out is left empty, where an id, a colour index or an offset is out of
// range.  Synchronises the stream.
static hipError_t runPieCensus(const PieCensusInput& in, PieCensusResult& out, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    out = PieCensusResult();
    out.vertexCount = in.vertexCount;
    out.sliceOffsets.assign(size_t(in.vertexCount) + 1u, 0u);
    if (in.vertexCount == 0) return hipSuccess;

    StageTimer timer("pieCensus");
    const size_t V = in.vertexCount;
    size_t scanBytes = 0;
    EM2_TRY(exclusiveScanU32ToU64Bytes(V + 1u, scanBytes));
    ArenaPlan plan;
    const size_t offWords = plan.take(256);                            // error, the number of listed vertices
    const size_t offSliceCount = plan.takeFor<uint32_t>(V + 1u);
    const size_t offZeroEnd = plan.bytes;
    const size_t offLong = plan.takeFor<uint32_t>(V);
    const size_t offOffsets = plan.takeFor<uint64_t>(V + 1u);
    const size_t offTemp = plan.take(scanBytes);
    DeviceBuffer arena;
    EM2_TRY(arena.allocate(plan.bytes));
    char* base = arena.as<char>();
    uint32_t* error = arenaAt<uint32_t>(base, offWords);
    uint32_t* longCount = error + 1;
    uint32_t* longVertices = arenaAt<uint32_t>(base, offLong);
    uint64_t* offsets = arenaAt<uint64_t>(base, offOffsets);
    EM2_TRY(hipMemsetAsync(base, 0, offZeroEnd, stream));

    PieCensusOutput slices = {arenaAt<uint32_t>(base, offSliceCount), offsets, nullptr, nullptr, nullptr};
    const dim3 threads(256);
    // a wave per listed vertex; the grid strides over a list whose length only the device knows
    const uint64_t waveBlocks = (V + 3u) / 4u;
    const dim3 waveGrid(uint32_t(waveBlocks > 4096u ? 4096u : waveBlocks));
    censusLaneKernel<false><<<dim3(gridFor(V)), threads, 0, stream>>>(in, slices, longVertices, longCount, error);
    EM2_TRY(hipGetLastError());
    censusWaveKernel<false><<<waveGrid, threads, 0, stream>>>(in, slices, longVertices, longCount, error);
    EM2_TRY(hipGetLastError());
    uint32_t words[2] = {0, 0};
    EM2_TRY(hipMemcpyAsync(words, error, sizeof(words), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (words[0]) {
        *inputError = words[0];
        return hipSuccess;
    }
    out.longVertexCount = words[1];
    EM2_TRY(timer.stage("count", stream));

    EM2_TRY(exclusiveScan(base + offTemp, scanBytes, slices.sliceCount, offsets, V + 1u, stream));
    uint64_t total = 0;
    EM2_TRY(hipMemcpyAsync(&total, offsets + V, sizeof(total), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("scan", stream));
    if (total > in.cellCount) return hipErrorUnknown;                  // (a slice holds at least one cell)

    DeviceBuffer dColor, dCells, dFraction;
    EM2_TRY(dColor.allocateFor<uint8_t>(size_t(total)));
    EM2_TRY(dCells.allocateFor<uint32_t>(size_t(total)));
    EM2_TRY(dFraction.allocateFor<double>(size_t(total)));
    slices.sliceColor = dColor.as<uint8_t>();
    slices.sliceCells = dCells.as<uint32_t>();
    slices.sliceFraction = dFraction.as<double>();
    censusLaneKernel<true><<<dim3(gridFor(V)), threads, 0, stream>>>(in, slices, longVertices, longCount, error);
    EM2_TRY(hipGetLastError());
    censusWaveKernel<true><<<waveGrid, threads, 0, stream>>>(in, slices, longVertices, longCount, error);
    EM2_TRY(hipGetLastError());
    EM2_TRY(timer.stage("fill", stream));
    EM2_TRY(toHost(out.sliceOffsets, offsets, V + 1u, stream));
    EM2_TRY(toHost(out.sliceColor, slices.sliceColor, size_t(total), stream));
    EM2_TRY(toHost(out.sliceCells, slices.sliceCells, size_t(total), stream));
    EM2_TRY(toHost(out.sliceFraction, slices.sliceFraction, size_t(total), stream));
    EM2_TRY(hipStreamSynchronize(stream));
    return timer.stage("results to the host", stream);
}

static size_t pieDrawWorkspaceBytes(uint32_t vertexCount, uint64_t edgeCount)
{
    return graphDrawWorkspaceBytes(vertexCount, edgeCount) + 256u + 4u * alignUp(size_t(vertexCount) * sizeof(uint32_t));
}

struct PieSlices {
    const uint64_t* offsets;
    uint64_t count;
    const int32_t* boundaryX;
    const int32_t* boundaryY;
    const uint8_t* largeArc;
};

// *inputError: the words of the classify and the prepare kernel; the outputs are untouched where it is not zero.
static hipError_t runGraphDrawPies(uint32_t vertexCount, const double* d_x, const double* d_y, const double* d_radius, uint64_t edgeCount,
                                   const uint32_t* d_v0, const uint32_t* d_v1, bool hideEdges, const DrawView& view, const PieSlices& slices,
                                   uint32_t* d_vertexTop, uint32_t* d_sliceTop, uint32_t* d_edgeHits, void* workspace,
                                   uint32_t* inputError, hipStream_t stream)
{
    char* at = static_cast<char*>(workspace) + graphDrawWorkspaceBytes(vertexCount, edgeCount);
    uint32_t* words = reinterpret_cast<uint32_t*>(at);                 // error, the three lists' lengths
    at += 256u;
    const size_t pitchBytes = alignUp(size_t(vertexCount) * sizeof(uint32_t));
    int32_t* radius256 = reinterpret_cast<int32_t*>(at);
    at += pitchBytes;
    uint32_t* lists = reinterpret_cast<uint32_t*>(at);
    const uint64_t listPitch = pitchBytes / sizeof(uint32_t);
    StageTimer timer("graphDrawPies");
    uint32_t host[4] = {0, 0, 0, 0};
    *inputError = 0;
    if (vertexCount) {
        EM2_TRY(hipMemsetAsync(words, 0, 256, stream));
        pieClassifyKernel<<<dim3(gridFor(vertexCount)), dim3(256), 0, stream>>>(vertexCount, d_radius, view.s256, slices.offsets, slices.count,
                                                                               radius256, lists, listPitch, words);
        EM2_TRY(hipGetLastError());
        EM2_TRY(hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (host[0]) {
            *inputError = host[0];
            return hipSuccess;
        }
        if (uint64_t(host[1]) + host[2] + host[3] != vertexCount) return hipErrorUnknown;
        EM2_TRY(timer.stage("classify", stream));
    }
    const int32_t *ux = nullptr, *uy = nullptr;
    EM2_TRY(runGraphDrawBase(vertexCount, d_x, d_y, edgeCount, d_v0, d_v1, hideEdges, view, d_vertexTop, d_edgeHits, workspace, inputError,
                             &ux, &uy, timer, stream));
    if (*inputError) return hipSuccess;
    const uint32_t lanes[3] = {1u, 64u, 256u};
    const char* stages[3] = {"vertices (lane)", "vertices (wave)", "vertices (workgroup)"};
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t listed = host[1u + k];
        if (!listed) continue;
        pieVerticesKernel<<<dim3(gridFor(uint64_t(listed) * lanes[k])), dim3(256), 0, stream>>>(lists + k * listPitch, listed, ux, uy, radius256,
                                                                                                view.size, lanes[k], d_vertexTop);
        EM2_TRY(hipGetLastError());
        EM2_TRY(timer.stage(stages[k], stream));
    }
    const uint64_t pixels = uint64_t(view.size) * uint64_t(view.size);
    pieSlicesKernel<<<dim3(gridFor(pixels)), dim3(256), 0, stream>>>(view.size, d_vertexTop, ux, uy, slices.offsets, slices.boundaryX,
                                                                     slices.boundaryY, slices.largeArc, d_sliceTop);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    return timer.stage("slices", stream);
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

uint32_t em2_pie_census_wave_cells(void) { return em2::kPieWaveCells; }

static int pieCensusCreate(const char* who, bool onDevice, uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells,
                           uint64_t cellCount, const uint32_t* idOfCell, uint32_t cellSetSize, const uint8_t* colorOfValue,
                           uint32_t valueCount, em2_pie_census** out)
{
    if (!out) return failNull(who);
    *out = nullptr;
    if (vertexCount && !cellOffsets) return failNull(who);
    if ((cellCount && !cells) || (cellSetSize && !idOfCell) || (valueCount && !colorOfValue)) return failNull(who);
    if (vertexCount == 0xffffffffu) return failArgument(who, "vertexCount must be below 2^32 - 1");
    if (cellCount > 0xffffffffull) return failArgument(who, "cellCount must be below 2^32");
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer dOffsets, dCells, dIds, dColors;
    em2::PieCensusInput in = {cellOffsets, cells, cellCount, idOfCell, cellSetSize, colorOfValue, valueCount, vertexCount};
    if (!onDevice && vertexCount) {
        EM2_HIP(dOffsets.upload(cellOffsets, size_t(vertexCount) + 1u));
        EM2_HIP(dCells.upload(cells, size_t(cellCount)));
        EM2_HIP(dIds.upload(idOfCell, size_t(cellSetSize)));
        EM2_HIP(dColors.upload(colorOfValue, size_t(valueCount)));
        in.cellOffsets = dOffsets.as<uint64_t>();
        in.cells = dCells.as<uint32_t>();
        in.idOfCell = dIds.as<uint32_t>();
        in.colorOfValue = dColors.as<uint8_t>();
    }
    std::unique_ptr<em2_pie_census> census(new em2_pie_census);
    uint32_t inputError = 0;
    EM2_HIP_FOR(who, em2::runPieCensus(in, census->result, &inputError, nullptr));
    if (inputError) {
        return failArgument(who, "an id is out of range (a cell not below cellSetSize, a value id not below valueCount, a colour index "
                                 "above 12) or the cell offsets do not ascend within cellCount");
    }
    *out = census.release();
    return EM2_OK;
}

int em2_pie_census_create(uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                          const uint32_t* idOfCell, uint32_t cellSetSize, const uint8_t* colorOfValue, uint32_t valueCount,
                          em2_pie_census** census)
{
    return pieCensusCreate("em2_pie_census", false, vertexCount, cellOffsets, cells, cellCount, idOfCell, cellSetSize, colorOfValue,
                           valueCount, census);
}

int em2_dev_pie_census(uint32_t vertexCount, const uint64_t* d_cellOffsets, const uint32_t* d_cells, uint64_t cellCount,
                       const uint32_t* d_idOfCell, uint32_t cellSetSize, const uint8_t* d_colorOfValue, uint32_t valueCount,
                       em2_pie_census** census)
{
    return pieCensusCreate("em2_dev_pie_census", true, vertexCount, d_cellOffsets, d_cells, cellCount, d_idOfCell, cellSetSize,
                           d_colorOfValue, valueCount, census);
}

int em2_pie_census_sizes(const em2_pie_census* census, uint32_t* vertexCount, uint64_t* sliceCount, uint32_t* waveVertexCount)
{
    if (!census) return failNull("em2_pie_census_sizes");
    const em2::PieCensusResult& r = census->result;
    if (vertexCount) *vertexCount = r.vertexCount;
    if (sliceCount) *sliceCount = r.sliceColor.size();
    if (waveVertexCount) *waveVertexCount = r.longVertexCount;
    return EM2_OK;
}

int em2_pie_census_get(const em2_pie_census* census, uint64_t* sliceOffsets, uint8_t* sliceColor, uint32_t* sliceCells, double* sliceFraction)
{
    if (!census) return failNull("em2_pie_census_get");
    const em2::PieCensusResult& r = census->result;
    if (sliceOffsets) std::copy(r.sliceOffsets.begin(), r.sliceOffsets.end(), sliceOffsets);
    if (sliceColor) std::copy(r.sliceColor.begin(), r.sliceColor.end(), sliceColor);
    if (sliceCells) std::copy(r.sliceCells.begin(), r.sliceCells.end(), sliceCells);
    if (sliceFraction) std::copy(r.sliceFraction.begin(), r.sliceFraction.end(), sliceFraction);
    return EM2_OK;
}

void em2_pie_census_free(em2_pie_census* census) { delete census; }

double em2_graph_draw_pies_wave_radius(void) { return double(em2::kPieWaveRadius) / 256.; }

size_t em2_dev_graph_draw_pies_workspace(uint32_t vertexCount, uint64_t edgeCount) { return em2::pieDrawWorkspaceBytes(vertexCount, edgeCount); }

static int devGraphDrawPies(const char* who, uint32_t vertexCount, const double* d_x, const double* d_y, const double* d_radius,
                            uint64_t edgeCount, const uint32_t* d_v0, const uint32_t* d_v1, int hideEdges, uint32_t sizePixels,
                            double xViewBoxCenter, double yViewBoxCenter, double viewBoxHalfSize, const uint64_t* d_sliceOffsets,
                            uint64_t sliceCount, const int32_t* d_boundaryX, const int32_t* d_boundaryY, const uint8_t* d_largeArc,
                            uint32_t* d_vertexTop, uint32_t* d_sliceTop, uint32_t* d_edgeHits, void* d_workspace, size_t workspaceBytes,
                            void* stream)
{
    em2::DrawView view;
    const int rc = em2::drawViewOf(who, vertexCount, edgeCount, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, view);
    if (rc != EM2_OK) return rc;
    if (sliceCount >= 0xffffffffull) return failArgument(who, "sliceCount must be below 2^32 - 1");
    if (!d_vertexTop || !d_sliceTop || !d_edgeHits || !d_workspace || (vertexCount && (!d_x || !d_y || !d_radius || !d_sliceOffsets)) ||
        (edgeCount && (!d_v0 || !d_v1)) || (sliceCount && (!d_boundaryX || !d_boundaryY || !d_largeArc))) {
        return failNull(who);
    }
    if (workspaceBytes < em2::pieDrawWorkspaceBytes(vertexCount, edgeCount)) return failArgument(who, "workspace too small");
    const em2::PieSlices slices = {d_sliceOffsets, sliceCount, d_boundaryX, d_boundaryY, d_largeArc};
    uint32_t inputError = 0;
    EM2_HIP_FOR(who, em2::runGraphDrawPies(vertexCount, d_x, d_y, d_radius, edgeCount, d_v0, d_v1, hideEdges != 0, view, slices, d_vertexTop,
                                           d_sliceTop, d_edgeHits, d_workspace, &inputError, static_cast<hipStream_t>(stream)));
    if (inputError & em2::kBadRadius) return failArgument(who, "a vertex radius is not between 0 and 8192 pixels");
    if (inputError & em2::kBadSlices) {
        return failArgument(who, "sliceOffsets must begin at 0, ascend strictly (every vertex has a slice) and end at sliceCount");
    }
    if (inputError & em2::kBadPosition) return failArgument(who, "a vertex position is not finite");
    if (inputError) return failArgument(who, "an edge's vertex is not below vertexCount");
    return EM2_OK;
}

int em2_dev_graph_draw_pies(uint32_t vertexCount, const double* d_x, const double* d_y, const double* d_radius, uint64_t edgeCount,
                            const uint32_t* d_v0, const uint32_t* d_v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter,
                            double yViewBoxCenter, double viewBoxHalfSize, const uint64_t* d_sliceOffsets, uint64_t sliceCount,
                            const int32_t* d_boundaryX, const int32_t* d_boundaryY, const uint8_t* d_largeArc, uint32_t* d_vertexTop,
                            uint32_t* d_sliceTop, uint32_t* d_edgeHits, void* d_workspace, size_t workspaceBytes, void* stream)
{
    return devGraphDrawPies("em2_dev_graph_draw_pies", vertexCount, d_x, d_y, d_radius, edgeCount, d_v0, d_v1, hideEdges, sizePixels,
                            xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, d_sliceOffsets, sliceCount, d_boundaryX, d_boundaryY, d_largeArc,
                            d_vertexTop, d_sliceTop, d_edgeHits, d_workspace, workspaceBytes, stream);
}

int em2_graph_draw_pies(uint32_t vertexCount, const double* x, const double* y, const double* radius, uint64_t edgeCount, const uint32_t* v0,
                        const uint32_t* v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                        double viewBoxHalfSize, const uint64_t* sliceOffsets, uint64_t sliceCount, const int32_t* boundaryX,
                        const int32_t* boundaryY, const uint8_t* largeArc, uint32_t* vertexTop, uint32_t* sliceTop, uint32_t* edgeHits)
{
    const char* who = "em2_graph_draw_pies";
    em2::DrawView view;
    const int rc = em2::drawViewOf(who, vertexCount, edgeCount, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, view);
    if (rc != EM2_OK) return rc;
    if (!vertexTop || !sliceTop || !edgeHits || (vertexCount && (!x || !y || !radius || !sliceOffsets)) || (edgeCount && (!v0 || !v1)) ||
        (sliceCount && (!boundaryX || !boundaryY || !largeArc))) {
        return failNull(who);
    }
    if (sliceCount >= 0xffffffffull) return failArgument(who, "sliceCount must be below 2^32 - 1");
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer dX, dY, dRadius, dV0, dV1, dOffsets, dBx, dBy, dArc, dTop, dSlice, dHits, dWorkspace;
    const size_t pixels = size_t(sizePixels) * sizePixels;
    const size_t workspaceBytes = em2::pieDrawWorkspaceBytes(vertexCount, edgeCount);
    EM2_HIP(dX.upload(x, vertexCount));
    EM2_HIP(dY.upload(y, vertexCount));
    EM2_HIP(dRadius.upload(radius, vertexCount));
    EM2_HIP(dV0.upload(v0, edgeCount));
    EM2_HIP(dV1.upload(v1, edgeCount));
    EM2_HIP(dOffsets.upload(sliceOffsets, vertexCount ? size_t(vertexCount) + 1u : 0u));
    EM2_HIP(dBx.upload(boundaryX, size_t(sliceCount)));
    EM2_HIP(dBy.upload(boundaryY, size_t(sliceCount)));
    EM2_HIP(dArc.upload(largeArc, size_t(sliceCount)));
    EM2_HIP(dTop.allocateFor<uint32_t>(pixels));
    EM2_HIP(dSlice.allocateFor<uint32_t>(pixels));
    EM2_HIP(dHits.allocateFor<uint32_t>(pixels));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int status = devGraphDrawPies(who, vertexCount, dX.as<double>(), dY.as<double>(), dRadius.as<double>(), edgeCount, dV0.as<uint32_t>(),
                                        dV1.as<uint32_t>(), hideEdges, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize,
                                        dOffsets.as<uint64_t>(), sliceCount, dBx.as<int32_t>(), dBy.as<int32_t>(), dArc.as<uint8_t>(),
                                        dTop.as<uint32_t>(), dSlice.as<uint32_t>(), dHits.as<uint32_t>(), dWorkspace.p, workspaceBytes, nullptr);
    if (status != EM2_OK) return status;
    EM2_HIP(dTop.download(vertexTop, pixels));
    EM2_HIP(dSlice.download(sliceTop, pixels));
    EM2_HIP(dHits.download(edgeHits, pixels));
    return EM2_OK;
}

}  // extern "C"
