// em2_draw.hip -- colours and the raster of a laid-out graph (the definitions are in include/em2_lsh.h).
//   * colorPartialsKernel / spectralColorsKernel   the minimum and maximum of the values (the page's loop,
//                          src/ExpressionMatrixHttpServerGraphs.cpp:1003-1015: numeric_limits<double>::max() is "no value", a NaN
//                          never replaces a bound because std::min / std::max compare with <), block partials first, which every
//                          block of the second kernel reduces again for itself; then spectralColor and color of
//                          src/color.cpp:13-79 per value, doubles with one rounding per operation.
//   * drawPrepareKernel    a thread per vertex and per edge: the one conversion from doubles, ux = floor((x - xMin) * s256)
//                          clamped to +-2^30, and the checks (a position that is not finite, an edge end not below
//                          vertexCount).  Nothing else runs, and no output is touched, before the host has seen them pass.
//   * drawVerticesKernel   `lanes` lanes per vertex (1 for radii of a few pixels, a wave above) stride over the pixels of
//                          the disc's bounding box inside the image; a covered pixel takes atomicMax(index + 1).
//   * drawEdgesKernel      a lane per edge: the range of steps k that lies in the image in closed form; an edge of at most
//                          kLongEdgeSteps steps in the image is drawn by its lane, a longer one goes to a list;
//   * drawLongEdgesKernel  a wave per listed edge, its lanes stride over k.  Every step is computed from k alone.
//   * composeKernel        a thread per pixel.
// Maximum and integer addition do not depend on the order of their operands, so no result depends on how the threads run; the
// order of the long edges' list does, and nothing reads it but the kernel that draws every member.
// The layers stay where the atomics are done, in the L2 (4 S^2 bytes each); no tile is staged in LDS.
// The view, the prepare kernel and the edge layer are also the raster with pies' (em2_pie.hip), through em2_draw.h.

#include "em2_device.h"
#include "em2_draw.h"
#include "em2_entry.h"
#include "em2_hip_util.h"

#include <cfloat>
#include <cmath>
#include <string>

namespace em2 {
namespace {

constexpr uint32_t kColorBlocks = 1024;
constexpr uint32_t kLongEdgeSteps = 64;            // an edge with more steps inside the image gets a wave
constexpr int64_t kWideRadius = 4 * 256;           // a radius above 4 pixels gets a wave per vertex
constexpr double kMaxRadiusPixels = 256.;
constexpr int32_t kClamp = 1 << 30;

// std::min(a, b) and std::max(a, b) as the page calls them: b only if it compares below (above) a.
__device__ __forceinline__ double minOf(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double maxOf(double a, double b) { return a < b ? b : a; }

__device__ __forceinline__ void blockMinMax(double& low, double& high, double* shared)
{
    for (int offset = 32; offset > 0; offset >>= 1) {
        low = minOf(low, __shfl_down(low, offset));
        high = maxOf(high, __shfl_down(high, offset));
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) {
        shared[2u * wave] = low;
        shared[2u * wave + 1u] = high;
    }
    __syncthreads();
    low = shared[0];
    high = shared[1];
    for (uint32_t w = 1; w < blockDim.x / 64u; ++w) {
        low = minOf(low, shared[2u * w]);
        high = maxOf(high, shared[2u * w + 1u]);
    }
}

__global__ void __launch_bounds__(256)
colorPartialsKernel(const double* __restrict__ values, uint64_t count, double* __restrict__ partials)
{
    __shared__ double shared[8];
    double low = DBL_MAX, high = -DBL_MAX;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const double value = values[i];
        if (value == DBL_MAX) continue;                                // :1010
        low = minOf(low, value);
        high = maxOf(high, value);
    }
    blockMinMax(low, high, shared);
    if (threadIdx.x == 0) {
        partials[2u * blockIdx.x] = low;
        partials[2u * blockIdx.x + 1u] = high;
    }
}

__global__ void __launch_bounds__(256)
spectralColorsKernel(const double* __restrict__ values, uint64_t count, const double* __restrict__ partials, uint32_t partialCount,
                     double minColorValue, double maxColorValue, int haveMin, int haveMax, uint32_t* __restrict__ rgb,
                     double* __restrict__ range)
{
    __shared__ double shared[8];
    double minValue = DBL_MAX, maxValue = -DBL_MAX;
    for (uint32_t b = threadIdx.x; b < partialCount; b += blockDim.x) {
        minValue = minOf(minValue, partials[2u * b]);
        maxValue = maxOf(maxValue, partials[2u * b + 1u]);
    }
    blockMinMax(minValue, maxValue, shared);
    if (!haveMin) minColorValue = minValue;                            // :1017-1022
    if (!haveMax) maxColorValue = maxValue;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        range[0] = minValue;
        range[1] = maxValue;
        range[2] = minColorValue;
        range[3] = maxColorValue;
    }
    const bool allBlack = minValue == maxValue || maxValue == -DBL_MAX;        // :1025
    const double scalingFactor = __ddiv_rn(1., maxColorValue - minColorValue);  // :1030
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        if (allBlack) {
            rgb[i] = EM2_COLOR_BLACK;
            continue;
        }
        const double value = values[i];
        if (value == DBL_MAX) {                                        // :1034
            rgb[i] = EM2_COLOR_NONE;
            continue;
        }
        const double x = scalingFactor * (value - minColorValue);
        double red, green;                                             // spectralColor, color.cpp:52-79; blue is 0
        if (x <= 0.) {
            red = 1.;
            green = 0.;
        } else if (x <= 0.5) {
            red = 1.;
            green = 2. * x;
        } else if (x < 1.) {
            red = 2. * (1. - x);
            green = 1.;
        } else {
            red = 0.;                                                  // a NaN comes here
            green = 1.;
        }
        red = maxOf(0., minOf(red, 1.));                               // color, color.cpp:16-23
        green = maxOf(0., minOf(green, 1.));
        const uint32_t r = uint32_t(int(red * 255.)), g = uint32_t(int(green * 255.));
        rgb[i] = (r << 16) | (g << 8);
    }
}

__device__ __forceinline__ int32_t toSubpixel(double position, double origin, double s256)
{
    double u = floor((position - origin) * s256);
    if (u > double(kClamp)) u = double(kClamp);
    if (u < -double(kClamp)) u = -double(kClamp);
    return int32_t(u);
}

__global__ void __launch_bounds__(256)
drawPrepareKernel(uint32_t vertexCount, const double* __restrict__ x, const double* __restrict__ y, uint64_t edgeCount,
                  const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1, DrawView view, int32_t* __restrict__ ux,
                  int32_t* __restrict__ uy, uint32_t* __restrict__ error)
{
    uint32_t bad = 0u;
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x, first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t v = first; v < vertexCount; v += stride) {
        const double px = x[v], py = y[v];
        if (!isfinite(px) || !isfinite(py)) {
            bad |= kBadPosition;
            continue;
        }
        ux[v] = toSubpixel(px, view.xMin, view.s256);
        uy[v] = toSubpixel(py, view.yMin, view.s256);
    }
    for (uint64_t e = first; e < edgeCount; e += stride) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) bad |= kBadEdge;
    }
    if (bad) atomicOr(error, bad);
}

__global__ void __launch_bounds__(256)
drawVerticesKernel(uint32_t vertexCount, const int32_t* __restrict__ ux, const int32_t* __restrict__ uy, DrawView view, uint32_t lanes,
                   uint32_t* __restrict__ vertexTop)
{
    const int32_t S = view.size;
    const int64_t R = view.radius;
    const uint64_t groups = uint64_t(gridDim.x) * blockDim.x / lanes;
    const uint32_t lane = threadIdx.x % lanes;
    for (uint64_t v = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / lanes; v < vertexCount; v += groups) {
        const int64_t cx = ux[v], cy = uy[v];
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
            if (dx * dx + dy * dy <= R * R || (i == ownI && j == ownJ)) atomicMax(vertexTop + uint64_t(j) * uint64_t(S) + uint64_t(i), uint32_t(v) + 1u);
        }
    }
}

// One edge as its steps: step k lies at (major0 + signM k, minor0 + signm floor((2 k dm + dM) / (2 dM))), k in [kLow, kHigh].
struct EdgeSteps {
    int64_t major0, minor0, dM, dm, kLow, kHigh;
    int32_t signM, signm;
    bool majorIsX;
};

__host__ __device__ inline int64_t floorDivide(int64_t a, int64_t b)       // b > 0
{
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__host__ __device__ inline int64_t ceilDivide(int64_t a, int64_t b) { return -floorDivide(-a, b); }      // b > 0

// The smallest k >= 0 whose minor offset floor((2 k dm + dM) / (2 dM)) is at least t (dm > 0).
__host__ __device__ inline int64_t firstStepWithOffset(int64_t t, int64_t dM, int64_t dm)
{
    const int64_t k = ceilDivide(2 * dM * t - dM, 2 * dm);
    return k < 0 ? 0 : k;
}

// The steps of the edge from pixel (i0, j0) to pixel (i1, j1) that lie in the image of S x S pixels; kLow > kHigh: none.
__host__ __device__ inline EdgeSteps clipEdge(int64_t i0, int64_t j0, int64_t i1, int64_t j1, int64_t S)
{
    EdgeSteps s;
    const int64_t dx = i1 - i0, dy = j1 - j0;
    const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    s.majorIsX = ax >= ay;
    s.major0 = s.majorIsX ? i0 : j0;
    s.minor0 = s.majorIsX ? j0 : i0;
    s.dM = s.majorIsX ? ax : ay;
    s.dm = s.majorIsX ? ay : ax;
    s.signM = (s.majorIsX ? dx : dy) < 0 ? -1 : 1;
    s.signm = (s.majorIsX ? dy : dx) < 0 ? -1 : 1;
    int64_t kLow = 0, kHigh = s.dM;
    // the major coordinate in [0, S - 1]
    if (s.signM > 0) {
        if (-s.major0 > kLow) kLow = -s.major0;
        if (S - 1 - s.major0 < kHigh) kHigh = S - 1 - s.major0;
    } else {
        if (s.major0 - (S - 1) > kLow) kLow = s.major0 - (S - 1);
        if (s.major0 < kHigh) kHigh = s.major0;
    }
    // the minor offset in [a, b], so that the minor coordinate is in [0, S - 1]; the offset does not decrease with k
    const int64_t a = s.signm > 0 ? -s.minor0 : s.minor0 - (S - 1);
    const int64_t b = s.signm > 0 ? S - 1 - s.minor0 : s.minor0;
    if (s.dm == 0) {
        if (a > 0 || b < 0) kHigh = kLow - 1;
    } else if (b < 0) {
        kHigh = kLow - 1;
    } else {
        if (a > 0) {
            const int64_t k = firstStepWithOffset(a, s.dM, s.dm);
            if (k > kLow) kLow = k;
        }
        const int64_t k = firstStepWithOffset(b + 1, s.dM, s.dm) - 1;
        if (k < kHigh) kHigh = k;
    }
    s.kLow = kLow;
    s.kHigh = kHigh;
    return s;
}

__device__ __forceinline__ void drawStep(const EdgeSteps& s, int64_t k, int64_t S, uint32_t* __restrict__ edgeHits)
{
    const int64_t major = s.major0 + s.signM * k;
    const int64_t minor = s.minor0 + (s.dM ? s.signm * ((2 * k * s.dm + s.dM) / (2 * s.dM)) : 0);
    const int64_t i = s.majorIsX ? major : minor, j = s.majorIsX ? minor : major;
    atomicAdd(edgeHits + uint64_t(j) * uint64_t(S) + uint64_t(i), 1u);
}

__device__ __forceinline__ EdgeSteps stepsOfEdge(uint64_t e, const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1,
                                                 const int32_t* __restrict__ ux, const int32_t* __restrict__ uy, int64_t S)
{
    const uint32_t a = v0[e], b = v1[e];
    return clipEdge(ux[a] >> 8, uy[a] >> 8, ux[b] >> 8, uy[b] >> 8, S);
}

__global__ void __launch_bounds__(256)
drawEdgesKernel(uint64_t edgeCount, const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1, const int32_t* __restrict__ ux,
                const int32_t* __restrict__ uy, int32_t size, uint32_t* __restrict__ edgeHits, uint32_t* __restrict__ longEdges,
                uint32_t* __restrict__ longEdgeCount)
{
    const int64_t S = size;
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const EdgeSteps s = stepsOfEdge(e, v0, v1, ux, uy, S);
        if (s.kLow > s.kHigh) continue;
        if (s.kHigh - s.kLow + 1 > int64_t(kLongEdgeSteps)) {
            longEdges[atomicAdd(longEdgeCount, 1u)] = uint32_t(e);          // (at most one entry per edge: the list holds edgeCount)
            continue;
        }
        for (int64_t k = s.kLow; k <= s.kHigh; ++k) drawStep(s, k, S, edgeHits);
    }
}

__global__ void __launch_bounds__(256)
drawLongEdgesKernel(const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1, const int32_t* __restrict__ ux,
                    const int32_t* __restrict__ uy, int32_t size, uint32_t* __restrict__ edgeHits, const uint32_t* __restrict__ longEdges,
                    const uint32_t* __restrict__ longEdgeCount)
{
    const int64_t S = size;
    const uint32_t listed = *longEdgeCount;
    const uint32_t waves = gridDim.x * (blockDim.x / 64u), lane = threadIdx.x & 63u;
    for (uint32_t at = blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6); at < listed; at += waves) {
        const EdgeSteps s = stepsOfEdge(longEdges[at], v0, v1, ux, uy, S);
        for (int64_t k = s.kLow + lane; k <= s.kHigh; k += 64) drawStep(s, k, S, edgeHits);
    }
}

__global__ void __launch_bounds__(256)
composeKernel(uint64_t pixelCount, const uint32_t* __restrict__ vertexTop, const uint32_t* __restrict__ edgeHits,
              const uint32_t* __restrict__ vertexRgb, uint32_t edgeShade, uint32_t* __restrict__ rgba)
{
    for (uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < pixelCount; p += uint64_t(gridDim.x) * blockDim.x) {
        uint32_t red = 255u, green = 255u, blue = 255u;
        const uint32_t top = vertexTop[p], hits = edgeHits[p];
        if (top) {
            const uint32_t color = vertexRgb ? vertexRgb[top - 1u] : 0u;
            red = (color >> 16) & 255u;
            green = (color >> 8) & 255u;
            blue = color & 255u;
        } else if (hits) {
            const uint64_t shade = uint64_t(edgeShade) * hits;
            red = green = blue = 255u - uint32_t(shade > 255u ? 255u : shade);
        }
        rgba[p] = red | (green << 8) | (blue << 16) | 0xff000000u;     // the bytes r, g, b, a in memory
    }
}

}  // namespace

size_t spectralColorsWorkspaceBytes() { return alignUp(size_t(kColorBlocks) * 2u * sizeof(double)); }

hipError_t runSpectralColors(const double* d_values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                             uint32_t* d_rgb, double* d_range, void* workspace, hipStream_t stream)
{
    double* partials = static_cast<double*>(workspace);
    const uint32_t blocks = gridFor(count) < kColorBlocks ? gridFor(count) : kColorBlocks;
    colorPartialsKernel<<<dim3(blocks), dim3(256), 0, stream>>>(d_values, count, partials);
    EM2_TRY(hipGetLastError());
    spectralColorsKernel<<<dim3(gridFor(count)), dim3(256), 0, stream>>>(d_values, count, partials, blocks, minColorValue, maxColorValue,
                                                                        haveMin, haveMax, d_rgb, d_range);
    return hipGetLastError();
}

size_t graphDrawWorkspaceBytes(uint32_t vertexCount, uint64_t edgeCount)
{
    return 256u + 2u * alignUp(size_t(vertexCount) * sizeof(int32_t)) + alignUp(size_t(edgeCount) * sizeof(uint32_t));
}

hipError_t runGraphDrawBase(uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                            const uint32_t* d_v1, bool hideEdges, const DrawView& view, uint32_t* d_vertexTop, uint32_t* d_edgeHits,
                            void* workspace, uint32_t* inputError, const int32_t** uxOut, const int32_t** uyOut, StageTimer& timer,
                            hipStream_t stream)
{
    char* at = static_cast<char*>(workspace);
    uint32_t* error = reinterpret_cast<uint32_t*>(at);
    uint32_t* longEdgeCount = error + 1;
    at += 256u;
    int32_t* ux = reinterpret_cast<int32_t*>(at);
    at += alignUp(size_t(vertexCount) * sizeof(int32_t));
    int32_t* uy = reinterpret_cast<int32_t*>(at);
    at += alignUp(size_t(vertexCount) * sizeof(int32_t));
    uint32_t* longEdges = reinterpret_cast<uint32_t*>(at);
    *uxOut = ux;
    *uyOut = uy;
    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    const uint64_t larger = vertexCount > edgeCount ? vertexCount : edgeCount;
    drawPrepareKernel<<<dim3(gridFor(larger)), dim3(256), 0, stream>>>(vertexCount, d_x, d_y, edgeCount, d_v0, d_v1, view, ux, uy, error);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (*inputError) return hipSuccess;
    EM2_TRY(timer.stage("prepare", stream));
    const size_t layerBytes = size_t(view.size) * size_t(view.size) * sizeof(uint32_t);
    EM2_TRY(hipMemsetAsync(d_vertexTop, 0, layerBytes, stream));
    EM2_TRY(hipMemsetAsync(d_edgeHits, 0, layerBytes, stream));
    if (!hideEdges && edgeCount) {
        drawEdgesKernel<<<dim3(gridFor(edgeCount)), dim3(256), 0, stream>>>(edgeCount, d_v0, d_v1, ux, uy, view.size, d_edgeHits, longEdges,
                                                                            longEdgeCount);
        EM2_TRY(hipGetLastError());
        // a wave per listed edge; the grid strides over a list whose length only the device knows
        const uint64_t waveBlocks = (edgeCount + 3u) / 4u;
        drawLongEdgesKernel<<<dim3(uint32_t(waveBlocks > 4096u ? 4096u : waveBlocks)), dim3(256), 0, stream>>>(
            d_v0, d_v1, ux, uy, view.size, d_edgeHits, longEdges, longEdgeCount);
        EM2_TRY(hipGetLastError());
        EM2_TRY(timer.stage("edges", stream));
    }
    return hipSuccess;
}

// *inputError: the prepare kernel's word; the outputs are untouched where it is not zero.
hipError_t runGraphDraw(uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                        const uint32_t* d_v1, bool hideEdges, const DrawView& view, uint32_t* d_vertexTop, uint32_t* d_edgeHits,
                        void* workspace, uint32_t* inputError, hipStream_t stream)
{
    StageTimer timer("graphDraw");
    const int32_t *ux = nullptr, *uy = nullptr;
    EM2_TRY(runGraphDrawBase(vertexCount, d_x, d_y, edgeCount, d_v0, d_v1, hideEdges, view, d_vertexTop, d_edgeHits, workspace, inputError,
                             &ux, &uy, timer, stream));
    if (*inputError) return hipSuccess;
    if (vertexCount) {
        const uint32_t lanes = view.radius > kWideRadius ? 64u : 1u;
        drawVerticesKernel<<<dim3(gridFor(uint64_t(vertexCount) * lanes)), dim3(256), 0, stream>>>(vertexCount, ux, uy, view, lanes, d_vertexTop);
        EM2_TRY(hipGetLastError());
    }
    EM2_TRY(hipStreamSynchronize(stream));
    return timer.stage("vertices", stream);
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

size_t em2_dev_spectral_colors_workspace(void) { return em2::spectralColorsWorkspaceBytes(); }

int em2_dev_spectral_colors(const double* d_values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                            uint32_t* d_rgb, double* d_range, void* d_workspace, size_t workspaceBytes, void* stream)
{
    const char* who = "em2_dev_spectral_colors";
    if (!d_range || !d_workspace || (count && (!d_values || !d_rgb))) return failNull(who);
    if (workspaceBytes < em2::spectralColorsWorkspaceBytes()) return failArgument(who, "workspace too small");
    EM2_HIP(em2::runSpectralColors(d_values, count, minColorValue, maxColorValue, haveMin, haveMax, d_rgb, d_range, d_workspace,
                                   static_cast<hipStream_t>(stream)));
    return EM2_OK;
}

int em2_spectral_colors(const double* values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                        uint32_t* rgb, double* range)
{
    const char* who = "em2_spectral_colors";
    if (!range || (count && (!values || !rgb))) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer dValues, dRgb, dRange, dWorkspace;
    EM2_HIP(dValues.upload(values, count));
    EM2_HIP(dRgb.allocateFor<uint32_t>(count));
    EM2_HIP(dRange.allocateFor<double>(4));
    EM2_HIP(dWorkspace.allocate(em2::spectralColorsWorkspaceBytes()));
    const int rc = em2_dev_spectral_colors(dValues.as<double>(), count, minColorValue, maxColorValue, haveMin, haveMax, dRgb.as<uint32_t>(),
                                           dRange.as<double>(), dWorkspace.p, em2::spectralColorsWorkspaceBytes(), nullptr);
    if (rc != EM2_OK) return rc;
    EM2_HIP(hipStreamSynchronize(nullptr));
    EM2_HIP(dRgb.download(rgb, count));
    EM2_HIP(dRange.download(range, 4));
    return EM2_OK;
}

uint32_t em2_graph_draw_long_edge_steps(void) { return em2::kLongEdgeSteps; }

size_t em2_dev_graph_draw_workspace(uint32_t vertexCount, uint64_t edgeCount) { return em2::graphDrawWorkspaceBytes(vertexCount, edgeCount); }

// The checks that need no device, and the view as the kernels take it (em2_draw.h: em2_pie.hip shares it).
extern "C++" int em2::drawViewOf(const char* who, uint32_t vertexCount, uint64_t edgeCount, uint32_t sizePixels, double xViewBoxCenter,
                    double yViewBoxCenter, double viewBoxHalfSize, em2::DrawView& view)
{
    if (sizePixels < 1 || sizePixels > em2::kMaxSizePixels) return failArgument(who, "sizePixels must be in [1, 8192]");
    if (vertexCount == 0xffffffffu) return failArgument(who, "vertexCount must be below 2^32 - 1");
    if (edgeCount >= (uint64_t(1) << 32)) return failArgument(who, "edgeCount must be below 2^32");
    if (!std::isfinite(viewBoxHalfSize) || viewBoxHalfSize <= 0.) return failArgument(who, "viewBoxHalfSize must be positive and finite");
    if (!std::isfinite(xViewBoxCenter) || !std::isfinite(yViewBoxCenter)) return failArgument(who, "the view box centre must be finite");
    view.xMin = xViewBoxCenter - viewBoxHalfSize;
    view.yMin = yViewBoxCenter - viewBoxHalfSize;
    view.s256 = double(sizePixels) * 256. / (2. * viewBoxHalfSize);
    view.size = int32_t(sizePixels);
    if (!std::isfinite(view.xMin) || !std::isfinite(view.yMin) || !std::isfinite(view.s256)) {
        return failArgument(who, "the view box does not convert to pixels");
    }
    view.radius = 0;
    return EM2_OK;
}

static int drawView(const char* who, uint32_t vertexCount, uint64_t edgeCount, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                    double viewBoxHalfSize, double vertexRadius, em2::DrawView& view)
{
    const int rc = em2::drawViewOf(who, vertexCount, edgeCount, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, view);
    if (rc != EM2_OK) return rc;
    const double radius = vertexRadius * view.s256;                    // in 1/256 pixel
    if (!(radius >= 0.) || radius > em2::kMaxRadiusPixels * 256.) return failArgument(who, "vertexRadius must be between 0 and 256 pixels");
    view.radius = std::llround(radius);
    return EM2_OK;
}

static int devGraphDraw(const char* who, uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                        const uint32_t* d_v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                        double viewBoxHalfSize, double vertexRadius, uint32_t* d_vertexTop, uint32_t* d_edgeHits, void* d_workspace,
                        size_t workspaceBytes, void* stream)
{
    em2::DrawView view;
    const int rc = drawView(who, vertexCount, edgeCount, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, vertexRadius, view);
    if (rc != EM2_OK) return rc;
    if (!d_vertexTop || !d_edgeHits || !d_workspace || (vertexCount && (!d_x || !d_y)) || (edgeCount && (!d_v0 || !d_v1))) return failNull(who);
    if (workspaceBytes < em2::graphDrawWorkspaceBytes(vertexCount, edgeCount)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    EM2_HIP(em2::runGraphDraw(vertexCount, d_x, d_y, edgeCount, d_v0, d_v1, hideEdges != 0, view, d_vertexTop, d_edgeHits, d_workspace,
                              &inputError, static_cast<hipStream_t>(stream)));
    if (inputError & em2::kBadPosition) return failArgument(who, "a vertex position is not finite");
    if (inputError) return failArgument(who, "an edge's vertex is not below vertexCount");
    return EM2_OK;
}

int em2_dev_graph_draw(uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                       const uint32_t* d_v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                       double viewBoxHalfSize, double vertexRadius, uint32_t* d_vertexTop, uint32_t* d_edgeHits, void* d_workspace,
                       size_t workspaceBytes, void* stream)
{
    return devGraphDraw("em2_dev_graph_draw", vertexCount, d_x, d_y, edgeCount, d_v0, d_v1, hideEdges, sizePixels, xViewBoxCenter,
                        yViewBoxCenter, viewBoxHalfSize, vertexRadius, d_vertexTop, d_edgeHits, d_workspace, workspaceBytes, stream);
}

int em2_graph_draw(uint32_t vertexCount, const double* x, const double* y, uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1,
                   int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter, double viewBoxHalfSize,
                   double vertexRadius, uint32_t* vertexTop, uint32_t* edgeHits)
{
    const char* who = "em2_graph_draw";
    em2::DrawView view;
    const int rc = drawView(who, vertexCount, edgeCount, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, vertexRadius, view);
    if (rc != EM2_OK) return rc;
    if (!vertexTop || !edgeHits || (vertexCount && (!x || !y)) || (edgeCount && (!v0 || !v1))) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer dX, dY, dV0, dV1, dTop, dHits, dWorkspace;
    const size_t pixels = size_t(sizePixels) * sizePixels;
    const size_t workspaceBytes = em2::graphDrawWorkspaceBytes(vertexCount, edgeCount);
    EM2_HIP(dX.upload(x, vertexCount));
    EM2_HIP(dY.upload(y, vertexCount));
    EM2_HIP(dV0.upload(v0, edgeCount));
    EM2_HIP(dV1.upload(v1, edgeCount));
    EM2_HIP(dTop.allocateFor<uint32_t>(pixels));
    EM2_HIP(dHits.allocateFor<uint32_t>(pixels));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int status = devGraphDraw(who, vertexCount, dX.as<double>(), dY.as<double>(), edgeCount, dV0.as<uint32_t>(), dV1.as<uint32_t>(),
                                    hideEdges, sizePixels, xViewBoxCenter, yViewBoxCenter, viewBoxHalfSize, vertexRadius,
                                    dTop.as<uint32_t>(), dHits.as<uint32_t>(), dWorkspace.p, workspaceBytes, nullptr);
    if (status != EM2_OK) return status;
    EM2_HIP(dTop.download(vertexTop, pixels));
    EM2_HIP(dHits.download(edgeHits, pixels));
    return EM2_OK;
}

int em2_dev_graph_compose(uint32_t sizePixels, const uint32_t* d_vertexTop, const uint32_t* d_edgeHits, const uint32_t* d_vertexRgb,
                          uint32_t edgeShade, uint8_t* d_rgba, void* stream)
{
    const char* who = "em2_dev_graph_compose";
    if (sizePixels < 1 || sizePixels > em2::kMaxSizePixels) return failArgument(who, "sizePixels must be in [1, 8192]");
    if (edgeShade < 1 || edgeShade > 255) return failArgument(who, "edgeShade must be in [1, 255]");
    if (!d_vertexTop || !d_edgeHits || !d_rgba) return failNull(who);
    if (reinterpret_cast<uintptr_t>(d_rgba) % 4u) return failArgument(who, "d_rgba is not aligned to 4 bytes");
    const uint64_t pixels = uint64_t(sizePixels) * sizePixels;
    em2::composeKernel<<<dim3(em2::gridFor(pixels)), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
        pixels, d_vertexTop, d_edgeHits, d_vertexRgb, edgeShade, reinterpret_cast<uint32_t*>(d_rgba));
    EM2_HIP(hipGetLastError());
    return EM2_OK;
}

int em2_graph_compose(uint32_t sizePixels, const uint32_t* vertexTop, const uint32_t* edgeHits, const uint32_t* vertexRgb, uint32_t vertexCount,
                      uint32_t edgeShade, uint8_t* rgba)
{
    const char* who = "em2_graph_compose";
    if (sizePixels < 1 || sizePixels > em2::kMaxSizePixels) return failArgument(who, "sizePixels must be in [1, 8192]");
    if (edgeShade < 1 || edgeShade > 255) return failArgument(who, "edgeShade must be in [1, 255]");
    if (!vertexTop || !edgeHits || !rgba || (vertexCount && !vertexRgb)) return failNull(who);
    const size_t pixels = size_t(sizePixels) * sizePixels;
    for (size_t p = 0; p < pixels; ++p) {
        if (vertexTop[p] > vertexCount) return failArgument(who, "a vertexTop entry is above vertexCount");
    }
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer dTop, dHits, dRgb, dRgba;
    EM2_HIP(dTop.upload(vertexTop, pixels));
    EM2_HIP(dHits.upload(edgeHits, pixels));
    EM2_HIP(dRgb.upload(vertexRgb, vertexCount));
    EM2_HIP(dRgba.allocate(pixels * 4u));
    const int rc = em2_dev_graph_compose(sizePixels, dTop.as<uint32_t>(), dHits.as<uint32_t>(), dRgb.as<uint32_t>(), edgeShade,
                                         dRgba.as<uint8_t>(), nullptr);
    if (rc != EM2_OK) return rc;
    EM2_HIP(hipStreamSynchronize(nullptr));
    EM2_HIP(hipMemcpy(rgba, dRgba.p, pixels * 4u, hipMemcpyDeviceToHost));
    return EM2_OK;
}

}  // extern "C"
