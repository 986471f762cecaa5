// em2_layout_pyramid_restatement.cpp -- the spring-electrical layout with the far field of the repulsion approximated over a
// pyramid of fixed depth on one thread, in plain loops: what the pyramid entries of csrc/em2_layout.hip must
// equal bit for bit.  Every floating-point operation and the order of every sum is written out here as DESIGN.md 3.20 and
// 3.19 state them; compile with -ffp-contract=off so that nothing fuses except the fmaf calls.  Includes nothing of the
// library.  Test infrastructure only.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

namespace {

constexpr float kC = 0.2f;                 // C * K^2 with K = 1
constexpr float kFloor = 1e-30f;           // delta
constexpr double kT = 0.9;
constexpr uint32_t kChunk = 256;
constexpr uint32_t kLeafTarget = 8;
constexpr uint32_t kMaxDepth = 10;
constexpr uint32_t kDepthAuto = 0xffffffffu;

uint32_t automaticDepth(uint32_t n)
{
    for (uint32_t depth = 0; depth < kMaxDepth; depth++) {
        if ((uint64_t(kLeafTarget) << (2 * depth)) >= n) return depth;
    }
    return kMaxDepth;
}

void initialPosition(uint32_t seed, uint32_t i, float side, float* x, float* y)
{
    uint64_t z = (uint64_t(seed) << 32 | i) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float ux = float(uint32_t(z >> 40)) * 0x1p-24f - 0.5f;
    const float uy = float(uint32_t(z >> 16) & 0xffffffu) * 0x1p-24f - 0.5f;
    *x = ux * side;
    *y = uy * side;
}

struct Graph {
    uint32_t n = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> neighbours;
    Graph(uint32_t n_, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount) : n(n_), offsets(size_t(n_) + 1, 0)
    {
        std::vector<std::vector<uint32_t>> lists(n);
        for (uint64_t e = 0; e < edgeCount; e++) {
            lists[e0[e]].push_back(e1[e]);
            lists[e1[e]].push_back(e0[e]);
        }
        for (uint32_t v = 0; v < n; v++) {
            std::sort(lists[v].begin(), lists[v].end());
            offsets[v + 1] = offsets[v] + lists[v].size();
            neighbours.insert(neighbours.end(), lists[v].begin(), lists[v].end());
        }
    }
};

// The sum of 256 doubles: v[t] += v[t + stride] for stride = 128, 64, ... 1.
double tree256(double* v)
{
    for (uint32_t stride = kChunk / 2; stride >= 1; stride /= 2) {
        for (uint32_t t = 0; t < stride; t++) v[t] += v[t + stride];
    }
    return v[0];
}

// Where level l begins in an array over all cells; level l is row-major, cell (bx, by) at by * 2^l + bx.
uint32_t levelBegin(uint32_t level) { return ((1u << (2 * level)) - 1) / 3; }

uint32_t quantise(float v, float lo, float side)
{
    if (side == 0.f) return 0;
    const float u = fminf(fmaxf((v - lo) / side, 0.f), 1.f);
    return uint32_t(u * 2147483648.f);
}

// The pyramid of one evaluation.
struct Pyramid {
    uint32_t depth = 0;
    float xmin = 0.f, ymin = 0.f, side = 0.f;
    std::vector<uint32_t> qx, qy;                  // per vertex
    std::vector<uint32_t> count;                   // per cell of every level
    std::vector<uint64_t> sumX, sumY;
    std::vector<float> mx, my;                     // the centroid of a cell that is not empty
    std::vector<uint32_t> leafBegin, leafVertices; // the vertices of leaf c, ascending: leafVertices[leafBegin[c] ... leafBegin[c + 1])

    uint32_t cellOf(uint32_t q, uint32_t level) const { return std::min((1u << level) - 1, q >> (31 - level)); }

    Pyramid(uint32_t n, uint32_t depth_, const float* x, const float* y) : depth(depth_), qx(n), qy(n)
    {
        float xmax = x[0], ymax = y[0];
        xmin = x[0];
        ymin = y[0];
        for (uint32_t i = 1; i < n; i++) {
            if (x[i] < xmin) xmin = x[i];
            if (x[i] > xmax) xmax = x[i];
            if (y[i] < ymin) ymin = y[i];
            if (y[i] > ymax) ymax = y[i];
        }
        side = fmaxf(xmax - xmin, ymax - ymin);
        const uint32_t cells = levelBegin(depth + 1), leaves = 1u << (2 * depth);
        count.assign(cells, 0);
        sumX.assign(cells, 0);
        sumY.assign(cells, 0);
        mx.assign(cells, 0.f);
        my.assign(cells, 0.f);
        std::vector<uint32_t> leafOf(n);
        for (uint32_t i = 0; i < n; i++) {
            qx[i] = quantise(x[i], xmin, side);
            qy[i] = quantise(y[i], ymin, side);
            leafOf[i] = cellOf(qy[i], depth) << depth | cellOf(qx[i], depth);
            const uint32_t c = levelBegin(depth) + leafOf[i];
            count[c]++;
            sumX[c] += qx[i];
            sumY[c] += qy[i];
        }
        leafBegin.assign(size_t(leaves) + 1, 0);
        for (uint32_t c = 0; c < leaves; c++) leafBegin[c + 1] = leafBegin[c] + count[levelBegin(depth) + c];
        leafVertices.resize(n);
        std::vector<uint32_t> next(leafBegin.begin(), leafBegin.end() - 1);
        for (uint32_t i = 0; i < n; i++) leafVertices[next[leafOf[i]]++] = i;
        for (uint32_t level = depth; level-- > 0;) {
            const uint32_t width = 1u << level;
            for (uint32_t by = 0; by < width; by++) {
                for (uint32_t bx = 0; bx < width; bx++) {
                    const uint32_t c = levelBegin(level) + by * width + bx;
                    for (uint32_t child = 0; child < 4; child++) {
                        const uint32_t d = levelBegin(level + 1) + (2 * by + child / 2) * (2 * width) + 2 * bx + child % 2;
                        count[c] += count[d];
                        sumX[c] += sumX[d];
                        sumY[c] += sumY[d];
                    }
                }
            }
        }
        for (uint32_t c = 0; c < cells; c++) {
            if (!count[c]) continue;
            const double tx = double(sumX[c]) / (double(count[c]) * 2147483648.0);
            const double ty = double(sumY[c]) / (double(count[c]) * 2147483648.0);
            mx[c] = float(double(xmin) + double(side) * tx);
            my[c] = float(double(ymin) + double(side) * ty);
        }
    }
};

// f for the positions (x, y); returns the energy.  terms (may be null): the addends of each vertex's two repulsion sums.
inline __attribute__((always_inline)) double forcesBody(const Graph& g, float gravity, uint32_t depth, const float* x, const float* y, float* fx,
                                                        float* fy, uint32_t* terms)
{
    const uint32_t n = g.n;
    const Pyramid pyramid(n, depth, x, y);
    std::vector<double> chunkEnergy;
    double leaves[kChunk];
    for (uint32_t i = 0; i < n; i++) {
        const float xi = x[i], yi = y[i];
        uint32_t termCount = 0;
        // the far field: the levels 2 ... depth, the cells of the parent's neighbourhood that are not the cell's own
        float farX = 0.f, farY = 0.f;
        for (uint32_t level = 2; level <= depth; level++) {
            const int64_t width = int64_t(1) << level;
            const int64_t ax = pyramid.cellOf(pyramid.qx[i], level), ay = pyramid.cellOf(pyramid.qy[i], level);
            for (int64_t by = 2 * ((ay >> 1) - 1); by <= 2 * ((ay >> 1) + 1) + 1; by++) {
                for (int64_t bx = 2 * ((ax >> 1) - 1); bx <= 2 * ((ax >> 1) + 1) + 1; bx++) {
                    if (bx < 0 || by < 0 || bx >= width || by >= width) continue;
                    if (std::max(std::abs(bx - ax), std::abs(by - ay)) <= 1) continue;
                    const uint32_t c = levelBegin(level) + uint32_t(by * width + bx);
                    if (!pyramid.count[c]) continue;
                    const float dx = xi - pyramid.mx[c], dy = yi - pyramid.my[c];
                    const float d2 = fmaf(dx, dx, dy * dy);
                    const float w = (kC * float(pyramid.count[c])) / fmaxf(d2, kFloor);
                    farX = fmaf(dx, w, farX);
                    farY = fmaf(dy, w, farY);
                    termCount++;
                }
            }
        }
        // the near field: the leaves around the vertex's own, their vertices ascending
        float nearX = 0.f, nearY = 0.f;
        {
            const int64_t width = int64_t(1) << depth;
            const int64_t ax = pyramid.cellOf(pyramid.qx[i], depth), ay = pyramid.cellOf(pyramid.qy[i], depth);
            for (int64_t by = ay - 1; by <= ay + 1; by++) {
                for (int64_t bx = ax - 1; bx <= ax + 1; bx++) {
                    if (bx < 0 || by < 0 || bx >= width || by >= width) continue;
                    const uint32_t leaf = uint32_t(by * width + bx);
                    for (uint32_t k = pyramid.leafBegin[leaf]; k < pyramid.leafBegin[leaf + 1]; k++) {
                        const uint32_t j = pyramid.leafVertices[k];
                        const float dx = xi - x[j], dy = yi - y[j];
                        const float d2 = fmaf(dx, dx, dy * dy);
                        const float w = kC / fmaxf(d2, kFloor);
                        nearX = fmaf(dx, w, nearX);
                        nearY = fmaf(dy, w, nearY);
                        termCount++;
                    }
                }
            }
        }
        const float rx = farX + nearX, ry = farY + nearY;
        if (terms) terms[i] = termCount;
        // from here on: DESIGN.md 3.19
        float ax = 0.f, ay = 0.f;
        for (uint64_t k = g.offsets[i]; k < g.offsets[i + 1]; k++) {
            const uint32_t j = g.neighbours[k];
            const float dx = xi - x[j], dy = yi - y[j];
            const float d = sqrtf(fmaf(dx, dx, dy * dy));
            ax = fmaf(dx, d, ax);
            ay = fmaf(dy, d, ay);
        }
        float fxi = rx - ax, fyi = ry - ay;
        fxi = fmaf(-gravity, xi, fxi);
        fyi = fmaf(-gravity, yi, fyi);
        fx[i] = fxi;
        fy[i] = fyi;
        if (i % kChunk == 0) std::fill(leaves, leaves + kChunk, 0.);
        leaves[i % kChunk] = double(fxi) * double(fxi) + double(fyi) * double(fyi);
        if (i % kChunk == kChunk - 1 || i == n - 1) chunkEnergy.push_back(tree256(leaves));
    }
    for (uint32_t t = 0; t < kChunk; t++) {
        double a = 0.;
        for (size_t c = t; c < chunkEnergy.size(); c += kChunk) a += chunkEnergy[c];
        leaves[t] = a;
    }
    return tree256(leaves);
}

// fmaf is exact either way: as the x86 instruction where the processor has it, as the C library's function elsewhere.
#if defined(__x86_64__) && defined(__GNUC__)
__attribute__((target("fma"))) double forcesWithFmaInstructions(const Graph& g, float gravity, uint32_t depth, const float* x, const float* y,
                                                                float* fx, float* fy, uint32_t* terms)
{
    return forcesBody(g, gravity, depth, x, y, fx, fy, terms);
}
#endif

double forcesPortable(const Graph& g, float gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy, uint32_t* terms)
{
    return forcesBody(g, gravity, depth, x, y, fx, fy, terms);
}

double forces(const Graph& g, float gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy, uint32_t* terms)
{
#if defined(__x86_64__) && defined(__GNUC__)
    static const bool haveFma = __builtin_cpu_supports("fma");
    if (haveFma) return forcesWithFmaInstructions(g, gravity, depth, x, y, fx, fy, terms);
#endif
    return forcesPortable(g, gravity, depth, x, y, fx, fy, terms);
}

uint32_t depthFor(uint32_t n, uint32_t depth) { return depth == kDepthAuto ? automaticDepth(n) : std::min(depth, kMaxDepth); }

}  // namespace

extern "C" {

uint32_t em2rp_automatic_depth(uint32_t vertexCount) { return automaticDepth(vertexCount); }

// The pyramid at the positions x / y (vertexCount > 0): box = (xmin, ymin, S); qx / qy [vertexCount]; count / sumX / sumY / mx /
// my [(4^(depth + 1) - 1) / 3], level l from (4^l - 1) / 3, row-major.
void em2rp_pyramid(uint32_t vertexCount, uint32_t depth, const float* x, const float* y, float* box, uint32_t* qx, uint32_t* qy, uint32_t* count,
                   uint64_t* sumX, uint64_t* sumY, float* mx, float* my)
{
    const Pyramid p(vertexCount, depthFor(vertexCount, depth), x, y);
    box[0] = p.xmin;
    box[1] = p.ymin;
    box[2] = p.side;
    std::copy(p.qx.begin(), p.qx.end(), qx);
    std::copy(p.qy.begin(), p.qy.end(), qy);
    std::copy(p.count.begin(), p.count.end(), count);
    std::copy(p.sumX.begin(), p.sumX.end(), sumX);
    std::copy(p.sumY.begin(), p.sumY.end(), sumY);
    std::copy(p.mx.begin(), p.mx.end(), mx);
    std::copy(p.my.begin(), p.my.end(), my);
}

// One evaluation at the given positions, no move.  terms [vertexCount] may be null.
void em2rp_layout_forces(uint32_t vertexCount, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, double gravity, uint32_t depth,
                         const float* x, const float* y, float* fx, float* fy, double* energy, uint32_t* terms)
{
    const Graph g(vertexCount, e0, e1, edgeCount);
    const double e = vertexCount ? forces(g, float(gravity), depthFor(vertexCount, depth), x, y, fx, fy, terms) : 0.;
    if (energy) *energy = e;
}

// The run.  result: [0] the iterations done, [1] the final step, [2] the final energy (infinity where there was no evaluation).
void em2rp_layout(uint32_t vertexCount, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, uint32_t seed, uint32_t maxIterationCount,
                  double tolerance, double gravity, double initialStep, uint32_t depth, float* x, float* y, double* result)
{
    const uint32_t n = vertexCount;
    const Graph g(n, e0, e1, edgeCount);
    const uint32_t d = depthFor(n, depth);
    const float side = sqrtf(float(n));
    for (uint32_t i = 0; i < n; i++) initialPosition(seed, i, side, x + i, y + i);
    double step = initialStep, energy = std::numeric_limits<double>::infinity();
    uint32_t progress = 0, iterations = 0;
    std::vector<float> fx(n), fy(n), nx(n), ny(n);
    while (n && iterations < maxIterationCount && !(step < tolerance)) {
        const double energy0 = energy;
        energy = forces(g, float(gravity), d, x, y, fx.data(), fy.data(), nullptr);
        const float stepF = float(step);
        for (uint32_t i = 0; i < n; i++) {
            const float m = sqrtf(fmaf(fx[i], fx[i], fy[i] * fy[i]));
            nx[i] = x[i];
            ny[i] = y[i];
            if (m > 0.f) {
                const float scale = stepF / m;
                nx[i] = fmaf(fx[i], scale, x[i]);
                ny[i] = fmaf(fy[i], scale, y[i]);
            }
        }
        memcpy(x, nx.data(), size_t(n) * sizeof(float));
        memcpy(y, ny.data(), size_t(n) * sizeof(float));
        if (energy < energy0) {
            if (++progress >= 5) {
                progress = 0;
                step /= kT;
            }
        } else {
            progress = 0;
            step *= kT;
        }
        iterations++;
    }
    result[0] = double(iterations);
    result[1] = step;
    result[2] = energy;
}

}  // extern "C"
