// em2_layout_restatement.cpp -- the spring-electrical layout of DESIGN.md 3.19 on one thread, in plain loops: what
// csrc/em2_layout.hip must equal bit for bit.  Every floating-point operation and the shape of every sum is written out here
// as DESIGN.md 3.19 states it; compile with -ffp-contract=off so that nothing fuses except the fmaf calls.  Test
// infrastructure only.
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
constexpr uint32_t kSliceCount = 16;
constexpr uint32_t kChunk = 256;

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

// f for the positions (x, y); returns the energy.  (Inlined into the two functions below, which differ in nothing but the
// instructions the compiler may use for fmaf.)
inline __attribute__((always_inline)) double forcesBody(const Graph& g, float gravity, const float* x, const float* y, float* fx, float* fy)
{
    const uint32_t n = g.n;
    const uint32_t sliceLength = (n + kSliceCount - 1) / kSliceCount;
    std::vector<double> chunkEnergy;
    double leaves[kChunk];
    for (uint32_t i = 0; i < n; i++) {
        const float xi = x[i], yi = y[i];
        float rx = 0.f, ry = 0.f;
        for (uint32_t s = 0; s < kSliceCount; s++) {
            const uint64_t begin = std::min<uint64_t>(uint64_t(s) * sliceLength, n);
            const uint64_t end = std::min<uint64_t>(begin + sliceLength, n);
            float px = 0.f, py = 0.f;
            for (uint64_t j = begin; j < end; j++) {
                const float dx = xi - x[j], dy = yi - y[j];
                const float d2 = fmaf(dx, dx, dy * dy);
                const float w = kC / fmaxf(d2, kFloor);
                px = fmaf(dx, w, px);
                py = fmaf(dy, w, py);
            }
            if (s == 0) {
                rx = px;
                ry = py;
            } else {
                rx += px;
                ry += py;
            }
        }
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

// fmaf is exact either way: as the x86 instruction where the processor has it (the library call costs three times the loop),
// as the C library's function elsewhere.
#if defined(__x86_64__) && defined(__GNUC__)
__attribute__((target("fma"))) double forcesWithFmaInstructions(const Graph& g, float gravity, const float* x, const float* y, float* fx, float* fy)
{
    return forcesBody(g, gravity, x, y, fx, fy);
}
#endif

double forcesPortable(const Graph& g, float gravity, const float* x, const float* y, float* fx, float* fy)
{
    return forcesBody(g, gravity, x, y, fx, fy);
}

double forces(const Graph& g, float gravity, const float* x, const float* y, float* fx, float* fy)
{
#if defined(__x86_64__) && defined(__GNUC__)
    static const bool haveFma = __builtin_cpu_supports("fma");
    if (haveFma) return forcesWithFmaInstructions(g, gravity, x, y, fx, fy);
#endif
    return forcesPortable(g, gravity, x, y, fx, fy);
}

}  // namespace

extern "C" {

void em2r_layout_initial(uint32_t vertexCount, uint32_t seed, float* x, float* y)
{
    const float side = sqrtf(float(vertexCount));
    for (uint32_t i = 0; i < vertexCount; i++) initialPosition(seed, i, side, x + i, y + i);
}

// One evaluation at the given positions, no move.
void em2r_layout_forces(uint32_t vertexCount, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, double gravity, const float* x,
                        const float* y, float* fx, float* fy, double* energy)
{
    const Graph g(vertexCount, e0, e1, edgeCount);
    const double e = vertexCount ? forces(g, float(gravity), x, y, fx, fy) : 0.;
    if (energy) *energy = e;
}

// The run.  result: [0] the iterations done, [1] the final step, [2] the final energy (the sum of |f|^2 of the last evaluation,
// infinity where there was none).
void em2r_layout(uint32_t vertexCount, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, uint32_t seed, uint32_t maxIterationCount,
                 double tolerance, double gravity, double initialStep, float* x, float* y, double* result)
{
    const uint32_t n = vertexCount;
    const Graph g(n, e0, e1, edgeCount);
    em2r_layout_initial(n, seed, x, y);
    double step = initialStep, energy = std::numeric_limits<double>::infinity();
    uint32_t progress = 0, iterations = 0;
    std::vector<float> fx(n), fy(n), nx(n), ny(n);
    while (n && iterations < maxIterationCount && !(step < tolerance)) {
        const double energy0 = energy;
        energy = forces(g, float(gravity), x, y, fx.data(), fy.data());
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
